// mmf_segments.hip — the cluster-shaped steps either side of the similarity kernels:
// everything the reference does with a vector of KMeans labels in Python loops.
//
//   segment_sort          labels -> members of every cluster in ascending row order (stable counting sort)
//   segment_mean          per-cluster mean of rows            preprocess_hypergraph.py:157-170 (mask + mean per cluster)
//   segment_offdiag_mean  mean off-diagonal similarity inside every cluster   :175-184 (K[idx][:, idx] gathers)
//   clique_pairs          all pairs inside every cluster      :395-400 (Python triple loop) after the dedup of :403
//   knn_pairs             undirected, de-duplicated k-NN pairs that no clique already contains   :386-388 + :403
//
// All of it is HBM / gather bound integer and f32 work: no matrix cores here.  Every kernel is deterministic
// (fixed summation order; the one atomic append feeds a sort).
#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

constexpr int SEG_CHUNK = 1024;          // labels per single-wave workgroup of the counting sort
constexpr int SEG_MAX = 16384;           // clusters the LDS histogram holds (64 KiB)

// ---- counting sort ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void seg_count_kernel(const int64_t* __restrict__ labels, int64_t n, int S,
                                                       uint32_t* __restrict__ block_hist, uint32_t* __restrict__ bad) {
  extern __shared__ uint32_t hist[];
  for (int s = threadIdx.x; s < S; s += 64) hist[s] = 0u;
  __syncthreads();
  const int64_t b0 = (int64_t)blockIdx.x * SEG_CHUNK;
  for (int i = threadIdx.x; i < SEG_CHUNK; i += 64) {
    const int64_t r = b0 + i;
    if (r < n) {
      const int64_t l = labels[r];
      if (l >= 0 && l < S) atomicAdd(&hist[(int)l], 1u);
      else atomicAdd(bad, 1u);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += 64) block_hist[(size_t)blockIdx.x * S + s] = hist[s];
}

// per label: exclusive prefix over the blocks (in place), total -> counts.  One workgroup per label; a thread owns a
// run of consecutive blocks (a serial walk of 256 blocks per label was 61 us of dependent global round trips).
__global__ __launch_bounds__(256) void seg_block_scan_kernel(uint32_t* __restrict__ block_hist, int nb, int S, int64_t* __restrict__ counts) {
  __shared__ uint32_t part[256];
  const int s = blockIdx.x, t = threadIdx.x;
  const int per = (nb + 255) / 256, b0 = t * per, b1 = (b0 + per < nb) ? b0 + per : nb;
  uint32_t sum = 0;
  for (int b = b0; b < b1; ++b) sum += block_hist[(size_t)b * S + s];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t v = (t >= o) ? part[t - o] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;
  for (int b = b0; b < b1; ++b) {
    const uint32_t c = block_hist[(size_t)b * S + s];
    block_hist[(size_t)b * S + s] = run;
    run += c;
  }
  if (t == 255) counts[s] = (int64_t)part[255];
}

// offsets[0..S] = exclusive scan of counts (one workgroup; S <= SEG_MAX)
__global__ __launch_bounds__(1024) void seg_offsets_kernel(const int64_t* __restrict__ counts, int S, int64_t* __restrict__ offsets) {
  __shared__ unsigned long long part[1024];
  const int t = threadIdx.x;
  const int per = (S + 1023) / 1024;
  const int b = t * per;
  int e = b + per;
  if (e > S) e = S;
  unsigned long long sum = 0;
  for (int i = b; i < e; ++i) sum += (unsigned long long)counts[i];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long v = (t >= o) ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = (t == 0) ? 0ull : part[t - 1];
  for (int i = b; i < e; ++i) { offsets[i] = (int64_t)run; run += (unsigned long long)counts[i]; }
  if (t == 1023) offsets[S] = (int64_t)part[1023];
}

// stable scatter: one wave walks its chunk in row order.  The lanes that share a label find each other with one ballot
// per label BIT (the mask of lanes that agree with this lane on every bit), so a step costs the same however many
// distinct labels its 64 rows carry (a leader loop over the distinct labels was 47 rounds per step at S = 100).
__global__ __launch_bounds__(64) void seg_scatter_kernel(const int64_t* __restrict__ labels, int64_t n, int S, int bits,
                                                         const uint32_t* __restrict__ block_hist,
                                                         const int64_t* __restrict__ offsets, int64_t* __restrict__ order) {
  extern __shared__ uint32_t cursor[];     // position of the next member of each label, relative to offsets[label]
  for (int s = threadIdx.x; s < S; s += 64) cursor[s] = block_hist[(size_t)blockIdx.x * S + s];
  __syncthreads();
  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * SEG_CHUNK;
  for (int i0 = 0; i0 < SEG_CHUNK; i0 += 64) {
    const int64_t r = b0 + i0 + lane;
    int l = -1;
    if (r < n) {
      const int64_t ll = labels[r];
      if (ll >= 0 && ll < S) l = (int)ll;
    }
    unsigned long long match = __ballot(l >= 0);
    for (int b = 0; b < bits; ++b) {
      const unsigned long long mb = __ballot((l >> b) & 1);
      match &= ((l >> b) & 1) ? mb : ~mb;
    }
    uint32_t cur = 0;
    if (l >= 0) cur = cursor[l];
    __syncthreads();                   // one wave per workgroup: orders the LDS reads above before the updates below
    if (l >= 0) {
      const uint32_t rank = (uint32_t)__popcll(match & ((1ull << lane) - 1ull));
      order[offsets[l] + (int64_t)(cur + rank)] = r;
      if (rank == 0) cursor[l] = cur + (uint32_t)__popcll(match);      // the label's first lane of this step
    }
    __syncthreads();
  }
}

size_t segment_sort_scratch_bytes(int64_t n, int64_t S) {
  const int64_t nb = (n + SEG_CHUNK - 1) / SEG_CHUNK;
  return (size_t)nb * (size_t)S * 4 + 256;
}

int launch_segment_sort(const int64_t* labels, int64_t n, int64_t S, int64_t* counts, int64_t* offsets, int64_t* order,
                        void* scratch, uint32_t* bad, hipStream_t s) {
  const int nb = (int)((n + SEG_CHUNK - 1) / SEG_CHUNK);
  uint32_t* block_hist = reinterpret_cast<uint32_t*>(scratch);
  const size_t lds = (size_t)S * 4;
  MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(seg_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(seg_scatter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  MMF_HIP(hipMemsetAsync(bad, 0, 4, s));
  hipLaunchKernelGGL(seg_count_kernel, dim3((unsigned)nb), dim3(64), lds, s, labels, n, (int)S, block_hist, bad);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_block_scan_kernel, dim3((unsigned)S), dim3(256), 0, s, block_hist, nb, (int)S, counts);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_offsets_kernel, dim3(1), dim3(1024), 0, s, counts, (int)S, offsets);
  MMF_LAUNCH_CHECK();
  int bits = 0;
  while ((int64_t(1) << bits) < S) ++bits;
  hipLaunchKernelGGL(seg_scatter_kernel, dim3((unsigned)nb), dim3(64), lds, s, labels, n, (int)S, bits, block_hist, offsets, order);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// ---- per-cluster mean of rows -----------------------------------------------------------------------------------
// Workgroup = (cluster, strip of 64 columns), 8 waves; wave w adds the cluster's rows w, w + 8, ... in member order
// (four row loads in flight, added in order), the eight partial sums are combined in wave order: one fixed summation
// order, coalesced 256-byte row segments.
constexpr int SM_W = 8;
__global__ __launch_bounds__(64 * SM_W) void seg_mean_kernel(const float* __restrict__ X, int64_t d, const int64_t* __restrict__ order,
                                                             const int64_t* __restrict__ offsets, float* __restrict__ out) {
  __shared__ float part[SM_W][64];
  const int c = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t col = (int64_t)blockIdx.y * 64 + lane;
  const int w = threadIdx.x >> 6;
  const int64_t b = offsets[c], e = offsets[c + 1];
  float acc = 0.f;
  if (col < d) {
    int64_t q = b + w;
    // eight row loads in flight per wave; the member indices of the NEXT trip are read while this trip's rows arrive
    // (index -> row is two dependent round trips otherwise).  The adds stay in member order.
    int64_t r[8];
    bool more = q + 7 * SM_W < e;
    if (more) {
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] = order[q + u * SM_W];
    }
    while (more) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = X[r[u] * d + col];
      q += 8 * SM_W;
      more = q + 7 * SM_W < e;
      if (more) {
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = order[q + u * SM_W];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += x[u];
    }
    for (; q < e; q += SM_W) acc += X[order[q] * d + col];
  }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && col < d) {
    float sum = part[0][lane];
#pragma unroll
    for (int i = 1; i < SM_W; ++i) sum += part[i][lane];
    out[(int64_t)c * d + col] = sum / (float)(e - b);            // empty cluster: 0 / 0 = NaN (the caller rejects it first)
  }
}

int launch_segment_mean(const float* X, int64_t d, const int64_t* order, const int64_t* offsets, int64_t S, float* out, hipStream_t s) {
  hipLaunchKernelGGL(seg_mean_kernel, dim3((unsigned)S, (unsigned)((d + 63) / 64)), dim3(64 * SM_W), 0, s, X, d, order, offsets, out);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// ---- mean off-diagonal similarity inside every cluster ------------------------------------------------------------
// row_sum[q] = sum over the other members b of K[member q][member b] (one wave per member, f64, lane-strided then a
// fixed butterfly); cluster mean = (sum of its row sums in member order) / (m (m - 1)).  Direct gathers: no
// "block sum minus diagonal" cancellation.
__global__ __launch_bounds__(256) void seg_row_sums_kernel(const float* __restrict__ K, int64_t n, const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ offsets, const int32_t* __restrict__ seg_of,
                                                           int64_t total, double* __restrict__ row_sum) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= total) return;
  const int c = seg_of[q];
  const int64_t b = offsets[c], e = offsets[c + 1];
  const float* row = K + order[q] * n;
  double acc = 0.0;
  for (int64_t p = b + lane; p < e; p += 64)
    if (p != q) acc += (double)row[order[p]];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) row_sum[q] = acc;
}

__global__ void seg_of_kernel(const int64_t* __restrict__ offsets, int S, int32_t* __restrict__ seg_of) {
  const int c = blockIdx.x;
  if (c >= S) return;
  for (int64_t q = offsets[c] + threadIdx.x; q < offsets[c + 1]; q += blockDim.x) seg_of[q] = c;
}

__global__ void seg_offdiag_final_kernel(const double* __restrict__ row_sum, const int64_t* __restrict__ offsets, int S,
                                         double* __restrict__ out_mean) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S) return;
  const int64_t b = offsets[c], e = offsets[c + 1], m = e - b;
  if (m <= 1) { out_mean[c] = __builtin_nan(""); return; }       // the reference skips such clusters (:178)
  double sum = 0.0;
  for (int64_t q = b; q < e; ++q) sum += row_sum[q];
  out_mean[c] = sum / ((double)m * (double)(m - 1));
}

size_t segment_offdiag_scratch_bytes(int64_t n) { return ws_bytes((size_t)n, 8) + ws_bytes((size_t)n, 4); }

int launch_segment_offdiag_mean(const float* K, int64_t n, const int64_t* order, const int64_t* offsets, int64_t S,
                                double* out_mean, void* scratch, hipStream_t s) {
  double* row_sum = reinterpret_cast<double*>(scratch);
  int32_t* seg_of = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(scratch) + ws_bytes((size_t)n, 8));
  MMF_TRY(launch_segment_member_clusters(offsets, S, seg_of, s));
  hipLaunchKernelGGL(seg_row_sums_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, K, n, order, offsets, seg_of, n, row_sum);
  MMF_LAUNCH_CHECK();
  return launch_segment_offdiag_final(row_sum, offsets, S, out_mean, s);
}

// its two ends, also for a K that is recomputed in panels (mmf_stream_stats.hip): the cluster of every member before the row
// sums, the clusters' means after the last of them
int launch_segment_member_clusters(const int64_t* offsets, int64_t S, int32_t* seg_of, hipStream_t s) {
  hipLaunchKernelGGL(seg_of_kernel, dim3((unsigned)S), dim3(256), 0, s, offsets, (int)S, seg_of);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_segment_offdiag_final(const double* row_sum, const int64_t* offsets, int64_t S, double* out_mean, hipStream_t s) {
  hipLaunchKernelGGL(seg_offdiag_final_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, row_sum, offsets, (int)S, out_mean);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// ---- clique expansion -----------------------------------------------------------------------------------------------
// Cluster c with members r_0 < r_1 < ... contributes the pairs (r_a, r_b), a < b — what `set(tuple(sorted(e)))` leaves of
// the reference's m (m - 1) ordered pairs (:395-404).  pair_off[c] = pairs of the clusters before c.
__global__ __launch_bounds__(1024) void clique_offsets_kernel(const int64_t* __restrict__ offsets, int S,
                                                              unsigned long long* __restrict__ pair_off, int64_t* __restrict__ out_count) {
  __shared__ unsigned long long part[1024];
  const int t = threadIdx.x;
  const int per = (S + 1023) / 1024;
  const int b = t * per;
  int e = b + per;
  if (e > S) e = S;
  auto pairs = [&](int c) { const unsigned long long m = (unsigned long long)(offsets[c + 1] - offsets[c]); return m * (m - (m ? 1 : 0)) / 2; };
  unsigned long long sum = 0;
  for (int i = b; i < e; ++i) sum += pairs(i);
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long v = (t >= o) ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = (t == 0) ? 0ull : part[t - 1];
  for (int i = b; i < e; ++i) { pair_off[i] = run; run += pairs(i); }
  if (t == 1023) *out_count = (int64_t)part[1023];
}

// one wave per member a: its partners b > a are consecutive in `order`, so `hi` is a coalesced copy
__global__ __launch_bounds__(256) void clique_fill_kernel(const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ seg_of, const unsigned long long* __restrict__ pair_off,
                                                          int64_t total, int64_t* __restrict__ lo, int64_t* __restrict__ hi, int64_t capacity) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= total) return;
  const int c = seg_of[q];
  const int64_t b = offsets[c], e = offsets[c + 1];
  const unsigned long long m = (unsigned long long)(e - b), a = (unsigned long long)(q - b);
  const unsigned long long base = pair_off[c] + a * m - a * (a + 1) / 2;      // pairs of members 0 .. a-1
  const int64_t ra = order[q];
  for (int64_t p = q + 1 + lane; p < e; p += 64) {
    const unsigned long long pos = base + (unsigned long long)(p - q - 1);
    if ((int64_t)pos < capacity) { lo[pos] = ra; hi[pos] = order[p]; }
  }
}

size_t clique_scratch_bytes(int64_t n, int64_t S) { return ws_bytes((size_t)S + 1, 8) + ws_bytes((size_t)n, 4); }

int launch_clique_pairs(const int64_t* order, const int64_t* offsets, int64_t n, int64_t S, int64_t* lo, int64_t* hi,
                        int64_t capacity, int64_t* out_count, void* scratch, hipStream_t s) {
  unsigned long long* pair_off = reinterpret_cast<unsigned long long*>(scratch);
  int32_t* seg_of = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(scratch) + ws_bytes((size_t)S + 1, 8));
  hipLaunchKernelGGL(clique_offsets_kernel, dim3(1), dim3(1024), 0, s, offsets, (int)S, pair_off, out_count);
  MMF_LAUNCH_CHECK();
  if (capacity > 0) {
    hipLaunchKernelGGL(seg_of_kernel, dim3((unsigned)S), dim3(256), 0, s, offsets, (int)S, seg_of);
    MMF_LAUNCH_CHECK();
    hipLaunchKernelGGL(clique_fill_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, order, offsets, seg_of, pair_off, n, lo, hi, capacity);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

// ---- k-NN pairs -------------------------------------------------------------------------------------------------
// Directed pair i -> j (j = nbr[i][t]) becomes the undirected (min, max).  It is dropped when a clique already holds it
// (labels given and equal) or when the same pair is also emitted by the smaller row (j < i and i in nbr[j]): what is
// left is duplicate-free without a sort.  Appended with one atomic per workgroup; the caller orders the union.
__global__ __launch_bounds__(1024) void knn_pairs_kernel(const int64_t* __restrict__ nbr, int64_t n, int k, const int64_t* __restrict__ labels,
                                                         int64_t* __restrict__ lo, int64_t* __restrict__ hi,
                                                         unsigned long long* __restrict__ count) {
  __shared__ unsigned int wcnt[16];
  __shared__ unsigned long long wbase;
  const int64_t t = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool keep = false;
  int64_t i = 0, j = 0;
  if (t < n * k) {
    i = t / k;
    j = nbr[t];
    keep = (j >= 0 && j < n && j != i);
    if (keep && labels && labels[i] == labels[j]) keep = false;
    if (keep && j < i) {
      for (int u = 0; u < k; ++u)
        if (nbr[j * k + u] == i) { keep = false; break; }
    }
  }
  // one reservation per workgroup: 20 000 waves appending through one counter queued up at the L2 (0.25 ms for 1.3 M pairs)
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wave] = (unsigned int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int run = 0;
    for (int w = 0; w < 16; ++w) { const unsigned int c = wcnt[w]; wcnt[w] = run; run += c; }
    wbase = run ? atomicAdd(count, (unsigned long long)run) : 0ull;
  }
  __syncthreads();
  if (keep) {
    const unsigned long long pos = wbase + wcnt[wave] + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    lo[pos] = i < j ? i : j;
    hi[pos] = i < j ? j : i;
  }
}

int launch_knn_pairs(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t* lo, int64_t* hi, int64_t* out_count,
                     hipStream_t s) {
  MMF_HIP(hipMemsetAsync(out_count, 0, 8, s));
  const int64_t total = n * k;
  if (total == 0) return MMF_OK;
  hipLaunchKernelGGL(knn_pairs_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(1024), 0, s, nbr, n, k, labels, lo, hi,
                     reinterpret_cast<unsigned long long*>(out_count));
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int segment_max_segments() { return SEG_MAX; }

}  // namespace mmf
