// mmf_knn_clique.hip — the edge list of the k-NN + KMeans hypergraph for every graph
// of a ragged batch, written in its documented order without a sort.
//
// Row i owns the edges (i, j), j > i:  the later members of its cluster  ∪  its k-NN partners from another cluster
// (j in nbr[i], or i in nbr[j]; kept once, by the rule of knn_pairs_kernel).  The first list is ascending in the
// cluster's member list; the second is short except at a hub.  One wave per row merges them into the row's slot.
//
//   kc_rows       row -> segment, global cluster id = segment * H + label, cluster sizes (atomic counts: order-free)
//   kc_members    one wave per segment: offsets of its H clusters, then a stable scatter (members ascending per cluster)
//   kc_knn        one thread per directed entry: keep / drop, then count (count entry) or append to its row's tail (fill)
//   kc_scan_*     exclusive scan of the row totals over all rows, 1024 rows per workgroup
//   kc_merge      one wave per row: sort the tail, merge it with the clique partners, write lo / hi
//
// Atomics only reserve space (a cluster's cursor, a row's tail cursor); the tail is sorted before it is merged, so the
// result does not depend on their order.  No cluster-count cap: the cursors live in global memory.
#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

constexpr int KC_SCAN = 1024;            // rows per workgroup of the row scan

__device__ __forceinline__ int kc_segment_of(const int64_t* __restrict__ ptr, int n_seg, int64_t i) {
  int lo = 0, hi = n_seg;                // last s with ptr[s] <= i (skips empty segments); i < ptr[n_seg]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void kc_rows_kernel(const int64_t* __restrict__ labels, int64_t n, int64_t H,
                                                      const int64_t* __restrict__ ptr, int n_seg, int32_t* __restrict__ gid,
                                                      int32_t* __restrict__ ccur, uint32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t l = labels[i];
  if (l < 0 || l >= H) { gid[i] = -1; atomicOr(bad, 1u); return; }
  const int32_t g = (int32_t)((int64_t)kc_segment_of(ptr, n_seg, i) * H + l);
  gid[i] = g;
  atomicAdd(&ccur[g], 1);
}

// One wave per segment.  ccur[s H + h] holds the size of cluster h; it becomes the cluster's first position in `members`
// (segment s's members fill ptr[s] .. ptr[s+1]), then the scatter advances it to the cluster's end.  The scatter walks the
// rows in order, 64 at a time; lanes of one label find each other with one ballot per label bit (seg_scatter_kernel), the
// first of them reserves the run.
__global__ __launch_bounds__(256) void kc_members_kernel(const int32_t* __restrict__ gid, const int64_t* __restrict__ ptr, int n_seg,
                                                         int64_t H, int bits, int32_t* __restrict__ ccur,
                                                         int32_t* __restrict__ members, int32_t* __restrict__ pos) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_seg) return;
  const int64_t r0 = ptr[s], r1 = ptr[s + 1];
  const int64_t base = s * H;
  int32_t run = (int32_t)r0;
  for (int64_t h0 = 0; h0 < H; h0 += 64) {
    const int64_t h = h0 + lane;
    const int32_t v = h < H ? ccur[base + h] : 0;
    int32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (h < H) ccur[base + h] = run + incl - v;
    run += __shfl(incl, 63);
  }
  __threadfence();                       // the offsets above are read back through atomics by other lanes of this wave
  for (int64_t i0 = r0; i0 < r1; i0 += 64) {
    const int64_t r = i0 + lane;
    const int32_t g = r < r1 ? gid[r] : -1;
    const int32_t l = g >= 0 ? (int32_t)(g - base) : -1;
    unsigned long long match = __ballot(l >= 0);
    for (int b = 0; b < bits; ++b) {
      const unsigned long long mb = __ballot((l >> b) & 1);
      match &= ((l >> b) & 1) ? mb : ~mb;
    }
    const int rank = __popcll(match & ((1ull << lane) - 1ull));
    int32_t first = 0;
    if (l >= 0 && rank == 0) first = atomicAdd(&ccur[g], (int32_t)__popcll(match));
    const int leader = l >= 0 ? __ffsll((long long)match) - 1 : lane;
    first = __shfl(first, leader);
    if (l >= 0) {
      members[first + rank] = (int32_t)r;
      pos[r] = first + rank;
    }
  }
}

// later members of row i's cluster (its clique partners)
__device__ __forceinline__ int32_t kc_later(const int32_t* __restrict__ gid, const int32_t* __restrict__ ccur,
                                            const int32_t* __restrict__ pos, int64_t i) {
  if (!gid) return 0;
  const int32_t g = gid[i];
  return g >= 0 ? ccur[g] - pos[i] - 1 : 0;
}

// The rule of knn_pairs_kernel, with "same label" meaning the same (segment, label).  FILL: the partner goes to the tail of
// its row's slot (after the clique partners), the cursor only reserves the place; otherwise the row's counter goes up.
template <bool FILL>
__global__ __launch_bounds__(256) void kc_knn_kernel(const int64_t* __restrict__ nbr, int64_t n, int k, const int32_t* __restrict__ gid,
                                                     const int32_t* __restrict__ ccur, const int32_t* __restrict__ pos,
                                                     uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ row_off,
                                                     int64_t* __restrict__ hi_out, int64_t capacity) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * k) return;
  const int64_t i = t / k, j = nbr[t];
  if (j < 0 || j >= n || j == i) return;
  if (gid && gid[i] == gid[j]) return;
  if (j < i) {
    for (int u = 0; u < k; ++u)
      if (nbr[j * k + u] == i) return;
  }
  const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
  const uint32_t slot = atomicAdd(&cnt[lo], 1u);
  if (FILL) {
    const unsigned long long p = row_off[lo] + (unsigned long long)kc_later(gid, ccur, pos, lo) + slot;
    if (p < row_off[lo + 1] && (int64_t)p < capacity) hi_out[p] = hi;
  }
}

// local exclusive scan of (tail + clique partners) per row inside a workgroup of KC_SCAN rows, and the workgroup's sum
__global__ __launch_bounds__(KC_SCAN) void kc_scan_local_kernel(const uint32_t* __restrict__ cnt, const int32_t* __restrict__ gid,
                                                                const int32_t* __restrict__ ccur, const int32_t* __restrict__ pos,
                                                                int64_t n, unsigned long long* __restrict__ row_off,
                                                                unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long wsum[KC_SCAN / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * KC_SCAN + threadIdx.x;
  const unsigned long long v = i < n ? (unsigned long long)cnt[i] + (unsigned long long)kc_later(gid, ccur, pos, i) : 0ull;
  unsigned long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  unsigned long long before = 0;
  for (int u = 0; u < w; ++u) before += wsum[u];
  if (i < n) row_off[i] = before + incl - v;
  if (threadIdx.x == KC_SCAN - 1) bsum[blockIdx.x] = before + incl;
}

// exclusive scan of the workgroup sums (one workgroup), the total, and the validity flag folded into the count
__global__ __launch_bounds__(1024) void kc_scan_blocks_kernel(unsigned long long* __restrict__ bsum, int64_t nb, int64_t n,
                                                              unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ bad,
                                                              int64_t* __restrict__ out_count) {
  __shared__ unsigned long long part[1024];
  const int t = threadIdx.x;
  const int64_t per = (nb + 1023) / 1024;
  const int64_t b = (int64_t)t * per;
  const int64_t e = b + per < nb ? b + per : nb;
  unsigned long long sum = 0;
  for (int64_t i = b; i < e; ++i) sum += bsum[i];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long v = (t >= o) ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = (t == 0) ? 0ull : part[t - 1];
  for (int64_t i = b; i < e; ++i) { const unsigned long long c = bsum[i]; bsum[i] = run; run += c; }
  if (t == 1023) {
    row_off[n] = part[1023];
    *out_count = *bad ? (int64_t)-1 : (int64_t)part[1023];
  }
}

__global__ __launch_bounds__(KC_SCAN) void kc_scan_add_kernel(const unsigned long long* __restrict__ bsum, int64_t n,
                                                              unsigned long long* __restrict__ row_off) {
  const int64_t i = (int64_t)blockIdx.x * KC_SCAN + threadIdx.x;
  if (i < n) row_off[i] += bsum[blockIdx.x];
}

__global__ __launch_bounds__(256) void kc_edge_ptr_kernel(const unsigned long long* __restrict__ row_off, const int64_t* __restrict__ ptr,
                                                          int n_seg, int64_t* __restrict__ edge_ptr) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s <= n_seg) edge_ptr[s] = (int64_t)row_off[ptr[s]];
}

// One wave per row.  Slot [b, e) of the row: c clique partners (members after the row in its cluster, ascending) and a
// tail of t k-NN partners that kc_knn_kernel<true> left unordered in hi[b + c, e).  No value is in both lists.
//   t <= 64: the tail is ranked in registers and parked in LDS; a clique partner lands at (its index + tail entries below
//            it), a tail entry at (its rank + clique partners below it): hi goes out as coalesced runs.
//   t >  64: a hub.  The tail is sorted where it lies (bitonic network over global memory, every compare ascending so the
//            virtual padding never moves), then merged from the front in chunks of 64 outputs by merge path: a chunk reads
//            before it writes, and what it writes lies below every tail entry that is still unread.  Slow, and correct.
__global__ __launch_bounds__(256) void kc_merge_kernel(const int32_t* __restrict__ gid, const int32_t* __restrict__ ccur,
                                                       const int32_t* __restrict__ pos, const int32_t* __restrict__ members, int64_t n,
                                                       const unsigned long long* __restrict__ row_off, int64_t* __restrict__ lo_out,
                                                       int64_t* __restrict__ hi_out, int64_t capacity) {
  __shared__ int64_t tail_s[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + w;
  if (i >= n) return;
  const int64_t b = (int64_t)row_off[i], e = (int64_t)row_off[i + 1];
  if (e > capacity || e <= b) return;
  const int64_t c = kc_later(gid, ccur, pos, i);
  const int64_t t = e - b - c;
  if (t < 0) return;                                             // inputs changed between count and fill
  const int32_t* mem = c > 0 ? members + pos[i] + 1 : members;   // the c clique partners
  for (int64_t q = lane; q < e - b; q += 64) lo_out[b + q] = i;
  int64_t* tail = hi_out + b + c;
  if (t <= 64) {
    const int64_t x = lane < t ? tail[lane] : INT64_MAX;
    int rank = 0;
    for (int u = 0; u < (int)t; ++u) {
      const int64_t y = __shfl(x, u);
      rank += (y < x || (y == x && u < lane)) ? 1 : 0;
    }
    if (lane < t) tail_s[w][rank] = x;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // one wave per row: its LDS writes are done before its reads
    __builtin_amdgcn_wave_barrier();
    if (lane < t) {                                              // clique partners below this tail entry
      const int64_t v = tail_s[w][lane];
      int64_t l = 0, h = c;
      while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if ((int64_t)mem[mid] < v) l = mid + 1; else h = mid;
      }
      hi_out[b + lane + l] = v;
    }
    for (int64_t q = lane; q < c; q += 64) {
      const int64_t m = (int64_t)mem[q];
      int below = 0;
      for (int u = 0; u < (int)t; ++u) below += tail_s[w][u] < m ? 1 : 0;
      hi_out[b + q + below] = m;
    }
    return;
  }
  // ---- hub ----
  int64_t P = 128;
  while (P < t) P <<= 1;
  for (int64_t kk = 2; kk <= P; kk <<= 1) {
    for (int64_t j = kk >> 1; j > 0; j >>= 1) {
      for (int64_t p = lane; p < (P >> 1); p += 64) {
        const int64_t a = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int64_t z = (j == (kk >> 1)) ? (a ^ (kk - 1)) : (a | j);
        if (z < t) {
          const int64_t va = tail[a], vz = tail[z];
          if (vz < va) { tail[a] = vz; tail[z] = va; }
        }
      }
      __threadfence();
    }
  }
  for (int64_t w0 = 0; w0 < c + t; w0 += 64) {
    const int64_t o = w0 + lane;                                 // output position inside the slot
    int64_t v = 0;
    if (o < c + t) {
      // a = clique partners among the first o outputs: the smallest a with mem[a] > tail[o - a - 1] failing, by bisection
      int64_t l = o > t ? o - t : 0, h = o < c ? o : c;
      while (l < h) {
        const int64_t a = (l + h) >> 1;                          // a < c and o - a - 1 >= 0 here
        if ((int64_t)mem[a] < tail[o - a - 1]) l = a + 1; else h = a;
      }
      const int64_t r = o - l;
      v = (l < c && (r >= t || (int64_t)mem[l] < tail[r])) ? (int64_t)mem[l] : tail[r];
    }
    __threadfence();
    if (o < c + t) hi_out[b + o] = v;
    __threadfence();
  }
}

size_t knn_clique_scratch_bytes(int64_t n, int64_t n_seg, int64_t H, bool with_labels) {
  size_t b = ws_bytes((size_t)n_seg + 1, 8) + ws_bytes((size_t)n, 4) + ws_bytes((size_t)((n + KC_SCAN - 1) / KC_SCAN) + 1, 8) + 256;
  if (with_labels) b += 3 * ws_bytes((size_t)n, 4) + ws_bytes((size_t)(n_seg * H), 4);
  return b;
}

namespace {
struct KcState {
  int64_t* d_ptr; uint32_t* cnt; unsigned long long* bsum; uint32_t* bad;
  int32_t *gid, *members, *pos, *ccur;
};

// the part both entries share: tables up, clusters and their member lists
int kc_prepare(const int64_t* labels, int64_t n, int64_t H, const int64_t* ptr_host, int64_t n_seg, char* scratch, KcState* st,
               hipStream_t s) {
  Workspace ws;
  ws.base = scratch;
  st->d_ptr = ws.take<int64_t>((size_t)n_seg + 1);
  st->cnt = ws.take<uint32_t>((size_t)n);
  st->bsum = ws.take<unsigned long long>((size_t)((n + KC_SCAN - 1) / KC_SCAN) + 1);
  st->bad = ws.take<uint32_t>(1);
  st->gid = st->members = st->pos = st->ccur = nullptr;
  MMF_TRY(upload_table(s, st->d_ptr, ptr_host, (size_t)(n_seg + 1) * 8));
  MMF_HIP(hipMemsetAsync(st->cnt, 0, (size_t)n * 4, s));
  MMF_HIP(hipMemsetAsync(st->bad, 0, 4, s));
  if (!labels) return MMF_OK;
  st->gid = ws.take<int32_t>((size_t)n);
  st->members = ws.take<int32_t>((size_t)n);
  st->pos = ws.take<int32_t>((size_t)n);
  st->ccur = ws.take<int32_t>((size_t)(n_seg * H));
  MMF_HIP(hipMemsetAsync(st->ccur, 0, (size_t)(n_seg * H) * 4, s));
  hipLaunchKernelGGL(kc_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, labels, n, H, st->d_ptr, (int)n_seg, st->gid,
                     st->ccur, st->bad);
  MMF_LAUNCH_CHECK();
  int bits = 0;
  while ((int64_t(1) << bits) < H) ++bits;
  hipLaunchKernelGGL(kc_members_kernel, dim3((unsigned)((n_seg + 3) / 4)), dim3(256), 0, s, st->gid, st->d_ptr, (int)n_seg, H, bits,
                     st->ccur, st->members, st->pos);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
}  // namespace

int launch_knn_clique_count(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t H, const int64_t* ptr_host,
                            int64_t n_seg, unsigned long long* row_off, int64_t* edge_ptr, int64_t* out_count, void* scratch,
                            hipStream_t s) {
  KcState st;
  MMF_TRY(kc_prepare(labels, n, H, ptr_host, n_seg, static_cast<char*>(scratch), &st, s));
  const int64_t total = n * k, nb = (n + KC_SCAN - 1) / KC_SCAN;
  if (total > 0) {
    hipLaunchKernelGGL(kc_knn_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, nbr, n, k, st.gid, st.ccur, st.pos,
                       st.cnt, (const unsigned long long*)nullptr, (int64_t*)nullptr, (int64_t)0);
    MMF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kc_scan_local_kernel, dim3((unsigned)nb), dim3(KC_SCAN), 0, s, st.cnt, st.gid, st.ccur, st.pos, n, row_off, st.bsum);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(kc_scan_blocks_kernel, dim3(1), dim3(1024), 0, s, st.bsum, nb, n, row_off, st.bad, out_count);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(kc_scan_add_kernel, dim3((unsigned)nb), dim3(KC_SCAN), 0, s, st.bsum, n, row_off);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(kc_edge_ptr_kernel, dim3((unsigned)((n_seg + 256) / 256)), dim3(256), 0, s, row_off, st.d_ptr, (int)n_seg, edge_ptr);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int launch_knn_clique_fill(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t H, const int64_t* ptr_host,
                           int64_t n_seg, const unsigned long long* row_off, int64_t* edge_index, int64_t capacity, void* scratch,
                           hipStream_t s) {
  KcState st;
  MMF_TRY(kc_prepare(labels, n, H, ptr_host, n_seg, static_cast<char*>(scratch), &st, s));
  int64_t* lo = edge_index;
  int64_t* hi = edge_index + capacity;
  const int64_t total = n * k;
  if (total > 0) {
    hipLaunchKernelGGL(kc_knn_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, nbr, n, k, st.gid, st.ccur, st.pos,
                       st.cnt, row_off, hi, capacity);
    MMF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kc_merge_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, st.gid, st.ccur, st.pos, st.members, n, row_off, lo,
                     hi, capacity);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf
