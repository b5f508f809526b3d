// mmf_pool.hip — super-patch aggregation over a cohort (include/mmf_hg_pool.h): what
// aggregate_wsi_super_patches does with one slide's KMeans labels (preprocess_hypergraph.py:157-197), for every slide of a
// ragged batch in a fixed number of launches and without a host synchronisation.
//
//   mmf_segment_sort_segmented    the stable counting sort of mmf_segments.hip, one histogram per (slide, chunk of 1024 labels),
//                                 prefix per (slide, label) over that slide's chunks, a multi-workgroup scan over all G counts
//   mmf_super_patches_segmented   seg_mean_kernel over all G clusters (launch_segment_mean), the row sums of seg_row_sums_kernel
//                                 with a per-slide row base, stats_partial_kernel's assignment of values to threads per block K_s
//                                 merged by stats_final_seg_kernel, the flat ragged median of mmf_edges.hip
//
// Integer, f32 and f64 work bound by HBM and gathers; every sum has the summation order of the plain kernel it restates, so every
// output carries the plain entry's bits.  No atomics on floats.
#include <algorithm>
#include <vector>

#include "../../include/mmf_hg_pool.h"
#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

constexpr int POOL_CHUNK = 1024;               // labels per single-wave workgroup (SEG_CHUNK of mmf_segments.hip)
constexpr int POOL_MAX_CLUSTERS = 16384;       // clusters per slide: the LDS histogram of one chunk is 64 KiB
constexpr int POOL_TILE = 2048;                // counts per workgroup of the offsets scan (256 threads x 8)
constexpr unsigned long long POOL_NONE = ~0ull;
enum { PCH_SEG = 0, PCH_ROW0 = 1, PCH_ROW1 = 2, PCH_ENTRY = 3 };      // chunk table: slide, first row, one past its last row

// ---- counting sort per slide ---------------------------------------------------------------------------------------
// workgroup = one chunk of one slide (no chunk straddles two slides); flags[0] = the lowest row with a label outside [0, C)
__global__ __launch_bounds__(64) void pool_count_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ tab, int C,
                                                        uint32_t* __restrict__ block_hist, unsigned long long* __restrict__ flags) {
  extern __shared__ uint32_t hist[];
  for (int l = threadIdx.x; l < C; l += 64) hist[l] = 0u;
  __syncthreads();
  const int64_t* e = tab + (size_t)blockIdx.x * PCH_ENTRY;
  const int64_t r0 = e[PCH_ROW0], r1 = e[PCH_ROW1];
  unsigned long long bad = POOL_NONE;
  for (int i = threadIdx.x; i < POOL_CHUNK; i += 64) {
    const int64_t r = r0 + i;
    if (r < r1) {
      const int64_t l = labels[r];
      if (l >= 0 && l < C) atomicAdd(&hist[(int)l], 1u);
      else if (bad == POOL_NONE) bad = (unsigned long long)r;          // rows ascend: the thread's first is its lowest
    }
  }
  if (bad != POOL_NONE) atomicMin(&flags[0], bad);
  __syncthreads();
  for (int l = threadIdx.x; l < C; l += 64) block_hist[(size_t)blockIdx.x * C + l] = hist[l];
}

// per (slide, label): exclusive prefix over the slide's chunks (in place), total -> counts[g].  One thread per g; neighbouring
// threads read neighbouring labels of the same chunk.
__global__ __launch_bounds__(256) void pool_chunk_scan_kernel(uint32_t* __restrict__ block_hist, const int64_t* __restrict__ cbase, int C,
                                                              int64_t G, int64_t* __restrict__ counts) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const int64_t sg = g / C, l = g - sg * C;
  uint32_t run = 0;
  for (int64_t b = cbase[sg]; b < cbase[sg + 1]; ++b) {
    const uint32_t c = block_hist[(size_t)b * C + l];
    block_hist[(size_t)b * C + l] = run;
    run += c;
  }
  counts[g] = (int64_t)run;
}

// offsets[0..G] = exclusive scan of counts, in three launches: tile sums (and flags[1] = the lowest empty g), the scan of the
// tile sums by one workgroup, the scan inside every tile
__global__ __launch_bounds__(256) void pool_tile_sum_kernel(const int64_t* __restrict__ counts, int64_t G, unsigned long long* __restrict__ tile_sum,
                                                            unsigned long long* __restrict__ flags) {
  __shared__ unsigned long long part[256];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * POOL_TILE + (int64_t)t * 8;
  unsigned long long sum = 0, empty = POOL_NONE;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int64_t i = i0 + u;
    if (i < G) {
      const int64_t c = counts[i];
      sum += (unsigned long long)c;
      if (c == 0 && empty == POOL_NONE) empty = (unsigned long long)i;
    }
  }
  if (empty != POOL_NONE) atomicMin(&flags[1], empty);
  part[t] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) part[t] += part[t + o];
    __syncthreads();
  }
  if (t == 0) tile_sum[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(1024) void pool_tile_scan_kernel(unsigned long long* __restrict__ tile_sum, int64_t ntiles, int64_t G,
                                                              int64_t* __restrict__ offsets) {
  __shared__ unsigned long long part[1024];
  const int t = threadIdx.x;
  const int64_t per = (ntiles + 1023) / 1024, b = (int64_t)t * per;
  int64_t e = b + per;
  if (e > ntiles) e = ntiles;
  unsigned long long sum = 0;
  for (int64_t i = b; i < e; ++i) sum += tile_sum[i];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long v = (t >= o) ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = part[t] - sum;
  for (int64_t i = b; i < e; ++i) { const unsigned long long c = tile_sum[i]; tile_sum[i] = run; run += c; }
  if (t == 1023) offsets[G] = (int64_t)part[1023];
}

__global__ __launch_bounds__(256) void pool_offsets_kernel(const int64_t* __restrict__ counts, int64_t G, const unsigned long long* __restrict__ tile_off,
                                                           int64_t* __restrict__ offsets) {
  __shared__ unsigned long long part[256];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * POOL_TILE + (int64_t)t * 8;
  unsigned long long c[8], sum = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) { c[u] = (i0 + u < G) ? (unsigned long long)counts[i0 + u] : 0ull; sum += c[u]; }
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned long long v = (t >= o) ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = tile_off[blockIdx.x] + part[t] - sum;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    if (i0 + u < G) offsets[i0 + u] = (int64_t)run;
    run += c[u];
  }
}

// seg_scatter_kernel (mmf_segments.hip) on one chunk of one slide: the lanes that share a label find each other with one
// ballot per label bit; the cursor of a label starts at the chunk's prefix inside its slide
__global__ __launch_bounds__(64) void pool_scatter_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ tab, int C, int bits,
                                                          const uint32_t* __restrict__ block_hist, const int64_t* __restrict__ offsets,
                                                          int64_t* __restrict__ order) {
  extern __shared__ uint32_t cursor[];
  for (int l = threadIdx.x; l < C; l += 64) cursor[l] = block_hist[(size_t)blockIdx.x * C + l];
  __syncthreads();
  const int64_t* e = tab + (size_t)blockIdx.x * PCH_ENTRY;
  const int64_t g0 = e[PCH_SEG] * C, r0 = e[PCH_ROW0], r1 = e[PCH_ROW1];
  const int lane = threadIdx.x;
  for (int i0 = 0; i0 < POOL_CHUNK; i0 += 64) {
    if (r0 + i0 >= r1) break;                      // uniform: the chunk's rows are used up
    const int64_t r = r0 + i0 + lane;
    int l = -1;
    if (r < r1) {
      const int64_t ll = labels[r];
      if (ll >= 0 && ll < C) l = (int)ll;
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
      order[offsets[g0 + l] + (int64_t)(cur + rank)] = r;
      if (rank == 0) cursor[l] = cur + (uint32_t)__popcll(match);
    }
    __syncthreads();
  }
}

__global__ void pool_status_kernel(const unsigned long long* __restrict__ flags, int64_t* __restrict__ status) {
  if (threadIdx.x < 2) status[threadIdx.x] = (flags[threadIdx.x] == POOL_NONE) ? (int64_t)-1 : (int64_t)flags[threadIdx.x];
}

// ---- mean off-diagonal similarity inside every cluster of every slide -----------------------------------------------
__global__ __launch_bounds__(64) void pool_seg_of_kernel(const int64_t* __restrict__ offsets, int32_t* __restrict__ seg_of) {
  const int64_t c = blockIdx.x;
  for (int64_t q = offsets[c] + threadIdx.x; q < offsets[c + 1]; q += 64) seg_of[q] = (int32_t)c;
}

// the body of seg_row_sums_kernel: one wave per member, lane-strided f64 sum, the same butterfly; the row of member q lies in
// its slide's block, and the columns are the members' rows inside the slide
__global__ __launch_bounds__(256) void pool_row_sums_kernel(const float* __restrict__ K, const int64_t* __restrict__ ptr,
                                                            const int64_t* __restrict__ kptr, int C, const int64_t* __restrict__ order,
                                                            const int64_t* __restrict__ offsets, const int32_t* __restrict__ seg_of,
                                                            int64_t total, double* __restrict__ row_sum) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= total) return;
  const int c = seg_of[q];
  if (c < 0) return;                               // a position behind the last member (rows with a bad label were skipped)
  const int64_t sg = c / C, p0 = ptr[sg], ns = ptr[sg + 1] - p0;
  const int64_t b = offsets[c], e = offsets[c + 1];
  const float* row = K + kptr[sg] + (order[q] - p0) * ns;
  double acc = 0.0;
  for (int64_t p = b + lane; p < e; p += 64)
    if (p != q) acc += (double)row[order[p] - p0];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) row_sum[q] = acc;
}

__global__ __launch_bounds__(256) void pool_offdiag_final_kernel(const double* __restrict__ row_sum, const int64_t* __restrict__ offsets, int64_t G,
                                                                 double* __restrict__ out_mean) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= G) return;
  const int64_t b = offsets[c], e = offsets[c + 1], m = e - b;
  if (m <= 1) { out_mean[c] = __builtin_nan(""); return; }
  double sum = 0.0;
  for (int64_t q = b; q < e; ++q) sum += row_sum[q];
  out_mean[c] = sum / ((double)m * (double)(m - 1));
}

// ---- statistic partials of every block K_s -------------------------------------------------------------------------
struct StatPartial { double s1, s2; float mn, mx; };     // same layout as in mmf_edges.hip

// stats_partial_kernel (mmf_edges.hip) on block sg with the grid the plain entry gives it: workgroup j of nb = pbase[sg+1] -
// pbase[sg]; thread tid of nb * 256 takes the groups of four values tid, tid + nth, ... and then the tail, around the pivot
// K_s[0].  The plain entry sees an aligned allocation and loads a group as one float4; a block that starts at an odd element is
// not aligned, and its groups are loaded value by value: the same values in the same order.
__global__ __launch_bounds__(256) void pool_stats_partial_kernel(const float* __restrict__ K, const int64_t* __restrict__ ptr,
                                                                 const int64_t* __restrict__ kptr, const int64_t* __restrict__ pbase, int64_t S,
                                                                 StatPartial* __restrict__ part, float* __restrict__ pivot) {
  int64_t lo = 0, hi = S - 1;                      // the slide sg with pbase[sg] <= blockIdx.x < pbase[sg+1]
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (pbase[mid + 1] > (int64_t)blockIdx.x) hi = mid; else lo = mid + 1;
  }
  const int64_t sg = lo, ns = ptr[sg + 1] - ptr[sg], count = ns * ns;
  const float* v = K + kptr[sg];
  const int64_t j = (int64_t)blockIdx.x - pbase[sg], nb = pbase[sg + 1] - pbase[sg];
  const double p = (double)v[0];
  double s1 = 0.0, s2 = 0.0;
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
  auto feed = [&](float x) {
    const double dx = (double)x - p;
    s1 += dx; s2 = __builtin_fma(dx, dx, s2);
    mn = fminf(mn, x); mx = fmaxf(mx, x);
  };
  const int64_t tid = j * 256 + threadIdx.x, nth = nb * 256;
  const int64_t n4 = count >> 2;
  if ((reinterpret_cast<uintptr_t>(v) & 15) == 0) {
    for (int64_t i = tid; i < n4; i += nth) {
      const f32x4 x = reinterpret_cast<const f32x4*>(v)[i];
      feed(x[0]); feed(x[1]); feed(x[2]); feed(x[3]);
    }
  } else {
    for (int64_t i = tid; i < n4; i += nth) {
      const float x0 = v[4 * i], x1 = v[4 * i + 1], x2 = v[4 * i + 2], x3 = v[4 * i + 3];
      feed(x0); feed(x1); feed(x2); feed(x3);
    }
  }
  for (int64_t i = n4 * 4 + tid; i < count; i += nth) feed(v[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s1 += __shfl_xor(s1, o);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  __shared__ StatPartial w[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) w[wave] = StatPartial{s1, s2, mn, mx};
  __syncthreads();
  if (threadIdx.x == 0) {
    StatPartial r = w[0];
    for (int i = 1; i < 4; ++i) { r.s1 += w[i].s1; r.s2 += w[i].s2; r.mn = fminf(r.mn, w[i].mn); r.mx = fmaxf(r.mx, w[i].mx); }
    part[blockIdx.x] = r;
    if (j == 0) pivot[sg] = v[0];
  }
}

// a slide without partials (its block goes through launch_array_stats) still has a pivot for the merge kernel to read
__global__ __launch_bounds__(256) void pool_pivot_fill_kernel(float* __restrict__ a, float* __restrict__ b, int64_t S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < S) { a[i] = 0.f; b[i] = 0.f; }
}

static constexpr int64_t kOneSweepMin = (int64_t)1 << 22;      // values from which mmf_array_stats takes its partials from the median's sweep

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_segment_sort_segmented(const int64_t* labels, int64_t n, const int64_t* ptr_host, int64_t n_seg, int64_t n_clusters,
                               int64_t* counts, int64_t* offsets, int64_t* order, int64_t* status, int device_id, void* hip_stream) {
  Call c("segment_sort_segmented", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 0 || n_clusters < 1) { set_error("%s: bad n / n_clusters", c.who); return MMF_E_INVALID; }
  MMF_TRY(check_offsets(c.who, "ptr", ptr_host, n_seg, 1, 0, n));
  if (n_clusters > POOL_MAX_CLUSTERS) {
    set_error("%s: at most %d clusters per segment are supported (got %lld)", c.who, POOL_MAX_CLUSTERS, (long long)n_clusters);
    return MMF_E_UNSUPPORTED;
  }
  if (n >= ((int64_t)1 << 31) || n_seg >= ((int64_t)1 << 31) || n_seg * n_clusters >= ((int64_t)1 << 31)) {
    set_error("%s: n and n_seg * n_clusters must be < 2^31", c.who);
    return MMF_E_UNSUPPORTED;
  }
  if (!counts || !offsets || !status || (n > 0 && (!labels || !order))) { set_error("%s: NULL pointer", c.who); return MMF_E_INVALID; }
  const int64_t G = n_seg * n_clusters, C = n_clusters;
  std::vector<int64_t> tab, cbase((size_t)n_seg + 1, 0);
  for (int64_t sg = 0; sg < n_seg; ++sg) {
    for (int64_t r = ptr_host[sg]; r < ptr_host[sg + 1]; r += POOL_CHUNK) {
      const int64_t ent[PCH_ENTRY] = {sg, r, r + POOL_CHUNK < ptr_host[sg + 1] ? r + POOL_CHUNK : ptr_host[sg + 1]};
      tab.insert(tab.end(), ent, ent + PCH_ENTRY);
    }
    cbase[sg + 1] = (int64_t)tab.size() / PCH_ENTRY;
  }
  const int64_t nchunks = cbase[n_seg], ntiles = (G + POOL_TILE - 1) / POOL_TILE;
  if (nchunks >= ((int64_t)1 << 31)) { set_error("%s: %lld workgroups", c.who, (long long)nchunks); return MMF_E_UNSUPPORTED; }
  MMF_TRY(c.begin(ws_bytes(tab.size() + 1, 8) + ws_bytes((size_t)n_seg + 1, 8) + ws_bytes((size_t)nchunks * (size_t)C + 1, 4) +
                  ws_bytes((size_t)ntiles, 8) + ws_bytes(2, 8)));
  const hipStream_t s = c.s;
  int64_t* d_tab = c.ws.take<int64_t>(tab.size() + 1);
  int64_t* d_cbase = c.ws.take<int64_t>((size_t)n_seg + 1);
  uint32_t* block_hist = c.ws.take<uint32_t>((size_t)nchunks * (size_t)C + 1);
  unsigned long long* tile_sum = c.ws.take<unsigned long long>((size_t)ntiles);
  unsigned long long* flags = c.ws.take<unsigned long long>(2);
  MMF_TRY(upload_table(s, d_tab, tab.data(), tab.size() * 8));
  MMF_TRY(upload_table(s, d_cbase, cbase.data(), cbase.size() * 8));
  MMF_HIP(hipMemsetAsync(flags, 0xff, 16, s));
  const size_t lds = (size_t)C * 4;
  if (nchunks > 0) {
    MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pool_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pool_count_kernel, dim3((unsigned)nchunks), dim3(64), lds, s, labels, d_tab, (int)C, block_hist, flags);
    MMF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pool_chunk_scan_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, block_hist, d_cbase, (int)C, G, counts);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_tile_sum_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, counts, G, tile_sum, flags);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_tile_scan_kernel, dim3(1), dim3(1024), 0, s, tile_sum, ntiles, G, offsets);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_offsets_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, counts, G, tile_sum, offsets);
  MMF_LAUNCH_CHECK();
  if (nchunks > 0) {
    int bits = 0;
    while ((int64_t(1) << bits) < C) ++bits;
    MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pool_scatter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pool_scatter_kernel, dim3((unsigned)nchunks), dim3(64), lds, s, labels, d_tab, (int)C, bits, block_hist, offsets, order);
    MMF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pool_status_kernel, dim3(1), dim3(64), 0, s, flags, status);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int mmf_super_patches_segmented(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, const int64_t* ptr_host,
                                int64_t n_seg, int64_t n_clusters, const int64_t* order, const int64_t* offsets,
                                const float* K_flat, float* super_f, float* super_p, double* intra_mean, double* k_stats,
                                int device_id, void* hip_stream) {
  Call c("super_patches_segmented", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 0 || d < 1 || dp < 1 || n_clusters < 1) { set_error("%s: bad n / d / dp / n_clusters", c.who); return MMF_E_INVALID; }
  MMF_TRY(check_offsets(c.who, "ptr", ptr_host, n_seg, 1, K_flat ? 1 : 0, n));
  if (n >= ((int64_t)1 << 31) || n_seg >= ((int64_t)1 << 31) || n_seg * n_clusters >= ((int64_t)1 << 31)) {
    set_error("%s: n and n_seg * n_clusters must be < 2^31", c.who);
    return MMF_E_UNSUPPORTED;
  }
  if ((d + 63) / 64 > 65535 || (dp + 63) / 64 > 65535) { set_error("%s: d and dp must be < 2^22", c.who); return MMF_E_UNSUPPORTED; }
  if (!order || !offsets || !super_f || !super_p || (n > 0 && (!F || !P)) || (K_flat && (!intra_mean || !k_stats))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  const int64_t G = n_seg * n_clusters, C = n_clusters;
  const size_t S1 = (size_t)n_seg + 1;
  if (!K_flat) {
    MMF_TRY(c.begin());
    MMF_TRY(launch_segment_mean(F, d, order, offsets, G, super_f, c.s));
    return launch_segment_mean(P, dp, order, offsets, G, super_p, c.s);
  }
  // the blocks: their offsets, the statistic workgroups of the small ones, the runs of small ones for the flat median and the
  // scratch of the large ones
  std::vector<int64_t> kptr(S1, 0), pbase(S1, 0);
  size_t med_need = 0, big_need = 0, copy_need = 0;
  auto aligned = [&](int64_t sg) { return (reinterpret_cast<uintptr_t>(K_flat + kptr[sg]) & 15) == 0; };
  for (int64_t sg = 0, run0 = 0; sg < n_seg; ++sg) {
    const int64_t ns = ptr_host[sg + 1] - ptr_host[sg], count = ns * ns;
    kptr[sg + 1] = kptr[sg] + count;
    const bool small = count < kOneSweepMin;
    pbase[sg + 1] = pbase[sg] + (small ? (count + 4095) / 4096 : 0);
    if (!small) big_need = std::max(big_need, array_stats_scratch_bytes(count));
    if (!small && !aligned(sg)) copy_need = std::max(copy_need, (size_t)count * 4);
    if (!small || sg + 1 == n_seg) {               // a run of small blocks [run0, e) ends here
      const int64_t e = small ? sg + 1 : sg;
      if (e > run0) {
        std::vector<int64_t> bptr((size_t)(e - run0) + 1);
        for (int64_t i = run0; i <= e; ++i) bptr[(size_t)(i - run0)] = kptr[i] - kptr[run0];
        med_need = std::max(med_need, lower_median_seg_scratch_bytes(bptr.data(), e - run0));
      }
      run0 = sg + 1;
    }
  }
  const int64_t nparts = pbase[n_seg];
  if (nparts >= ((int64_t)1 << 31)) { set_error("%s: %lld workgroups", c.who, (long long)nparts); return MMF_E_UNSUPPORTED; }
  MMF_TRY(c.begin(3 * ws_bytes(S1, 8) + ws_bytes((size_t)n, 4) + ws_bytes((size_t)n, 8) + ws_bytes((size_t)nparts * sizeof(StatPartial) + 1, 1) +
                  2 * ws_bytes((size_t)n_seg, 4) + ws_bytes(med_need + 1, 1) + ws_bytes(big_need + 1, 1) + ws_bytes(copy_need + 1, 1)));
  const hipStream_t s = c.s;
  int64_t* d_ptr = c.ws.take<int64_t>(S1);
  int64_t* d_kptr = c.ws.take<int64_t>(S1);
  int64_t* d_pbase = c.ws.take<int64_t>(S1);
  int32_t* seg_of = c.ws.take<int32_t>((size_t)n);
  double* row_sum = c.ws.take<double>((size_t)n);
  StatPartial* part = reinterpret_cast<StatPartial*>(c.ws.take<char>((size_t)nparts * sizeof(StatPartial) + 1));
  float* pivot = c.ws.take<float>((size_t)n_seg);
  float* med = c.ws.take<float>((size_t)n_seg);
  char* med_scratch = c.ws.take<char>(med_need + 1);
  char* big_scratch = c.ws.take<char>(big_need + 1);
  float* big_copy = reinterpret_cast<float*>(c.ws.take<char>(copy_need + 1));
  MMF_TRY(upload_table(s, d_ptr, ptr_host, S1 * 8));
  MMF_TRY(upload_table(s, d_kptr, kptr.data(), S1 * 8));
  MMF_TRY(upload_table(s, d_pbase, pbase.data(), S1 * 8));
  // pooled features and positions: seg_mean_kernel over all G clusters
  MMF_TRY(launch_segment_mean(F, d, order, offsets, G, super_f, s));
  MMF_TRY(launch_segment_mean(P, dp, order, offsets, G, super_p, s));
  // mean off-diagonal similarity inside every cluster
  MMF_HIP(hipMemsetAsync(seg_of, 0xff, (size_t)n * 4, s));
  hipLaunchKernelGGL(pool_seg_of_kernel, dim3((unsigned)G), dim3(64), 0, s, offsets, seg_of);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_row_sums_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, K_flat, d_ptr, d_kptr, (int)C, order, offsets, seg_of, n,
                     row_sum);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_offdiag_final_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, row_sum, offsets, G, intra_mean);
  MMF_LAUNCH_CHECK();
  // the five statistics of every block: partials and merge of the small blocks, their medians run by run ...
  hipLaunchKernelGGL(pool_pivot_fill_kernel, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, s, pivot, med, n_seg);
  MMF_LAUNCH_CHECK();
  if (nparts > 0) {
    hipLaunchKernelGGL(pool_stats_partial_kernel, dim3((unsigned)nparts), dim3(256), 0, s, K_flat, d_ptr, d_kptr, d_pbase, n_seg, part, pivot);
    MMF_LAUNCH_CHECK();
  }
  MMF_TRY(launch_stats_finish_seg(part, d_pbase, pivot, d_ptr, d_ptr, n_seg, k_stats, s));
  for (int64_t sg = 0, run0 = 0; sg < n_seg; ++sg) {
    const int64_t ns = ptr_host[sg + 1] - ptr_host[sg];
    const bool small = ns * ns < kOneSweepMin;
    if (!small || sg + 1 == n_seg) {
      const int64_t e = small ? sg + 1 : sg;
      if (e > run0) {
        std::vector<int64_t> bptr((size_t)(e - run0) + 1);
        for (int64_t i = run0; i <= e; ++i) bptr[(size_t)(i - run0)] = kptr[i] - kptr[run0];
        MMF_TRY(launch_lower_median_seg(K_flat + kptr[run0], bptr.data(), e - run0, med + run0, med_scratch, s));
      }
      run0 = sg + 1;
    }
  }
  MMF_TRY(launch_stats_set_median_seg(med, n_seg, k_stats, s));
  // ... and the large blocks one by one through the plain entry's own path (its partials come out of the median's one sweep).
  // That sweep hands values to lanes by the block's alignment, and the plain call sees an aligned allocation: a block that
  // starts off a 16-byte boundary is swept from an aligned copy (one more pass over a block of 16 MiB or more).
  for (int64_t sg = 0; sg < n_seg; ++sg) {
    const int64_t ns = ptr_host[sg + 1] - ptr_host[sg], count = ns * ns;
    if (count < kOneSweepMin) continue;
    const float* v = K_flat + kptr[sg];
    if (!aligned(sg)) {
      MMF_HIP(hipMemcpyAsync(big_copy, v, (size_t)count * 4, hipMemcpyDeviceToDevice, s));
      v = big_copy;
    }
    MMF_TRY(launch_array_stats(v, count, k_stats + 5 * sg, big_scratch, s));
  }
  return MMF_OK;
}

}  // extern "C"
