// mmf_hgconv.hip — hypergraph propagation  out = D^-1 H W B^-1 H^T x  on the incidence edge_index [2, E] (DESIGN.md §4.35,
// include/ext/mmf_hg_hgconv.h).  The reference applies torch_geometric's HypergraphConv to every edge list this library builds
// (downstream_survival/models/cust_omics.py:58,101); underneath, that is two scatter-adds with float atomics.  Here both steps are
// gather-sums over a canonical CSR, so the bits depend neither on the order of the columns of edge_index nor on the run:
//
//   plan      keys e * N + v and v * M + e of every valid pair, one radix sort each (only the bits in use), then the offsets by a
//             bounds search on the sorted keys: eptr / emem (members of a hyperedge, node ids ascending), nptr / nmem (hyperedges of a
//             node, ids ascending), and the scales Binv_e = 1 / B_e, Dinv_v = 1 / D_v.  A pair with an id outside its range gets the
//             key N * M, sorts behind every valid pair and lies past the last offset: it is counted nowhere and addresses nothing.
//   gather    out[r, :] = (scale[r] *) (scale2[r] *) sum over j in [ptr[r], ptr[r + 1]) of src[col[j], :], the sum a sequential f32
//             chain in the order of the row (no fma: the build has -ffp-contract=off; no tree; no atomics).
//
// One group of L lanes owns one row, L the power of two that covers the row's float4 (or float) columns, at most 64: a wave per row
// when C is wide, 64 / L rows per wave when it is narrow.  The group fetches the row's ids L at a time with one load and hands
// them out with lane reads; the gathers of 8 members are issued before their adds, which stay in order — the order rule fixes the
// add chain, not the load order.  A row is never split.  Rows go to waves in row order, four waves to a workgroup: the hardware's
// workgroup dispatch is the dynamic row counter (DESIGN.md §4.35 "Hub rows").
#include <hipcub/hipcub.hpp>

#include "mmf_dev.h"
#include "mmf_host.h"
#include "mmf_hgshare.h"

namespace mmf {

constexpr int HG_BATCH = 8;            // members whose gathers are in flight before their adds

// ---- plan ---------------------------------------------------------------------------------------------------------------------------
// status [2] (memset to all ones before): lowest column with a bad node id, lowest column with a bad hyperedge id.
__global__ __launch_bounds__(256) void hg_keys_kernel(const int64_t* __restrict__ ei, int64_t E, int64_t N, int64_t M,
                                                      unsigned long long* __restrict__ k_edge, unsigned long long* __restrict__ k_node,
                                                      unsigned long long* __restrict__ status) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= E) return;
  const int64_t v = ei[j], e = ei[E + j];
  const bool bad_v = v < 0 || v >= N, bad_e = e < 0 || e >= M;
  if (bad_v) atomicMin(status + 0, (unsigned long long)j);
  if (bad_e) atomicMin(status + 1, (unsigned long long)j);
  const bool ok = !bad_v && !bad_e;                                  // checked before the pair is counted or used in a key
  const unsigned long long last = (unsigned long long)N * (unsigned long long)M;
  k_edge[j] = ok ? (unsigned long long)e * (unsigned long long)N + (unsigned long long)v : last;
  k_node[j] = ok ? (unsigned long long)v * (unsigned long long)M + (unsigned long long)e : last;
}

// sorted keys row * inner + member (then the keys `last` of the pairs left out) -> ptr [R + 1], mem [E].  Thread j looks at the
// boundary in front of position j (j = E: the end) and writes the offsets of the rows that begin there.
__global__ __launch_bounds__(256) void hg_csr_kernel(const unsigned long long* __restrict__ keys, int64_t E, unsigned long long last,
                                                     unsigned long long inner, int64_t R, int64_t* __restrict__ ptr,
                                                     int32_t* __restrict__ mem) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j > E) return;
  int64_t cur = R, prev = -1;
  if (j < E) {
    const unsigned long long k = keys[j];
    int32_t m = 0;
    if (k < last) { cur = (int64_t)(k / inner); m = (int32_t)(k - (unsigned long long)cur * inner); }
    mem[j] = m;
  }
  if (j > 0) {
    const unsigned long long k = keys[j - 1];
    prev = k < last ? (int64_t)(k / inner) : R;
  }
  for (int64_t r = prev + 1; r <= cur; ++r) ptr[r] = j;
}

// Binv_e = 1 / (float)B_e, 0 for an empty hyperedge; D_v = the f32 chain of w over the node's hyperedges in ascending order
// (without weights a chain of ones: the degree, which the chain cannot carry past 2^24), Dinv_v = 1 / D_v, 0 for D_v = 0.
__global__ __launch_bounds__(256) void hg_scales_kernel(const int64_t* __restrict__ eptr, int64_t M, const int64_t* __restrict__ nptr,
                                                        const int32_t* __restrict__ nmem, int64_t N, const float* __restrict__ w,
                                                        float* __restrict__ edge_scale, float* __restrict__ node_scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < M) {
    const int64_t b = eptr[i + 1] - eptr[i];
    edge_scale[i] = b > 0 ? 1.0f / (float)b : 0.0f;
  } else if (i < M + N) {
    const int64_t v = i - M, beg = nptr[v], end = nptr[v + 1];
    float d = 0.0f;
    if (w) {
      for (int64_t j = beg; j < end; ++j) d = d + w[nmem[j]];
    } else {
      const int64_t deg = end - beg;
      d = (float)(deg < ((int64_t)1 << 24) ? deg : ((int64_t)1 << 24));
    }
    node_scale[v] = d != 0.0f ? 1.0f / d : 0.0f;
  }
}

int hg_key_bits(int64_t N, int64_t M) {
  const unsigned long long last = (unsigned long long)N * (unsigned long long)M;
  int bits = 1;
  while (bits < 64 && (last >> bits) != 0) ++bits;
  return bits;
}

static size_t hg_sort_temp(int64_t E, int bits, hipStream_t s) {
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)E, 0, bits, s);
  return (tb + 255) & ~size_t(255);
}

// ---- gather-sum ---------------------------------------------------------------------------------------------------------------------
struct GatherSumArgs {
  const int64_t* ptr; const int32_t* col; int64_t rows;
  const float* src; int64_t src_stride; int C;
  const float* scale; const float* scale2;
  float* out; int64_t out_stride;
  int lg;                     // log2 of the lanes per row (FULL: 6)
};

// VEC = 4: C, both row pitches and both bases are multiples of four floats; VEC = 1: any C, any pitch.  FULL: one wave per row.
template <int VEC, bool FULL>
__global__ __launch_bounds__(256) void hg_gather_sum_kernel(GatherSumArgs a) {
  typedef HgVec<VEC> V;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lg = FULL ? 6 : a.lg;
  const int L = 1 << lg;
  const int sub = lane & (L - 1);
  const int64_t r = FULL ? wave : wave * (64 >> lg) + (lane >> lg);
  if (r >= a.rows) return;                               // a whole group leaves together: every lane read below is of a live lane
  const int64_t beg = a.ptr[r], end = a.ptr[r + 1];
  for (int c0 = 0; c0 < a.C; c0 += L * VEC) {           // one trip unless the row is wider than 64 lanes
    const int c = c0 + sub * VEC;
    const bool live = c < a.C;
    typename V::T acc = V::zero();
    for (int64_t j0 = beg; j0 < end; j0 += L) {
      const int cnt = end - j0 < (int64_t)L ? (int)(end - j0) : L;
      const int myid = sub < cnt ? a.col[j0 + sub] : 0;  // the next L ids of the row: one load
      for (int b = 0; b < cnt; b += HG_BATCH) {
        typename V::T v[HG_BATCH];
#pragma unroll
        for (int u = 0; u < HG_BATCH; ++u) {
          v[u] = V::zero();
          if (b + u < cnt) {                             // uniform over the group
            int id;
            if constexpr (FULL) id = __builtin_amdgcn_readlane(myid, __builtin_amdgcn_readfirstlane(b + u));
            else id = __shfl(myid, b + u, L);
            if (live) v[u] = V::load(a.src + (int64_t)id * a.src_stride + c);
          }
        }
        // the chain, in the row's order.  A slot past the row's end holds +0: acc starts at +0 and no sum of it is -0, so
        // acc + 0 leaves every bit of acc as it is
#pragma unroll
        for (int u = 0; u < HG_BATCH; ++u) acc = V::add(acc, v[u]);
      }
    }
    if (a.scale) acc = V::mul(acc, a.scale[r]);
    if (a.scale2) acc = V::mul(acc, a.scale2[r]);
    if (live) V::store(a.out + r * a.out_stride + c, acc);
  }
}

static int launch_gather_sum(const int64_t* ptr, const int32_t* col, int64_t rows, const float* src, int64_t src_stride, int64_t C,
                             const float* scale, const float* scale2, float* out, int64_t out_stride, hipStream_t s) {
  if (rows <= 0 || C <= 0) return MMF_OK;
  const bool vec = C % 4 == 0 && src_stride % 4 == 0 && out_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int64_t units = vec ? C / 4 : C;
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < units) ++lg;
  GatherSumArgs a{ptr, col, rows, src, src_stride, (int)C, scale, scale2, out, out_stride, lg};
  const int64_t per_wave = 64 >> lg, waves = (rows + per_wave - 1) / per_wave;
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  if (vec) {
    if (lg == 6) hipLaunchKernelGGL((hg_gather_sum_kernel<4, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((hg_gather_sum_kernel<4, false>), grid, block, 0, s, a);
  } else {
    if (lg == 6) hipLaunchKernelGGL((hg_gather_sum_kernel<1, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((hg_gather_sum_kernel<1, false>), grid, block, 0, s, a);
  }
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int hg_check_sizes(const char* who, int64_t N, int64_t M, int64_t E) {
  if (N < 0 || M < 0 || E < 0) {
    set_error("%s: num_nodes, num_edges and the pair count must be >= 0 (got %lld, %lld, %lld)", who, (long long)N, (long long)M, (long long)E);
    return MMF_E_INVALID;
  }
  if (N >= HG_LIMIT || M >= HG_LIMIT || E >= HG_LIMIT) {
    set_error("%s: num_nodes, num_edges and the pair count must be < 2^31 (got %lld, %lld, %lld)", who, (long long)N, (long long)M, (long long)E);
    return MMF_E_UNSUPPORTED;
  }
  return MMF_OK;
}

// the plan's steps as launches (mmf_hgshare.h): mmf_incidence_plan below and mmf_incidence_pair_plan (mmf_hgpair.hip) enqueue the same
int hg_launch_keys(const int64_t* edge_index, int64_t E, int64_t N, int64_t M, unsigned long long* k_edge, unsigned long long* k_node,
                   int64_t* status, hipStream_t s) {
  hipLaunchKernelGGL(hg_keys_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, edge_index, E, N, M, k_edge, k_node,
                     reinterpret_cast<unsigned long long*>(status));
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int hg_launch_csr(const unsigned long long* sorted, int64_t E, unsigned long long last, unsigned long long inner, int64_t R, int64_t* ptr,
                  int32_t* mem, hipStream_t s) {
  hipLaunchKernelGGL(hg_csr_kernel, dim3((unsigned)((E + 1 + 255) / 256)), dim3(256), 0, s, sorted, E, last, inner, R, ptr, mem);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int hg_launch_scales(const int64_t* eptr, int64_t M, const int64_t* nptr, const int32_t* nmem, int64_t N, const float* w, float* edge_scale,
                     float* node_scale, hipStream_t s) {
  hipLaunchKernelGGL(hg_scales_kernel, dim3((unsigned)((M + N + 255) / 256)), dim3(256), 0, s, eptr, M, nptr, nmem, N, w, edge_scale, node_scale);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_incidence_plan_bytes(int64_t num_nodes, int64_t num_edges, int64_t num_pairs, int64_t* bytes_out) {
  const char* who = "incidence_plan_bytes";
  MMF_TRY(hg_check_sizes(who, num_nodes, num_edges, num_pairs));
  if (!bytes_out) { set_error("%s: bytes_out is NULL", who); return MMF_E_INVALID; }
  bytes_out[0] = (num_edges + 1) * 8;      // eptr int64 [M + 1]
  bytes_out[1] = num_pairs * 4;            // emem int32 [E]
  bytes_out[2] = (num_nodes + 1) * 8;      // nptr int64 [N + 1]
  bytes_out[3] = num_pairs * 4;            // nmem int32 [E]
  bytes_out[4] = num_edges * 4;            // edge_scale f32 [M]
  bytes_out[5] = num_nodes * 4;            // node_scale f32 [N]
  return MMF_OK;
}

int mmf_incidence_plan(const int64_t* edge_index, int64_t num_pairs, int64_t num_nodes, int64_t num_edges, const float* hyperedge_weight,
                       int64_t* eptr, int32_t* emem, int64_t* nptr, int32_t* nmem, float* edge_scale, float* node_scale, int64_t* status,
                       int device_id, void* hip_stream) {
  Call c("incidence_plan", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, E = num_pairs;
  MMF_TRY(hg_check_sizes(c.who, N, M, E));
  if (!eptr || !nptr || !status || (E > 0 && (!edge_index || !emem || !nmem)) || (M > 0 && !edge_scale) || (N > 0 && !node_scale)) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  const int bits = hg_key_bits(N, M);
  const size_t temp = E > 0 ? hg_sort_temp(E, bits, s) : 0;
  MMF_TRY(c.workspace(3 * ws_bytes((size_t)E + 1, 8) + temp + 256, &c.ws));
  unsigned long long* k_edge = c.ws.take<unsigned long long>((size_t)E + 1);
  unsigned long long* k_node = c.ws.take<unsigned long long>((size_t)E + 1);
  unsigned long long* sorted = c.ws.take<unsigned long long>((size_t)E + 1);
  void* sort_tmp = c.ws.take<char>(temp + 1);
  MMF_HIP(hipMemsetAsync(status, 0xff, 16, s));
  const unsigned long long last = (unsigned long long)N * (unsigned long long)M;
  if (E > 0) {
    MMF_TRY(hg_launch_keys(edge_index, E, N, M, k_edge, k_node, status, s));
    size_t tb = temp;
    MMF_HIP(hipcub::DeviceRadixSort::SortKeys(sort_tmp, tb, k_edge, sorted, (int)E, 0, bits, s));
  }
  MMF_TRY(hg_launch_csr(sorted, E, last, (unsigned long long)N, M, eptr, emem, s));
  if (E > 0) {
    size_t tb = temp;
    MMF_HIP(hipcub::DeviceRadixSort::SortKeys(sort_tmp, tb, k_node, sorted, (int)E, 0, bits, s));
  }
  MMF_TRY(hg_launch_csr(sorted, E, last, (unsigned long long)M, N, nptr, nmem, s));
  if (M + N > 0) MMF_TRY(hg_launch_scales(eptr, M, nptr, nmem, N, hyperedge_weight, edge_scale, node_scale, s));
  return MMF_OK;
}

int mmf_csr_gather_sum(const int64_t* ptr, const int32_t* col, int64_t rows, const float* src, int64_t src_stride, int64_t channels,
                       const float* scale, const float* scale2, float* out, int64_t out_stride, int device_id, void* hip_stream) {
  Call c("csr_gather_sum", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (rows < 0 || channels < 0 || src_stride < channels || out_stride < channels) {
    set_error("%s: rows and channels must be >= 0 and both row pitches at least `channels` (got %lld, %lld, %lld, %lld)", c.who, (long long)rows,
              (long long)channels, (long long)src_stride, (long long)out_stride);
    return MMF_E_INVALID;
  }
  if (rows >= HG_LIMIT || channels >= HG_LIMIT) { set_error("%s: rows and channels must be < 2^31", c.who); return MMF_E_UNSUPPORTED; }
  if (rows > 0 && channels > 0 && (!ptr || !out)) { set_error("%s: NULL pointer", c.who); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  return launch_gather_sum(ptr, col, rows, src, src_stride, channels, scale, scale2, out, out_stride, c.s);
}

int mmf_hypergraph_propagate(const int64_t* eptr, const int32_t* emem, const int64_t* nptr, const int32_t* nmem, const float* edge_scale,
                             const float* node_scale, const float* hyperedge_weight, const float* x, int64_t x_stride, int64_t num_nodes,
                             int64_t num_edges, int64_t channels, float* Y, float* out, int transpose, int device_id, void* hip_stream) {
  Call c("hypergraph_propagate", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, C = channels;
  MMF_TRY(hg_check_sizes(c.who, N, M, 0));
  if (C < 0 || C >= HG_LIMIT || x_stride < C) {
    set_error("%s: channels must lie in [0, 2^31) and the row pitch of x be at least `channels` (got %lld, %lld)", c.who, (long long)C, (long long)x_stride);
    return MMF_E_INVALID;
  }
  if (!eptr || !nptr || (M > 0 && !edge_scale) || (N > 0 && !node_scale && !transpose) || (C > 0 && ((N > 0 && (!x || !out)) || (M > 0 && !Y)))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  // Y_e = (sum * Binv_e) * w_e over the hyperedge's nodes; out_v = sum * Dinv_v over the node's hyperedges (transpose: no scale —
  // the caller has multiplied x by Dinv, DESIGN.md §4.35 "Backward")
  MMF_TRY(launch_gather_sum(eptr, emem, M, x, x_stride, C, edge_scale, hyperedge_weight, Y, C, c.s));
  return launch_gather_sum(nptr, nmem, N, Y, C, C, transpose ? nullptr : node_scale, nullptr, out, C, c.s);
}

}  // extern "C"
