// mmf_hgpair.hip — hypergraph propagation with one weight per (node, hyperedge) pair and the softmax over the pairs of a row
// (include/ext/mmf_hg_hgpair.h): the operator underneath torch_geometric's HypergraphConv(use_attention=True), and
// what lets a layer use the edge_weights [E] that every builder of this library returns next to edge_index.
//
//   pair plan   mmf_incidence_plan's keys, offsets and scales (the launches of mmf_hgconv.hip), the two radix sorts as SortPairs
//               with the column number as the value: epos / npos name, for every CSR slot, the column of edge_index it came from.
//               The sort is stable: the copies of a repeated pair sit in ascending column order.
//   gather      hg_gather_sum_kernel with one more operand per member: the group loads the L positions next to the L ids, gathers
//               the L weights a[pos], and hands both out with lane reads; the gathers of 8 members are issued before their
//               multiply-adds, which stay in the row's order.  acc = acc + (a * x): two rounded operations, no fma.
//   scales      one thread per row: the chains of a (and a * w) that the "weight" normalisation divides by
//   grad_a      one wave per hyperedge, L lanes per slot: the two dot64 of the header, scattered through epos
//   softmax     one wave per row: the maximum as an integer key (a lane reduction: exact, order-free), e = cexp(score - max)
//               lanewise for 64 slots at a time, Z the chain of e handed out by lane reads in slot order, then the divide; the
//               backward is the same walk with the chain of alpha * g
//
// No fma (the build has -ffp-contract=off), no atomics at all, no runtime exponential.
#include <hipcub/hipcub.hpp>

#include "mmf_dev.h"
#include "mmf_host.h"
#include "mmf_hgshare.h"

namespace mmf {

constexpr int HP_BATCH = 8;            // members whose gathers are in flight before their multiply-adds

// ---- pair plan ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hp_iota_kernel(int32_t* __restrict__ cols, int64_t E) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < E) cols[j] = (int32_t)j;
}

// the sorted values behind the last valid key are the columns of the pairs left out: those slots hold 0
__global__ __launch_bounds__(256) void hp_pos_tail_kernel(const unsigned long long* __restrict__ sorted, int64_t E, unsigned long long last,
                                                          int32_t* __restrict__ pos) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < E && sorted[j] >= last) pos[j] = 0;
}

static size_t hp_sort_temp(int64_t E, int bits, hipStream_t s) {
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const int32_t*)nullptr,
                                           (int32_t*)nullptr, (int)E, 0, bits, s);
  return (tb + 255) & ~size_t(255);
}

// ---- scales of the "weight" normalisation ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hp_scales_kernel(const int64_t* __restrict__ eptr, const int32_t* __restrict__ epos, int64_t M,
                                                        const int64_t* __restrict__ nptr, const int32_t* __restrict__ nmem,
                                                        const int32_t* __restrict__ npos, int64_t N, const float* __restrict__ a,
                                                        const float* __restrict__ w, float* __restrict__ edge_scale,
                                                        float* __restrict__ node_scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < M) {
    float b = 0.0f;
    for (int64_t j = eptr[i]; j < eptr[i + 1]; ++j) b = b + a[epos[j]];
    edge_scale[i] = b != 0.0f ? 1.0f / b : 0.0f;
  } else if (i < M + N) {
    const int64_t v = i - M, beg = nptr[v], end = nptr[v + 1];
    float d = 0.0f;
    if (w) {
      for (int64_t j = beg; j < end; ++j) d = d + a[npos[j]] * w[nmem[j]];
    } else {
      for (int64_t j = beg; j < end; ++j) d = d + a[npos[j]];
    }
    node_scale[v] = d != 0.0f ? 1.0f / d : 0.0f;
  }
}

// ---- weighted gather-sum ------------------------------------------------------------------------------------------------------------
struct PairGatherArgs {
  const int64_t* ptr; const int32_t* col; const int32_t* pos; const float* a; int64_t rows;
  const float* src; int64_t src_stride; int C;
  const float* scale; const float* scale2;
  float* out; int64_t out_stride;
  int lg;                     // log2 of the lanes per row (FULL: 6)
};

// VEC = 4: C, both row pitches and both bases are multiples of four floats; VEC = 1: any C, any pitch.  FULL: one wave per row.
template <int VEC, bool FULL>
__global__ __launch_bounds__(256) void hp_gather_sum_kernel(PairGatherArgs a) {
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
      int myid = 0;
      float myw = 0.f;
      if (sub < cnt) {                                   // the next L ids and positions of the row: one load each, then the L weights
        myid = a.col[j0 + sub];
        myw = a.a[a.pos[j0 + sub]];
      }
      for (int b = 0; b < cnt; b += HP_BATCH) {
        typename V::T v[HP_BATCH];
        float wv[HP_BATCH];
#pragma unroll
        for (int u = 0; u < HP_BATCH; ++u) {
          v[u] = V::zero();
          wv[u] = 0.f;
          if (b + u < cnt) {                             // uniform over the group
            int id;
            if constexpr (FULL) {
              const int from = __builtin_amdgcn_readfirstlane(b + u);
              id = __builtin_amdgcn_readlane(myid, from);
              wv[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myw), from));
            } else {
              id = __shfl(myid, b + u, L);
              wv[u] = __shfl(myw, b + u, L);
            }
            if (live) v[u] = V::load(a.src + (int64_t)id * a.src_stride + c);
          }
        }
        // the chain, in the row's order.  A slot past the row's end holds the weight +0 and the row +0: acc starts at +0 and no
        // sum of it is -0, so acc + (+0 * +0) leaves every bit of acc as it is
#pragma unroll
        for (int u = 0; u < HP_BATCH; ++u) acc = V::add(acc, V::mul(v[u], wv[u]));
      }
    }
    if (a.scale) acc = V::mul(acc, a.scale[r]);
    if (a.scale2) acc = V::mul(acc, a.scale2[r]);
    if (live) V::store(a.out + r * a.out_stride + c, acc);
  }
}

static int launch_pair_gather(const int64_t* ptr, const int32_t* col, const int32_t* pos, const float* w, int64_t rows, const float* src,
                              int64_t src_stride, int64_t C, const float* scale, const float* scale2, float* out, int64_t out_stride,
                              hipStream_t s) {
  if (rows <= 0 || C <= 0) return MMF_OK;
  const bool vec = C % 4 == 0 && src_stride % 4 == 0 && out_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int64_t units = vec ? C / 4 : C;
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < units) ++lg;
  PairGatherArgs a{ptr, col, pos, w, rows, src, src_stride, (int)C, scale, scale2, out, out_stride, lg};
  const int64_t per_wave = 64 >> lg, waves = (rows + per_wave - 1) / per_wave;
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  if (vec) {
    if (lg == 6) hipLaunchKernelGGL((hp_gather_sum_kernel<4, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((hp_gather_sum_kernel<4, false>), grid, block, 0, s, a);
  } else {
    if (lg == 6) hipLaunchKernelGGL((hp_gather_sum_kernel<1, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((hp_gather_sum_kernel<1, false>), grid, block, 0, s, a);
  }
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// ---- grad_a -------------------------------------------------------------------------------------------------------------------------
// One wave per hyperedge; L = 2^lg lanes per slot (the power of two that covers C, at most 64), 64 / L slots side by side.  Lane l of
// a slot's group takes the columns l, l + 64, ...: dot64's lane partials (L < 64 only when C <= L).
__global__ __launch_bounds__(256) void hp_weight_grad_kernel(const int64_t* __restrict__ eptr, const int32_t* __restrict__ emem,
                                                             const int32_t* __restrict__ epos, const float* __restrict__ gp,
                                                             const float* __restrict__ x, int64_t x_stride, const float* __restrict__ Y,
                                                             const float* __restrict__ T, int64_t M, int C, float* __restrict__ grad_a, int lg) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= M) return;                                    // uniform over the wave
  const int L = 1 << lg, sub = lane & (L - 1), rsub = lane >> lg, R = 64 >> lg;
  const int64_t beg = eptr[e], end = eptr[e + 1];
  const float* Ye = Y + e * C;
  const float* Te = T + e * C;
  for (int64_t j0 = beg; j0 < end; j0 += R) {            // uniform: every lane takes part in the trees below
    const int64_t j = j0 + rsub;
    const bool ok = j < end;
    const int64_t v = ok ? emem[j] : 0;
    float p1 = 0.f, p2 = 0.f;
    if (ok) {
      const float* gv = gp + v * C;
      const float* xv = x + v * x_stride;
      for (int c = sub; c < C; c += 64) {
        p1 = p1 + gv[c] * Ye[c];
        p2 = p2 + xv[c] * Te[c];
      }
    }
    const float d1 = ro_tree(p1, L), d2 = ro_tree(p2, L);
    if (ok && sub == 0) grad_a[epos[j]] = d1 + d2;
  }
}

// ---- softmax over the slots of a row ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hp_softmax_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ pos, int64_t rows,
                                                         const float* __restrict__ score, float* __restrict__ alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                 // uniform over the wave
  const int64_t beg = ptr[r], end = ptr[r + 1];
  if (beg >= end) return;
  uint32_t key = 0u;                                     // below the key of every float
  for (int64_t j = beg + lane; j < end; j += 64) {
    const uint32_t k = ro_key(score[pos[j]]);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)key, h, 64);
    key = other > key ? other : key;
  }
  const float m = ro_unkey(key);
  float z = 0.f;
  for (int64_t j0 = beg; j0 < end; j0 += 64) {
    const int cnt = end - j0 < 64 ? (int)(end - j0) : 64;
    float ev = 0.f;
    if (lane < cnt) {
      const int32_t p = pos[j0 + lane];
      ev = ro_cexp(score[p] - m);
      alpha[p] = ev;                                     // parked; the same lane divides it below
    }
    for (int u = 0; u < cnt; ++u)                        // the chain, in slot order
      z = z + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ev), __builtin_amdgcn_readfirstlane(u)));
  }
  for (int64_t j = beg + lane; j < end; j += 64) {
    const int32_t p = pos[j];
    alpha[p] = alpha[p] / z;
  }
}

__global__ __launch_bounds__(256) void hp_softmax_backward_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ pos, int64_t rows,
                                                                  const float* __restrict__ alpha, const float* __restrict__ g,
                                                                  float* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t beg = ptr[r], end = ptr[r + 1];
  float c = 0.f;
  for (int64_t j0 = beg; j0 < end; j0 += 64) {
    const int cnt = end - j0 < 64 ? (int)(end - j0) : 64;
    float t = 0.f;
    if (lane < cnt) {
      const int32_t p = pos[j0 + lane];
      t = alpha[p] * g[p];
    }
    for (int u = 0; u < cnt; ++u)
      c = c + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), __builtin_amdgcn_readfirstlane(u)));
  }
  for (int64_t j = beg + lane; j < end; j += 64) {
    const int32_t p = pos[j];
    grad[p] = alpha[p] * (g[p] - c);
  }
}

static int hp_check_rows(const char* who, int64_t rows, int64_t E) {
  if (rows < 0 || E < 0) {
    set_error("%s: the row count and the pair count must be >= 0 (got %lld, %lld)", who, (long long)rows, (long long)E);
    return MMF_E_INVALID;
  }
  if (rows >= HG_LIMIT || E >= HG_LIMIT) {
    set_error("%s: the row count and the pair count must be < 2^31 (got %lld, %lld)", who, (long long)rows, (long long)E);
    return MMF_E_UNSUPPORTED;
  }
  return MMF_OK;
}

static int hp_check_channels(const char* who, int64_t C, int64_t x_stride) {
  if (C < 0 || x_stride < C) {
    set_error("%s: channels must be >= 0 and the row pitch of x at least `channels` (got %lld, %lld)", who, (long long)C, (long long)x_stride);
    return MMF_E_INVALID;
  }
  if (C >= HG_LIMIT) { set_error("%s: channels must be < 2^31 (got %lld)", who, (long long)C); return MMF_E_UNSUPPORTED; }
  return MMF_OK;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_incidence_pair_plan(const int64_t* edge_index, int64_t num_pairs, int64_t num_nodes, int64_t num_edges, const float* hyperedge_weight,
                            int64_t* eptr, int32_t* emem, int32_t* epos, int64_t* nptr, int32_t* nmem, int32_t* npos, float* edge_scale,
                            float* node_scale, int64_t* status, int device_id, void* hip_stream) {
  Call c("incidence_pair_plan", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, E = num_pairs;
  MMF_TRY(hg_check_sizes(c.who, N, M, E));
  if (!eptr || !nptr || !status || (E > 0 && (!edge_index || !emem || !nmem || !epos || !npos)) || (M > 0 && !edge_scale) ||
      (N > 0 && !node_scale)) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  const int bits = hg_key_bits(N, M);
  const size_t temp = E > 0 ? hp_sort_temp(E, bits, s) : 0;
  MMF_TRY(c.workspace(3 * ws_bytes((size_t)E + 1, 8) + ws_bytes((size_t)E + 1, 4) + temp + 256, &c.ws));
  unsigned long long* k_edge = c.ws.take<unsigned long long>((size_t)E + 1);
  unsigned long long* k_node = c.ws.take<unsigned long long>((size_t)E + 1);
  unsigned long long* sorted = c.ws.take<unsigned long long>((size_t)E + 1);
  int32_t* cols = c.ws.take<int32_t>((size_t)E + 1);
  void* sort_tmp = c.ws.take<char>(temp + 1);
  MMF_HIP(hipMemsetAsync(status, 0xff, 16, s));
  const unsigned long long last = (unsigned long long)N * (unsigned long long)M;
  const dim3 grid_e((unsigned)((E + 255) / 256)), block(256);
  if (E > 0) {
    MMF_TRY(hg_launch_keys(edge_index, E, N, M, k_edge, k_node, status, s));
    hipLaunchKernelGGL(hp_iota_kernel, grid_e, block, 0, s, cols, E);
    MMF_LAUNCH_CHECK();
    size_t tb = temp;
    MMF_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, tb, k_edge, sorted, cols, epos, (int)E, 0, bits, s));
  }
  MMF_TRY(hg_launch_csr(sorted, E, last, (unsigned long long)N, M, eptr, emem, s));
  if (E > 0) {
    hipLaunchKernelGGL(hp_pos_tail_kernel, grid_e, block, 0, s, sorted, E, last, epos);
    MMF_LAUNCH_CHECK();
    size_t tb = temp;
    MMF_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, tb, k_node, sorted, cols, npos, (int)E, 0, bits, s));
  }
  MMF_TRY(hg_launch_csr(sorted, E, last, (unsigned long long)M, N, nptr, nmem, s));
  if (E > 0) {
    hipLaunchKernelGGL(hp_pos_tail_kernel, grid_e, block, 0, s, sorted, E, last, npos);
    MMF_LAUNCH_CHECK();
  }
  if (M + N > 0) MMF_TRY(hg_launch_scales(eptr, M, nptr, nmem, N, hyperedge_weight, edge_scale, node_scale, s));
  return MMF_OK;
}

int mmf_pair_scales(const int64_t* eptr, const int32_t* epos, const int64_t* nptr, const int32_t* nmem, const int32_t* npos,
                    const float* pair_weight, const float* hyperedge_weight, int64_t num_nodes, int64_t num_edges, int64_t num_pairs,
                    float* edge_scale, float* node_scale, int device_id, void* hip_stream) {
  Call c("pair_scales", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, E = num_pairs;
  MMF_TRY(hg_check_sizes(c.who, N, M, E));
  if (!eptr || !nptr || (E > 0 && (!epos || !nmem || !npos || !pair_weight)) || (M > 0 && !edge_scale) || (N > 0 && !node_scale)) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  if (M + N > 0) {
    hipLaunchKernelGGL(hp_scales_kernel, dim3((unsigned)((M + N + 255) / 256)), dim3(256), 0, c.s, eptr, epos, M, nptr, nmem, npos, N, pair_weight,
                       hyperedge_weight, edge_scale, node_scale);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

int mmf_hypergraph_propagate_pairs(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const int64_t* nptr, const int32_t* nmem,
                                   const int32_t* npos, const float* edge_scale, const float* node_scale, const float* hyperedge_weight,
                                   const float* pair_weight, int64_t num_pairs, const float* x, int64_t x_stride, int64_t num_nodes,
                                   int64_t num_edges, int64_t channels, float* Y, float* out, int transpose, int device_id, void* hip_stream) {
  Call c("hypergraph_propagate_pairs", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, C = channels, E = num_pairs;
  MMF_TRY(hg_check_sizes(c.who, N, M, E));
  MMF_TRY(hp_check_channels(c.who, C, x_stride));
  if (!eptr || !nptr || (E > 0 && (!emem || !epos || !nmem || !npos || !pair_weight)) || (M > 0 && !edge_scale) ||
      (N > 0 && !node_scale && !transpose) || (C > 0 && ((N > 0 && (!x || !out)) || (M > 0 && !Y)))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  MMF_TRY(launch_pair_gather(eptr, emem, epos, pair_weight, M, x, x_stride, C, edge_scale, hyperedge_weight, Y, C, c.s));
  return launch_pair_gather(nptr, nmem, npos, pair_weight, N, Y, C, C, transpose ? nullptr : node_scale, nullptr, out, C, c.s);
}

int mmf_pair_weight_grad(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const float* gprime, const float* x, int64_t x_stride,
                         const float* Y, const float* T, int64_t num_nodes, int64_t num_edges, int64_t channels, int64_t num_pairs,
                         float* grad_a, int device_id, void* hip_stream) {
  Call c("pair_weight_grad", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, C = channels, E = num_pairs;
  MMF_TRY(hg_check_sizes(c.who, N, M, E));
  MMF_TRY(hp_check_channels(c.who, C, x_stride));
  if (!eptr || (E > 0 && (!emem || !epos || !grad_a)) || (C > 0 && ((N > 0 && (!gprime || !x)) || (M > 0 && (!Y || !T))))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  if (E == 0) return MMF_OK;
  MMF_TRY(c.begin());
  MMF_HIP(hipMemsetAsync(grad_a, 0, (size_t)E * 4, c.s));
  if (M == 0 || C == 0) return MMF_OK;
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < C) ++lg;
  hipLaunchKernelGGL(hp_weight_grad_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, c.s, eptr, emem, epos, gprime, x, x_stride, Y, T, M, (int)C,
                     grad_a, lg);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int mmf_pair_softmax(const int64_t* ptr, const int32_t* pos, int64_t rows, int64_t num_pairs, const float* score, float* alpha,
                     int device_id, void* hip_stream) {
  Call c("pair_softmax", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(hp_check_rows(c.who, rows, num_pairs));
  if (!ptr || (num_pairs > 0 && (!pos || !score || !alpha))) { set_error("%s: NULL pointer", c.who); return MMF_E_INVALID; }
  if (num_pairs == 0) return MMF_OK;
  MMF_TRY(c.begin());
  MMF_HIP(hipMemsetAsync(alpha, 0, (size_t)num_pairs * 4, c.s));
  if (rows == 0) return MMF_OK;
  hipLaunchKernelGGL(hp_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.s, ptr, pos, rows, score, alpha);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int mmf_pair_softmax_backward(const int64_t* ptr, const int32_t* pos, int64_t rows, int64_t num_pairs, const float* alpha,
                              const float* grad_alpha, float* grad_score, int device_id, void* hip_stream) {
  Call c("pair_softmax_backward", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(hp_check_rows(c.who, rows, num_pairs));
  if (!ptr || (num_pairs > 0 && (!pos || !alpha || !grad_alpha || !grad_score))) { set_error("%s: NULL pointer", c.who); return MMF_E_INVALID; }
  if (num_pairs == 0) return MMF_OK;
  MMF_TRY(c.begin());
  MMF_HIP(hipMemsetAsync(grad_score, 0, (size_t)num_pairs * 4, c.s));
  if (rows == 0) return MMF_OK;
  hipLaunchKernelGGL(hp_softmax_backward_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.s, ptr, pos, rows, alpha, grad_alpha, grad_score);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // extern "C"
