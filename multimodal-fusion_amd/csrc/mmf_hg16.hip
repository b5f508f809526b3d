// mmf_hg16.hip — 16-bit activations for the hypergraph branch (include/ext/mmf_hg_hg16.h): the gather-sums of
// mmf_hgconv.hip and mmf_hgpair.hip, the weight gradient of mmf_hgpair.hip and the kernels of mmf_readout.hip that touch rows of x,
// for x, Y, out and grad_x stored as f16 or bf16.  Every value is widened exactly when it is loaded, every chain runs in f32
// registers in the order of the f32 kernels, and a stored 16-bit tensor is rounded once, at its store (H16::r16, mmf_hgshare.h).
//
//   gather    hg_gather_sum_kernel / hp_gather_sum_kernel in one template: L lanes per row, the row's ids (and, by MODE, the source
//             rows' scales and the pair weights) fetched L at a time and handed out with lane reads, the gathers of 8 members in
//             flight before their adds.  A lane owns 8 columns through one 16-byte load (VEC = 8) or 1 column through a 2-byte
//             load (VEC = 1): a row of C = 256 takes 32 lanes, two rows share a wave; C >= 512 takes a wave; above 512 the column
//             loop makes a second trip.  The gathered rows stay packed until their adds: 4 registers per member, not 8.
//   grad_a    hp_weight_grad_kernel with g' = f32(G) * node_scale formed on the fly
//   readout   ro_chunk_kernel and ro_backward_kernel for x of type T; the launches that do not read x are mmf_readout.hip's
//
// No fma (the build has -ffp-contract=off), no atomics, no LDS, no runtime exponential.
#include "mmf_dev.h"
#include "mmf_host.h"
#include "mmf_hgshare.h"

namespace mmf {

constexpr int H16_BATCH = 8;           // members whose gathers are in flight before their adds

// ---- gather-sum ---------------------------------------------------------------------------------------------------------------------
struct Gather16Args {
  const int64_t* ptr; const int32_t* col; const int32_t* pos; const float* a; int64_t rows;
  const uint16_t* src; int64_t src_stride; int C;
  const float* src_scale; const float* scale; const float* scale2; const float* bias;
  uint16_t* out; int64_t out_stride;
  int lg;                     // log2 of the lanes per row (FULL: 6)
};

// VEC = 8: C and both row pitches are multiples of 8 elements, both bases 16-byte aligned; VEC = 1: any C, any pitch.  FULL: one
// wave per row.  MODE & 1: a scale per source row; MODE & 2: the pair operand.
template <int DT, int VEC, bool FULL, int MODE>
__global__ __launch_bounds__(256) void h16_gather_sum_kernel(Gather16Args a) {
  typedef Raw16<VEC> V;
  typedef H16<DT> H;
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
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    for (int64_t j0 = beg; j0 < end; j0 += L) {
      const int cnt = end - j0 < (int64_t)L ? (int)(end - j0) : L;
      int myid = 0;
      float mys = 0.f, myw = 0.f;
      if (sub < cnt) {                                   // the next L ids of the row: one load (and their scales / weights)
        myid = a.col[j0 + sub];
        if constexpr ((MODE & 1) != 0) mys = a.src_scale[myid];
        if constexpr ((MODE & 2) != 0) myw = a.a[a.pos[j0 + sub]];
      }
      for (int b = 0; b < cnt; b += H16_BATCH) {
        V v[H16_BATCH];
        float sv[H16_BATCH], wv[H16_BATCH];
#pragma unroll
        for (int u = 0; u < H16_BATCH; ++u) {
          v[u] = V::zero();
          sv[u] = 0.f;
          wv[u] = 0.f;
          if (b + u < cnt) {                             // uniform over the group
            int id;
            if constexpr (FULL) {
              const int from = __builtin_amdgcn_readfirstlane(b + u);
              id = __builtin_amdgcn_readlane(myid, from);
              if constexpr ((MODE & 1) != 0) sv[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mys), from));
              if constexpr ((MODE & 2) != 0) wv[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myw), from));
            } else {
              id = __shfl(myid, b + u, L);
              if constexpr ((MODE & 1) != 0) sv[u] = __shfl(mys, b + u, L);
              if constexpr ((MODE & 2) != 0) wv[u] = __shfl(myw, b + u, L);
            }
            if (live) v[u] = V::load(a.src + (int64_t)id * a.src_stride + c);
          }
        }
        // the chain, in the row's order.  A slot past the row's end holds the row +0 (and the scale and the weight +0): acc starts
        // at +0 and no sum of it is -0, so acc + (+0) leaves every bit of acc as it is
#pragma unroll
        for (int u = 0; u < H16_BATCH; ++u) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            float t = H::widen(v[u].get(i));
            if constexpr ((MODE & 1) != 0) t = t * sv[u];
            if constexpr ((MODE & 2) != 0) t = wv[u] * t;
            acc[i] = acc[i] + t;
          }
        }
      }
    }
    if (live) {
      uint32_t h[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float f = acc[i];
        if (a.scale) f = f * a.scale[r];
        if (a.scale2) f = f * a.scale2[r];
        if (a.bias) f = f + a.bias[c + i];
        h[i] = H::r16(f);
      }
      V::store(a.out + r * a.out_stride + c, h);
    }
  }
}

template <int DT, int VEC, int MODE>
static void launch_gather16_form(const Gather16Args& a, dim3 grid, hipStream_t s) {
  if (a.lg == 6) hipLaunchKernelGGL((h16_gather_sum_kernel<DT, VEC, true, MODE>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((h16_gather_sum_kernel<DT, VEC, false, MODE>), grid, dim3(256), 0, s, a);
}

template <int DT, int VEC>
static void launch_gather16_mode(const Gather16Args& a, dim3 grid, hipStream_t s) {
  const int mode = (a.src_scale ? 1 : 0) | (a.a ? 2 : 0);
  if (mode == 0) launch_gather16_form<DT, VEC, 0>(a, grid, s);
  else if (mode == 1) launch_gather16_form<DT, VEC, 1>(a, grid, s);
  else if (mode == 2) launch_gather16_form<DT, VEC, 2>(a, grid, s);
  else launch_gather16_form<DT, VEC, 3>(a, grid, s);
}

static int launch_gather16(int dtype, const int64_t* ptr, const int32_t* col, const int32_t* pos, const float* w, int64_t rows, const void* src,
                           int64_t src_stride, int64_t C, const float* src_scale, const float* scale, const float* scale2, const float* bias,
                           void* out, int64_t out_stride, hipStream_t s) {
  if (rows <= 0 || C <= 0) return MMF_OK;
  const bool vec = C % 8 == 0 && src_stride % 8 == 0 && out_stride % 8 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int64_t units = vec ? C / 8 : C;
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < units) ++lg;
  Gather16Args a{ptr, col, pos, w, rows, static_cast<const uint16_t*>(src), src_stride, (int)C, src_scale, scale, scale2, bias,
                 static_cast<uint16_t*>(out), out_stride, lg};
  const int64_t per_wave = 64 >> lg, waves = (rows + per_wave - 1) / per_wave;
  const dim3 grid((unsigned)((waves + 3) / 4));
  if (dtype == MMF_F16) {
    if (vec) launch_gather16_mode<MMF_F16, 8>(a, grid, s);
    else launch_gather16_mode<MMF_F16, 1>(a, grid, s);
  } else {
    if (vec) launch_gather16_mode<MMF_BF16, 8>(a, grid, s);
    else launch_gather16_mode<MMF_BF16, 1>(a, grid, s);
  }
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// ---- grad_a -------------------------------------------------------------------------------------------------------------------------
// hp_weight_grad_kernel (mmf_hgpair.hip) with every row widened from T and g' = f32(G) * node_scale formed on the fly.
template <int DT>
__global__ __launch_bounds__(256) void h16_weight_grad_kernel(const int64_t* __restrict__ eptr, const int32_t* __restrict__ emem,
                                                              const int32_t* __restrict__ epos, const uint16_t* __restrict__ G,
                                                              const float* __restrict__ node_scale, const uint16_t* __restrict__ x,
                                                              int64_t x_stride, const uint16_t* __restrict__ Y, const uint16_t* __restrict__ T,
                                                              int64_t M, int C, float* __restrict__ grad_a, int lg) {
  typedef H16<DT> H;
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= M) return;                                    // uniform over the wave
  const int L = 1 << lg, sub = lane & (L - 1), rsub = lane >> lg, R = 64 >> lg;
  const int64_t beg = eptr[e], end = eptr[e + 1];
  const uint16_t* Ye = Y + e * C;
  const uint16_t* Te = T + e * C;
  for (int64_t j0 = beg; j0 < end; j0 += R) {            // uniform: every lane takes part in the trees below
    const int64_t j = j0 + rsub;
    const bool ok = j < end;
    const int64_t v = ok ? emem[j] : 0;
    float p1 = 0.f, p2 = 0.f;
    if (ok) {
      const uint16_t* gv = G + v * C;
      const uint16_t* xv = x + v * x_stride;
      const float ns = node_scale[v];
      for (int c = sub; c < C; c += 64) {
        p1 = p1 + (H::widen(gv[c]) * ns) * H::widen(Ye[c]);
        p2 = p2 + H::widen(xv[c]) * H::widen(Te[c]);
      }
    }
    const float d1 = ro_tree(p1, L), d2 = ro_tree(p2, L);
    if (ok && sub == 0) grad_a[epos[j]] = d1 + d2;
  }
}

// ---- readout: chunks ------------------------------------------------------------------------------------------------------------------
struct Readout16Args {
  const uint16_t* x; int64_t x_stride; const float* gate; const int64_t* ptr; const int32_t* table;
  int64_t num_chunks, N, S; int C;
  const uint32_t* segkey;
  float* part_u; float* part_z; float* e_out;
  int lg;                     // log2 of the lanes per chunk (FULL: 6)
};

// ro_chunk_kernel (mmf_readout.hip) for x of type T.  VEC = 8: C and the row pitch of x are multiples of 8 elements and its base is
// 16-byte aligned; VEC = 1: any C, any pitch.  The partials stay f32.
template <int DT, int VEC, bool FULL>
__global__ __launch_bounds__(256) void h16_ro_chunk_kernel(Readout16Args a) {
  typedef Raw16<VEC> V;
  typedef H16<DT> H;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lg = FULL ? 6 : a.lg;
  const int L = 1 << lg;
  const int sub = lane & (L - 1);
  const int64_t ch = FULL ? wave : wave * (64 >> lg) + (lane >> lg);
  if (ch >= a.num_chunks) return;                        // a whole group leaves together: every lane read below is of a live lane
  RoChunk k;
  if (!ro_chunk(a.table, a.ptr, ch, a.S, a.N, k)) return;
  const float m = ro_unkey(a.segkey[k.s]);
  float z = 0.f;
  int c0 = 0;
  do {                                                   // one trip unless the row is wider than the group (or C = 0: z alone)
    const int c = c0 + sub * VEC;
    const bool live = c < a.C;
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    z = 0.f;
    for (int j0 = 0; j0 < k.cnt; j0 += L) {
      const int nb = k.cnt - j0 < L ? k.cnt - j0 : L;
      float e = 0.f;
      if (sub < nb) {                                    // the next L gates of the chunk: one load
        e = ro_cexp(a.gate[k.row + j0 + sub] - m);
        if (c0 == 0) a.e_out[k.row + j0 + sub] = e;
      }
      for (int b = 0; b < nb; b += RO_BATCH) {
        V v[RO_BATCH];
        float ev[RO_BATCH];
#pragma unroll
        for (int u = 0; u < RO_BATCH; ++u) {
          v[u] = V::zero();
          ev[u] = 0.f;
          if (b + u < nb) {                              // uniform over the group
            if constexpr (FULL) ev[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), __builtin_amdgcn_readfirstlane(b + u)));
            else ev[u] = __shfl(e, b + u, L);
            if (live) v[u] = V::load(a.x + (k.row + j0 + b + u) * a.x_stride + c);
          }
        }
        // both chains, in row order; a slot past the chunk's end adds +0 (or +0 * +0)
#pragma unroll
        for (int u = 0; u < RO_BATCH; ++u) {
          z = z + ev[u];
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = acc[i] + ev[u] * H::widen(v[u].get(i));
        }
      }
    }
    if (live) {
      float* dst = a.part_u + ch * a.C + c;              // VEC = 8: C % 8 == 0 and the workspace is 256-byte aligned
      if constexpr (VEC == 8) {
        *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
      } else {
        dst[0] = acc[0];
      }
    }
    c0 += L * VEC;
  } while (c0 < a.C);
  if (sub == 0) a.part_z[ch] = z;
}

// ---- readout: backward ----------------------------------------------------------------------------------------------------------------
// ro_backward_kernel (mmf_readout.hip) for x and grad_x of type T
template <int DT, bool GATE>
__global__ __launch_bounds__(256) void h16_ro_backward_kernel(const uint16_t* __restrict__ x, int64_t x_stride, const float* __restrict__ alpha,
                                                              const int64_t* __restrict__ ptr, const int32_t* __restrict__ table,
                                                              int64_t num_chunks, int64_t N, int64_t S, int C, const float* __restrict__ out,
                                                              const float* __restrict__ G, uint16_t* __restrict__ gx, float* __restrict__ gg,
                                                              int lg) {
  typedef H16<DT> H;
  const int lane = threadIdx.x & 63;
  const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= num_chunks) return;
  RoChunk k;
  if (!ro_chunk(table, ptr, ch, S, N, k)) return;         // uniform over the wave
  const int L = 1 << lg, sub = lane & (L - 1), rsub = lane >> lg, R = 64 >> lg;
  const float* g = G + (int64_t)k.s * C;
  float r = 0.f;
  if (GATE) {
    const float* o = out + (int64_t)k.s * C;
    float p = 0.f;
    for (int c = sub; c < C; c += 64) p = p + g[c] * o[c];
    r = __shfl(ro_tree(p, L), 0, L);
  }
  for (int j0 = 0; j0 < k.cnt; j0 += R * RO_ROWS) {
    float al[RO_ROWS], p[RO_ROWS];
    int64_t row[RO_ROWS];
    bool ok[RO_ROWS];
#pragma unroll
    for (int u = 0; u < RO_ROWS; ++u) {
      const int j = j0 + u * R + rsub;
      ok[u] = j < k.cnt;
      row[u] = k.row + (ok[u] ? j : 0);
      al[u] = ok[u] ? alpha[row[u]] : 0.f;
      p[u] = 0.f;
    }
    for (int c = sub; c < C; c += 64) {                   // lane l takes the columns l, l + 64, ...: dot64's lane partials
      const float gv = g[c];
      float xv[RO_ROWS];
#pragma unroll
      for (int u = 0; u < RO_ROWS; ++u) xv[u] = (GATE && ok[u]) ? H::widen(x[row[u] * x_stride + c]) : 0.f;
#pragma unroll
      for (int u = 0; u < RO_ROWS; ++u) {
        if (GATE) p[u] = p[u] + gv * xv[u];
        if (ok[u]) gx[row[u] * C + c] = (uint16_t)H::r16(al[u] * gv);
      }
    }
    if (GATE) {
#pragma unroll
      for (int u = 0; u < RO_ROWS; ++u) {
        const float d = ro_tree(p[u], L);                 // every lane takes part: no lane read inside a divergent branch
        if (ok[u] && sub == 0) gg[row[u]] = al[u] * (d - r);
      }
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static int h16_check_dtype(const char* who, int dtype, const char* f32_entry) {
  if (dtype == MMF_F16 || dtype == MMF_BF16) return MMF_OK;
  if (dtype == MMF_F32) {
    set_error("%s: dtype MMF_F32: this entry takes f16 / bf16 rows; the f32 entry is %s", who, f32_entry);
    return MMF_E_UNSUPPORTED;
  }
  set_error("%s: unknown dtype %d (MMF_F16 or MMF_BF16)", who, dtype);
  return MMF_E_INVALID;
}

static int h16_check_channels(const char* who, int64_t C, int64_t x_stride) {
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

int mmf_csr_gather_sum_16(const int64_t* ptr, const int32_t* col, const int32_t* pos, const float* a, int64_t rows, const void* src,
                          int64_t src_stride, int64_t channels, int dtype, const float* src_scale, const float* scale, const float* scale2,
                          const float* bias, void* out, int64_t out_stride, int device_id, void* hip_stream) {
  Call c("csr_gather_sum_16", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (rows < 0 || channels < 0 || src_stride < channels || out_stride < channels) {
    set_error("%s: rows and channels must be >= 0 and both row pitches at least `channels` (got %lld, %lld, %lld, %lld)", c.who, (long long)rows,
              (long long)channels, (long long)src_stride, (long long)out_stride);
    return MMF_E_INVALID;
  }
  if (rows >= HG_LIMIT || channels >= HG_LIMIT) { set_error("%s: rows and channels must be < 2^31", c.who); return MMF_E_UNSUPPORTED; }
  MMF_TRY(h16_check_dtype(c.who, dtype, "mmf_csr_gather_sum"));
  if ((rows > 0 && channels > 0 && (!ptr || !out)) || ((pos != nullptr) != (a != nullptr))) {
    set_error("%s: NULL pointer (ptr, out; pos and a go together)", c.who);
    return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  return launch_gather16(dtype, ptr, col, pos, a, rows, src, src_stride, channels, src_scale, scale, scale2, bias, out, out_stride, c.s);
}

int mmf_hypergraph_propagate_16(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const int64_t* nptr, const int32_t* nmem,
                                const int32_t* npos, const float* edge_scale, const float* node_scale, const float* hyperedge_weight,
                                const float* pair_weight, int64_t num_pairs, const void* x, int64_t x_stride, int64_t num_nodes,
                                int64_t num_edges, int64_t channels, int dtype, const float* bias, void* Y, void* out, int transpose,
                                int device_id, void* hip_stream) {
  Call c("hypergraph_propagate_16", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, C = channels, E = num_pairs;
  MMF_TRY(hg_check_sizes(c.who, N, M, E));
  MMF_TRY(h16_check_channels(c.who, C, x_stride));
  MMF_TRY(h16_check_dtype(c.who, dtype, pair_weight ? "mmf_hypergraph_propagate_pairs" : "mmf_hypergraph_propagate"));
  // the transposed form reads node_scale too: it is the hyperedge step's src_scale
  if (!eptr || !nptr || (E > 0 && (!emem || !nmem || (pair_weight && (!epos || !npos)))) || (M > 0 && !edge_scale) || (N > 0 && !node_scale) ||
      (C > 0 && ((N > 0 && (!x || !out)) || (M > 0 && !Y)))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  const int32_t* ep = pair_weight ? epos : nullptr;
  const int32_t* np = pair_weight ? npos : nullptr;
  MMF_TRY(launch_gather16(dtype, eptr, emem, ep, pair_weight, M, x, x_stride, C, transpose ? node_scale : nullptr, edge_scale, hyperedge_weight,
                          nullptr, Y, C, c.s));
  return launch_gather16(dtype, nptr, nmem, np, pair_weight, N, Y, C, C, nullptr, transpose ? nullptr : node_scale, nullptr,
                         transpose ? nullptr : bias, out, C, c.s);
}

int mmf_pair_weight_grad_16(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const void* G, const float* node_scale, const void* x,
                            int64_t x_stride, const void* Y, const void* T, int64_t num_nodes, int64_t num_edges, int64_t channels,
                            int64_t num_pairs, int dtype, float* grad_a, int device_id, void* hip_stream) {
  Call c("pair_weight_grad_16", device_id, hip_stream);
  MMF_TRY(c.on_device());
  const int64_t N = num_nodes, M = num_edges, C = channels, E = num_pairs;
  MMF_TRY(hg_check_sizes(c.who, N, M, E));
  MMF_TRY(h16_check_channels(c.who, C, x_stride));
  MMF_TRY(h16_check_dtype(c.who, dtype, "mmf_pair_weight_grad"));
  if (!eptr || (E > 0 && (!emem || !epos || !grad_a)) || (N > 0 && !node_scale) || (C > 0 && ((N > 0 && (!G || !x)) || (M > 0 && (!Y || !T))))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  if (E == 0) return MMF_OK;
  MMF_TRY(c.begin());
  MMF_HIP(hipMemsetAsync(grad_a, 0, (size_t)E * 4, c.s));
  if (M == 0 || C == 0) return MMF_OK;
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < C) ++lg;
  const dim3 grid((unsigned)((M + 3) / 4)), block(256);
  const uint16_t *g16 = static_cast<const uint16_t*>(G), *x16 = static_cast<const uint16_t*>(x), *y16 = static_cast<const uint16_t*>(Y),
                 *t16 = static_cast<const uint16_t*>(T);
  if (dtype == MMF_F16) hipLaunchKernelGGL((h16_weight_grad_kernel<MMF_F16>), grid, block, 0, c.s, eptr, emem, epos, g16, node_scale, x16, x_stride,
                                           y16, t16, M, (int)C, grad_a, lg);
  else hipLaunchKernelGGL((h16_weight_grad_kernel<MMF_BF16>), grid, block, 0, c.s, eptr, emem, epos, g16, node_scale, x16, x_stride, y16, t16, M,
                          (int)C, grad_a, lg);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int mmf_attention_readout_16(const void* x, int64_t x_stride, int dtype, const float* gate, const int64_t* ptr_dev, const int32_t* table_dev,
                             int64_t num_chunks, int64_t N, int64_t S, int64_t C, float* out, float* alpha, float* seg_max, float* seg_sum,
                             int device_id, void* hip_stream) {
  Call c("attention_readout_16", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(ro_check(c.who, num_chunks, N, S, C, x_stride));
  MMF_TRY(h16_check_dtype(c.who, dtype, "mmf_attention_readout"));
  if (!ptr_dev || (S > 0 && (!seg_max || !seg_sum || (C > 0 && !out))) || (N > 0 && (!gate || !alpha || !table_dev || (C > 0 && !x)))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  if (S == 0) return MMF_OK;
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  MMF_TRY(c.workspace(ws_bytes((size_t)num_chunks * (size_t)C + 1, 4) + ws_bytes((size_t)num_chunks + 1, 4) + ws_bytes(2 * (size_t)S, 4), &c.ws));
  float* part_u = c.ws.take<float>((size_t)num_chunks * (size_t)C + 1);
  float* part_z = c.ws.take<float>((size_t)num_chunks + 1);
  uint32_t* segkey = c.ws.take<uint32_t>(2 * (size_t)S);
  int32_t* first_chunk = reinterpret_cast<int32_t*>(segkey + S);
  MMF_HIP(hipMemsetAsync(segkey, 0, 2 * (size_t)S * 4, s));
  if (num_chunks > 0) {
    MMF_TRY(ro_launch_max(gate, ptr_dev, table_dev, num_chunks, S, N, segkey, first_chunk, s));
    const bool vec = C % 8 == 0 && x_stride % 8 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int64_t units = vec ? C / 8 : C;
    int lg = 0;
    while (lg < 6 && ((int64_t)1 << lg) < units) ++lg;
    Readout16Args a{static_cast<const uint16_t*>(x), x_stride, gate, ptr_dev, table_dev, num_chunks, N, S, (int)C, segkey, part_u, part_z, alpha, lg};
    const int64_t per_wave = 64 >> lg, waves = (num_chunks + per_wave - 1) / per_wave;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    if (dtype == MMF_F16) {
      if (vec) {
        if (lg == 6) hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_F16, 8, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_F16, 8, false>), grid, block, 0, s, a);
      } else {
        if (lg == 6) hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_F16, 1, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_F16, 1, false>), grid, block, 0, s, a);
      }
    } else {
      if (vec) {
        if (lg == 6) hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_BF16, 8, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_BF16, 8, false>), grid, block, 0, s, a);
      } else {
        if (lg == 6) hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_BF16, 1, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((h16_ro_chunk_kernel<MMF_BF16, 1, false>), grid, block, 0, s, a);
      }
    }
    MMF_LAUNCH_CHECK();
  }
  MMF_TRY(ro_launch_finish(ptr_dev, first_chunk, segkey, part_u, part_z, num_chunks, S, C, out, seg_max, seg_sum, s));
  if (num_chunks > 0) MMF_TRY(ro_launch_alpha(ptr_dev, table_dev, num_chunks, S, N, seg_sum, alpha, s));
  return MMF_OK;
}

int mmf_attention_readout_backward_16(const void* x, int64_t x_stride, int dtype, const float* alpha, const int64_t* ptr_dev,
                                      const int32_t* table_dev, int64_t num_chunks, const float* out, const float* grad_out, int64_t N, int64_t S,
                                      int64_t C, void* grad_x, float* grad_gate, int device_id, void* hip_stream) {
  Call c("attention_readout_backward_16", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(ro_check(c.who, num_chunks, N, S, C, x_stride));
  MMF_TRY(h16_check_dtype(c.who, dtype, "mmf_attention_readout_backward"));
  if (!ptr_dev || (N > 0 && (!alpha || !table_dev || (C > 0 && (!grad_out || !grad_x || (grad_gate && (!x || !out))))))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  if (num_chunks == 0) return MMF_OK;
  MMF_TRY(c.begin());
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < C) ++lg;
  const dim3 grid((unsigned)((num_chunks + 3) / 4)), block(256);
  const uint16_t* x16 = static_cast<const uint16_t*>(x);
  uint16_t* gx16 = static_cast<uint16_t*>(grad_x);
  if (dtype == MMF_F16) {
    if (grad_gate) hipLaunchKernelGGL((h16_ro_backward_kernel<MMF_F16, true>), grid, block, 0, c.s, x16, x_stride, alpha, ptr_dev, table_dev, num_chunks,
                                      N, S, (int)C, out, grad_out, gx16, grad_gate, lg);
    else hipLaunchKernelGGL((h16_ro_backward_kernel<MMF_F16, false>), grid, block, 0, c.s, x16, x_stride, alpha, ptr_dev, table_dev, num_chunks, N, S,
                            (int)C, out, grad_out, gx16, grad_gate, lg);
  } else {
    if (grad_gate) hipLaunchKernelGGL((h16_ro_backward_kernel<MMF_BF16, true>), grid, block, 0, c.s, x16, x_stride, alpha, ptr_dev, table_dev, num_chunks,
                                      N, S, (int)C, out, grad_out, gx16, grad_gate, lg);
    else hipLaunchKernelGGL((h16_ro_backward_kernel<MMF_BF16, false>), grid, block, 0, c.s, x16, x_stride, alpha, ptr_dev, table_dev, num_chunks, N, S,
                            (int)C, out, grad_out, gx16, grad_gate, lg);
  }
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // extern "C"
