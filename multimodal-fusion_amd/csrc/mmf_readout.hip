// mmf_readout.hip — attention readout over a ragged batch: inside every segment a softmax of the gate, then the gate-weighted sum of
// the rows of x (include/ext/mmf_hg_readout.h).  The reference ends its HypergraphNetwork with torch_geometric's
// GlobalAttention (downstream_survival/models/cust_omics.py:69,108); underneath, that is a scatter-max, an exp and two scatter-adds
// with float atomics.  Here every sum is a sequential f32 chain at two levels — the rows of a chunk of 64, then the chunks of a
// segment — so the bits depend on neither the launch nor the run:
//
//   max       one wave per chunk: the largest gate as an order-preserving integer key, one integer atomic max per chunk into the
//             segment's key word (exact, order-free); the first chunk of a segment leaves its number behind
//   chunks    one group of L lanes per chunk, L the power of two that covers the row's float4 (or float) columns, at most 64: a
//             wave per chunk when C is wide, 64 / L chunks per wave when it is narrow.  The group fetches L gates with one load,
//             computes e = cexp(gate - max) lanewise and hands the values out with lane reads; the x loads of 8 rows are issued
//             before their multiply-adds, which stay in row order.  Partials: z [chunks], u [chunks][C]; e is parked in alpha
//   finish    one thread per (segment, column): the chains of the segment's partials in chunk order, the divide, seg_max, seg_sum
//   alpha     one lane per row: alpha = e / Z
//   backward  one wave per chunk, L lanes per row: grad_x = alpha G, and for the gate the two dot64 of the header
//
// No fma (the build has -ffp-contract=off), no atomics on floats, no runtime exponential: cexp below is the header's definition.
#include "mmf_dev.h"
#include "mmf_host.h"
#include "mmf_hgshare.h"

namespace mmf {

static_assert(MMF_READOUT_CHUNK == 64, "a chunk is the rows one wave holds a gate of each: the kernels below are written for 64");
// RO_BATCH, RO_ROWS, RO_LIMIT, the header's scalar definitions (cexp, the float keys), the dot64 tree and the chunk record (RoChunk,
// ro_chunk): mmf_hgshare.h

// ---- max ------------------------------------------------------------------------------------------------------------------------
// segkey [S] and first_chunk [S] are zeroed before: key 0 lies below the key of every float
__global__ __launch_bounds__(256) void ro_max_kernel(const float* __restrict__ gate, const int64_t* __restrict__ ptr,
                                                     const int32_t* __restrict__ table, int64_t num_chunks, int64_t S, int64_t N,
                                                     uint32_t* __restrict__ segkey, int32_t* __restrict__ first_chunk) {
  const int lane = threadIdx.x & 63;
  const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= num_chunks) return;
  RoChunk k;
  if (!ro_chunk(table, ptr, ch, S, N, k)) return;                   // uniform over the wave
  uint32_t key = lane < k.cnt ? ro_key(gate[k.row + lane]) : 0u;
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)key, h, 64);
    key = other > key ? other : key;
  }
  if (lane == 0) {
    atomicMax(segkey + k.s, key);
    if (k.first) first_chunk[k.s] = (int32_t)ch;
  }
}

// ---- chunks ---------------------------------------------------------------------------------------------------------------------
struct ReadoutArgs {
  const float* x; int64_t x_stride; const float* gate; const int64_t* ptr; const int32_t* table;
  int64_t num_chunks, N, S; int C;
  const uint32_t* segkey;
  float* part_u; float* part_z; float* e_out;
  int lg;                     // log2 of the lanes per chunk (FULL: 6)
};

template <int VEC> struct RoVec;
template <> struct RoVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
  static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
  static __device__ __forceinline__ T mul(T a, float s) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
};
template <> struct RoVec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
  static __device__ __forceinline__ T add(T a, T b) { return a + b; }
  static __device__ __forceinline__ T mul(T a, float s) { return s * a; }
};

// VEC = 4: C, the row pitch of x and its base are multiples of four floats; VEC = 1: any C, any pitch.  FULL: one wave per chunk.
template <int VEC, bool FULL>
__global__ __launch_bounds__(256) void ro_chunk_kernel(ReadoutArgs a) {
  typedef RoVec<VEC> V;
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
    typename V::T acc = V::zero();
    z = 0.f;
    for (int j0 = 0; j0 < k.cnt; j0 += L) {
      const int nb = k.cnt - j0 < L ? k.cnt - j0 : L;
      float e = 0.f;
      if (sub < nb) {                                    // the next L gates of the chunk: one load
        e = ro_cexp(a.gate[k.row + j0 + sub] - m);
        if (c0 == 0) a.e_out[k.row + j0 + sub] = e;
      }
      for (int b = 0; b < nb; b += RO_BATCH) {
        typename V::T v[RO_BATCH];
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
        // both chains, in row order.  A slot past the chunk's end holds e = +0 and x = +0: z and acc start at +0 and no sum of
        // theirs is -0, so adding +0 (or +0 * +0) leaves every bit as it is
#pragma unroll
        for (int u = 0; u < RO_BATCH; ++u) {
          z = z + ev[u];
          acc = V::add(acc, V::mul(v[u], ev[u]));
        }
      }
    }
    if (live) V::store(a.part_u + ch * a.C + c, acc);
    c0 += L * VEC;
  } while (c0 < a.C);
  if (sub == 0) a.part_z[ch] = z;
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ro_finish_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ first_chunk,
                                                        const uint32_t* __restrict__ segkey, const float* __restrict__ part_u,
                                                        const float* __restrict__ part_z, int64_t num_chunks, int64_t S, int C,
                                                        float* __restrict__ out, float* __restrict__ seg_max, float* __restrict__ seg_sum) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t Cw = C > 0 ? C : 1;
  if (t >= S * Cw) return;
  const int64_t s = t / Cw;
  const int c = (int)(t - s * Cw);
  const bool live = c < C;
  const int64_t n = ptr[s + 1] - ptr[s];
  const int64_t nq = (n + 63) / 64, f = n > 0 ? first_chunk[s] : 0;
  if (n <= 0 || f < 0 || f + nq > num_chunks) {          // an empty segment (or one the chunk table does not cover)
    if (live) out[s * C + c] = 0.f;
    if (c == 0) { seg_max[s] = -INFINITY; seg_sum[s] = 0.f; }
    return;
  }
  float Z = 0.f, U = 0.f;
  for (int64_t q = 0; q < nq; q += RO_BATCH) {
    float zv[RO_BATCH], uv[RO_BATCH];
#pragma unroll
    for (int u = 0; u < RO_BATCH; ++u) {
      zv[u] = 0.f;
      uv[u] = 0.f;
      if (q + u < nq) {
        zv[u] = part_z[f + q + u];
        if (live) uv[u] = part_u[(f + q + u) * C + c];
      }
    }
#pragma unroll
    for (int u = 0; u < RO_BATCH; ++u) {                 // chunk order; a slot past the end adds +0
      Z = Z + zv[u];
      U = U + uv[u];
    }
  }
  if (live) out[s * C + c] = U / Z;
  if (c == 0) { seg_max[s] = ro_unkey(segkey[s]); seg_sum[s] = Z; }
}

__global__ __launch_bounds__(256) void ro_alpha_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ table, int64_t num_chunks,
                                                       int64_t S, int64_t N, const float* __restrict__ seg_sum, float* __restrict__ alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= num_chunks) return;
  RoChunk k;
  if (!ro_chunk(table, ptr, ch, S, N, k)) return;
  if (lane < k.cnt) alpha[k.row + lane] = alpha[k.row + lane] / seg_sum[k.s];
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
template <bool GATE>
__global__ __launch_bounds__(256) void ro_backward_kernel(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ alpha,
                                                          const int64_t* __restrict__ ptr, const int32_t* __restrict__ table,
                                                          int64_t num_chunks, int64_t N, int64_t S, int C, const float* __restrict__ out,
                                                          const float* __restrict__ G, float* __restrict__ gx, float* __restrict__ gg, int lg) {
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
      for (int u = 0; u < RO_ROWS; ++u) xv[u] = (GATE && ok[u]) ? x[row[u] * x_stride + c] : 0.f;
#pragma unroll
      for (int u = 0; u < RO_ROWS; ++u) {
        if (GATE) p[u] = p[u] + gv * xv[u];
        if (ok[u]) gx[row[u] * C + c] = al[u] * gv;
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

// ---- host -----------------------------------------------------------------------------------------------------------------------
int ro_check(const char* who, int64_t num_chunks, int64_t N, int64_t S, int64_t C, int64_t x_stride) {
  if (num_chunks < 0 || N < 0 || S < 0 || C < 0) {
    set_error("%s: the chunk count, N, S and C must be >= 0 (got %lld, %lld, %lld, %lld)", who, (long long)num_chunks, (long long)N, (long long)S,
              (long long)C);
    return MMF_E_INVALID;
  }
  if (x_stride < C) { set_error("%s: the row pitch of x (%lld) must be at least C (%lld)", who, (long long)x_stride, (long long)C); return MMF_E_INVALID; }
  if (num_chunks >= RO_LIMIT || N >= RO_LIMIT || S >= RO_LIMIT || C >= RO_LIMIT || S * (C > 0 ? C : 1) >= ((int64_t)1 << 39)) {
    set_error("%s: the chunk count, N, S and C must be < 2^31 and S x C < 2^39 (got %lld, %lld, %lld, %lld)", who, (long long)num_chunks, (long long)N,
              (long long)S, (long long)C);
    return MMF_E_UNSUPPORTED;
  }
  if (num_chunks > N || num_chunks * MMF_READOUT_CHUNK < N) {        // every row lies in a chunk, no chunk is empty
    set_error("%s: %lld chunks cannot hold %lld rows", who, (long long)num_chunks, (long long)N);
    return MMF_E_INVALID;
  }
  return MMF_OK;
}

static unsigned ro_wave_grid(int64_t waves) { return (unsigned)((waves + 3) / 4); }

// the launches of the forward around the chunk kernel (mmf_hgshare.h): mmf_attention_readout below and mmf_attention_readout_16
// (mmf_hg16.hip) enqueue the same
int ro_launch_max(const float* gate, const int64_t* ptr, const int32_t* table, int64_t num_chunks, int64_t S, int64_t N, uint32_t* segkey,
                  int32_t* first_chunk, hipStream_t s) {
  hipLaunchKernelGGL(ro_max_kernel, dim3(ro_wave_grid(num_chunks)), dim3(256), 0, s, gate, ptr, table, num_chunks, S, N, segkey, first_chunk);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int ro_launch_finish(const int64_t* ptr, const int32_t* first_chunk, const uint32_t* segkey, const float* part_u, const float* part_z,
                     int64_t num_chunks, int64_t S, int64_t C, float* out, float* seg_max, float* seg_sum, hipStream_t s) {
  const int64_t threads = S * (C > 0 ? C : 1);
  hipLaunchKernelGGL(ro_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ptr, first_chunk, segkey, part_u, part_z,
                     num_chunks, S, (int)C, out, seg_max, seg_sum);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int ro_launch_alpha(const int64_t* ptr, const int32_t* table, int64_t num_chunks, int64_t S, int64_t N, const float* seg_sum, float* alpha,
                    hipStream_t s) {
  hipLaunchKernelGGL(ro_alpha_kernel, dim3(ro_wave_grid(num_chunks)), dim3(256), 0, s, ptr, table, num_chunks, S, N, seg_sum, alpha);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int64_t mmf_attention_readout_table(const int64_t* ptr_host, int64_t S, int32_t* table_out, int64_t capacity) {
  const char* who = "attention_readout_table";
  if (S >= RO_LIMIT) { set_error("%s: S must be < 2^31 (got %lld)", who, (long long)S); return MMF_E_UNSUPPORTED; }
  MMF_TRY(check_offsets(who, "ptr", ptr_host, S, 0, 0, kAnyRows));
  int64_t chunks = 0;
  for (int64_t s = 0; s < S; ++s) chunks += (ptr_host[s + 1] - ptr_host[s] + MMF_READOUT_CHUNK - 1) / MMF_READOUT_CHUNK;
  if (ptr_host[S] >= RO_LIMIT || chunks >= RO_LIMIT) {
    set_error("%s: N and the chunk count must be < 2^31 (got %lld, %lld)", who, (long long)ptr_host[S], (long long)chunks);
    return MMF_E_UNSUPPORTED;
  }
  if (table_out) {
    if (capacity < chunks) { set_error("%s: a table of %lld records is needed (capacity %lld)", who, (long long)chunks, (long long)capacity); return MMF_E_INVALID; }
    int64_t q = 0;
    for (int64_t s = 0; s < S; ++s)
      for (int64_t row = ptr_host[s]; row < ptr_host[s + 1]; row += MMF_READOUT_CHUNK, ++q) {
        table_out[2 * q] = (int32_t)s;
        table_out[2 * q + 1] = (int32_t)row;
      }
  }
  return chunks;
}

int mmf_attention_readout(const float* x, int64_t x_stride, const float* gate, const int64_t* ptr_dev, const int32_t* table_dev,
                          int64_t num_chunks, int64_t N, int64_t S, int64_t C, float* out, float* alpha, float* seg_max, float* seg_sum,
                          int device_id, void* hip_stream) {
  Call c("attention_readout", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(ro_check(c.who, num_chunks, N, S, C, x_stride));
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
    const bool vec = C % 4 == 0 && x_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int64_t units = vec ? C / 4 : C;
    int lg = 0;
    while (lg < 6 && ((int64_t)1 << lg) < units) ++lg;
    ReadoutArgs a{x, x_stride, gate, ptr_dev, table_dev, num_chunks, N, S, (int)C, segkey, part_u, part_z, alpha, lg};
    const int64_t per_wave = 64 >> lg;
    const dim3 grid(ro_wave_grid((num_chunks + per_wave - 1) / per_wave)), block(256);
    if (vec) {
      if (lg == 6) hipLaunchKernelGGL((ro_chunk_kernel<4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((ro_chunk_kernel<4, false>), grid, block, 0, s, a);
    } else {
      if (lg == 6) hipLaunchKernelGGL((ro_chunk_kernel<1, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((ro_chunk_kernel<1, false>), grid, block, 0, s, a);
    }
    MMF_LAUNCH_CHECK();
  }
  MMF_TRY(ro_launch_finish(ptr_dev, first_chunk, segkey, part_u, part_z, num_chunks, S, C, out, seg_max, seg_sum, s));
  if (num_chunks > 0) MMF_TRY(ro_launch_alpha(ptr_dev, table_dev, num_chunks, S, N, seg_sum, alpha, s));
  return MMF_OK;
}

int mmf_attention_readout_backward(const float* x, int64_t x_stride, const float* alpha, const int64_t* ptr_dev, const int32_t* table_dev,
                                   int64_t num_chunks, const float* out, const float* grad_out, int64_t N, int64_t S, int64_t C,
                                   float* grad_x, float* grad_gate, int device_id, void* hip_stream) {
  Call c("attention_readout_backward", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(ro_check(c.who, num_chunks, N, S, C, x_stride));
  if (!ptr_dev || (N > 0 && (!alpha || !table_dev || (C > 0 && (!grad_out || !grad_x || (grad_gate && (!x || !out))))))) {
    set_error("%s: NULL pointer", c.who);
    return MMF_E_INVALID;
  }
  if (num_chunks == 0) return MMF_OK;
  MMF_TRY(c.begin());
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < C) ++lg;
  const dim3 grid(ro_wave_grid(num_chunks)), block(256);
  if (grad_gate) hipLaunchKernelGGL((ro_backward_kernel<true>), grid, block, 0, c.s, x, x_stride, alpha, ptr_dev, table_dev, num_chunks, N, S, (int)C,
                                    out, grad_out, grad_x, grad_gate, lg);
  else hipLaunchKernelGGL((ro_backward_kernel<false>), grid, block, 0, c.s, x, x_stride, alpha, ptr_dev, table_dev, num_chunks, N, S, (int)C, out,
                          grad_out, grad_x, grad_gate, lg);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // extern "C"
