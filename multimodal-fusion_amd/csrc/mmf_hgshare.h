// mmf_hgshare.h — what mmf_hgconv.hip, mmf_readout.hip, mmf_hgpair.hip and mmf_hg16.hip share: the device helpers whose arithmetic is
// part of a header's rule (the canonical exponential and the dot64 tree of include/ext/mmf_hg_readout.h, the float4 / float row
// vector of the gather-sums, the widening, the rounding r16 and the 8-wide row vector of include/ext/mmf_hg_hg16.h), the chunk record
// of the readout, and the host helpers of the incidence plan (mmf_hgconv.hip) and of the readout (mmf_readout.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmf_hg.h"

namespace mmf {

// ---- the scalar definitions of include/ext/mmf_hg_readout.h -----------------------------------------------------------------------
constexpr float RO_LOG2E = 1.4426950408889634f;
constexpr float RO_LN2_HI = 0.693145751953125f;
constexpr float RO_LN2_LO = 1.428606765330187e-06f;
constexpr float RO_C2 = (float)(1.0 / 2), RO_C3 = (float)(1.0 / 6), RO_C4 = (float)(1.0 / 24), RO_C5 = (float)(1.0 / 120),
                RO_C6 = (float)(1.0 / 720), RO_C7 = (float)(1.0 / 5040);

__device__ __forceinline__ float ro_cexp(float t) {
  if (t < -87.0f) return 0.0f;
  const float n = rintf(t * RO_LOG2E);
  const float r = (t - n * RO_LN2_HI) - n * RO_LN2_LO;
  float p = RO_C7;
  p = p * r; p = p + RO_C6;
  p = p * r; p = p + RO_C5;
  p = p * r; p = p + RO_C4;
  p = p * r; p = p + RO_C3;
  p = p * r; p = p + RO_C2;
  p = p * r; p = p + 1.0f;
  p = p * r; p = p + 1.0f;
  return p * __int_as_float(((int)n + 127) << 23);
}

// float -> unsigned key with the order of the floats (-0 < +0), and back
__device__ __forceinline__ uint32_t ro_key(float g) {
  const uint32_t u = __float_as_uint(g);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ro_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the halving tree of dot64 over a group of L lanes (L < 64 only when C <= L: the levels left out would add +0 to partials that
// are never -0); lane 0 of the group ends with the value
__device__ __forceinline__ float ro_tree(float p, int L) {
  for (int h = L >> 1; h >= 1; h >>= 1) p = p + __shfl_down(p, h, L);
  return p;
}

// ---- a lane's share of a row of the gather-sums: four columns or one --------------------------------------------------------------
template <int VEC> struct HgVec;
template <> struct HgVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
  static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
  static __device__ __forceinline__ T mul(T a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
};
template <> struct HgVec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
  static __device__ __forceinline__ T add(T a, T b) { return a + b; }
  static __device__ __forceinline__ T mul(T a, float s) { return a * s; }
};

// ---- 16-bit storage, f32 arithmetic (include/ext/mmf_hg_hg16.h) -------------------------------------------------------------------
// DT = MMF_F16 / MMF_BF16.  widen is exact; r16 is round-to-nearest-even of a finite f32: for bf16 on the bits (the header's formula),
// for f16 the device's conversion, which keeps subnormals and overflows to infinity under the build's flags (the f16 denormal mode of
// a kernel is always IEEE; tests/test_gpu_hg16.py pins both).  That conversion is written as the instruction itself: as a cast, the
// compiler folds the f32 multiply or add in front of it into v_fma_mixlo_f16, which rounds the exact result once to f16 — not the
// rule's rounded f32 operation followed by r16 (2 of 38016 values of a readout's grad_x differed that way).
template <int DT> struct H16;
template <> struct H16<MMF_BF16> {
  static __device__ __forceinline__ float widen(uint32_t b) { return __uint_as_float(b << 16); }
  static __device__ __forceinline__ uint32_t r16(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
};
template <> struct H16<MMF_F16> {
  static __device__ __forceinline__ float widen(uint32_t b) { return (float)__builtin_bit_cast(_Float16, (uint16_t)b); }
  static __device__ __forceinline__ uint32_t r16(float f) {
    uint32_t h;
    asm("v_cvt_f16_f32_e32 %0, %1" : "=v"(h) : "v"(f));
    return h & 0xffffu;
  }
};

// a lane's share of a 16-bit row as it is loaded and stored: eight columns in one 16-byte access, or one column
template <int VEC> struct Raw16;
template <> struct Raw16<8> {
  uint4 q;
  static __device__ __forceinline__ Raw16 zero() { return {make_uint4(0u, 0u, 0u, 0u)}; }
  static __device__ __forceinline__ Raw16 load(const uint16_t* p) { return {*reinterpret_cast<const uint4*>(p)}; }
  __device__ __forceinline__ uint32_t get(int i) const {
    const uint32_t w = (i >> 1) == 0 ? q.x : (i >> 1) == 1 ? q.y : (i >> 1) == 2 ? q.z : q.w;
    return (i & 1) ? (w >> 16) : (w & 0xffffu);
  }
  static __device__ __forceinline__ void store(uint16_t* p, const uint32_t* h) {
    *reinterpret_cast<uint4*>(p) = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  }
};
template <> struct Raw16<1> {
  uint16_t q;
  static __device__ __forceinline__ Raw16 zero() { return {(uint16_t)0}; }
  static __device__ __forceinline__ Raw16 load(const uint16_t* p) { return {*p}; }
  __device__ __forceinline__ uint32_t get(int) const { return q; }
  static __device__ __forceinline__ void store(uint16_t* p, const uint32_t* h) { *p = (uint16_t)h[0]; }
};

// ---- the readout's chunk record (mmf_readout.hip, mmf_hg16.hip) -------------------------------------------------------------------
constexpr int RO_BATCH = 8;            // rows whose loads are in flight before their multiply-adds
constexpr int RO_ROWS = 4;             // backward: rows per lane group in flight
constexpr int64_t RO_LIMIT = (int64_t)1 << 31;

// A record of the chunk table, checked against the offsets before anything is addressed with it: a record that does not lie inside
// its segment (a table that belongs to other offsets) is skipped, it reads and writes nothing.
struct RoChunk { int s; int64_t row; int cnt; bool first; };
__device__ __forceinline__ bool ro_chunk(const int32_t* __restrict__ table, const int64_t* __restrict__ ptr, int64_t ch, int64_t S, int64_t N,
                                         RoChunk& k) {
  k.s = table[2 * ch];
  k.row = table[2 * ch + 1];
  if (k.s < 0 || k.s >= S) return false;
  const int64_t beg = ptr[k.s], end = ptr[k.s + 1];
  if (beg < 0 || end > N || k.row < beg || k.row >= end) return false;
  k.cnt = end - k.row < 64 ? (int)(end - k.row) : 64;
  k.first = k.row == beg;
  return true;
}

// mmf_readout.hip: the argument check of both readout entries and the launches of the forward that do not read x
int ro_check(const char* who, int64_t num_chunks, int64_t N, int64_t S, int64_t C, int64_t x_stride);
int ro_launch_max(const float* gate, const int64_t* ptr, const int32_t* table, int64_t num_chunks, int64_t S, int64_t N, uint32_t* segkey,
                  int32_t* first_chunk, hipStream_t s);
int ro_launch_finish(const int64_t* ptr, const int32_t* first_chunk, const uint32_t* segkey, const float* part_u, const float* part_z,
                     int64_t num_chunks, int64_t S, int64_t C, float* out, float* seg_max, float* seg_sum, hipStream_t s);
int ro_launch_alpha(const int64_t* ptr, const int32_t* table, int64_t num_chunks, int64_t S, int64_t N, const float* seg_sum, float* alpha,
                    hipStream_t s);

// ---- mmf_hgconv.hip: the steps of the incidence plan, for the pair plan of mmf_hgpair.hip ------------------------------------------
constexpr int64_t HG_LIMIT = (int64_t)1 << 31;
int hg_key_bits(int64_t N, int64_t M);
int hg_check_sizes(const char* who, int64_t N, int64_t M, int64_t E);
// keys e * N + v -> k_edge, v * M + e -> k_node of every valid pair (N * M for the others), status as mmf_incidence_plan (memset before)
int hg_launch_keys(const int64_t* edge_index, int64_t E, int64_t N, int64_t M, unsigned long long* k_edge, unsigned long long* k_node,
                   int64_t* status, hipStream_t s);
// sorted keys row * inner + member -> ptr [R + 1], mem [E]
int hg_launch_csr(const unsigned long long* sorted, int64_t E, unsigned long long last, unsigned long long inner, int64_t R, int64_t* ptr,
                  int32_t* mem, hipStream_t s);
int hg_launch_scales(const int64_t* eptr, int64_t M, const int64_t* nptr, const int32_t* nmem, int64_t N, const float* w, float* edge_scale,
                     float* node_scale, hipStream_t s);

}  // namespace mmf
