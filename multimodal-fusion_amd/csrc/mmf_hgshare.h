// mmf_hgshare.h — what mmf_hgconv.hip, mmf_readout.hip and mmf_hgpair.hip share: the device helpers whose arithmetic is part of a
// header's rule (the canonical exponential and the dot64 tree of include/ext/mmf_hg_readout.h, the float4 / float row vector of the
// gather-sums), and the host helpers of the incidence plan that live in mmf_hgconv.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
