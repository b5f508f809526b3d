// mmf_rerank_combined.h — the re-rank kernel of the combined key K = K_h * K_g (device code), shared by
// its two launchers: launch_rerank_combined (mmf_topk.hip: rows in order, the exact passes) and launch_rerank_combined_ext
// (mmf_topk_anyk.hip: gathered rows and staged keys, the passes of mmf_simtopk_combined_fast_anyk).
#ifndef MMF_RERANK_COMBINED_H
#define MMF_RERANK_COMBINED_H

#include <type_traits>

#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

constexpr int RR_WAVES = 4;
constexpr int RR_MAXC = 1024;   // candidates per row: 2 x col_splits x cap <= 1024 (pick_splits, mmf_api.hip)

struct RerankCombinedArgs {
  const float* X; const float* Y; int64_t d; int64_t m;   // query rows / candidate rows of F ([.][d] f32)
  const float* rx; const float* cy;                       // their chains chain(f, f)
  const float* Pq; const float* Pc; int dp;               // positions ([.][dp] f32)
  const float* pnq; const float* pnc;                     // chain(p, p)
  float neg_lambda_h, neg_lambda_g;
  int k, out_stride, exclude_self;
  int64_t row_offset, col_offset, n_rows;
  const uint32_t* cand_cnt; const uint32_t* cand_ids; const uint32_t* overflow; int lists, cap;
  int64_t* out_idx; float* out_val;
  int32_t* fail_rows; uint32_t* fail_count; uint32_t* cand_total;
};

// One pass of several: the k entries go to columns out_off .. out_off + k - 1 of the row, the entry of rank
// k - 1 leaves (key, local id) in the row's floor slot for the next pass's scan, and only the last pass (no floor slot) pads.
struct RerankCombinedPassArgs : RerankCombinedArgs {
  int out_off;
  float* floor_key_out; uint32_t* floor_id_out;
};

// The passes of mmf_simtopk_combined_fast_anyk, launch_select's `row_ids` and `key_out`: list position `pos`
// (lists, overflow word, floor slot) is row row_ids[pos] of the queries (null: pos) — F, P, chains, self, outputs and the fail
// list go by row — and every emitted entry leaves its canonical key (the float the floor test compares) in key_out, laid out like
// out_val (null: none).
struct RerankCombinedExtArgs : RerankCombinedPassArgs {
  const int32_t* row_ids;
  float* key_out;
};

// PASS = false is the single-pass re-rank as it was (the same instructions); PASS = true adds only what sits under
// `if constexpr (PASS)`, EXT (with PASS) only what sits under `if constexpr (EXT)`.
template <bool VEC4, bool PASS = false, bool EXT = false>
__global__ __launch_bounds__(64 * RR_WAVES) void rerank_combined_kernel(
    std::conditional_t<EXT, RerankCombinedExtArgs, std::conditional_t<PASS, RerankCombinedPassArgs, RerankCombinedArgs>> a) {
  static_assert(!EXT || PASS, "row ids and staged keys come with the pass arguments");
  __shared__ float skey[RR_WAVES][RR_MAXC];
  __shared__ float sval[RR_WAVES][RR_MAXC];
  __shared__ uint32_t sid[RR_WAVES][RR_MAXC];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t pos = (int64_t)blockIdx.x * RR_WAVES + wave;   // list position
  if (pos >= a.n_rows) return;
  int64_t row = pos;                                            // row of the queries
  if constexpr (EXT) { if (a.row_ids) row = a.row_ids[pos]; }
  float* key = skey[wave];
  float* val = sval[wave];
  uint32_t* id = sid[wave];

  bool failed = a.overflow[pos] != 0;
  const bool was_overflow = failed;
  int total = 0;
  for (int l = 0; l < a.lists && !failed; ++l) {
    const uint32_t cn = a.cand_cnt[pos * a.lists + l];
    if (cn > (uint32_t)a.cap || total + (int)cn > RR_MAXC) { failed = true; break; }
    const int64_t base = (pos * a.lists + l) * a.cap;
    for (uint32_t e = lane; e < cn; e += 64) id[total + e] = a.cand_ids[base + e];
    total += (int)cn;
  }
  const int64_t grow = a.row_offset + row;
  int valid = 0;
  if (!failed) {
    __builtin_amdgcn_wave_barrier();
    const float ri = a.rx[row], pni = a.pnq[row];
    float pi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) pi[e] = (e < a.dp) ? a.Pq[row * a.dp + e] : 0.0f;
    for (int e = lane; e < total; e += 64) {
      const uint32_t j = id[e];
      const bool self = a.exclude_self && (a.col_offset + (int64_t)j == grow);
      float kx = kNegInf, vx = kNegInf;
      if (!self && (int64_t)j < a.m) {
        float dot = 0.0f;
        if constexpr (VEC4) {
          const f32x4* xp = reinterpret_cast<const f32x4*>(a.X + row * a.d);
          const f32x4* yp = reinterpret_cast<const f32x4*>(a.Y + (int64_t)j * a.d);
          for (int64_t q = 0; q < (a.d >> 2); ++q) {
            const f32x4 xv = xp[q], yv = yp[q];
            dot = __builtin_fmaf(xv[0], yv[0], dot);
            dot = __builtin_fmaf(xv[1], yv[1], dot);
            dot = __builtin_fmaf(xv[2], yv[2], dot);
            dot = __builtin_fmaf(xv[3], yv[3], dot);
          }
        } else {
          for (int64_t q = 0; q < a.d; ++q) dot = __builtin_fmaf(a.X[row * a.d + q], a.Y[(int64_t)j * a.d + q], dot);
        }
        float pj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pj[u] = (u < a.dp) ? a.Pc[(int64_t)j * a.dp + u] : 0.0f;
        const float eh = key_from_dot<MMF_RBF>(dot, ri, a.cy[j], a.neg_lambda_h);
        const float eg = pos_exponent<8>(pi, pj, pni, a.pnc[j], a.neg_lambda_g);
        kx = combined_key(eh, eg);
        vx = combined_val(eh, eg);
        if (kx != kx) kx = kNegInf;   // NaN keys rank last (undefined for non-finite inputs, as everywhere)
        ++valid;
      } else {
        id[e] = kNoIdx;
      }
      key[e] = kx;
      val[e] = vx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) valid += __shfl_xor(valid, o);
    if (valid < a.k) failed = true;
  }
  if (failed) {
    if (lane == 0) {
      const uint32_t slot = atomicAdd(a.fail_count, 1u);
      a.fail_rows[slot] = (int32_t)row;
      atomicAdd(a.fail_count + (was_overflow ? 1 : 2), 1u);   // reason counters, as select
    }
    return;
  }
  if (a.cand_total && lane == 0) atomicAdd(a.cand_total + (blockIdx.x & 255), (uint32_t)total);
  __builtin_amdgcn_wave_barrier();
  int64_t* oi = a.out_idx + row * a.out_stride;
  float* ov = a.out_val + row * a.out_stride;
  if constexpr (PASS) { oi += a.out_off; ov += a.out_off; }
  for (int e = lane; e < total; e += 64) {
    const uint32_t ie = id[e];
    if (ie == kNoIdx) continue;
    const float ke = key[e];
    int rank = 0;
    for (int f = 0; f < total; ++f) {
      const uint32_t jf = id[f];
      rank += (jf != kNoIdx && better(key[f], jf, ke, ie)) ? 1 : 0;
    }
    if (rank < a.k) { oi[rank] = a.col_offset + (int64_t)ie; ov[rank] = val[e]; }
    if constexpr (PASS) {
      // the next pass's floor: the key the scan compares (NaN already -inf) and the list's id, before col_offset — as select
      if (a.floor_key_out && rank == a.k - 1) { a.floor_key_out[pos] = ke; a.floor_id_out[pos] = ie; }
    }
    if constexpr (EXT) {
      if (a.key_out && rank < a.k) a.key_out[row * a.out_stride + a.out_off + rank] = ke;
    }
  }
  if constexpr (PASS) {
    if (!a.floor_key_out)
      for (int t = a.k + lane; t < a.out_stride - a.out_off; t += 64) { oi[t] = -1; ov[t] = kNegInf; }
  } else {
    for (int t = a.k + lane; t < a.out_stride; t += 64) { oi[t] = -1; ov[t] = kNegInf; }
  }
}

}  // namespace mmf

#endif  // MMF_RERANK_COMBINED_H
