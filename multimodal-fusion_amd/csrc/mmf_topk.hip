// mmf_topk.hip — mmf_simtopk_combined (include/mmf_hg_topk.h): the k best columns per row of the combined
// similarity K = K_h * K_g (build_hypergraph/similarity_kernel.py:88-124) without the N x N matrix.
//
// The scan is the exact f32 scan with the combined key in its epilogue (mmf_scan_f32.hip, COMB); this file holds the re-rank
// of its lists and the entry with its host checks.  The driver is the exact pass of mmf_api.hip (run_simtopk_combined).
//
// Re-rank: one wave per row.  The row's 2 x col_splits exact lists hold every column of its final top-(k + self) (they are
// truncated by the final order, never by an approximation), so the wave recomputes key and value of each listed column with
// the canonical fmaf chains over F and P — the same pos_exponent / combined_key as the scan, so the same bits — drops the
// row itself by identity, and ranks by COUNTING: an entry's rank is the number of entries that beat it under better(), ranks
// are distinct because a column sits in one list only, and every entry of rank < k writes itself.  No sort, no rounds of k.
//
// k + self > 44 (mmf_simtopk_combined_anyk, include/ext/mmf_hg_topk_anyk.h) runs several passes of scan and
// re-rank: the PASS instantiations write a pass's entries behind the previous pass's columns and leave the per-row floor (key,
// local id) of the last entry for the next scan, as launch_select does for the plain key.
//
// The kernel itself lives in mmf_rerank_combined.h: mmf_topk_anyk.hip launches its EXT instantiations (gathered rows, staged keys).
#include <math.h>
#include <string.h>

#include <type_traits>

#include "mmf_dev.h"
#include "mmf_host.h"
#include "mmf_rerank_combined.h"

namespace mmf {

int launch_rerank_combined(const SelectProblem& p, const CandLists& L, hipStream_t s) {
  if (p.n_rows <= 0) return MMF_OK;
  const int stride = p.out_stride ? p.out_stride : p.k;
  if (p.dtype != MMF_F32 || p.row_ids || p.perm || !p.Pq || !p.Pc || !p.pnq || !p.pnc || p.dp < 1 || p.dp > 8 || p.out_off < 0 ||
      p.k < 1 || p.out_off + p.k > stride || (p.floor_key_out && !p.floor_id_out) || L.lists * L.cap > RR_MAXC) {
    set_error("rerank_combined: f32 rows in order, both sides' positions (1 <= dp <= 8), columns inside the row, at most %d candidates per row", RR_MAXC);
    return MMF_E_INTERNAL;
  }
  const bool pass = p.out_off != 0 || p.floor_key_out != nullptr;   // one pass of several: the kernel with out_off and floors
  RerankCombinedPassArgs a{};
  a.X = static_cast<const float*>(p.X); a.Y = static_cast<const float*>(p.Y); a.d = p.d; a.m = p.m;
  a.rx = p.rx; a.cy = p.cy; a.Pq = p.Pq; a.Pc = p.Pc; a.dp = p.dp; a.pnq = p.pnq; a.pnc = p.pnc;
  a.neg_lambda_h = -p.lambda; a.neg_lambda_g = -p.lambda_g;
  a.k = p.k; a.out_stride = stride; a.exclude_self = p.exclude_self;
  a.row_offset = p.row_offset; a.col_offset = p.col_offset; a.n_rows = p.n_rows;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.overflow = L.overflow; a.lists = L.lists; a.cap = L.cap;
  a.out_idx = p.out_idx; a.out_val = p.out_val;
  a.fail_rows = p.fail_rows; a.fail_count = p.fail_count; a.cand_total = p.cand_total;
  const dim3 grid((unsigned)((p.n_rows + RR_WAVES - 1) / RR_WAVES));
  const bool vec4 = (p.d % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.X) & 15) == 0) && ((reinterpret_cast<uintptr_t>(p.Y) & 15) == 0);
  if (pass) {
    a.out_off = p.out_off; a.floor_key_out = p.floor_key_out; a.floor_id_out = p.floor_id_out;
    if (vec4) hipLaunchKernelGGL((rerank_combined_kernel<true, true>), grid, dim3(64 * RR_WAVES), 0, s, a);
    else hipLaunchKernelGGL((rerank_combined_kernel<false, true>), grid, dim3(64 * RR_WAVES), 0, s, a);
  } else {
    const RerankCombinedArgs& a1 = a;
    if (vec4) hipLaunchKernelGGL(rerank_combined_kernel<true>, grid, dim3(64 * RR_WAVES), 0, s, a1);
    else hipLaunchKernelGGL(rerank_combined_kernel<false>, grid, dim3(64 * RR_WAVES), 0, s, a1);
  }
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_simtopk_combined(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g, int k,
                         int exclude_self, const int64_t* ptr_host, int64_t n_segments, int64_t* out_idx, float* out_val,
                         const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const char* who = "simtopk_combined";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (n < 0) { set_error("%s: n must be >= 0 (got %lld)", who, (long long)n); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (n > 0 && !F) { set_error("%s: F is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !P) { set_error("%s: P is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  const int64_t one_graph[2] = {0, n};
  const bool segmented = ptr_host != nullptr || n_segments != 0;
  if (segmented) MMF_TRY(check_offsets(who, "ptr_host", ptr_host, n_segments, 0, 0, n));
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  const int kk = k + (exclude_self ? 1 : 0);
  if (kk > 44) { set_error("%s: k + self = %d > 44 is not supported (the multi-pass floors are a follow-up)", who, kk); return MMF_E_UNSUPPORTED; }
  if (n >= (int64_t)1 << 31) { set_error("%s: n must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT) {
    set_error("%s: precision %d: only MMF_PREC_AUTO and MMF_PREC_EXACT (the 16-bit scan does not form this key)", who, prec);
    return MMF_E_UNSUPPORTED;
  }
  if (opts && opts->col_splits < 0) { set_error("%s: col_splits must be >= 0 (got %d)", who, opts->col_splits); return MMF_E_INVALID; }
  if (n == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }
  return run_simtopk_combined(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, segmented ? ptr_host : one_graph,
                              segmented ? n_segments : 1, out_idx, out_val, opts, stats, device_id, hip_stream);
}

}  // extern "C"
