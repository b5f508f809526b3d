// mmf_topk_anyk.hip — the re-rank of the combined key for the passes of mmf_simtopk_combined_fast_anyk
// (include/ext/mmf_hg_topk16_anyk.h): the EXT instantiations of rerank_combined_kernel (mmf_rerank_combined.h).
// launch_rerank_combined (mmf_topk.hip) keeps its kernels and its refusal of gathered rows; this launcher adds the two things
// launch_select already has for the plain key:
//   * p.row_ids — list position pos is row row_ids[pos] of the queries: the exact rescan of the rows a pass could not finish runs
//     over gathered rows (ExactPass, mmf_api.hip; the exact scan of the combined key takes them as it is);
//   * p.key_out — the canonical combined key of every emitted entry, laid out like out_val: a later pass re-ranks into staging
//     rows, and anyk_count_kernel / anyk_emit_kernel (mmf_fast_anyk.hip) compare those keys with the row's floor.
#include "mmf_dev.h"
#include "mmf_host.h"
#include "mmf_rerank_combined.h"

namespace mmf {

int launch_rerank_combined_ext(const SelectProblem& p, const CandLists& L, hipStream_t s) {
  if (p.n_rows <= 0) return MMF_OK;
  const int stride = p.out_stride ? p.out_stride : p.k;
  if (p.dtype != MMF_F32 || p.perm || !p.Pq || !p.Pc || !p.pnq || !p.pnc || p.dp < 1 || p.dp > 8 || p.out_off < 0 || p.k < 1 ||
      p.out_off + p.k > stride || (p.floor_key_out && !p.floor_id_out) || L.lists * L.cap > RR_MAXC) {
    set_error("rerank_combined_ext: f32 rows (in order or gathered), both sides' positions (1 <= dp <= 8), columns inside the row, at most %d candidates per row", RR_MAXC);
    return MMF_E_INTERNAL;
  }
  RerankCombinedExtArgs a{};
  a.X = static_cast<const float*>(p.X); a.Y = static_cast<const float*>(p.Y); a.d = p.d; a.m = p.m;
  a.rx = p.rx; a.cy = p.cy; a.Pq = p.Pq; a.Pc = p.Pc; a.dp = p.dp; a.pnq = p.pnq; a.pnc = p.pnc;
  a.neg_lambda_h = -p.lambda; a.neg_lambda_g = -p.lambda_g;
  a.k = p.k; a.out_stride = stride; a.exclude_self = p.exclude_self;
  a.row_offset = p.row_offset; a.col_offset = p.col_offset; a.n_rows = p.n_rows;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.overflow = L.overflow; a.lists = L.lists; a.cap = L.cap;
  a.out_idx = p.out_idx; a.out_val = p.out_val;
  a.fail_rows = p.fail_rows; a.fail_count = p.fail_count; a.cand_total = p.cand_total;
  a.out_off = p.out_off; a.floor_key_out = p.floor_key_out; a.floor_id_out = p.floor_id_out;
  a.row_ids = p.row_ids; a.key_out = p.key_out;
  const dim3 grid((unsigned)((p.n_rows + RR_WAVES - 1) / RR_WAVES));
  const bool vec4 = (p.d % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.X) & 15) == 0) && ((reinterpret_cast<uintptr_t>(p.Y) & 15) == 0);
  if (vec4) hipLaunchKernelGGL((rerank_combined_kernel<true, true, true>), grid, dim3(64 * RR_WAVES), 0, s, a);
  else hipLaunchKernelGGL((rerank_combined_kernel<false, true, true>), grid, dim3(64 * RR_WAVES), 0, s, a);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf
