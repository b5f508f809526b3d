/* mmf_hg_topk_anyk.h — the top-k of the combined similarity K = K_h * K_g for ANY k.  mmf_simtopk_combined
 * (mmf_hg_topk.h), mmf_simtopk_combined_segmented_exact (mmf_hg_seg_exact.h) and mmf_simtopk_combined_xy (mmf_hg_topk_xy.h)
 * refuse k + self > 44, what one pass of the exact scan's lists holds; these entries run as many passes as k needs: each pass
 * is one exact scan that offers only what ranks after the per-row floor (key, id) where the previous pass ended, and one
 * re-rank that writes its entries behind the previous pass's columns and records the next floor — the pass loop the plain key
 * has had since mmf_simtopk_ex took k + self > 44.  An addition to ABI version 3 of mmf_hg.h, whose conventions hold (status
 * codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list EXPORTS_TOPK_ANYK of
 * multimodal-fusion_amd/_lib.py.
 *
 * Output contract: per row, the first k entries of the total order (key descending, reported id ascending) over the admissible
 * columns of its segment (of the candidates, for the two-set entry); key_ij = eh + eg and val_ij = expf(eh) * expf(eg) from the
 * canonical fmaf chains, so the values are bitwise the entries of mmf_sim_dense_combined; a pair is dropped iff exclude_self and
 * the two reported ids are equal; a row with fewer than k admissible columns gets them first, then id -1 and value -inf.  For
 * k + self <= 44 the output is bit for bit the corresponding existing entry's (one pass, the same launches).  For any k' >= k
 * the first k columns of the k' result are the k result: a pass boundary is a cut in one total order, not a new ranking.
 *
 * Workspace, cached per (device, stream): that of the corresponding existing entry, plus 8 bytes per row of floors when
 * k + self > 44.  Nothing grows with k beyond the outputs.
 *
 * Host-synchronous: mmf_simtopk_combined_anyk with offsets once (the re-rank's fail counts of all passes, an internal
 * invariant), once more when a segment is short of k admissible columns; without offsets, and mmf_simtopk_combined_xy_anyk, once
 * (the exact pass's fail count), and once per earlier piece when the pieces of a call do not fit one set of lists.  ptr_host is
 * read on the host during the call and may be freed when it returns.
 */
#ifndef MMF_HG_TOPK_ANYK_H
#define MMF_HG_TOPK_ANYK_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The argument list of mmf_simtopk_combined.  ptr_host NULL and n_segments 0: one graph, the launch loop of
 * mmf_simtopk_combined with its passes.  Offsets given: every segment with rows and at least k admissible columns from the
 * table-driven launch of mmf_simtopk_combined_segmented_exact, one scan and one re-rank over all rows per pass; the segments
 * short of k columns keep the launch loop.  Any k >= 1; f32 rows, dp <= 8.  opts (may be NULL): precision MMF_PREC_AUTO or
 * MMF_PREC_EXACT (both: the exact scan); col_splits as the corresponding existing entry (with offsets: 0 or a power of two);
 * profile is honoured, the rest is ignored.  stats (may be NULL) as the existing entries; with several passes scan_ms covers the
 * whole pass loop and rerank_ms is 0.
 * Checked on the host before any device call, every message naming the entry and the argument: device_id < 0 ->
 * MMF_E_UNSUPPORTED first; MMF_E_INVALID for n < 0, d < 1, dp < 1, k < 1, a negative or non-finite lambda, a NULL F / P /
 * out_idx / out_val with n > 0, bad offsets, a negative col_splits (with offsets: one that is no power of two);
 * MMF_E_UNSUPPORTED for dp > 8, n >= 2^31, MMF_PREC_FAST / _FAST_BF16.  n == 0 is a no-op. */
int mmf_simtopk_combined_anyk(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g, int k,
                              int exclude_self, const int64_t* ptr_host, int64_t n_segments, int64_t* out_idx, float* out_val,
                              const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream);

/* The argument list of mmf_simtopk_combined_xy: queries against candidates, ids row_offset + i and col_offset + j, the row-slice
 * recognition and the nc == 0 fill of that entry.  Any k >= 1.  Precision MMF_PREC_AUTO or MMF_PREC_EXACT both mean the exact
 * scan; MMF_PREC_FAST / _FAST_BF16 return MMF_E_UNSUPPORTED (the 16-bit combined scans stop at k + self = 20).  The other host
 * checks are those of mmf_simtopk_combined_xy under this entry's name, minus the k + self > 44 refusal. */
int mmf_simtopk_combined_xy_anyk(const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc,
                                 int64_t d, int64_t dp, float lambda_h, float lambda_g, int k, int exclude_self,
                                 int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                                 const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_TOPK_ANYK_H */
