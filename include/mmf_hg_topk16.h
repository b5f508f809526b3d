/* mmf_hg_topk16.h — the top-k of the combined similarity K = K_h * K_g on the 16-bit matrix cores: the result
 * of mmf_simtopk_combined (mmf_hg_topk.h) for ONE graph, bit for bit, from an f16 / bf16 candidate scan, an exact re-rank and
 * an exact answer for the rows the scan could not certify.  An addition to ABI version 3 of mmf_hg.h, whose conventions hold
 * (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list EXPORTS_TOPK16 of
 * multimodal-fusion_amd/_lib.py.
 *
 * Output contract: identical to mmf_simtopk_combined, indices and values.  With chain and sq_from of mmf_hg.h,
 *     eh = (-lambda_h) * sq_from(chain(f_i,f_i), chain(f_j,f_j), chain(f_i,f_j))     eg likewise over P (dp terms)
 *     key_ij = eh + eg                     (one f32 add)         val_ij = expf(eh) * expf(eg)
 *     rank: key descending, then column id ascending; self dropped by identity when exclude_self;
 *     a row short of admissible columns gets those first, then id -1 and value -inf.
 * How: the 16-bit images of the features (the MMF_RBF images of the 16-bit scan, a common power-of-two scale) give an
 * approximate feature exponent; the position exponent is formed canonically in the scan's epilogue, so only the feature term is
 * approximate.  Every column whose approximate key lies within a proven margin of the row's k-th best is kept (lists of 16
 * entries per lane for k + self <= 11, 32 for 12..20), the re-rank recomputes key and value of every kept column with the
 * canonical f32 chains, and a row whose margin band did not fit its lists is flagged and answered by the exact f32 scan of
 * mmf_simtopk_combined over its 128-row block (all rows when more than a quarter of the blocks hold one).
 *
 * Limits: f32 inputs, one graph, k + self <= 20, 1 <= d <= 4096, dp <= 8, n < 2^31.
 *
 * Workspace, cached per (device, stream): the 16-bit image of F (2 bytes x d rounded up to 128 per row), 8 bytes per row of
 * chains, the candidate lists (2 * col_splits lists of 16 or 32 entries per row, with their keys when col_splits > 1), and
 * 768 bytes per row of the shared list block's unused overflow slots; when rows were flagged, in a second block, the f32 image
 * of F and the exact pass's lists.  Nothing grows with n * n.
 *
 * Host-synchronous: once per call (the re-rank's fail count, with the first 1024 flagged row ids); when rows were flagged, once
 * more for the exact pass's fail count, and once in between if more than 1024 rows were flagged.
 */
#ifndef MMF_HG_TOPK16_H
#define MMF_HG_TOPK16_H

#include "mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The argument list of mmf_simtopk_combined, so the two can be swapped.  out_idx [n,k] int64, out_val [n,k] f32 (device).
 * ptr_host / n_segments must be NULL, 0: ragged batches stay on mmf_simtopk_combined.
 * opts (may be NULL): precision MMF_PREC_FAST = f16 operands, MMF_PREC_FAST_BF16 = bf16 operands, MMF_PREC_EXACT = the exact
 * scan of mmf_simtopk_combined unchanged, MMF_PREC_AUTO = the f16 scan in the range DESIGN.md §4.17 measured it to pay
 * (512 <= d <= 1536, k + self <= 11), else the exact one; col_splits (rounded up to a power of two, bounded by the re-rank's
 * 1024 candidates per row) and profile are honoured, the rest is ignored.  stats (may be NULL): precision_used (what ran), col_splits, scan_grid, candidates,
 * fallback_rows (rows flagged by the scan or the re-rank), overflow_rows / short_rows (why), and under profile prep_ms /
 * scan_ms / rerank_ms / fallback_ms (the exact pass over the flagged rows' blocks).
 * Checked on the host before any device call, every message naming the entry and the argument: device_id < 0 ->
 * MMF_E_UNSUPPORTED first; MMF_E_INVALID for n < 0, d < 1, dp < 1, k < 1, a negative or non-finite lambda, a NULL F / P /
 * out_idx / out_val with n > 0, an unknown precision, col_splits < 0; MMF_E_UNSUPPORTED for a ragged batch, dp > 8,
 * k + self > 20, d > 4096, n >= 2^31.  n == 0 is a no-op.  A lambda of 0 is valid and drops its term. */
int mmf_simtopk_combined_fast(const float* F, const float* P, int64_t n, int64_t d, int64_t dp,
                              float lambda_h, float lambda_g, int k, int exclude_self,
                              const int64_t* ptr_host, int64_t n_segments,
                              int64_t* out_idx, float* out_val,
                              const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                              int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_TOPK16_H */
