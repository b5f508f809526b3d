/* mmf_hg_topk16_seg.h — the 16-bit top-k of the combined similarity K = K_h * K_g for every graph of a ragged batch in one call
 * (DESIGN.md §4.18): the result of mmf_simtopk_combined (mmf_hg_topk.h) with ptr_host / n_segments, bit for bit, from ONE
 * table-driven launch of the f16 / bf16 candidate scan of mmf_simtopk_combined_fast (mmf_hg_topk16.h), one exact re-rank over all
 * rows, and the exact scan for the rows the 16-bit scan could not certify.  An addition to ABI version 3 of mmf_hg.h, whose
 * conventions hold (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list
 * EXPORTS_TOPK16_SEG of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: identical to mmf_simtopk_combined's for the same offsets, indices and values — key_ij = eh + eg, val_ij =
 * expf(eh) * expf(eg), rank by key descending, then column id ascending; a row only ever gets columns of its own segment, as
 * global row ids; a segment with fewer than k admissible columns gets those first, then id -1 and value -inf.
 * How: every segment with at least k admissible columns is copied into one 16-bit operand image, padded to a multiple of 128
 * rows (padding: zero operands, bias -inf), so a block of 128 queries never straddles two segments and a tile of 128 candidates
 * never holds another segment's columns.  A host-built work table (8 x int32 per workgroup: the block's image position, its row
 * of F, its real queries, the tile range, the id offset, the list slot and the segment's last row) replaces the block index; the
 * scale, the maxima and the largest position chain of the error margin are taken over all rows of the batch, a superset of any
 * one segment, so the margin is at least a per-segment call's.  Segments short of columns, and every segment under
 * MMF_PREC_EXACT, are slices of the exact pass of mmf_simtopk_combined; flagged rows are answered per segment by that pass over
 * their 128-row blocks (counted from the segment's first row, adjacent blocks merged; the whole segment when more than a quarter
 * of its blocks hold a flagged row).
 *
 * Limits: f32 inputs, k + self <= 20, 1 <= d <= 4096, dp <= 8, n < 2^31.
 *
 * Workspace, cached per (device, stream): the 16-bit image (2 bytes x d rounded up to 128 per position), 8 bytes per row of
 * chains, 4 bytes per position of gather table, 32 bytes per workgroup of work table, the candidate lists (2 x the largest range
 * count lists of 16 or 32 entries per row, with their keys when a segment is split); in a second block the f32 image of F and the
 * exact pass's lists when a segment or a flagged row goes there.  Nothing grows with n * n.
 *
 * Host-synchronous: data-dependent — once per call (the re-rank's fail count with the first 1024 flagged row ids); once more for
 * the exact pass's fail count when a segment or a flagged row went there, and once in between if more than 1024 rows were flagged.
 * ptr_host is read on the host during the call.
 */
#ifndef MMF_HG_TOPK16_SEG_H
#define MMF_HG_TOPK16_SEG_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The argument list of mmf_simtopk_combined.  ptr_host [n_segments + 1] host int64 offsets, required: they start at 0, do not
 * decrease and end at n; empty segments are allowed; n_segments >= 0.  out_idx [n,k] int64, out_val [n,k] f32 (device).
 * opts (may be NULL): precision MMF_PREC_FAST = f16 operands, MMF_PREC_FAST_BF16 = bf16 operands, MMF_PREC_EXACT = the exact pass
 * for every segment, MMF_PREC_AUTO = the f16 scan in the range DESIGN.md §4.18 measured it to pay (512 <= d <= 1536, k + self <=
 * 11), else the exact pass; col_splits: 0 (automatic: at most two) or a power of two — every segment is cut into at most that
 * many column ranges, at most one per tile of the segment, bounded by the re-rank's 1024 candidates per row; profile is
 * honoured, the rest is ignored.  stats (may be NULL): precision_used, col_splits (the largest range
 * count of a segment), scan_grid (work-table entries), candidates, fallback_rows (rows of served segments the scan or the re-rank
 * flagged), overflow_rows / short_rows (why), and under profile prep_ms / scan_ms / rerank_ms / fallback_ms.
 * Checked on the host before any device call, every message naming the entry and the argument: device_id < 0 ->
 * MMF_E_UNSUPPORTED first; MMF_E_INVALID for n < 0, d < 1, dp < 1, k < 1, a negative or non-finite lambda, a NULL F / P /
 * out_idx / out_val with n > 0, bad offsets, an unknown precision, a col_splits that is negative or no power of two;
 * MMF_E_UNSUPPORTED for dp > 8, k + self > 20, d > 4096, n >= 2^31.  n == 0 is a no-op.  A lambda of 0 is valid and drops its term. */
int mmf_simtopk_combined_fast_segmented(const float* F, const float* P, int64_t n, int64_t d, int64_t dp,
                                        float lambda_h, float lambda_g, int k, int exclude_self,
                                        const int64_t* ptr_host, int64_t n_segments,
                                        int64_t* out_idx, float* out_val,
                                        const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                                        int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_TOPK16_SEG_H */
