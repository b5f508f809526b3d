/* mmf_hg_seg_exact.h — the exact f32 top-k for every segment of a ragged batch from ONE table-driven launch of the exact scan
 * (DESIGN.md §4.20), for the rows the 16-bit scans cannot serve: MMF_PREC_EXACT, k + self > 20 above d = 512, d > 4096, and the
 * exact form of mmf_simtopk_combined with offsets.  mmf_simtopk_segmented and mmf_simtopk_combined answer such a batch with one
 * scan and one re-rank per segment, one after the other; these entries build a host work table (one workgroup per block of 128
 * rows of a segment and column range), upload it, and issue one scan and one re-rank over all rows.  An addition to ABI version 3
 * of mmf_hg.h, whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the
 * list EXPORTS_SEG_EXACT of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: per segment s, bit for bit, mmf_simtopk_ex(precision = exact, row_offset = x_ptr[s], col_offset = y_ptr[s]) —
 * indices are rows of all of Y (of X for a self call), ranked by canonical key descending, then id ascending; a row only ever
 * gets columns of its own segment; a segment with fewer than k admissible columns gets those first, then id -1 and value -inf
 * (such segments, if any, are answered by the launch loop of mmf_simtopk_segmented, after the table-driven launch).
 *
 * Workspace, cached per (device, stream): the f32 image of Y (and of X unless X is Y; 4 bytes x d rounded up to 32 per row), 4
 * bytes per row of scalars, 64 bytes per workgroup of work table, and per row 2 x (largest range count) lists of 16 / 32 / 48 ids.
 *
 * Host-synchronous: once per call, for the re-rank's fail counts (an internal invariant: the exact lists cannot overflow); once
 * more when a segment is short of k admissible columns.  The offsets are read on the host during the call.
 */
#ifndef MMF_HG_SEG_EXACT_H
#define MMF_HG_SEG_EXACT_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The argument list of mmf_simtopk_segmented.  Y NULL: X against itself (m and y_ptr_host ignored).  Any d, f32 / bf16 / f16
 * rows, the four metrics of mmf_simtopk, any k >= 1: k + self > 44 runs passes of at most 44 entries, each one scan launch with
 * per-row floors and one re-rank.  opts (may be NULL): precision MMF_PREC_AUTO or MMF_PREC_EXACT (both: this exact scan);
 * col_splits 0 (automatic: runs of column tiles sized so that the call makes about 1024 workgroups — many segments are one
 * range each, a few large ones are split) or a power of two: every served segment is cut into at most that many column ranges,
 * at most one per 128 columns of the segment, bounded by the re-rank's 1024 candidates per row; profile is honoured, the rest
 * is ignored.  stats (may be NULL): precision_used = MMF_PREC_EXACT, col_splits = the largest range count of a segment,
 * scan_grid = work-table entries, candidates, and under profile prep_ms / scan_ms / rerank_ms.
 * Checked on the host before any device call, every message naming the entry: device_id < 0 -> MMF_E_UNSUPPORTED first;
 * MMF_E_INVALID for bad shapes or dtype, a NULL X (n > 0), Y (m > 0) or output, a bad metric, MMF_RBF without lambda > 0, k < 1,
 * bad offsets, a col_splits that is negative or no power of two; MMF_E_UNSUPPORTED for MMF_PREC_FAST / _FAST_BF16 and n or m >=
 * 2^31.  n == 0 is a no-op. */
int mmf_simtopk_segmented_exact(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                mmf_simtopk_stats* stats, int device_id, void* hip_stream);

/* The argument list of mmf_simtopk_combined (mmf_hg_topk.h) with ptr_host required: the top-k of K_h * K_g of every graph of a
 * batch, bit for bit mmf_simtopk_combined(ptr_host), from one launch of the exact scan with the combined key and one re-rank over
 * all rows.  k + self <= 44 (the combined re-rank has no floors); f32 rows, dp <= 8; opts / stats as above.  The host checks are
 * those of mmf_simtopk_combined, plus col_splits 0 or a power of two. */
int mmf_simtopk_combined_segmented_exact(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                                         float lambda_g, int k, int exclude_self, const int64_t* ptr_host, int64_t n_segments,
                                         int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                                         int device_id, void* hip_stream);

/* Host only (no device, no stream): the work table of the two entries above for the offsets x_ptr_host / y_ptr_host (NULL: the
 * self call), k, exclude_self and col_splits.  Entry e is table_host[8 e .. 8 e + 7] = segment, first row of X, real queries (<=
 * 128), first row of the segment in Y, first and end tile (of 128 columns, inside the segment), number of the column range,
 * columns of the segment.  Returns the entry count (>= 0) and writes the entries when table_host is not NULL and `capacity`
 * entries hold them, and the list slots per row (2 x the largest range count) into *lists_out when that is not NULL; a negative
 * status for bad offsets, k < 1, a bad col_splits or too small a capacity. */
int64_t mmf_segmented_exact_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int k, int exclude_self,
                                  int col_splits, int64_t* table_host, int64_t capacity, int* lists_out);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_SEG_EXACT_H */
