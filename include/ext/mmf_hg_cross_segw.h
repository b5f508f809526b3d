/* mmf_hg_cross_segw.h — the cross-segment top-k on the WIDE 16-bit scan: what mmf_simtopk_cross_segments
 * (mmf_hg_cross_seg.h) answers — for every row of a ragged batch, the k best columns among the rows of all OTHER segments — for
 * feature dims above 1024, where mmf_simtopk_cross_segments_fast (mmf_hg_cross_seg16.h) stops: 1024 < d <= 4096 with k <= 20.  The
 * candidates come from the k-streamed wide scan on the PLAIN 16-bit images of both sides (column = row of Y, no
 * segment padding, no id map) and are re-ranked exactly; what makes the scan cross-segment is a per-row column mask in its epilogue
 * and a work table that leaves out the tiles every row of a block excludes.  An addition to ABI version 3 of mmf_hg.h, whose
 * conventions hold (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list
 * CROSS_SEGW_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: that of mmf_simtopk_cross_segments, bit for bit (ids and values) — ids are rows of all of Y, order is canonical
 * key descending, then id ascending; no -1 / -inf fill.  Rows the 16-bit path cannot certify (an audited loss, a list that came up
 * short) are redone by the exact cross-segment scan, all of them in one launch.  There are no overflow lists on this path: a row
 * with more columns inside its margin band than a list holds is such a row.
 *
 * Workspace, cached per (device, stream): the 16-bit image of Y (and of X unless X is Y) at the dim padded to 128, 4 bytes per row
 * of scalars, 8 bytes per row of mask bounds, 32 bytes per workgroup of work table, per row 2 x (largest entry count of a row
 * block) lists of 16 (k <= 11) or 32 ids — with their keys when a block has more than one entry; when rows are flagged, in the
 * second slot the f32 image of Y and of the flagged rows.
 *
 * Host-synchronous: once per call, for the re-rank's fail counts; once more only when rows were flagged.  The offsets are read on
 * the host during the call.
 */
#ifndef MMF_HG_CROSS_SEGW_H
#define MMF_HG_CROSS_SEGW_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mmf_simtopk_cross_segments (Y NULL: X against itself with y_ptr = x_ptr).  opts (may be NULL): precision
 * MMF_PREC_FAST (f16 operands) or MMF_PREC_FAST_BF16 takes the wide 16-bit scan, MMF_PREC_AUTO means MMF_PREC_FAST where the wide
 * scan serves (d, k) and the exact driver elsewhere (it does NOT forward to mmf_simtopk_cross_segments_fast: routing between the
 * two 16-bit entries is the caller's), MMF_PREC_EXACT forwards to the exact driver of mmf_simtopk_cross_segments; col_splits 0
 * (automatic) or a power of two, the runs the admissible tiles of every row block are cut into; select_wait_event is refused;
 * query_order is ignored (off); profile is honoured.  The wide scan serves 1024 < d <= 4096 with k <= 20 (there is no self to
 * exclude: mmf_wide_scan_supported(d, k, 0)); elsewhere MMF_PREC_FAST / _FAST_BF16 return MMF_E_UNSUPPORTED with a message naming d
 * and k.  Operands are f16 or bf16 roundings of rows of any of the three dtypes, for all four metrics.
 * stats (may be NULL): precision_used 2 / 3 (1 where the exact driver ran), scan_grid = work-table entries, col_splits = the
 * largest entry count of a row block, candidates, fallback_rows (rows redone exactly), overflow_rows / short_rows, and under
 * profile prep_ms / scan_ms / rerank_ms / fallback_ms.
 * Checked on the host before any device call, every message naming the entry (simtopk_cross_segments_wide): the refusals of
 * mmf_simtopk_cross_segments in its order and wording (device_id < 0 first; shapes, dtype, NULL operands or outputs, metric,
 * lambda, k, offsets, col_splits, the "segment %lld has %lld admissible columns" refusal), a precision outside the four values ->
 * MMF_E_INVALID, select_wait_event -> MMF_E_UNSUPPORTED, an unserved (d, k) under MMF_PREC_FAST / _FAST_BF16 ->
 * MMF_E_UNSUPPORTED.  n == 0 is a no-op. */
int mmf_simtopk_cross_segments_wide(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                    float lambda, int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments,
                                    int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                                    int device_id, void* hip_stream);

/* Host only (no device, no stream): the work table the entry above launches for the offsets x_ptr_host / y_ptr_host (NULL: the
 * self call), the feature dim d, k and col_splits.  Row blocks are 128 consecutive rows of X, whatever the segments; column tiles
 * are the 128-row tiles of the plain image of Y (m rounded up to 256 rows).  Entry e is table_host[8 e .. 8 e + 7], int32:
 *   0, 1  first row of the block (operand position = list row)      2  real queries (<= 128)
 *   3, 4  first and end tile                                        5  first tile of the entry's mask window
 *   6     first list slot of the entry: 2 x its number among its block's entries, in tile order
 *   7     end tile of the mask window (words 5 and 7 equal: no tile of the entry needs the mask)
 * A tile every row of the block excludes is in no entry; a run that would span such tiles is two entries.  Entries come longest
 * run first.  Automatic col_splits: the smallest power of two R with (row blocks) x R >= 256, no run shorter than 8 tiles; forced
 * or automatic, R is at most 16 (k <= 11) or 8, so that a row's lists fit the re-rank.
 * Returns the entry count (>= 0) and writes the entries when table_host is not NULL and `capacity` entries hold them, and the
 * list slots per row (2 x the largest entry count of a row block) into *lists_out when that is not NULL; a negative status for
 * bad offsets, k < 1, a bad col_splits, too small a capacity, or (MMF_E_UNSUPPORTED) a (d, k) the wide scan does not serve. */
int64_t mmf_cross_segments_wide_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int64_t d, int k,
                                      int col_splits, int32_t* table_host, int64_t capacity, int* lists_out);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_CROSS_SEGW_H */
