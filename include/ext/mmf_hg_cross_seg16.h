/* mmf_hg_cross_seg16.h — the cross-segment top-k on the 16-bit scan: what mmf_simtopk_cross_segments
 * (mmf_hg_cross_seg.h) answers — for every row of a ragged batch, the k best columns among the rows of all OTHER segments — with
 * the candidates generated on the 16-bit matrix cores and re-ranked exactly.  A cross-segment answer walks (almost) all of Y, so
 * the scan runs on the PLAIN 16-bit images of both sides (column = row of Y, no segment padding, no id map); what makes it
 * cross-segment is a column mask in the scan's epilogue that differs per query row, and a work table that leaves out the tiles
 * every row of a block excludes.  An addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device
 * pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list CROSS_SEG16_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: that of mmf_simtopk_cross_segments, bit for bit (ids and values) — ids are rows of all of Y, order is canonical
 * key descending, then id ascending; no -1 / -inf fill.  Rows the 16-bit path cannot certify (an audited loss, a full overflow
 * list, a list that came up short) are redone by the exact cross-segment scan, all of them in one launch.
 *
 * Workspace, cached per (device, stream): the 16-bit image of Y (and of X unless X is Y), 4 bytes per row of scalars, 8 bytes
 * per row of mask bounds, 32 bytes per workgroup of work table, per row 2 x (largest entry count of a row block) lists of 15 /
 * 16 / 32 ids and an overflow list of 192; when rows are flagged, in the second slot the f32 image of Y and of the flagged rows.
 *
 * Host-synchronous: once per call, for the re-rank's fail counts; once more only when rows were flagged.  The offsets are read on
 * the host during the call.
 */
#ifndef MMF_HG_CROSS_SEG16_H
#define MMF_HG_CROSS_SEG16_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mmf_simtopk_cross_segments (Y NULL: X against itself with y_ptr = x_ptr).  opts (may be NULL): precision
 * MMF_PREC_FAST (f16 operands) or MMF_PREC_FAST_BF16 takes the 16-bit scan, MMF_PREC_AUTO means MMF_PREC_FAST, MMF_PREC_EXACT
 * forwards to the exact driver of mmf_simtopk_cross_segments; col_splits 0 (automatic) or a power of two, the runs the admissible
 * tiles of every row block are cut into; select_wait_event is refused; query_order is ignored (off); profile is honoured.  The
 * 16-bit scan serves d <= 1024 with k <= 20 and d <= 512 with k <= 44 (mmf_fast_scan_supported(d, k, 0)); elsewhere
 * MMF_PREC_FAST / _FAST_BF16 return MMF_E_UNSUPPORTED with a message naming d and k, and MMF_PREC_AUTO runs the exact driver.
 * stats (may be NULL): precision_used 2 / 3 (1 where the exact driver ran), scan_grid = work-table entries, col_splits = the
 * largest entry count of a row block, candidates, fallback_rows (rows redone exactly), overflow_rows / short_rows, and under
 * profile prep_ms / scan_ms / rerank_ms / fallback_ms.
 * Checked on the host before any device call, every message naming the entry: the refusals of mmf_simtopk_cross_segments in its
 * order and wording (device_id < 0 first; shapes, dtype, NULL operands or outputs, metric, lambda, k, offsets, col_splits, the
 * "segment %lld has %lld admissible columns" refusal), a precision outside the four values -> MMF_E_INVALID, select_wait_event
 * -> MMF_E_UNSUPPORTED, an unserved (d, k) under MMF_PREC_FAST / _FAST_BF16 -> MMF_E_UNSUPPORTED.  n == 0 is a no-op. */
int mmf_simtopk_cross_segments_fast(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                    float lambda, int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments,
                                    int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                                    int device_id, void* hip_stream);

/* Host only (no device, no stream): the work table the entry above launches for the offsets x_ptr_host / y_ptr_host (NULL: the
 * self call), the feature dim d, k and col_splits.  Row blocks are QT = 256 (d <= 512) or 128 (d <= 1024) consecutive rows of X,
 * whatever the segments; column tiles are the 32-row tiles of the plain image of Y.  Entry e is table_host[8 e .. 8 e + 7], int32:
 * first row of the block, the same again (operand position = list row), real queries (<= QT), first and end tile, list slot (the
 * entry's number among its block's entries, in tile order), first and end tile of its mask window (equal: none).  A tile every
 * row of the block excludes is in no entry; a run that would span such tiles is two entries.  Entries come longest run first.
 * Returns the entry count (>= 0) and writes the entries when table_host is not NULL and `capacity` entries hold them, and the
 * list slots per row (2 x the largest entry count of a row block) into *lists_out when that is not NULL; a negative status for
 * bad offsets, k < 1, a bad col_splits, too small a capacity, or (MMF_E_UNSUPPORTED) a (d, k) the 16-bit scan does not serve. */
int64_t mmf_cross_segments_fast_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int64_t d, int k,
                                      int col_splits, int32_t* table_host, int64_t capacity, int* lists_out);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_CROSS_SEG16_H */
