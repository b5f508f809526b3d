/* mmf_hg_wide_seg.h — the segmented form of the wide 16-bit scan: block-diagonal k-NN over a ragged batch
 * whose feature dim lies above 1024, e.g. the patch graphs of every slide of a cohort embedded at d = 1280, 1536 or 2560.
 * mmf_simtopk_segmented (mmf_hg.h) keeps its behaviour — above d = 1024 it refuses MMF_PREC_FAST and sends every segment to
 * the exact pass, two launches per segment; the entry below serves those shapes with ONE launch of the wide scan, driven by a
 * host-built work table.
 *
 * An addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`,
 * mmf_last_error); bound from the list EXPORTS_WIDE_SEG of multimodal-fusion_amd/_lib.py.
 */
#ifndef MMF_HG_WIDE_SEG_H
#define MMF_HG_WIDE_SEG_H

#include "mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mmf_simtopk_segmented, with the same meaning: query rows [x_ptr[s], x_ptr[s+1]) of X are ranked only against
 * candidate rows [y_ptr[s], y_ptr[s+1]) of Y (Y == NULL: Y = X, y_ptr = x_ptr); out_idx [n,k] holds GLOBAL row ids of Y, a row
 * whose segment has fewer than k admissible columns gets them first, then id -1 / value -inf.
 *
 * Outputs are, bit for bit, those of one mmf_simtopk_ex per segment with row_offset = x_ptr[s] and col_offset = y_ptr[s].
 *
 * For 1024 < d <= 4096 and k + self <= 20 (mmf_wide_scan_supported of mmf_hg_wide.h) the 16-bit candidates come from the wide
 * scan in one launch: MMF_PREC_FAST and MMF_PREC_FAST_BF16 are accepted, MMF_PREC_AUTO resolves to MMF_PREC_FAST, and
 * opts->col_splits — 0 (automatic) or a power of two, anything else is MMF_E_INVALID — is honoured: every segment's columns
 * are scanned in that many ranges, at most one per 128 columns of the segment and at most 16 (k + self <= 11) or 8.  Segments
 * with fewer than k admissible columns, rows the scan cannot certify (stats.fallback_rows) and every segment under
 * MMF_PREC_EXACT go through the exact pass, as in mmf_simtopk_segmented.  stats: precision_used 2 or 3, col_splits = the
 * largest number of ranges of a segment, scan_grid = workgroups of the scan launch, near_rows = -1.
 *
 * For every other shape (d <= 1024, d > 4096, k + self > 20) and under MMF_PREC_EXACT the call IS mmf_simtopk_segmented, with
 * that entry's refusals and texts — a nonzero col_splits is MMF_E_UNSUPPORTED there, MMF_PREC_FAST beyond what the 16-bit scans
 * cover is MMF_E_UNSUPPORTED ("does not support").  opts->select_wait_event is refused (MMF_E_UNSUPPORTED) for every shape;
 * opts->query_order is ignored.
 *
 * All checks run on the host before any device call, every message naming the entry ("simtopk_segmented_wide") and the
 * argument: device_id < 0 -> MMF_E_UNSUPPORTED first; then shapes, dtype, metric, lambda, k, offsets, options, precision,
 * outputs.  n == 0 is a no-op.
 *
 * Host-synchronous: once per call, plus a copy of the flagged rows' ids (data dependent) when some rows need the exact pass,
 * as mmf_simtopk_segmented.  x_ptr_host / y_ptr_host are read during the call only. */
int mmf_simtopk_segmented_wide(const void* X, int64_t n, const void* Y, int64_t m, int64_t d,
                               int in_dtype, int metric, float lambda, int k, int exclude_self,
                               const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments,
                               int64_t* out_idx, float* out_val,
                               const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                               int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_WIDE_SEG_H */
