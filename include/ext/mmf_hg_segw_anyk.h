/* mmf_hg_segw_anyk.h — the segmented wide 16-bit top-k for any k: what mmf_simtopk_segmented_exact answers for a
 * ragged batch, for any k >= 1 at 1024 < d <= 4096, with the candidates of EVERY pass taken from the wide 16-bit scan.
 * mmf_simtopk_segmented_wide (mmf_hg_wide_seg.h) stops at one pass (k + self <= 20) and mmf_simtopk_segmented_fast_anyk
 * (mmf_hg_seg_anyk.h) at d = 1024; this entry runs the passes of the latter over the former's segment-padded images and work table:
 * each later pass scans under a ceiling per operand position derived from the row's floor with the wide scan's margin
 * (mmf_simtopk_wide_anyk, mmf_hg_wide_anyk.h), and the exact re-rank drops the already-emitted columns that slip
 * under it.  An addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, host offsets,
 * `device_id`, `hip_stream`, mmf_last_error); bound from the list SEGW_ANYK_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: per segment, bit for bit (ids and values), that of mmf_simtopk_segmented_exact — i.e. of mmf_simtopk_ex with
 * MMF_PREC_EXACT, row_offset = x_ptr[s], col_offset = y_ptr[s]: out_idx (global rows of Y) / out_val [n, k], canonical key
 * descending, then id ascending.  A segment with fewer than k admissible columns gets those first, then -1 / -inf (it is answered by
 * the exact launch loop, as in mmf_simtopk_segmented_wide); an empty segment is skipped.
 *
 * Workspace, cached per (device, stream): that of mmf_simtopk_segmented_wide at depth 20, plus per row 8 bytes of floors, 12 bytes
 * of per-pass bookkeeping, 4 bytes of segment offsets and a staging row of 20 x 16 bytes, and 4 bytes of ceiling per position of the
 * padded query image; when rows take the exact rescan, in the second slot the f32 image of Y and of those rows.
 *
 * Host-synchronous: once per pass (the re-rank's fail counts and the yield histogram travel together); once more in a pass that
 * sends rows to the exact rescan (the rows are read to the host and grouped per segment: two launches per segment with such rows).
 */
#ifndef MMF_HG_SEGW_ANYK_H
#define MMF_HG_SEGW_ANYK_H

#include "mmf_hg_fast_anyk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mmf_simtopk_segmented_fast_anyk (`info`: host pointer, may be NULL; exact_rows[p] counts rows of SERVED segments
 * only: those with rows and at least k admissible columns).  opts (may be NULL): precision MMF_PREC_FAST (f16 operands) /
 * MMF_PREC_FAST_BF16 run the passes, MMF_PREC_AUTO means MMF_PREC_FAST, MMF_PREC_EXACT forwards to mmf_simtopk_segmented_exact's
 * behaviour (info: one pass); col_splits 0 (automatic: one range per segment) or a power of two, the column ranges every segment is
 * scanned in (at most one per 128 columns of the segment, and as many as the re-rank's capacity per row holds at 32-entry lists) — the
 * work table is built once, at depth 20, and every pass launches it; select_wait_event is refused; query_order is ignored (off).
 * k + self <= 20: the call IS mmf_simtopk_segmented_wide — same launches, same bits (info: one pass).
 * bf16 operands are served but lose: their margin is eight times f16's, so several already-emitted columns per row
 * slip under the ceiling and shrink every later pass's yield, and most rows' margin bands outgrow a 32-entry list on a schedule
 * without overflow lists, where a row whose lists crowd is flagged for the exact rescan.
 * One yield per pass for the whole call; MMF_ANYK_SHORT_DIV (environment, read per call, default 64, 1 .. 65536): a pass emits
 * the largest yield that leaves at most n_served / MMF_ANYK_SHORT_DIV unflagged rows short of it; results do not depend on it.  A
 * yield below 1, or the 15th pass, finishes every served row by the exact scan from its floor.  A served segment with fewer unemitted
 * columns than a pass is deep stays in the work table: its lists come up short, the re-rank flags its rows and they take the rescan.
 * stats (may be NULL): those of the first pass, with fallback_rows summed over the passes.
 * Checked on the host before any device call, every message naming the entry: the refusals of mmf_simtopk_segmented_wide in its
 * order and wording (device_id < 0 first; shapes, dtype, NULL X, metric, lambda, k, offsets, NULL Y, col_splits -> MMF_E_INVALID,
 * select_wait_event -> MMF_E_UNSUPPORTED; k + self > 44 is NOT refused here), a precision outside the four values ->
 * MMF_E_INVALID; then d <= 1024 -> MMF_E_UNSUPPORTED in a message naming mmf_simtopk_segmented_fast_anyk, d > 4096 under a fast
 * precision -> MMF_E_UNSUPPORTED, NULL outputs -> MMF_E_INVALID.  n == 0 is a no-op. */
int mmf_simtopk_segmented_wide_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                    float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                    int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                    mmf_simtopk_stats* stats, int device_id, void* hip_stream, mmf_fast_anyk_info* info);

/* Host only (no device): how the entry above serves (d, k, exclude_self) under MMF_PREC_FAST: the answers of mmf_wide_anyk_plan
 * (mmf_hg_wide_anyk.h) — returns 1 where the call runs more than one pass, 0 where a single pass serves
 * (mmf_simtopk_segmented_wide), with *scan_kk / *first_yield / *min_passes as there (each may be NULL); d <= 1024 and d > 4096:
 * MMF_E_UNSUPPORTED; d < 1 or k < 1: MMF_E_INVALID. */
int mmf_segmented_wide_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_SEGW_ANYK_H */
