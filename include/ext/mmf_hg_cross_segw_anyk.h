/* mmf_hg_cross_segw_anyk.h — the wide 16-bit cross-segment top-k for any k: what mmf_simtopk_cross_segments
 * (mmf_hg_cross_seg.h) answers — for every row of a ragged batch, the k best columns among the rows of all OTHER segments — for
 * any k >= 1 at 1024 < d <= 4096, with the candidates of EVERY pass taken from the wide 16-bit scan.
 * mmf_simtopk_cross_segments_wide (mmf_hg_cross_segw.h) stops at one pass (k <= 20), and mmf_simtopk_cross_segments_fast_anyk
 * (mmf_hg_cross_seg_anyk.h) at d = 1024; this entry runs the passes of the latter over the former's plain images, work table and
 * per-row column mask: each later pass scans under a ceiling per row derived from the row's floor with the wide scan's margin
 * (mmf_simtopk_wide_anyk, mmf_hg_wide_anyk.h), and the exact re-rank drops the already-emitted columns of other
 * segments that slip under it.  An addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers,
 * host offsets, `device_id`, `hip_stream`, mmf_last_error); bound from the list CROSS_WIDE_ANYK_EXPORTS of
 * multimodal-fusion_amd/_lib.py.
 *
 * Output contract: that of mmf_simtopk_cross_segments, bit for bit (ids and values) — out_idx (rows of all of Y) / out_val [n, k],
 * canonical key descending, then id ascending; never a column of the row's own segment; no -1 / -inf fill (a segment with rows and
 * fewer than k columns outside itself is refused on the host).
 *
 * Workspace, cached per (device, stream): that of mmf_simtopk_cross_segments_wide at depth 20, plus per row 8 bytes of floors,
 * 8 bytes of per-pass bookkeeping and a staging row of 20 x 16 bytes, and 4 bytes of ceiling per row of the padded query image;
 * when rows take the exact rescan, in the second slot the f32 image of Y and of those rows, their exact lists and floors.
 *
 * Host-synchronous: once per pass (the re-rank's fail counts and the yield histogram travel together); once more in a pass that
 * sends rows to the exact rescan (the rows are read to the host, which builds the exact cross-segment table over them: one exact
 * scan launch and one re-rank per 44 entries, whatever the number of segments the rows lie in).  The rescan itself does not
 * synchronise: its fail count (an internal invariant: zero) travels with the next pass's read, and only a call whose LAST pass
 * rescanned reads it with one more synchronisation before it returns.  The offsets are read on the host.
 */
#ifndef MMF_HG_CROSS_SEGW_ANYK_H
#define MMF_HG_CROSS_SEGW_ANYK_H

#include "mmf_hg_fast_anyk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mmf_simtopk_cross_segments_fast_anyk.  opts (may be NULL): precision MMF_PREC_FAST (f16 operands) /
 * MMF_PREC_FAST_BF16 run the passes, MMF_PREC_AUTO means MMF_PREC_FAST, MMF_PREC_EXACT forwards to the exact driver of
 * mmf_simtopk_cross_segments (info: one pass); col_splits 0 (automatic) or a power of two, the runs the admissible tiles of every
 * row block are cut into — the work table is built once, at depth 20, and every pass launches it; select_wait_event is refused;
 * query_order is ignored (off).  k <= 20: the call IS mmf_simtopk_cross_segments_wide — same launches, same bits (info: one pass).
 * bf16 operands are served but lose: their margin is eight times f16's, so several already-emitted columns per
 * row slip under the ceiling and shrink every later pass's yield, and most rows' margin bands outgrow a 32-entry list on a
 * schedule without overflow lists, where a row whose lists crowd is flagged for the exact rescan.
 * One yield per pass for the whole call; MMF_ANYK_SHORT_DIV (environment, read per call, default 64, 1 .. 65536): a pass emits
 * the largest yield that leaves at most n / MMF_ANYK_SHORT_DIV unflagged rows short of it; results do not depend on it.  A yield
 * below 1, or the 15th pass, finishes every row by the exact scan from its floor.  A row with fewer unemitted columns outside its
 * segment than a pass is deep stays in the work table: its lists come up short, the re-rank flags it and it takes the exact rescan.
 * stats (may be NULL): those of the first pass, with fallback_rows summed over the passes.
 * Checked on the host before any device call, every message naming the entry: the refusals of mmf_simtopk_cross_segments_wide in
 * its order and wording (device_id < 0 first; shapes, dtype, NULL X, metric, lambda, k, offsets, NULL Y, col_splits, a precision
 * outside the four values -> MMF_E_INVALID, select_wait_event -> MMF_E_UNSUPPORTED); then d <= 1024 -> MMF_E_UNSUPPORTED in a
 * message naming mmf_simtopk_cross_segments_fast_anyk, d > 4096 under a fast precision -> MMF_E_UNSUPPORTED, NULL outputs, the
 * "segment %lld has %lld admissible columns" refusal.  n == 0 is a no-op. */
int mmf_simtopk_cross_segments_wide_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                         float lambda, int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                         int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                         mmf_simtopk_stats* stats, int device_id, void* hip_stream, mmf_fast_anyk_info* info);

/* Host only (no device): how the entry above serves (d, k) under MMF_PREC_FAST.  A row's own segment is masked, so no slot goes to
 * self: the answers of mmf_wide_anyk_plan(d, k, 0, ...) (mmf_hg_wide_anyk.h) — returns 1 where the call runs more than one pass,
 * 0 where a single pass serves (mmf_simtopk_cross_segments_wide), with *scan_kk / *first_yield / *min_passes as there (each may
 * be NULL); d <= 1024 and d > 4096: MMF_E_UNSUPPORTED; d < 1 or k < 1: MMF_E_INVALID. */
int mmf_cross_segments_wide_anyk_plan(int64_t d, int k, int* scan_kk, int* first_yield, int* min_passes);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_CROSS_SEGW_ANYK_H */
