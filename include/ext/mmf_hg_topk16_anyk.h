/* mmf_hg_topk16_anyk.h — the 16-bit top-k of the combined similarity K = K_h * K_g for any k: what
 * mmf_simtopk_combined_anyk (mmf_hg_topk_anyk.h) answers, for one graph or a ragged batch, for any k >= 1 at 1 <= d <= 4096, with
 * the candidates of EVERY pass taken from the 16-bit scan of the combined key.  mmf_simtopk_combined_fast (mmf_hg_topk16.h) and
 * mmf_simtopk_combined_fast_segmented (mmf_hg_topk16_seg.h) stop at one pass (k + self <= 20); this entry runs passes of depth 20
 * over the segmented entry's segment-padded image and work table (one graph is a batch of one segment): each later pass scans
 * under a ceiling per row derived from the row's floor — the last entry it has emitted — with the combined key's margin
 * (mmf_scan_b16c.hip, "Ceilings"), and the exact re-rank drops the already-emitted columns that slip under it.  An addition to ABI
 * version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, host offsets, `device_id`, `hip_stream`,
 * mmf_last_error); bound from the list TOPK16_ANYK_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: that of mmf_simtopk_combined_anyk, bit for bit (ids and values).  Per row the first k entries of the total order
 * (key = eh + eg descending, then id ascending) over the admissible columns of its segment; out_idx holds global rows of F, out_val
 * the entries of mmf_sim_dense_combined bit for bit.  A segment (or graph) with fewer than k admissible columns gets those first,
 * then -1 / -inf (it is answered by the exact launch loop, as in mmf_simtopk_combined_fast_segmented); an empty segment is skipped.
 * For any k' >= k the first k columns of the k' result are the k result.
 *
 * Workspace, cached per (device, stream): that of mmf_simtopk_combined_fast_segmented at depth 20, plus per row 8 bytes of floors,
 * 12 bytes of per-pass bookkeeping, 4 bytes of segment offsets, 4 bytes of ceiling and a staging row of 20 x 16 bytes; when rows
 * take the exact rescan, in the second slot the f32 image of F and of those rows.
 *
 * Host-synchronous: once per pass (the re-rank's fail counts and the yield histogram travel together); in a pass that sends rows to
 * the exact rescan once more for the rows (read to the host and grouped per segment: two launches per segment with such rows) and
 * once for the rescan's fail count.
 */
#ifndef MMF_HG_TOPK16_ANYK_H
#define MMF_HG_TOPK16_ANYK_H

#include "mmf_hg_fast_anyk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The 17 arguments of mmf_simtopk_combined (mmf_hg_topk.h) and `info` (host pointer, may be NULL; exact_rows[p] counts rows of
 * SERVED segments only: those with rows and at least k admissible columns).  ptr_host == NULL with n_segments == 0: one graph;
 * offsets given: every graph of a ragged batch.  f32 rows, dp <= 8, n < 2^31.
 * opts (may be NULL): precision MMF_PREC_FAST (f16 operands) / MMF_PREC_FAST_BF16 run the passes, MMF_PREC_AUTO means
 * MMF_PREC_FAST, MMF_PREC_EXACT forwards to the drivers behind mmf_simtopk_combined_anyk (info: one pass); col_splits 0 (automatic)
 * or a power of two, the column ranges every segment is scanned in (at most one per 128 columns of the segment, and as many as the
 * re-rank's capacity per row holds at 32-entry lists) — the work table is built once and every pass launches it.
 * k + self <= 20 under a fast precision: the call IS mmf_simtopk_combined_fast (one graph) or mmf_simtopk_combined_fast_segmented
 * (offsets given) — same launches, same bits (info: one pass).
 * One yield per pass for the whole call; MMF_ANYK_SHORT_DIV (environment, read per call, default 64, 1 .. 65536): a pass emits the
 * largest yield that leaves at most n_served / MMF_ANYK_SHORT_DIV unflagged rows short of it; results do not depend on it.  The rows
 * short of a pass's yield and the rows the scan or the re-rank flagged are gathered, per segment, into an exact scan of the combined
 * key from their floors, and join the next 16-bit pass.  A yield below 1, or the 15th pass, finishes every served row by the exact
 * scan from its floor.  A served segment with fewer unemitted columns than a pass is deep stays in the work table: its lists come up
 * short, the re-rank flags its rows and they take the rescan.
 * stats (may be NULL): those of the first pass, with fallback_rows summed over the passes.
 * Checked on the host before any device call, every message naming the entry: the refusals of the two one-pass entries in their
 * order and wording (device_id < 0 first; n, d, dp, k, lambda_h, lambda_g, NULL F / P / out_idx / out_val -> MMF_E_INVALID; the
 * offsets, when given, as mmf_simtopk_combined checks them; dp > 8, d > 4096, n >= 2^31 -> MMF_E_UNSUPPORTED; a precision outside
 * the four values and a col_splits that is neither 0 nor a power of two -> MMF_E_INVALID) — without their k + self > 20 refusal.
 * n == 0 is a no-op. */
int mmf_simtopk_combined_fast_anyk(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g, int k,
                                   int exclude_self, const int64_t* ptr_host, int64_t n_segments, int64_t* out_idx, float* out_val,
                                   const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                                   mmf_fast_anyk_info* info);

/* Host only (no device): how the entry above serves (d, k, exclude_self) under a fast precision.  Returns 1 where the call runs
 * more than one pass (k + self > 20), 0 where a single pass serves; *scan_kk: the depth of the first scan (k + self, or 20 beyond one
 * pass), *first_yield: the entries the first pass emits (*scan_kk - self), *min_passes: 1, or 1 + ceil((k - first_yield) /
 * (20 - self)) — every later pass emits at most 20 - self entries (each pointer may be NULL).  d < 1 or k < 1: MMF_E_INVALID;
 * d > 4096: MMF_E_UNSUPPORTED. */
int mmf_combined_fast_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_TOPK16_ANYK_H */
