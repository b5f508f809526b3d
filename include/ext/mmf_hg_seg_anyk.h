/* mmf_hg_seg_anyk.h — the segmented 16-bit top-k for any k: what mmf_simtopk_segmented_exact answers for a ragged
 * batch, for any k >= 1 at d <= 1024, with the candidates of EVERY pass taken from the 16-bit matrix cores.  mmf_simtopk_segmented
 * stops at one pass (k + self <= 44 at d <= 512, <= 20 at 512 < d <= 1024); this entry runs the passes of mmf_simtopk_fast_anyk
 * (mmf_hg_fast_anyk.h) over the segmented call's images and work table: each later pass scans under a ceiling per
 * row derived from the row's floor, and the exact re-rank drops the already-emitted columns that slip under it.  An addition to
 * ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, host offsets, `device_id`, `hip_stream`,
 * mmf_last_error); bound from the list SEG_ANYK_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: per segment, bit for bit (ids and values), that of mmf_simtopk_segmented_exact — i.e. of mmf_simtopk_ex with
 * MMF_PREC_EXACT, row_offset = x_ptr[s], col_offset = y_ptr[s]: out_idx (global rows of Y) / out_val [n, k], canonical key
 * descending, then id ascending.  A segment with fewer than k admissible columns gets those first, then -1 / -inf (it is answered by
 * the exact launch loop, as in mmf_simtopk_segmented); an empty segment is skipped.
 *
 * Workspace, cached per (device, stream): that of mmf_simtopk_segmented at the pass depth, plus per row 8 bytes of floors, 12 bytes
 * of per-pass bookkeeping, 4 bytes of segment offsets and a staging row of (pass depth) x 16 bytes, and 4 bytes of ceiling per
 * position of the padded query image; when rows take the exact rescan, in the second slot the f32 image of Y and of those rows.
 *
 * Host-synchronous: once per pass (the re-rank's fail counts and the yield histogram travel together); once more in a pass that
 * sends rows to the exact rescan (the rows are read to the host and grouped per segment: two launches per segment with such rows).
 */
#ifndef MMF_HG_SEG_ANYK_H
#define MMF_HG_SEG_ANYK_H

#include "mmf_hg_fast_anyk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mmf_simtopk_segmented, and `info` (host pointer, may be NULL; mmf_fast_anyk_info of mmf_hg_fast_anyk.h — here
 * exact_rows[p] counts rows of SERVED segments only: those with rows and at least k admissible columns).  opts (may be NULL):
 * precision MMF_PREC_FAST (f16 operands) / MMF_PREC_FAST_BF16 run the passes, MMF_PREC_AUTO means MMF_PREC_FAST, MMF_PREC_EXACT
 * forwards to mmf_simtopk_segmented_exact's behaviour; col_splits and select_wait_event are refused.  Where one pass holds k + self
 * the call IS mmf_simtopk_segmented: same launches, same bits (info: one pass).  d > 1024 with k + self > 20 is refused with
 * MMF_E_UNSUPPORTED: the wide segmented scan has no ceilings.
 * One yield per pass for the whole call; MMF_ANYK_SHORT_DIV (environment, read per call, default 64, 1 .. 65536): a pass emits
 * the largest yield that leaves at most n_served / MMF_ANYK_SHORT_DIV unflagged rows short of it; results do not depend on it.
 * stats (may be NULL): those of the first pass, with fallback_rows summed over the passes.
 * Checked on the host before any device call, every message naming the entry: the refusals of mmf_simtopk_segmented in its order
 * and wording (device_id < 0 first; shapes, dtype, NULL X, metric, lambda, k, offsets, NULL Y), then col_splits /
 * select_wait_event and the unserved (d, k) -> MMF_E_UNSUPPORTED, then NULL outputs; a precision outside the four values ->
 * MMF_E_INVALID.  n == 0 is a no-op. */
int mmf_simtopk_segmented_fast_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                    float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                    int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                    mmf_simtopk_stats* stats, int device_id, void* hip_stream, mmf_fast_anyk_info* info);

/* Host only (no device): how the entry above serves (d, k, exclude_self) under MMF_PREC_FAST.  For d <= 1024 the answers of
 * mmf_fast_anyk_plan: returns 1 where it runs more than one pass, 0 where a single pass serves (mmf_simtopk_segmented), with
 * *scan_kk / *first_yield / *min_passes as there (each may be NULL).  d > 1024: 0 where one pass of the wide segmented scan serves,
 * MMF_E_UNSUPPORTED beyond it (and for d > 4096).  d < 1 or k < 1: MMF_E_INVALID. */
int mmf_segmented_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_SEG_ANYK_H */
