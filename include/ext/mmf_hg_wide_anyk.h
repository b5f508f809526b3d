/* mmf_hg_wide_anyk.h — the wide 16-bit top-k for any k: what mmf_simtopk_ex answers, for any k >= 1 at
 * 1024 < d <= 4096, with the candidates of EVERY pass taken from the wide 16-bit scan (mmf_scan_b16w.hip).  One pass of that scan
 * holds k + self <= 20 entries per row; mmf_simtopk_ex refuses MMF_PREC_FAST beyond that, and mmf_simtopk_fast_anyk
 * (mmf_hg_fast_anyk.h) runs several passes only at d <= 1024.  This entry is its twin above 1024: each later pass scans under a
 * per-row CEILING derived from the row's floor (the last entry it has emitted) and the WIDE scan's error margin, so the lists fill
 * with what ranks after the floor, and the exact re-rank drops the few already-emitted columns that slip under the ceiling.  An
 * addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`,
 * mmf_last_error); bound from the list WIDE_ANYK_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: that of mmf_simtopk_ex with MMF_PREC_EXACT, bit for bit (ids and values): out_idx / out_val [n, k], canonical
 * key descending, then id ascending.
 *
 * Workspace, cached per (device, stream): that of the wide fast path of mmf_simtopk_ex at depth 20, plus per row 12 bytes of
 * floors and ceiling, 16 bytes of per-pass bookkeeping and a staging row of 20 x 16 bytes; when rows take the exact rescan, in the
 * second slot the f32 image of Y and of those rows.
 *
 * Host-synchronous: once per pass (the re-rank's fail counts and the yield histogram travel together); once more in a pass that
 * sends rows to the exact rescan.
 */
#ifndef MMF_HG_WIDE_ANYK_H
#define MMF_HG_WIDE_ANYK_H

#include "mmf_hg_fast_anyk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of mmf_simtopk_fast_anyk, `info` (host pointer, may be NULL; the struct of mmf_hg_fast_anyk.h) included.  opts
 * (may be NULL): precision MMF_PREC_FAST (f16 operands) / MMF_PREC_FAST_BF16 run the passes, MMF_PREC_AUTO means MMF_PREC_FAST,
 * MMF_PREC_EXACT forwards to the exact path of mmf_simtopk_ex (any d > 1024); col_splits and profile as in mmf_simtopk_ex; query_order is
 * checked and has no effect (the wide scan has no query order, symmetric scan or panels); select_wait_event is refused.  Where
 * one pass holds k + self (<= 20) the call IS the wide fast call of mmf_simtopk_ex: same launches, same bits (info: one pass).
 * MMF_ANYK_SHORT_DIV and MMF_WIDE_SINK (environment, read per call) as in mmf_simtopk_fast_anyk and mmf_simtopk_ex; results do not
 * depend on them.
 * stats (may be NULL): those of the first pass, with fallback_rows summed over the passes.
 * Checked on the host before any device call, every message naming the entry: the refusals of mmf_simtopk_ex in its order and
 * wording (device_id < 0 first; shapes, dtype, NULL X, metric, lambda, k), then a precision outside the four values ->
 * MMF_E_INVALID, select_wait_event -> MMF_E_UNSUPPORTED, d <= 1024 -> MMF_E_UNSUPPORTED (call mmf_simtopk_fast_anyk there),
 * d > 4096 under a fast precision -> MMF_E_UNSUPPORTED, then NULL outputs and k beyond the admissible columns.
 * n == 0 is a no-op. */
int mmf_simtopk_wide_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                          int k, int exclude_self, int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                          const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                          mmf_fast_anyk_info* info);

/* Host only (no device): how the entry above serves (d, k, exclude_self) under MMF_PREC_FAST, with the semantics of
 * mmf_fast_anyk_plan.  Returns 1 where it runs more than one pass, 0 where a single pass serves (k + self <= 20: the wide fast call
 * of mmf_simtopk_ex), a negative status where it refuses (d < 1, k < 1: MMF_E_INVALID; d <= 1024, d > 4096: MMF_E_UNSUPPORTED).
 * *scan_kk (may be NULL): the depth of a pass, self's slot included — 20, or k + self where a single pass serves; *first_yield:
 * the entries per row the first pass emits; *min_passes: the passes a call needs at least (every later pass emitting 20 - self
 * entries, i.e. without ghosts). */
int mmf_wide_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_WIDE_ANYK_H */
