/* mmf_hg_fast_anyk.h — the 16-bit top-k for any k: what mmf_simtopk_ex answers, for any k >= 1 at d <= 1024, with
 * the candidates of EVERY pass taken from the 16-bit matrix cores.  One pass of the 16-bit scan holds k + self <= 44 entries per
 * row at d <= 512 and k + self <= 20 at 512 < d <= 1024; mmf_simtopk_ex refuses MMF_PREC_FAST beyond that.  This entry runs
 * several passes: each later pass scans under a per-row CEILING derived from the row's floor (the last entry it has emitted), so
 * the scan's lists fill with what ranks after the floor, and the exact re-rank drops the few already-emitted columns that slip
 * under the ceiling.  An addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers,
 * `device_id`, `hip_stream`, mmf_last_error); bound from the list FAST_ANYK_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: that of mmf_simtopk_ex with MMF_PREC_EXACT, bit for bit (ids and values): out_idx / out_val [n, k], canonical
 * key descending, then id ascending.
 *
 * Workspace, cached per (device, stream): that of the fast path of mmf_simtopk_ex at the pass depth, plus per row 12 bytes of
 * floors and ceiling, 16 bytes of per-pass bookkeeping and a staging row of (pass depth) x 16 bytes; when rows take the exact
 * rescan, in the second slot the f32 image of Y and of those rows.
 *
 * Host-synchronous: once per pass (the re-rank's fail counts and the yield histogram travel together); once more in a pass that
 * sends rows to the exact rescan.
 */
#ifndef MMF_HG_FAST_ANYK_H
#define MMF_HG_FAST_ANYK_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMF_FAST_ANYK_MAX_PASSES 16

/* What the passes of a call did (host memory, written before the call returns).  Pass p emitted yield[p] entries for EVERY row;
 * ghost_max[p] is the largest number of already-emitted columns the re-rank dropped for a row of that pass (0 for pass 0, which
 * has no floor); exact_rows[p] the rows that took the exact rescan in that pass — flagged by the scan, or short of yield[p]
 * certified entries — and n for a pass the exact driver finished.  Only the first MMF_FAST_ANYK_MAX_PASSES passes are recorded;
 * `passes` counts them all. */
typedef struct mmf_fast_anyk_info {
  int32_t passes;
  int32_t yield[MMF_FAST_ANYK_MAX_PASSES];
  int32_t ghost_max[MMF_FAST_ANYK_MAX_PASSES];
  int64_t exact_rows[MMF_FAST_ANYK_MAX_PASSES];
} mmf_fast_anyk_info;

/* The arguments of mmf_simtopk_ex, and `info` (host pointer, may be NULL).  opts (may be NULL): precision MMF_PREC_FAST (f16
 * operands) / MMF_PREC_FAST_BF16 run the passes, MMF_PREC_AUTO means MMF_PREC_FAST, MMF_PREC_EXACT forwards to the exact path of
 * mmf_simtopk_ex; col_splits, query_order and profile as in mmf_simtopk_ex (query_order and the symmetric scan apply to the first
 * pass only); select_wait_event is refused.  Where one pass holds k + self the call IS the fast call of mmf_simtopk_ex: same
 * launches, same bits (info: one pass).  d > 1024 with k + self > 20 is refused with MMF_E_UNSUPPORTED by THIS entry
 * (mmf_simtopk_wide_anyk, mmf_hg_wide_anyk.h, serves it); d > 1024 with k + self <= 20 is mmf_simtopk_ex's wide scan.
 * MMF_ANYK_SHORT_DIV (environment, read per call, default 64, 1 .. 65536): a pass emits the largest yield that leaves at most
 * n / MMF_ANYK_SHORT_DIV unflagged rows short of it; results do not depend on it.
 * stats (may be NULL): those of the first pass, with fallback_rows summed over the passes.
 * Checked on the host before any device call, every message naming the entry: the refusals of mmf_simtopk_ex in its order and
 * wording (device_id < 0 first; shapes, dtype, NULL X, metric, lambda, k), then select_wait_event and the unserved (d, k) ->
 * MMF_E_UNSUPPORTED, then NULL outputs and k beyond the admissible columns; a precision outside the four values -> MMF_E_INVALID.
 * n == 0 is a no-op. */
int mmf_simtopk_fast_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                          int k, int exclude_self, int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                          const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                          mmf_fast_anyk_info* info);

/* Host only (no device): how the entry above serves (d, k, exclude_self) under MMF_PREC_FAST.  Returns 1 where it runs more than
 * one pass, 0 where a single pass serves (the fast call of mmf_simtopk_ex), a negative status where it refuses (d < 1, k < 1:
 * MMF_E_INVALID; d > 1024 beyond one pass, d > 4096: MMF_E_UNSUPPORTED).  *scan_kk (may be NULL): the depth of a pass, self's
 * slot included — 44 at d <= 512, 20 at d <= 1024 (and for the wide scan), k + self where a single pass serves; *first_yield: the
 * entries per row the first pass emits; *min_passes: the passes a call needs at least (every later pass emitting scan_kk - self
 * entries, i.e. without ghosts). */
int mmf_fast_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_FAST_ANYK_H */
