/* mmf_hg_topk16_xy_anyk.h — the 16-bit top-k of the combined similarity K = K_h * K_g for TWO node sets and any k (DESIGN.md
 * §4.34): what mmf_simtopk_combined_xy_anyk (mmf_hg_topk_anyk.h) answers — queries against candidates with an id offset on each
 * side, or rows [lo, hi) of one graph against all of it — for any k >= 1 at 1 <= d <= 4096, with the candidates of EVERY pass taken
 * from the 16-bit scan of the combined key.  mmf_simtopk_combined_xy (mmf_hg_topk_xy.h) stops at one pass (k + self <= 20); this
 * entry runs the passes of mmf_simtopk_combined_fast_anyk (mmf_hg_topk16_anyk.h) over that entry's two-sided image and work table:
 * each later pass scans under a ceiling per query derived from the query's floor — the last entry it has emitted — with the combined
 * key's margin (mmf_scan_b16c.hip, "Ceilings" and "Two-set form": scale, maxima and the largest position chain are taken over the
 * union of both sides, so a query's margin word is at least a self call's and the ceiling never masks a column that ranks after the
 * floor), and the exact re-rank drops the already-emitted columns that slip under it.  An addition to ABI version 3 of mmf_hg.h,
 * whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list
 * TOPK16_XY_ANYK_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: that of mmf_simtopk_combined_xy_anyk on the same arguments, bit for bit (ids and values).  Per query the first k
 * entries of the total order (key = eh + eg descending, then reported id ascending) over the admissible candidates; out_idx holds
 * col_offset + candidate row, out_val the entries of mmf_sim_dense_combined bit for bit.  A pair is dropped iff exclude_self and
 * row_offset + i == col_offset + j.  A query with fewer than k admissible candidates gets them first, then -1 / -inf; nq == 0 is a
 * no-op and nc == 0 fills every row with -1 / -inf.  For any k' >= k the first k columns of the k' result are the k result.
 *
 * Workspace, cached per (device, stream): that of mmf_simtopk_combined_xy's 16-bit path at depth 20 (both sides' chains, the joint
 * positions, one 16-bit image of the candidates and — unless the queries are rows of them — the queries, the work table, 32-entry
 * lists for the queries), plus per query 8 bytes of floors (for a row slice from the candidates' first row on), 12 bytes of per-pass
 * bookkeeping, 4 bytes of ceiling and a staging row of 20 x 16 bytes; when queries take the exact rescan, in the second slot the f32
 * image of the candidates and of those queries.
 *
 * Host-synchronous: once per pass (the re-rank's fail counts and the yield histogram travel together); in a pass that sends queries
 * to the exact rescan once more for their list (read to the host, sorted, one gathered group against all candidates) and once for
 * the rescan's fail count.
 */
#ifndef MMF_HG_TOPK16_XY_ANYK_H
#define MMF_HG_TOPK16_XY_ANYK_H

#include "mmf_hg_fast_anyk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The 20 arguments of mmf_simtopk_combined_xy (mmf_hg_topk_xy.h) and `info` (host pointer, may be NULL).  f32 rows, dp <= 8,
 * row_offset + nq and col_offset + nc < 2^31.  Queries that point into the candidates (Fq = Fc + r0 * d and Pq = Pc + r0 * dp with
 * r0 + nq <= nc) are recognised as a row slice, as in mmf_simtopk_combined_xy: one image, one set of chains.
 * opts (may be NULL): precision MMF_PREC_FAST (f16 operands) / MMF_PREC_FAST_BF16 run the passes, MMF_PREC_AUTO means
 * MMF_PREC_FAST, MMF_PREC_EXACT forwards to the driver behind mmf_simtopk_combined_xy_anyk (any d; info: one pass); col_splits
 * 0 (automatic) or a power of two, the column ranges the candidates are scanned in (at most one per 128 candidates, and as many as
 * the re-rank's capacity per row holds at 32-entry lists) — the work table is built and uploaded once and every pass launches it.
 * k + self <= 20 under a fast precision: the call IS mmf_simtopk_combined_xy's 16-bit path — same launches, same bits (info: one
 * pass).  A call with fewer than k + self candidates is served exactly, as mmf_simtopk_combined_xy serves it (info: one pass).
 * Pass 0 is that path's work at depth 20: 20 - self entries per query into the k-wide output rows, and each query's floor.  A later
 * pass computes the ceilings from the floors, resets lists, counts, seeds and overflow words, scans the same device work table
 * under the ceilings (with the seed union when there is more than one column range), audits, and re-ranks both sides' rows into
 * staging rows with canonical keys; count, yield and emit follow.
 * One yield per pass for the whole call; MMF_ANYK_SHORT_DIV (environment, read per call, default 64, 1 .. 65536): a pass emits the
 * largest yield that leaves at most nq / MMF_ANYK_SHORT_DIV unflagged queries short of it; results do not depend on it.  The queries
 * short of a pass's yield and the queries the scan or the re-rank flagged are gathered into the exact two-set scan of the combined
 * key from their floors, and join the next 16-bit pass.  A yield below 1, or the 15th pass, finishes every query by the exact scan
 * from its floor.  A call with fewer unemitted candidates than a pass is deep keeps its work table: the lists come up short, the
 * re-rank flags the queries and they take the rescan.  MMF_DEBUG_FLAG_ROWS (environment, a test hook) flags the first queries in
 * every pass.
 * stats (may be NULL): those of the first pass, with fallback_rows summed over the passes.
 * Checked on the host before any device call, every message naming the entry: the refusals of mmf_simtopk_combined_xy in their order
 * and wording (device_id < 0 first; nq, nc, d, dp, k, row_offset, col_offset, lambda_h, lambda_g, NULL Fq / Pq / Fc / Pc / out_idx /
 * out_val, a precision outside the four values -> MMF_E_INVALID; a col_splits that is neither 0 nor a power of two ->
 * MMF_E_INVALID; dp > 8, d > 4096 under a fast precision, row_offset + nq or col_offset + nc >= 2^31 -> MMF_E_UNSUPPORTED) —
 * without its k + self > 44 and k + self > 20 refusals.
 * How the call serves (d, k, exclude_self): mmf_combined_fast_anyk_plan (mmf_hg_topk16_anyk.h) answers for this entry too. */
int mmf_simtopk_combined_xy_fast_anyk(const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc,
                                      int64_t d, int64_t dp, float lambda_h, float lambda_g, int k, int exclude_self,
                                      int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                                      const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                                      mmf_fast_anyk_info* info);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_TOPK16_XY_ANYK_H */
