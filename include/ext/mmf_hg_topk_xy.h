/* mmf_hg_topk_xy.h — the top-k of the combined similarity K = K_h * K_g of one set of rows (the queries) against another (the
 * candidates), without the nq x nc matrix: what mmf_simtopk_combined (mmf_hg_topk.h) and
 * mmf_simtopk_combined_fast (mmf_hg_topk16.h) compute for one F against itself, with the two sides and their id offsets apart —
 * new patches against an existing slide, two registered sections in one coordinate frame, or a row panel [lo, hi) of one graph
 * against all of it (the row-sharded multi-GPU driver, multimodal-fusion_amd/distributed.py: sharded_simtopk_combined).  An
 * addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`,
 * mmf_last_error); bound from the list EXPORTS_TOPK_XY of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: mmf_simtopk_combined's, per pair (query i, candidate j) — key_ij = eh + eg, val_ij = expf(eh) * expf(eg) from
 * the same canonical fmaf chains, so the same bits; the reported id is col_offset + j; rank by key descending, then reported id
 * ascending; a pair is dropped iff exclude_self and row_offset + i == col_offset + j (identity of ids, not of storage); a query
 * with fewer than k admissible candidates gets them first, then id -1 and value -inf.  A lambda of 0 is valid and drops its term.
 *
 * Row slice: when Fq / Pq point at row r0 of Fc / Pc (the same row of both, nq rows inside nc) the call is a row slice of a
 * self problem: one operand image and one set of chains are built (as mmf_simtopk recognises a row slice of Y), and with
 * row_offset = col_offset + r0 the result equals rows r0 .. r0 + nq - 1 of mmf_simtopk_combined(Fc, Pc, nc, ...) shifted by
 * col_offset, bit for bit in ids and values, under every precision.
 *
 * How (MMF_PREC_FAST / _FAST_BF16): the candidates are copied into one 16-bit operand image from position 0, padded to a multiple
 * of 128 rows (padding: zero operands, bias -inf); queries that are no slice of the candidates follow from the next multiple of
 * 128.  The table-driven launch of the f16 / bf16 candidate scan of mmf_simtopk_combined_fast reads one 8 x int32 entry per
 * block of 128 queries and column range (the block's image position, its row in the joint numbering candidates-then-queries,
 * its real queries, the candidate tile range, id offset 0, the list slot, the last candidate row); the scale, the four maxima
 * and the largest position chain of the error margin are taken over BOTH sides, a superset of what each bound needs.  One exact
 * re-rank over all queries; the rows the scan could not certify are answered by the exact scan over their 128-row blocks
 * (adjacent blocks merged; all queries when more than a quarter of the blocks hold a flagged row).
 *
 * Limits: f32 inputs, dp <= 8, row_offset + nq and col_offset + nc < 2^31; MMF_PREC_EXACT any d and k + self <= 44;
 * MMF_PREC_FAST / _FAST_BF16 k + self <= 20 and 1 <= d <= 4096.
 *
 * Workspace, cached per (device, stream).  Exact: the f32 images of both sides (one for a slice), 8 bytes per row of chains, the
 * exact lists.  16-bit: the image (2 bytes x d rounded up to 128 per position), 8 bytes per row of chains, for two sets a copy
 * of both sides' positions, 32 bytes per workgroup of work table, the candidate lists of the QUERIES only (2 x column ranges
 * lists of 16 or 32 entries per query, with their keys when there is more than one range); in a second block the f32 images
 * and the exact lists when a flagged row goes there.  Nothing grows with nq * nc.
 *
 * Host-synchronous: data-dependent — exact: once (the exact pass's fail count); 16-bit: once per call (the re-rank's fail count
 * with the first 1024 flagged row ids), once more for the exact pass's fail count when a flagged row went there, and once in
 * between if more than 1024 rows were flagged.  No host arguments.
 */
#ifndef MMF_HG_TOPK_XY_H
#define MMF_HG_TOPK_XY_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fq [nq,d], Pq [nq,dp]: the queries; Fc [nc,d], Pc [nc,dp]: the candidates (device, f32, row-major).  out_idx [nq,k] int64,
 * out_val [nq,k] f32 (device).  opts (may be NULL): precision MMF_PREC_EXACT = the exact f32 scan, MMF_PREC_FAST = f16 operands,
 * MMF_PREC_FAST_BF16 = bf16 operands (a call with fewer than k + self candidates is served exactly under either),
 * MMF_PREC_AUTO = the f16 scan in the range DESIGN.md §4.19 measured it to pay against this entry's own exact arm (512 <= d <=
 * 1536, k + self <= 11, at least k + self candidates), else the exact scan; col_splits: 0 (automatic) or the column
 * ranges every query block is scanned in (rounded up to a power of two, bounded by the candidate tiles and the re-rank's 1024
 * candidates per row); profile is honoured, the rest is ignored.  stats (may be NULL): precision_used, col_splits, scan_grid,
 * candidates, fallback_rows, overflow_rows / short_rows (why), and under profile prep_ms / scan_ms / rerank_ms / fallback_ms.
 * Checked on the host before any device call, every message naming the entry and the argument: device_id < 0 ->
 * MMF_E_UNSUPPORTED first; MMF_E_INVALID for nq < 0, nc < 0, d < 1, dp < 1, k < 1, a negative row_offset / col_offset, a
 * negative or non-finite lambda, a NULL Fq / Pq / out_idx / out_val with nq > 0, a NULL Fc / Pc with nq > 0 and nc > 0, an
 * unknown precision, a negative col_splits; MMF_E_UNSUPPORTED for dp > 8, k + self > 44, under MMF_PREC_FAST / _FAST_BF16
 * k + self > 20 or d > 4096, row_offset + nq or col_offset + nc >= 2^31.  nq == 0 is a no-op; nc == 0 with nq > 0 fills
 * -1 / -inf. */
int mmf_simtopk_combined_xy(const float* Fq, const float* Pq, int64_t nq,
                            const float* Fc, const float* Pc, int64_t nc,
                            int64_t d, int64_t dp, float lambda_h, float lambda_g, int k, int exclude_self,
                            int64_t row_offset, int64_t col_offset,
                            int64_t* out_idx, float* out_val,
                            const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_TOPK_XY_H */
