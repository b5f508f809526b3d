/* mmf_hg_cross_seg.h — the cross-segment top-k: for every row of a ragged batch, the k best columns among the
 * rows of all OTHER segments.  Every other segmented entry is block diagonal (a row only gets columns of its own segment); this
 * one is the complement: leave-one-slide-out nearest neighbours, inter-slide edges of a cohort hypergraph, matching new slides
 * against a bank that already holds sections of the same patients.  One table-driven launch of the exact f32 scan (the kernel of
 * mmf_hg_seg_exact.h with a column mask: a key whose column lies in the row block's own segment becomes -inf) and one re-rank over
 * all rows per pass.  An addition to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers,
 * `device_id`, `hip_stream`, mmf_last_error); bound from the list CROSS_SEG_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: row i of segment s gets the top k of row i against every row j of Y with j < y_ptr[s] or j >= y_ptr[s + 1],
 * ranked by canonical key descending, then id ascending; ids are rows of all of Y (of X for a self call).  Bit for bit this is
 * what the exact mmf_simtopk_ex gives for that row against those columns (the two runs of Y concatenated, ids mapped back).
 * There is no -1 / -inf fill: a call in which a segment with rows has fewer than k admissible columns is refused.
 *
 * Workspace, cached per (device, stream): that of mmf_simtopk_segmented_exact — the f32 image of Y (and of X unless X is Y), 4
 * bytes per row of scalars, 64 bytes per workgroup of work table, and per row 2 x (largest range count) lists of 16 / 32 / 48 ids.
 *
 * Host-synchronous: once per call, for the re-rank's fail counts (an internal invariant: the exact lists cannot overflow).  The
 * offsets are read on the host during the call.
 */
#ifndef MMF_HG_CROSS_SEG_H
#define MMF_HG_CROSS_SEG_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Y NULL: X against itself, with y_ptr = x_ptr (m and y_ptr_host ignored).  There is no exclude_self: a row's self lies inside its
 * own segment.  Segment s of X (rows x_ptr[s] .. x_ptr[s + 1]) excludes rows y_ptr[s] .. y_ptr[s + 1] of Y; a segment with no rows
 * of Y excludes nothing, a segment with no rows of X asks nothing.  Any d, f32 / bf16 / f16 rows, the four metrics of mmf_simtopk,
 * any k >= 1: k > 44 runs passes of at most 44 entries, each one scan launch with per-row floors and one re-rank.  opts (may be
 * NULL): precision MMF_PREC_AUTO or MMF_PREC_EXACT (both: this exact scan); col_splits 0 (automatic: runs of column tiles sized
 * so that the call makes about 1024 workgroups) or a power of two, the column ranges the admissible tiles of every row block are
 * cut into (a range that spans the block's own segment counts twice), bounded by the re-rank's 1024 candidates per row; profile
 * is honoured, the rest is ignored.  stats (may be NULL): precision_used = MMF_PREC_EXACT, col_splits = the largest range count of
 * a row block, scan_grid = work-table entries, candidates, and under profile prep_ms / scan_ms / rerank_ms.
 * Checked on the host before any device call, every message naming the entry: device_id < 0 -> MMF_E_UNSUPPORTED first;
 * MMF_E_INVALID for bad shapes or dtype, a NULL X (n > 0), Y (m > 0) or output, a bad metric, MMF_RBF without lambda > 0, k < 1,
 * bad offsets, a col_splits that is negative or no power of two, and any segment with rows that has fewer than k admissible
 * columns, m - (y_ptr[s + 1] - y_ptr[s]) < k (the message names the segment and both numbers); MMF_E_UNSUPPORTED for
 * MMF_PREC_FAST / _FAST_BF16 (no 16-bit scan serves this entry yet) and n or m >= 2^31.  n == 0 is a no-op. */
int mmf_simtopk_cross_segments(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                               float lambda, int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments,
                               int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                               int device_id, void* hip_stream);

/* Host only (no device, no stream): the work table of the entry above for the offsets x_ptr_host / y_ptr_host (NULL: the self
 * call), k and col_splits.  Entry e is table_host[8 e .. 8 e + 7] = segment, first row of X, real queries (<= 128), first excluded
 * row of Y (y_ptr[s]), first and end tile (of 128 rows of ALL of Y, from row 0), number of the column range, end of the excluded
 * rows (y_ptr[s + 1]).  A tile that lies wholly inside the excluded rows is in no entry; a range that would span them is two
 * entries with numbers of their own.  Entries come longest run first (the launch's tail is made of short runs).  Returns the
 * entry count (>= 0) and writes the entries when table_host is not NULL and `capacity` entries hold them, and the list slots per
 * row (2 x the largest range count of a row block) into *lists_out when that is not NULL; a negative status for bad offsets,
 * k < 1, a bad col_splits or too small a capacity. */
int64_t mmf_cross_segments_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int k, int col_splits,
                                 int64_t* table_host, int64_t capacity, int* lists_out);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_CROSS_SEG_H */
