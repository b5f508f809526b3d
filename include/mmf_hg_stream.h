/* mmf_hg_stream.h — super-patch statistics of a slide whose similarity matrix does not fit: the six numbers
 * aggregate_wsi_super_patches takes from K = K_h * K_g (build_hypergraph/preprocess_hypergraph.py:172-197: the mean off-diagonal
 * similarity inside every cluster; mean, std, min, max and median of K) without K ever being whole in memory.  Additions to ABI
 * version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound
 * from the list EXPORTS_STREAM of multimodal-fusion_amd/_lib.py.
 *
 * K is recomputed from (F, P) in panels of whole rows by the kernel of mmf_sim_dense_combined, whose rows do not depend on the
 * panel they are computed in.  Every reduction runs panel by panel with the assignment of values to lanes and the order of
 * additions that the plain entries have on the stored matrix, so both outputs carry, bit for bit, what
 *     mmf_sim_dense_combined(F, P) -> K;  mmf_segment_offdiag_mean(K, order, offsets);  mmf_array_stats(K, n * n)
 * return for a 16-byte aligned K in the same environment (MMF_MEDIAN_RADIX set or not), whatever `panel_rows`:
 *   - a member's row sum needs that member's row only: the panel that holds the row computes it;
 *   - mean and std are f64 sums around the pivot K[0][0] per lane.  mmf_array_stats takes them from its median's one sweep when
 *     it runs one (2^22 <= n * n, in-bracket buffer of 5 % at most 2 GiB, MMF_MEDIAN_RADIX unset): K as flat rows of 4096 values,
 *     wave (b, w) of min((rows + 3) / 4, 2040) workgroups on rows 4 b + w, + 4 grid, ..., the ragged last row in a launch of
 *     its own; otherwise from its partial kernel: min(ceil(n * n / 4096), 2048) workgroups, thread t on the groups of four
 *     values t, t + threads, ... and then the scalar tail.  Here every lane's running (s1, s2, min, max) is kept on the device
 *     between the panels and reduced once after the last; a flat row (a group of four) that straddles two panels waits in front
 *     of the next panel;
 *   - the median is exact: the one sweep over a bracket placed by 32768 sampled pairs, with the four-pass radix select behind it.
 * K is recomputed once on the one-sweep path (five times when the bracket's verdict fails) and four times otherwise (the
 * statistics ride on the first radix pass).  A block of fewer than 2^22 values (16 MiB) is materialised inside the workspace.
 *
 * Workspace, cached per (device, stream) like every entry's: R * n + 4096 floats of panel (R = panel_rows, 0 = about 1 GiB,
 * at least 128 and at most n rows), the f32 image of F (mmf_padded_dim-style padding of n x d floats), the median's scratch
 * (mmf_array_stats' own: 5 % of n * n floats on the one-sweep path, at most 2 GiB, else a few KiB), 24 bytes per lane of at
 * most 2048 x 256 lanes, 2056 partials, and per row 4 bytes of squared norm, 8 of row sum, 4 of cluster id and 4 of member
 * position.  Nothing grows with n * n beyond the median's own 5 %.
 *
 * Host synchronisations: data-dependent, as mmf_array_stats (one wait for the bracket's verdict on the one-sweep path).
 */
#ifndef MMF_HG_STREAM_H
#define MMF_HG_STREAM_H

#include "mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The statistics aggregate_wsi_super_patches takes from K = K_h * K_g ([n,n] f32, never stored):
 *   intra_mean [n_clusters] (f64): mmf_segment_offdiag_mean(K, order, offsets) — NaN for a cluster of < 2 rows
 *   k_stats [5] (f64):             mmf_array_stats(K, n*n) — mean, unbiased std, min, max, lower median
 * K is recomputed from (F, P) in row panels of `panel_rows` rows (0 = about 1 GiB).  order/offsets: as mmf_segment_sort
 * leaves them; order == NULL: intra_mean is not touched.  n >= 2, dp >= 1, device_id < 0 -> MMF_E_UNSUPPORTED. */
int mmf_super_patch_stats_streamed(const float* F, const float* P, int64_t n, int64_t d, int64_t dp,
                                   float lambda_h, float lambda_g, const int64_t* order, const int64_t* offsets,
                                   int64_t n_clusters, int64_t panel_rows, double* intra_mean, double* k_stats,
                                   int device_id, void* hip_stream);
/* bytes of workspace that call asks for with these arguments in the current environment; touches no device */
int64_t mmf_super_patch_stats_streamed_bytes(int64_t n, int64_t d, int64_t dp, int64_t n_clusters, int64_t panel_rows);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_STREAM_H */
