/* mmf_hg_pool.h — super-patch aggregation over a cohort: what aggregate_wsi_super_patches does with the
 * KMeans labels of ONE slide (build_hypergraph/preprocess_hypergraph.py:157-197: the member sort, the per-cluster means of features
 * and positions, the mean off-diagonal similarity inside every cluster, the five statistics of K), for every slide of a ragged
 * batch in a fixed number of launches.  Additions to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device
 * pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list EXPORTS_POOL of multimodal-fusion_amd/_lib.py.
 *
 * Segment s is rows ptr_host[s] .. ptr_host[s+1]-1.  ptr_host is a HOST int64 array [n_seg + 1] (starts at 0, never decreases, ends
 * at n), checked before any device work and copied at call time: the caller may free it when the call returns.  Labels are local
 * to their segment, in [0, n_clusters); global cluster g = s * n_clusters + label; G = n_seg * n_clusters.  Neither entry waits
 * for the stream, whatever n_seg (one exception, inherited: a block K_s of 2^22 values or more goes through mmf_array_stats' one
 * sweep, whose verdict is one host read per such block).
 */
#ifndef MMF_HG_POOL_H
#define MMF_HG_POOL_H

#include "mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stable counting sort of every segment on its own: order[offsets[g] .. offsets[g+1]) holds the rows (GLOBAL row ids) of cluster
 * g in ascending order — per slice what mmf_segment_sort(labels_s, n_s, n_clusters) returns, with ptr[s] added; counts [G];
 * offsets [G + 1], the exclusive scan over all G counts.
 * status (device int64 [2]): status[0] = the lowest row whose label lies outside [0, n_clusters), or -1 (such rows are skipped);
 * status[1] = the lowest g with counts[g] == 0, or -1.  Both stay on the device for the caller's one read.
 * Limits: n_clusters <= 16384 (the LDS histogram of one segment), G < 2^31, n < 2^31. */
int mmf_segment_sort_segmented(const int64_t* labels, int64_t n, const int64_t* ptr_host, int64_t n_seg, int64_t n_clusters,
                               int64_t* counts, int64_t* offsets, int64_t* order, int64_t* status, int device_id, void* hip_stream);

/* Pooling over the sorted members.  Every output carries the bits of the plain entry on the segment's slice:
 *   super_f [G, d], super_p [G, dp]   mmf_segment_mean(F_s), mmf_segment_mean(P_s)
 *   intra_mean [G] (f64)              mmf_segment_offdiag_mean(K_s): NaN for a cluster of fewer than two rows
 *   k_stats [n_seg][5] (f64)          mmf_array_stats(K_s, n_s^2): mean, unbiased std, min, max, lower median
 * K_flat: the blocks K_s [n_s, n_s] row-major at kptr[s] = sum_{t<s} n_t^2 (the layout of mmf_sim_dense_combined_segmented);
 * NULL: intra_mean and k_stats are not written (and may be NULL).  With K_flat every segment needs at least one row.
 * order / offsets: what mmf_segment_sort_segmented wrote, with status == {-1, -1} (an empty cluster's means are NaN). */
int mmf_super_patches_segmented(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, const int64_t* ptr_host,
                                int64_t n_seg, int64_t n_clusters, const int64_t* order, const int64_t* offsets,
                                const float* K_flat, float* super_f, float* super_p, double* intra_mean, double* k_stats,
                                int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_POOL_H */
