/* mmf_hg_kmeans_ragged.h — scikit-learn's KMeans fit for every block of a ragged batch whose blocks have feature widths of
 * their own, in one call.  mmf_kmeans_fit_segmented takes one feature dimension for all segments; the grouping
 * step of a cohort clusters the rows of an n_s x m_s WSI x TMA block per slide, and m_s differs from slide to slide.  An addition
 * to ABI version 3 of mmf_hg.h, whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`,
 * mmf_last_error); bound from the list EXPORTS_KMEANS_RAGGED of multimodal-fusion_amd/_lib.py.
 *
 * Output contract: for every segment, bit for bit what mmf_kmeans_fit returns on that block with the segment's row of
 * first_centres and the shared uniforms: labels, centres, seeds and every info field but [6].
 *
 * How: consecutive segments, in call order, run as one lockstep group, as in mmf_kmeans_fit_segmented.  A group's mean-centred
 * copy has one internal width, that of its widest segment rounded up to 32, with zeros behind each segment's own columns; the
 * means, the variances, the tolerance tol * mean(var), the centring and the convergence test's shift sum are taken over the
 * segment's own width.  The input is never zero-padded.  A group holds at most 16384 / (n_init * n_clusters) segments, fewer
 * than 2^31 / n_init rows and a bounded scratch, and closes before a segment that would make its padded volume (rows x internal
 * width, summed) exceed twice the unpadded one (rows x own width rounded up to 32): pass the segments sorted by width for tight
 * groups.  mmf_kmeans_ragged_groups answers how a call would be grouped.
 *
 * Host-synchronous: once per Lloyd iteration of each group (one small status block), once more per group when info is given.
 * All work is issued on `hip_stream`.  The segment table and the random stream are read on the host during the call.
 */
#ifndef MMF_HG_KMEANS_RAGGED_H
#define MMF_HG_KMEANS_RAGGED_H

#include "../mmf_hg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* V: device f32 [n_values], one flat buffer.  Segment s is rows[s] x width[s], row-major, at element xoff[s]; the blocks need
 * not be adjacent or in memory order (xoff, rows, width: HOST int64 [n_seg]).  first_centres: HOST int64 [n_seg][n_init], rows
 * local to the segment; uniforms: HOST f64 [n_init][n_clusters - 1][trials], shared by all segments (may be NULL when
 * n_clusters == 1).  labels: device int64 [sum rows], segment after segment in call order, 0 .. n_clusters - 1 within each;
 * centres: device f32 or NULL, segment s is [n_clusters][width[s]] at element n_clusters * sum_{t<s} width[t]; seeds: device int64
 * [n_seg][n_init][n_clusters] or NULL, rows local to the segment; info: HOST f64 [n_seg][7 + 2 n_init] or NULL, the fields of
 * mmf_kmeans_fit_segmented ([6]: the Lloyd lockstep iterations of the segment's group).
 * Checked on the host before any device call, every message naming the entry and the first bad segment: device_id < 0 ->
 * MMF_E_UNSUPPORTED first; MMF_E_INVALID for n_seg < 1, n_clusters < 1, n_init < 1, trials < 1, max_iter < 1, tol < 0, a NULL V,
 * table, first_centres, uniforms (n_clusters > 1) or labels, rows[s] < n_clusters, width[s] < 1, xoff[s] < 0,
 * xoff[s] + rows[s] * width[s] > n_values, a first centre outside [0, rows[s]); MMF_E_UNSUPPORTED where one segment alone breaks
 * a limit of mmf_kmeans_fit: n_init * n_clusters > 16384, trials > 64, n_init * rows[s] >= 2^31. */
int mmf_kmeans_fit_ragged(const float* V, int64_t n_values, const int64_t* xoff, const int64_t* rows, const int64_t* width,
                          int64_t n_seg, int64_t n_clusters, int64_t n_init, int trials, const int64_t* first_centres,
                          const double* uniforms, int max_iter, double tol, int64_t* labels, float* centres, int64_t* seeds,
                          double* info, int device_id, void* hip_stream);

/* Host only (no device, no stream): the lockstep groups of a call with these rows and widths.  Group g is the segments
 * bounds[g] .. bounds[g + 1] - 1 (bounds: [n_seg + 1], the first count + 1 entries are written); ds[s] (may be NULL) is the
 * internal width of segment s's group.  Returns the group count (>= 1), or a negative status: MMF_E_INVALID for NULL rows, width
 * or bounds, n_seg < 1, n_clusters < 1, n_init < 1, trials < 1, rows[s] < n_clusters or width[s] < 1; MMF_E_UNSUPPORTED for the
 * per-segment limits above. */
int64_t mmf_kmeans_ragged_groups(const int64_t* rows, const int64_t* width, int64_t n_seg, int64_t n_clusters, int64_t n_init,
                                 int trials, int64_t* bounds, int64_t* ds);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_KMEANS_RAGGED_H */
