"""Step 1 of process_single_file for every slide of a ragged cohort in one call: super-patch aggregation
(build_hypergraph/preprocess_hypergraph.py:87-199 of the reference; aggregate_wsi_super_patches here), DESIGN.md §4.12.

Slide s is rows ptr[s] .. ptr[s+1]-1 of the features / positions (n_s patches), given by exactly one of ``ptr`` ([S + 1] offsets)
/ ``batch`` ([N] sorted slide id per row).  With C super patches per slide, slide s's super patches are rows s*C .. (s+1)*C - 1 of
the outputs, its similarity block K_s is [n_s, n_s] row-major at k_ptr[s] = sum_{t<s} n_t^2 of one flat f32 buffer, and features,
positions, block and statistics are bit for bit those of ``aggregate_wsi_super_patches`` on that slide.

    counts, offsets, order, status = segment_sort_segmented(labels, C, ptr=p)                  # mmf_segment_sort_segmented
    super_f, super_p, intra, k_stats = pool_super_patches_segmented(F, P, order, offsets, C, ptr=p, K_flat=K)
    sf, sp, stats, K_flat, k_ptr = aggregate_wsi_super_patches_segmented(F, P, C, ptr=p)       # the mirror over the cohort

Every argument error is raised on the host before the device is touched, and names the first bad slide.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops, ragged
from .kmeans import segmented_labels
from .super_patch_stats import super_patch_stats_streamed
from .build_hypergraph import preprocess_hypergraph, similarity_kernel
from .build_hypergraph._common import compute_device, result_device_like_preprocess, to_gpu

STREAM_MIN_VALUES = 1 << 22   # a block of fewer values (16 MiB) is stored even when it alone exceeds the budget
MAX_CLUSTERS = 16384          # clusters per slide (the LDS histogram of one slide's chunk, csrc/mmf_pool.hip)


_cohort_labels = segmented_labels      # looked up at call time: a test puts labels of its own in its place


def _check_clusters(sizes, n_clusters: int, what: str) -> None:
    """What scikit-learn raises for a slide with fewer rows than clusters, with the slide named; the per-slide limit; G < 2^31."""
    ragged.check_kmeans_sizes(sizes, n_clusters, what, "slide")
    if n_clusters > MAX_CLUSTERS:
        raise ValueError(f"{what}: slide 0: at most {MAX_CLUSTERS} clusters per slide are supported (got {n_clusters})")
    if len(sizes) * n_clusters >= 2 ** 31:
        raise ValueError(f"{what}: slide {len(sizes) - 1}: {len(sizes)} slides x {n_clusters} clusters must stay below 2^31")


def group_plan(sizes, budget_bytes: int) -> List[Tuple[int, int]]:
    """Consecutive slides [a, b) whose blocks K_s (n_s^2 f32 each) fit `budget_bytes` together (ragged.budget_groups); a
    slide whose block alone is larger is a group of its own."""
    return [(a, b) for a, b, _ in ragged.budget_groups([int(v) for v in sizes], int(budget_bytes))]


# ---------------------------------------------------------------------------------------------------
# the two C entries
# ---------------------------------------------------------------------------------------------------
def segment_sort_segmented(labels: torch.Tensor, n_clusters: int, *, ptr=None, batch=None):
    """ops.segment_sort of every slide's labels (local, in [0, n_clusters)) in one call (mmf_segment_sort_segmented).  Returns
    (counts int64 [G], offsets int64 [G + 1], order int64 [n] of GLOBAL row ids, status int64 [2]), all on the device, with
    G = S * n_clusters and cluster g = s * n_clusters + label: order[offsets[g]:offsets[g+1]] are the rows of cluster g, ascending.
    status[0] is the lowest row with a label outside its range or -1 (such rows are skipped), status[1] the lowest empty g or -1.
    Nothing is read back: the call returns without waiting for the stream."""
    what = "segment_sort_segmented"
    if labels.dim() != 1:
        raise ValueError(f"{what}: expected a flat 1-D label vector, got shape {tuple(labels.shape)}")
    n, C = labels.numel(), int(n_clusters)
    p = ragged.offsets(ptr, batch, n, what=what, unit="slide")
    S = p.numel() - 1
    if C < 1 or C > MAX_CLUSTERS:
        raise ValueError(f"{what}: slide 0: n_clusters must lie in [1, {MAX_CLUSTERS}] (got {C})")
    if S * C >= 2 ** 31:
        raise ValueError(f"{what}: slide {S - 1}: {S} slides x {C} clusters must stay below 2^31")
    ops._need_gpu(labels, what)
    lab = labels.to(torch.int64).contiguous()
    dev = lab.device
    counts = torch.empty((S * C,), dtype=torch.int64, device=dev)
    offsets = torch.empty((S * C + 1,), dtype=torch.int64, device=dev)
    order = torch.empty((n,), dtype=torch.int64, device=dev)
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    ops._call("mmf_segment_sort_segmented", dev, ops._p(lab), n, ops._hp(p), S, C, ops._p(counts), ops._p(offsets), ops._p(order),
              ops._p(status))
    return counts, offsets, order, status


def pool_super_patches_segmented(F: torch.Tensor, P: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, n_clusters: int, *,
                                 ptr, K_flat: Optional[torch.Tensor] = None):
    """The pooling of every slide over the members that segment_sort_segmented found (mmf_super_patches_segmented).  Returns
    (super_f f32 [G, D], super_p f32 [G, dp], intra_mean f64 [G], k_stats f64 [S, 5]) on the device; the last two are None without
    K_flat.  Per slide the bits of ops.segment_mean(F_s), ops.segment_mean(P_s), ops.segment_offdiag_mean(K_s) (NaN for a cluster
    of fewer than two rows) and of the five doubles of mmf_array_stats(K_s).  K_flat: the blocks in the layout of
    ops.sim_dense_combined_segmented.  Nothing is read back: the call returns without waiting for the stream (a block of 2^22
    values or more takes mmf_array_stats' one sweep, which reads its verdict: one wait per such block)."""
    what = "pool_super_patches_segmented"
    if F.dim() != 2 or P.dim() != 2 or P.shape[0] != F.shape[0]:
        raise ValueError(f"{what}: slide 0: features [N, D] and positions [N, dp] must share N")
    n, C = F.shape[0], int(n_clusters)
    p = ragged.offsets(ptr, None, n, what=what, unit="slide", min_rows=0 if K_flat is None else 1)
    S = p.numel() - 1
    if C < 1 or S * C >= 2 ** 31:
        raise ValueError(f"{what}: slide 0: bad n_clusters {C}")
    if order.numel() != n or offsets.numel() != S * C + 1:
        raise ValueError(f"{what}: slide 0: order must hold {n} rows and offsets {S * C + 1} entries "
                         f"(got {order.numel()} and {offsets.numel()})")
    if K_flat is not None:
        total = int(ragged.block_offsets(p)[-1])
        if K_flat.dim() != 1 or K_flat.numel() != total:
            raise ValueError(f"{what}: slide {S - 1}: K_flat holds {K_flat.numel()} values, the blocks of the slides {total}")
    ops._need_gpu(F, what)
    F, P = F.float().contiguous(), P.float().contiguous()
    dev = F.device
    if P.device != dev or order.device != dev or offsets.device != dev or (K_flat is not None and K_flat.device != dev):
        raise ValueError(f"{what}: all tensors must share a device")
    order, offsets = order.to(torch.int64).contiguous(), offsets.to(torch.int64).contiguous()
    super_f = torch.empty((S * C, F.shape[1]), dtype=torch.float32, device=dev)
    super_p = torch.empty((S * C, P.shape[1]), dtype=torch.float32, device=dev)
    intra = k_stats = None
    if K_flat is not None:
        K_flat = K_flat.float().contiguous()
        intra = torch.empty((S * C,), dtype=torch.float64, device=dev)
        k_stats = torch.empty((S, 5), dtype=torch.float64, device=dev)
    ops._call("mmf_super_patches_segmented", dev, ops._p(F), ops._p(P), n, F.shape[1], P.shape[1], ops._hp(p), S, C, ops._p(order),
              ops._p(offsets), ops._p(K_flat), ops._p(super_f), ops._p(super_p), ops._p(intra), ops._p(k_stats))
    return super_f, super_p, intra, k_stats


# ---------------------------------------------------------------------------------------------------
# aggregate_wsi_super_patches over a cohort
# ---------------------------------------------------------------------------------------------------
def aggregate_wsi_super_patches_segmented(wsi_features: torch.Tensor, wsi_positions: torch.Tensor, num_super_patches: int,
                                          lambda_h: float = 1.0, lambda_g: float = 1.0, device: Optional[torch.device] = None,
                                          wsi_similarity_flat: Optional[torch.Tensor] = None, *, ptr=None, batch=None,
                                          keep_similarity: bool = True, budget_bytes: Optional[int] = None,
                                          return_info: bool = False):
    """aggregate_wsi_super_patches of every slide of a cohort: (super_features [S*C, D], super_positions [S*C, dp], one stats dict per
    slide, K_flat f32 [sum n_s^2] or None, k_ptr host int64 [S + 1]) — and an info dict (kmeans_backend, per slide ambiguous_draws /
    ambiguous_trials, None with the 'sklearn' backend; the groups) with return_info=True.  Tensors live on `device` (None: the
    features' device if it is a GPU, else the CPU, as the plain mirror).  Each stats dict equals the plain mirror's for that slide.

    The labels come from one kmeans_fit_predict_segmented call.  `wsi_similarity_flat`, if given, is used as K (the blocks in the
    layout of ops.sim_dense_combined_segmented) and returned; otherwise K is computed.  With keep_similarity=False no K is
    returned and the slides are processed in groups of consecutive slides whose blocks fit `budget_bytes` together (default:
    similarity_kernel.STREAM_BYTES).  A slide whose block alone exceeds the budget runs alone, and if that block holds 2^22 values
    or more it is never stored: its statistics come from super_patch_stats_streamed, which recomputes K in row panels
    (similarity_kernel.PANEL_ROWS) and returns the same bits (a smaller block over the budget, 16 MiB at most, is still stored).
    info["streamed"] says per group whether that happened.  One host read per group (status, intra means, statistics) besides
    the KMeans call's own.  An empty cluster raises ValueError(f"slide {s}: Cluster {c} is empty")."""
    what = "aggregate_wsi_super_patches_segmented"
    if wsi_features.dim() != 2 or wsi_positions.dim() != 2:
        raise ValueError(f"{what}: slide 0: wsi_features [N, D] and wsi_positions [N, dp] must be 2-D")
    if wsi_positions.shape[0] != wsi_features.shape[0]:
        raise ValueError(f"{what}: slide 0: wsi_features have {wsi_features.shape[0]} rows, wsi_positions {wsi_positions.shape[0]}")
    N, C = wsi_features.shape[0], int(num_super_patches)
    p = ragged.offsets(ptr, batch, N, what=what, unit="slide", min_rows=1)
    sizes = (p[1:] - p[:-1]).tolist()
    S = len(sizes)
    _check_clusters(sizes, C, what)
    k_ptr = ragged.block_offsets(p)
    if wsi_similarity_flat is not None and (wsi_similarity_flat.dim() != 1 or wsi_similarity_flat.numel() != int(k_ptr[-1])):
        raise ValueError(f"{what}: slide {S - 1}: wsi_similarity_flat must be the flat 1-D buffer of the blocks: it holds "
                         f"{wsi_similarity_flat.numel()} values, the blocks of the slides {int(k_ptr[-1])}")
    budget = int(similarity_kernel.STREAM_BYTES if budget_bytes is None else budget_bytes)
    whole = keep_similarity or wsi_similarity_flat is not None
    plan = [(0, S, False)] if whole else ragged.budget_groups([int(v) for v in sizes], budget)
    groups = [(a, b) for a, b, _ in plan]
    # a slide that budget_groups set apart is streamed unless its block is small enough to go through the plain routines anyway
    streamed = [bool(alone) and not whole and int(sizes[a]) ** 2 >= STREAM_MIN_VALUES for a, _, alone in plan]
    out_dev = result_device_like_preprocess(wsi_features, device)
    dev = out_dev if out_dev.type == "cuda" else compute_device(wsi_features, wsi_positions)
    F, P = to_gpu(wsi_features, dev), to_gpu(wsi_positions, dev)
    lh, lg = float(lambda_h), float(lambda_g)
    K_all = to_gpu(wsi_similarity_flat, dev) if wsi_similarity_flat is not None else None
    labels, draws, trials = _cohort_labels(F, p, C)
    super_f = torch.empty((S * C, F.shape[1]), dtype=torch.float32, device=dev)
    super_p = torch.empty((S * C, P.shape[1]), dtype=torch.float32, device=dev)
    stats: List[Dict] = []
    for (a, b), stream in zip(groups, streamed):
        r0, r1 = int(p[a]), int(p[b])
        local = (p[a:b + 1] - r0).contiguous()
        Fg, Pg = F[r0:r1], P[r0:r1]
        if stream:
            K = None
        elif K_all is not None:
            K = K_all[int(k_ptr[a]):int(k_ptr[b])]
        else:
            K, _ = ops.sim_dense_combined_segmented(Fg, Pg, lh, lg, ptr=local)
            if whole:
                K_all = K
        _, offsets, order, status = segment_sort_segmented(labels[r0:r1], C, ptr=local)
        sf, sp, intra, k_stats = pool_super_patches_segmented(Fg, Pg, order, offsets, C, ptr=local, K_flat=K)
        if stream:                                     # one slide: its local rows are the rows mmf_segment_sort would give
            intra, k_stats = super_patch_stats_streamed(Fg, Pg, order, offsets, C, lh, lg, panel_rows=similarity_kernel.PANEL_ROWS)
        super_f[a * C:b * C], super_p[a * C:b * C] = sf, sp
        host = torch.cat([status.to(torch.float64), intra, k_stats.reshape(-1)]).cpu().numpy()      # the group's one host read
        del K
        G = (b - a) * C
        if host[0] >= 0:
            r = int(host[0])
            s = a + int(np.searchsorted(local.numpy(), r, side="right")) - 1
            raise ValueError(f"{what}: slide {s}: row {r0 + r} has a label outside [0, {C})")
        if host[1] >= 0:
            g = int(host[1])
            raise ValueError(f"slide {a + g // C}: Cluster {g % C} is empty")
        intra32 = host[2:2 + G].astype(np.float32).reshape(b - a, C)      # each cluster's mean is an f32 `.item()` upstream
        st32 = host[2 + G:].astype(np.float32).reshape(b - a, 5).tolist()
        for i in range(b - a):
            v = intra32[i][~np.isnan(intra32[i])]
            stats.append({"num_original_patches": int(sizes[a + i]), "num_super_patches": C,
                          "avg_intra_cluster_similarity": float(np.mean(v.astype(np.float64))) if v.size else 0.0,
                          "wsi_similarity_matrix_stats": dict(zip(ops.STAT_KEYS, st32[i]))})
    K_out = K_all.to(out_dev) if (keep_similarity and K_all is not None) else None
    res = (super_f.to(out_dev), super_p.to(out_dev), stats, K_out, k_ptr)
    if return_info:
        info = {"kmeans_backend": preprocess_hypergraph.KMEANS_BACKEND, "ambiguous_draws": draws, "ambiguous_trials": trials,
                "groups": [list(g) for g in groups], "streamed": streamed}
        return res + (info,)
    return res
