"""Steps 2 and 3 of process_single_file for every slide of a ragged cohort in one call: the WSI x TMA similarity with its five
statistics (build_hypergraph/preprocess_hypergraph.py:248-265) and the grouping of its rows (:297-306); and the edge-weight
median filter of the rebuild (:885-897) for every slide of a cohort's edge list.

Slide s pairs wsi[wsi_ptr[s]:wsi_ptr[s+1]] (n_s super patches) with tma[tma_ptr[s]:tma_ptr[s+1]] (m_s TMA patches).  Its
similarity block is [n_s, m_s] row-major at s_ptr[s] = sum_{t<s} n_t m_t of one flat f32 buffer, and block and statistics are bit
for bit those of ``compute_wsi_tma_similarity`` on that slide.  The chain over a cohort:

    S_flat, s_ptr, sim_stats = compute_wsi_tma_similarity_segmented(wsi, pos, tma, wsi_ptr=wp, tma_ptr=tp)
    labels, group_stats, info = group_by_similarity_segmented(S_flat, G, wsi_ptr=wp, tma_ptr=tp)
    ei, ew, eptr, hg = build_hypergraph_knn_kmeans_segmented(wsi, tma, labels, wsi_ptr=wp, tma_ptr=tp)
    ei, ew, eptr, flt = filter_edges_by_median_segmented(ei, ew, eptr, ratio)

Every argument error is raised on the host before the device is touched (and before the "needs a ROCm device" RuntimeError),
and names the first bad slide.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, kmeans_ragged, ops, ragged
from .kmeans import segmented_labels
from .build_hypergraph import preprocess_hypergraph
from .build_hypergraph._common import compute_device, result_device_like_preprocess, to_gpu


# ---------------------------------------------------------------------------------------------------
# the two C entries
# ---------------------------------------------------------------------------------------------------
def sim_dense_stats_segmented(X: torch.Tensor, Y: torch.Tensor, *, x_ptr=None, x_batch=None, y_ptr=None, y_batch=None,
                              metric="rbf_direct", lam: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """ops.sim_dense_stats(X_s, Y_s, metric="rbf_direct") of every segment in one call (mmf_sim_dense_stats_segmented).  Returns
    (S_flat f32 [sum n_s m_s] on X's device, s_ptr int64 [S + 1] on the HOST, stats f64 [S, 5] on the device: mean, unbiased std,
    min, max, lower median).  Block s is S_flat[s_ptr[s]:s_ptr[s+1]].view(n_s, m_s); block and stats[s] carry the bits of the plain
    call on the segment's rows.  Nothing is read back: the call returns without waiting for the stream."""
    what = "sim_dense_stats_segmented"
    X = ops._feat(X, what + " X")
    Y = ops._feat(Y, what + " Y")
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"{what}: slide 0: X has D={X.shape[1]}, Y has D={Y.shape[1]}")
    if ops._metric(metric) != _lib.RBF_DIRECT:
        raise ValueError(f"{what}: only metric='rbf_direct' is supported (got {metric!r})")
    xp, yp = ragged.two_sided(X.shape[0], Y.shape[0], x_ptr, x_batch, y_ptr, y_batch, xs="x_", ys="y_", what=what, unit="slide",
                              min_rows=(1, 1))
    s_ptr = ragged.block_offsets(xp, yp)
    ops._need_gpu(X, what)
    if Y.device != X.device:
        raise ValueError(f"{what}: X and Y must share a device")
    Y = Y.to(X.dtype)
    S = xp.numel() - 1
    out = torch.empty((int(s_ptr[-1]),), dtype=torch.float32, device=X.device)
    stats = torch.empty((S, 5), dtype=torch.float64, device=X.device)
    ops._call("mmf_sim_dense_stats_segmented", X.device, ops._p(X), X.shape[0], ops._p(Y), Y.shape[0], X.shape[1], ops._DT[X.dtype],
              _lib.RBF_DIRECT, float(lam), ops._hp(xp), ops._hp(yp), S, ops._p(out), ops._p(stats))
    return out, s_ptr, stats


def lower_median_segmented(v: torch.Tensor, *, ptr=None, batch=None) -> torch.Tensor:
    """ops.lower_median (torch.median) of every block v[ptr[s]:ptr[s+1]] of a flat f32 tensor: device f32 [S], without a host
    synchronisation (mmf_lower_median_segmented).  Every block needs at least one value."""
    what = "lower_median_segmented"
    if v.dim() != 1:
        raise ValueError(f"{what}: expected a flat 1-D tensor, got shape {tuple(v.shape)}")
    p = ragged.offsets(ptr, batch, v.numel(), what=what, unit="slide", min_rows=1)
    ops._need_gpu(v, what)
    v = v.contiguous().float()
    out = torch.empty((p.numel() - 1,), dtype=torch.float32, device=v.device)
    ops._call("mmf_lower_median_segmented", v.device, ops._p(v), ops._hp(p), p.numel() - 1, ops._p(out))
    return out


# ---------------------------------------------------------------------------------------------------
# compute_wsi_tma_similarity over a cohort
# ---------------------------------------------------------------------------------------------------
def compute_wsi_tma_similarity_segmented(wsi_features: torch.Tensor, wsi_positions: torch.Tensor, tma_features: torch.Tensor,
                                         lambda_h: float = 1.0, lambda_g: float = 1.0, device: Optional[torch.device] = None, *,
                                         wsi_ptr=None, wsi_batch=None, tma_ptr=None,
                                         tma_batch=None) -> Tuple[torch.Tensor, torch.Tensor, List[Dict]]:
    """compute_wsi_tma_similarity of every slide of a cohort: (S_flat f32 [sum n_s m_s] on `device` (None: the features' device
    if it is a GPU, else the CPU, as the plain mirror), s_ptr host int64 [S + 1], one statistics dict per slide).  The dicts hold
    Python scalars as the plain mirror's do (the f32-rounded `.item()` values), out of ONE device -> host copy of the [S, 5]
    array.  `wsi_positions` and `lambda_g` are accepted and ignored, as in the mirror."""
    what = "compute_wsi_tma_similarity_segmented"
    if wsi_features.dim() != 2 or tma_features.dim() != 2:
        raise ValueError(f"{what}: wsi_features and tma_features must be 2-D [N, D]")
    if wsi_features.shape[1] != tma_features.shape[1]:
        raise ValueError(f"{what}: slide 0: wsi_features have D={wsi_features.shape[1]}, tma_features D={tma_features.shape[1]}")
    wp, tp = ragged.two_sided(wsi_features.shape[0], tma_features.shape[0], wsi_ptr, wsi_batch, tma_ptr, tma_batch, xs="wsi_",
                              ys="tma_", what=what, unit="slide", min_rows=(1, 1))
    out_dev = result_device_like_preprocess(wsi_features, device)
    dev = out_dev if out_dev.type == "cuda" else compute_device(wsi_features, tma_features)
    S_flat, s_ptr, stats = sim_dense_stats_segmented(to_gpu(wsi_features, dev), to_gpu(tma_features, dev), x_ptr=wp, y_ptr=tp,
                                                     metric="rbf_direct", lam=float(lambda_h))
    return S_flat.to(out_dev), s_ptr, ops._stats_dict(stats)


def similarity_block(S_flat: torch.Tensor, s_ptr, sizes: Sequence[Tuple[int, int]], s: int) -> torch.Tensor:
    """The [n_s, m_s] view of slide s; sizes[s] = (n_s, m_s)."""
    n_s, m_s = int(sizes[s][0]), int(sizes[s][1])
    return S_flat[int(s_ptr[s]):int(s_ptr[s + 1])].view(n_s, m_s)


# ---------------------------------------------------------------------------------------------------
# group_by_similarity over a cohort
# ---------------------------------------------------------------------------------------------------
def width_plan(n_sizes: Sequence[int], m_sizes: Sequence[int]) -> List[Dict]:
    """The slides of a cohort by TMA width.  Slide s clusters the n_s rows of an [n_s, m_s] matrix, and one segmented fit
    (kmeans_fit_predict_segmented) takes one feature dimension: the slides grouped by m_s, one fit per distinct width, in order of
    first appearance, each holding its slides in slide order.  group_by_similarity_segmented runs this plan when it has one
    entry, and with the 'sklearn' backend; a plan of several widths on the 'device' backend is ONE ragged fit instead
    (kmeans_ragged.kmeans_fit_predict_ragged).  Per fit: 'width', 'slides', 'fit_ptr' (offsets of the slides' rows in the fit's
    concatenated input: the labels fit_ptr[i]:fit_ptr[i+1] return to slide slides[i]) and 'adjacent' (the slides are
    consecutive, so their blocks are one contiguous piece of S_flat and need no copy)."""
    fits: Dict[int, Dict] = {}
    for s, (n_s, m_s) in enumerate(zip(n_sizes, m_sizes)):
        f = fits.setdefault(int(m_s), {"width": int(m_s), "slides": [], "fit_ptr": [0]})
        f["slides"].append(s)
        f["fit_ptr"].append(f["fit_ptr"][-1] + int(n_s))
    for f in fits.values():
        f["adjacent"] = f["slides"] == list(range(f["slides"][0], f["slides"][0] + len(f["slides"])))
    return list(fits.values())


def group_by_similarity_segmented(S_flat: torch.Tensor, num_groups: int, *, wsi_ptr=None, wsi_batch=None, tma_ptr=None,
                                  tma_batch=None, method: str = "kmeans"):
    """group_by_similarity of every slide's block of S_flat (the layout of compute_wsi_tma_similarity_segmented): (labels int32
    numpy [n_wsi], 0 .. num_groups - 1 within each slide; one stats dict per slide: method, num_groups, group_sizes; info:
    kmeans_backend and per slide ambiguous_draws / ambiguous_trials, None with the 'sklearn' backend).

    Slide s clusters the rows of an n_s x m_s matrix, so the feature dimension differs between slides.  With the 'device' backend
    and more than one distinct m_s the whole cohort is ONE kmeans_fit_predict_ragged call on S_flat itself (kmeans_ragged.py,
    DESIGN.md §4.22): every block keeps its own width for the means, the variances, scikit-learn's tolerance tol * mean(var) and
    the centring, and nothing is copied.  The input is never zero-padded to a common width, which would change that tolerance;
    only the fit's internal mean-centred copy is, where a zero column adds an exact 0.0.  One distinct width is one
    kmeans_fit_predict_segmented call, as before.  The 'sklearn' backend runs the reference's own call on the host, one fit per
    distinct width (width_plan), slide by slide."""
    what = "group_by_similarity_segmented"
    if method != "kmeans":
        raise ValueError(f"Unknown grouping method: {method}")
    if S_flat.dim() != 1:
        raise ValueError(f"{what}: S_flat must be the flat 1-D buffer of the blocks, got shape {tuple(S_flat.shape)}")
    num_groups = int(num_groups)
    wp, tp = ragged.two_sided(None, None, wsi_ptr, wsi_batch, tma_ptr, tma_batch, xs="wsi_", ys="tma_", what=what, unit="slide",
                              min_rows=(1, 1))
    s_ptr = ragged.block_offsets(wp, tp)
    if S_flat.numel() != int(s_ptr[-1]):
        raise ValueError(f"{what}: slide {wp.numel() - 2}: S_flat holds {S_flat.numel()} values, the blocks of the slides {int(s_ptr[-1])}")
    n_sizes, m_sizes = (wp[1:] - wp[:-1]).tolist(), (tp[1:] - tp[:-1]).tolist()
    ragged.check_kmeans_sizes(n_sizes, num_groups, what, "slide")
    S, n_wsi = len(n_sizes), int(wp[-1])
    dev = compute_device(S_flat)
    F = to_gpu(S_flat, dev)
    sp = s_ptr.tolist()
    backend = preprocess_hypergraph.KMEANS_BACKEND
    labels = torch.empty((n_wsi,), dtype=torch.int64, device=dev)
    draws: Optional[List[int]] = [0] * S if backend == "device" else None
    trials: Optional[List[int]] = [0] * S if backend == "device" else None
    plan = width_plan(n_sizes, m_sizes)
    if backend == "device" and len(plan) > 1:      # one ragged fit on S_flat itself: every slide's block with its own width
        labels, _, _, fit_info = kmeans_ragged.kmeans_fit_predict_ragged(F, num_groups, rows=n_sizes, widths=m_sizes, xoff=sp[:-1], n_init=10,
                                                                         seed=42, return_info=True)
        draws = [int(i["ambiguous_draws"]) for i in fit_info]
        trials = [int(i["ambiguous_trials"]) for i in fit_info]
        plan = []
    for fit in plan:
        sl, m = fit["slides"], fit["width"]
        if fit["adjacent"]:
            X = F[sp[sl[0]]:sp[sl[-1] + 1]].view(-1, m)
        else:
            X = torch.cat([F[sp[s]:sp[s + 1]].view(-1, m) for s in sl], dim=0)
        lab, fit_draws, fit_trials = segmented_labels(X, fit["fit_ptr"], num_groups)
        if fit["adjacent"]:
            labels[int(wp[sl[0]]):int(wp[sl[-1] + 1])] = lab
        else:
            dest = torch.cat([torch.arange(int(wp[s]), int(wp[s + 1])) for s in sl])
            labels[dest.to(dev)] = lab
        if draws is not None:
            for i, s in enumerate(sl):
                draws[s], trials[s] = fit_draws[i], fit_trials[i]
    slide_of_row = ragged.segment_ids(wp).to(dev)
    sizes = torch.bincount(slide_of_row * num_groups + labels, minlength=S * num_groups).cpu().view(S, num_groups).tolist()
    stats = [{"method": "kmeans", "num_groups": num_groups, "group_sizes": [int(v) for v in row]} for row in sizes]
    info = {"kmeans_backend": backend, "ambiguous_draws": draws, "ambiguous_trials": trials}
    return labels.cpu().numpy().astype(np.int32), stats, info


# ---------------------------------------------------------------------------------------------------
# the rebuild's edge-weight median filter over a cohort
# ---------------------------------------------------------------------------------------------------
def median_thresholds(medians: torch.Tensor, ratio: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(threshold f64, threshold f32) per slide from the f32 medians: `median.item() * ratio` is a float64 product
    (preprocess_hypergraph.py:887-888), and `weights >= threshold` compares an f32 tensor with a Python scalar, which torch
    rounds to the tensor's dtype first — the f32 threshold is that rounding."""
    thr64 = medians.to(torch.float64) * float(ratio)
    return thr64, thr64.to(torch.float32)


def filter_edges_by_median_segmented(edge_index: torch.Tensor, edge_weights: torch.Tensor, edge_ptr, ratio: float):
    """The edge-weight median filter of rebuild_hypergraph_from_similarity (:885-897) for every slide of the output of
    build_hypergraph_knn_kmeans_segmented: slide s keeps its edges with weight >= median(weights of slide s) * ratio.  Returns
    (edge_index [2, E'], edge_weights [E'], edge_ptr [S + 1] int64, one dict per slide: threshold (float64, the mirror's value),
    num_edges_after_threshold, threshold_ratio), tensors on the inputs' device.  One host read: the thresholds and the kept
    counts in one copy (edge_ptr is read on the host as every offset array is; pass host offsets to keep it at one).  A slide
    without edges raises ValueError, as torch.median of an empty tensor does."""
    what = "filter_edges_by_median_segmented"
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_weights.dim() != 1 or edge_index.shape[1] != edge_weights.shape[0]:
        raise ValueError(f"{what}: expected edge_index [2, E] and edge_weights [E], got {tuple(edge_index.shape)} and {tuple(edge_weights.shape)}")
    E = edge_weights.shape[0]
    p = ragged.offsets(edge_ptr, None, E, side="edge_", what=what, unit="slide")
    empty = torch.nonzero(p[1:] == p[:-1]).reshape(-1)
    if empty.numel():
        raise ValueError(f"{what}: slide {int(empty[0])} has no edges: the median of an empty tensor is undefined")
    S = p.numel() - 1
    out_dev = edge_weights.device
    dev = compute_device(edge_weights)
    w = to_gpu(edge_weights, dev)
    ei = edge_index.detach().to(device=dev, dtype=torch.int64).contiguous()
    med = lower_median_segmented(w, ptr=p)
    thr64, thr32 = median_thresholds(med, ratio)
    slide_of_edge = ragged.segment_ids(p).to(dev)
    mask = w >= thr32[slide_of_edge]
    kept = torch.zeros(S, dtype=torch.int64, device=dev).index_add_(0, slide_of_edge, mask.to(torch.int64))
    host = torch.stack([thr64, kept.to(torch.float64)], dim=1).cpu()          # the one host read
    kept_h = host[:, 1].to(torch.int64)
    E2 = int(kept_h.sum())
    # ordered compaction without a second read: kept edge e goes to position (number of kept edges before e); the others to a
    # spare slot at the end that is cut off
    pos = torch.where(mask, torch.cumsum(mask.to(torch.int64), 0) - 1, torch.full_like(slide_of_edge, E2))
    ew2 = torch.empty((E2 + 1,), dtype=torch.float32, device=dev).scatter_(0, pos, w)[:E2]
    ei2 = torch.empty((2, E2 + 1), dtype=torch.int64, device=dev).scatter_(1, pos.unsqueeze(0).expand(2, -1), ei)[:, :E2].contiguous()
    new_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(kept_h, 0)])
    stats = [{"threshold": float(t), "num_edges_after_threshold": int(k), "threshold_ratio": ratio}
             for t, k in zip(host[:, 0].tolist(), kept_h.tolist())]
    return ei2.to(out_dev), ew2.contiguous().to(out_dev), new_ptr.to(out_dev), stats
