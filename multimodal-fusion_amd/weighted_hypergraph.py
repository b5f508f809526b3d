"""The threshold-by-median weighted hypergraph (build_hypergraph/similarity_kernel.py:126-306) of every graph of a ragged
batch in one call: what a GNN data loader needs for each sample of a mini-batch, without one Python call per graph.

Segment s is rows ``ptr[s] .. ptr[s+1]-1`` of features / positions, given by exactly one of ``ptr`` ([S + 1] offsets) /
``batch`` ([N] sorted segment id per row, PyG's convention).  Segment s's edges are bit for bit those of
``build_weighted_hypergraph(F_s, P_s, lambda_h, lambda_g, ratio)`` with both ids shifted by ``ptr[s]``.

Consecutive segments go in groups whose blocks K_s (n_s^2 f32 each) fit ``similarity_kernel.STREAM_BYTES`` together; a group
costs one launch per step and two host synchronisations (the medians, then the edge count).  A segment whose block alone is
larger takes the plain builder's streaming path (K recomputed in row panels), as ``build_weighted_hypergraph`` would.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops, ragged
from .build_hypergraph import similarity_kernel
from .build_hypergraph._common import compute_device, f32_ceil, result_device_like_kernel, to_gpu

SEGMENT_MEAN_MAX = 16384      # segments per mmf_segment_mean launch (the cluster steps' limit, csrc/mmf_segments.hip)


def f32_ceil_array(x: np.ndarray) -> np.ndarray:
    """_common.f32_ceil of every element of a float64 array: the smallest float32 >= x (NaN stays NaN)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = x.astype(np.float32)
        up = t.astype(np.float64) < x
    t[up] = np.nextafter(t[up], np.float32(np.inf))
    return t


def _segments(features: torch.Tensor, positions: torch.Tensor, ptr, batch, what: str) -> torch.Tensor:
    """Host offsets, checked before any device work: shapes, ptr / batch, and at least two rows per segment."""
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    p = ragged.offsets(ptr, batch, features.shape[0], what=what)
    sizes = p[1:] - p[:-1]
    small = torch.nonzero(sizes <= 1)
    if small.numel():
        s = int(small[0])
        raise ValueError(f"{what}: segment {s}: Number of nodes must be greater than 1, got N={int(sizes[s])}. "
                         f"Hypergraph construction requires at least 2 nodes.")
    return p


_groups = ragged.budget_groups      # the name tests and DESIGN.md know it by


def _need_ratio(ratio, what: str) -> None:
    if ratio is None:                             # the plain builder fails at `median_sim * None` (similarity_kernel.py:188)
        raise TypeError(f"{what}: unsupported operand type(s) for *: 'float' and 'NoneType' (threshold_median_ratio is required)")


def build_weighted_hypergraph_segmented(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0,
                                        lambda_g: float = 1.0, threshold_median_ratio: float = None,
                                        device: Optional[torch.device] = None, *, ptr=None,
                                        batch=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """build_weighted_hypergraph of every segment: (edge_index [2, E] int64 with global row ids, edge_weights [E] f32,
    edge_ptr [S + 1] int64; segment s's edges are edge_ptr[s]:edge_ptr[s+1]), on `device` (None: the features' device).
    As the plain mirror: a segment of N <= 1 rows raises ValueError and ratio None TypeError, here before any device work."""
    what = "build_weighted_hypergraph_segmented"
    p = _segments(features, positions, ptr, batch, what)
    _need_ratio(threshold_median_ratio, what)
    ratio = float(threshold_median_ratio)
    out_dev = result_device_like_kernel(features, device)
    dev = compute_device(features, positions) if out_dev.type != "cuda" else out_dev
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    lh, lg = float(lambda_h), float(lambda_g)
    sizes = (p[1:] - p[:-1]).tolist()
    eis, ews, counts = [], [], []
    for a, b, streamed in _groups(sizes, similarity_kernel.STREAM_BYTES):
        r0, r1 = int(p[a]), int(p[b])
        Fg, Pg = F[r0:r1], P[r0:r1]
        if streamed:                              # the plain builder's path for a block that is not kept
            med = ops.combined_offdiag_median(Fg, Pg, lh, lg, similarity_kernel.PANEL_ROWS).item()
            thr = f32_ceil(med * ratio)
            ei, ew = ops.combined_threshold_edges(Fg, Pg, thr, lh, lg, similarity_kernel.PANEL_ROWS)
            cnt = [ei.shape[1]]
        else:
            local = p[a:b + 1] - r0
            K, _ = ops.sim_dense_combined_segmented(Fg, Pg, lh, lg, ptr=local)
            med = ops.offdiag_lower_median_segmented(K, ptr=local).cpu().numpy().astype(np.float64)
            thr = f32_ceil_array(med * ratio)
            ei, ew, eptr = ops.threshold_edges_segmented(K, thr, ptr=local)
            cnt = (eptr[1:] - eptr[:-1]).tolist()
            del K
        eis.append(ei + r0 if r0 else ei)
        ews.append(ew)
        counts.extend(cnt)
    edge_index = torch.cat(eis, dim=1) if len(eis) > 1 else eis[0]
    edge_weights = torch.cat(ews) if len(ews) > 1 else ews[0]
    edge_ptr = torch.zeros(len(counts) + 1, dtype=torch.int64)
    edge_ptr[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0)
    return edge_index.to(out_dev).contiguous(), edge_weights.to(out_dev), edge_ptr.to(out_dev)


def segment_mean_pool(features: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """[S, D] mean of every segment's rows (mmf_segment_mean over order = arange(N), offsets = ptr: one launch per
    16384 segments), on the features' device.  Matches torch.mean per slice to within f32 rounding, not bit for bit."""
    dev = compute_device(features)
    X = to_gpu(features, dev)
    n, S = X.shape[0], p.numel() - 1
    order = torch.arange(n, dtype=torch.int64, device=dev)
    offsets = p.to(dev)
    parts = []
    for a in range(0, S, SEGMENT_MEAN_MAX):
        b = min(a + SEGMENT_MEAN_MAX, S)
        seg = ops.Segments(None, offsets[a:b + 1], order, n, b - a)
        parts.append(ops.segment_mean(X, seg))
    out = torch.cat(parts) if len(parts) > 1 else parts[0]
    return out.to(features.device)


def build_hypergraph_data_segmented(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0,
                                    lambda_g: float = 1.0, threshold_median_ratio: float = None, use_pooling: bool = True,
                                    device: Optional[torch.device] = None, *, ptr=None, batch=None) -> dict:
    """build_hypergraph_data of every segment, packed as a PyG Batch would be: x [N, D], edge_index [2, E] (global ids),
    edge_attr [E], pos [N, dp], batch [N] (segment id per row), ptr [S + 1], and pooled_feature [S, D] (the mean of every
    segment's rows) when use_pooling — all on `device` (None: the features' device)."""
    what = "build_hypergraph_data_segmented"
    p = _segments(features, positions, ptr, batch, what)
    _need_ratio(threshold_median_ratio, what)
    if device is None:
        device = features.device
    features = features.to(device)
    positions = positions.to(device)
    edge_index, edge_weights, _ = build_weighted_hypergraph_segmented(features, positions, lambda_h, lambda_g,
                                                                      threshold_median_ratio, device, ptr=p)
    result = {"x": features, "edge_index": edge_index, "edge_attr": edge_weights, "pos": positions,
              "batch": ragged.segment_ids(p).to(device), "ptr": p.to(device)}
    if use_pooling:
        result["pooled_feature"] = segment_mean_pool(features, p)
    return result
