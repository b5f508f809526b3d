"""The k best columns per row of the combined similarity K = K_h * K_g (the RBF of the patch features times the RBF of the patch
positions, build_hypergraph/similarity_kernel.py:88-124) of one graph or of every graph of a ragged batch, and the directed
edge list they make.  K is never stored: the exact f32 scan ranks by the exponent of K in its epilogue
(mmf_simtopk_combined, include/mmf_hg_topk.h), so the cost in memory is N * k, not N * N.

The reference has no counterpart: its only sparse form of K is the median threshold of build_weighted_hypergraph, which keeps
half of all pairs.  Segments are given by exactly one of ``ptr`` ([S + 1] offsets) / ``batch`` ([N] sorted segment id per row,
PyG's convention); without either the rows are one graph.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib, ops, ragged
from .build_hypergraph._common import compute_device, result_device_like_kernel, to_gpu
from .weighted_hypergraph import segment_mean_pool


def _inputs(features: torch.Tensor, positions: torch.Tensor, k: int, ptr, batch, what: str) -> torch.Tensor:
    """Host offsets ([0, N] for one graph), checked before any device work: shapes, k, ptr / batch."""
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if ptr is None and batch is None:
        return torch.tensor([0, features.shape[0]], dtype=torch.int64)
    return ragged.offsets(ptr, batch, features.shape[0], what=what, allow_no_segments=True)


def simtopk_combined(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *,
                     ptr=None, batch=None, exclude_self: bool = True, col_splits: int = 0, return_stats: bool = False,
                     profile: bool = False):
    """(idx [N, k] int64, val [N, k] f32[, stats dict]): per row the k columns of its own segment with the largest
    exp(-lambda_h |f_i - f_j|^2) * exp(-lambda_g |p_i - p_j|^2), ranked by the exponent (then by id), val the product itself —
    the entry ops.sim_dense_combined writes, bit for bit.  idx holds global row ids; a row whose segment has fewer than k
    admissible columns gets them first, then -1 / -inf.  CPU tensors are computed on the current GPU and the result moved back."""
    what = "simtopk_combined"
    p = _inputs(features, positions, k, ptr, batch, what)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    n, d = F.shape
    idx = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    if n > 0:
        one = ptr is None and batch is None
        opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        ops._call("mmf_simtopk_combined", dev, ops._p(F), ops._p(P), n, d, P.shape[1], float(lambda_h), float(lambda_g), int(k),
                  int(bool(exclude_self)), ops._hp(None if one else p), 0 if one else p.numel() - 1, ops._p(idx), ops._p(val),
                  ctypes.byref(opts), ctypes.byref(stats))
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def build_topk_weighted_hypergraph(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                   k: int = 5, device: Optional[torch.device] = None, *, ptr=None,
                                   batch=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The directed top-k edges of every segment: (edge_index [2, E] int64 with global row ids, edge_weights [E] f32, edge_ptr
    [S + 1] int64; segment s's edges are edge_ptr[s]:edge_ptr[s+1]) on `device` (None: the features' device), the layout of
    build_weighted_hypergraph_segmented.  Edge (i, idx[i, r]) with weight val[i, r]; rows ascend and r ascends within a row; a
    segment of n_s rows gives n_s * min(k, n_s - 1) edges (the -1 entries are dropped)."""
    what = "build_topk_weighted_hypergraph"
    p = _inputs(features, positions, k, ptr, batch, what)
    out_dev = result_device_like_kernel(features, device)
    dev = compute_device(features, positions) if out_dev.type != "cuda" else out_dev
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    idx, val = simtopk_combined(F, P, lambda_h, lambda_g, k, ptr=p)
    keep = idx >= 0
    rows = torch.arange(idx.shape[0], dtype=torch.int64, device=dev).unsqueeze(1).expand_as(idx)
    edge_index = torch.stack([rows[keep], idx[keep]])
    sizes = p[1:] - p[:-1]
    edge_ptr = torch.zeros(p.numel(), dtype=torch.int64)
    edge_ptr[1:] = torch.cumsum(sizes * torch.clamp(sizes - 1, min=0, max=int(k)), 0)
    return edge_index.to(out_dev).contiguous(), val[keep].to(out_dev), edge_ptr.to(out_dev)


def build_topk_hypergraph_data(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                               k: int = 5, use_pooling: bool = True, device: Optional[torch.device] = None, *, ptr=None,
                               batch=None) -> dict:
    """build_topk_weighted_hypergraph packed as build_hypergraph_data_segmented packs its edges: x [N, D], edge_index [2, E]
    (global ids), edge_attr [E], pos [N, dp], batch [N] (segment id per row), ptr [S + 1], and pooled_feature [S, D] (the mean of
    every segment's rows) when use_pooling — all on `device` (None: the features' device)."""
    what = "build_topk_hypergraph_data"
    p = _inputs(features, positions, k, ptr, batch, what)
    if device is None:
        device = features.device
    features = features.to(device)
    positions = positions.to(device)
    edge_index, edge_weights, _ = build_topk_weighted_hypergraph(features, positions, lambda_h, lambda_g, k, device, ptr=p)
    result = {"x": features, "edge_index": edge_index, "edge_attr": edge_weights, "pos": positions,
              "batch": ragged.segment_ids(p).to(device), "ptr": p.to(device)}
    if use_pooling:
        result["pooled_feature"] = segment_mean_pool(features, p)
    return result
