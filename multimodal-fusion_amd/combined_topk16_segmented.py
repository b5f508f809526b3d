"""The k best columns per row of the combined similarity K = K_h * K_g of EVERY graph of a ragged batch from one launch of the
16-bit scan (mmf_simtopk_combined_fast_segmented, include/ext/mmf_hg_topk16_seg.h): the result of
``combined_topk.simtopk_combined(ptr=...)``, bit for bit, from an f16 / bf16 candidate scan of the combined key over one padded
operand image, an exact re-rank, and the exact scan for the segments with fewer than k admissible columns and for the rows the
16-bit scan could not certify.  k + self <= 20, feature dim <= 4096, position dim <= 8, f32 inputs.  Segments are given by exactly
one of ``ptr`` ([S + 1] offsets) / ``batch`` ([N] sorted segment id per row, PyG's convention).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib, ops, ragged
from .build_hypergraph._common import compute_device, result_device_like_kernel, to_gpu
from .weighted_hypergraph import segment_mean_pool


def _inputs(features: torch.Tensor, positions: torch.Tensor, k: int, ptr, batch, precision: str, col_splits: int, what: str) -> torch.Tensor:
    """Host offsets, checked before any device work or library call: shapes, k, the precision's name, col_splits, ptr / batch.
    The entry refuses what it does not support (k + self > 20, D > 4096, dp > 8) with its own words."""
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    cs = int(col_splits)
    if cs < 0 or (cs & (cs - 1)) != 0:
        raise ValueError(f"{what}: col_splits must be 0 or a power of two (got {col_splits})")
    return ragged.offsets(ptr, batch, features.shape[0], what=what, allow_no_segments=True)


def simtopk_combined_fast_segmented(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                    k: int = 5, *, ptr=None, batch=None, exclude_self: bool = True, precision: str = "auto",
                                    col_splits: int = 0, return_stats: bool = False, profile: bool = False):
    """(idx [N, k] int64, val [N, k] f32[, stats dict]): ``combined_topk.simtopk_combined(ptr=...)``'s result, the same bits — per
    row the k best columns of its own segment as global row ids; a row whose segment has fewer than k admissible columns gets them
    first, then -1 / -inf.  ``precision``: "fast" scans f16 images of the features, "fast_bf16" bf16 images, "exact" runs the
    exact f32 pass, "auto" takes the f16 scan in the measured range (512 <= D <= 1536, k + self <= 11) and the
    exact pass elsewhere; stats["precision_used"] says which ran and stats["fallback_rows"] how many rows of scanned segments went
    to the exact pass.  ``col_splits``: 0 (automatic: two ranges for a batch of fewer than 256 row blocks, else one) or a power of
    two, the column ranges every segment is cut into at most (and at most one per 128-column tile of the segment).  CPU tensors
    are computed on the current GPU and the result moved back."""
    what = "simtopk_combined_fast_segmented"
    p = _inputs(features, positions, k, ptr, batch, precision, col_splits, what)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    n, d = F.shape
    idx = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    if n > 0:
        opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        ops._call("mmf_simtopk_combined_fast_segmented", dev, ops._p(F), ops._p(P), n, d, P.shape[1], float(lambda_h), float(lambda_g),
                  int(k), int(bool(exclude_self)), ops._hp(p), p.numel() - 1, ops._p(idx), ops._p(val), ctypes.byref(opts),
                  ctypes.byref(stats))
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def build_topk_weighted_hypergraph_fast_segmented(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0,
                                                  lambda_g: float = 1.0, k: int = 5, device: Optional[torch.device] = None, *, ptr=None,
                                                  batch=None, precision: str = "auto") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The directed top-k edges of every segment in ``combined_topk.build_topk_weighted_hypergraph``'s layout: (edge_index [2, E]
    int64 with global row ids, edge_weights [E] f32, edge_ptr [S + 1] int64) on `device` (None: the features' device).  Edge
    (i, idx[i, r]) with weight val[i, r]; rows ascend and r ascends within a row; a segment of n_s rows gives
    n_s * min(k, n_s - 1) edges."""
    what = "build_topk_weighted_hypergraph_fast_segmented"
    p = _inputs(features, positions, k, ptr, batch, precision, 0, what)
    out_dev = result_device_like_kernel(features, device)
    dev = compute_device(features, positions) if out_dev.type != "cuda" else out_dev
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    idx, val = simtopk_combined_fast_segmented(F, P, lambda_h, lambda_g, k, ptr=p, precision=precision)
    keep = idx >= 0
    rows = torch.arange(idx.shape[0], dtype=torch.int64, device=dev).unsqueeze(1).expand_as(idx)
    edge_index = torch.stack([rows[keep], idx[keep]])
    sizes = p[1:] - p[:-1]
    edge_ptr = torch.zeros(p.numel(), dtype=torch.int64)
    edge_ptr[1:] = torch.cumsum(sizes * torch.clamp(sizes - 1, min=0, max=int(k)), 0)
    return edge_index.to(out_dev).contiguous(), val[keep].to(out_dev), edge_ptr.to(out_dev)


def build_topk_hypergraph_data_fast(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                    k: int = 5, use_pooling: bool = True, device: Optional[torch.device] = None, *, ptr=None,
                                    batch=None, precision: str = "auto") -> dict:
    """build_topk_weighted_hypergraph_fast_segmented packed as ``combined_topk.build_topk_hypergraph_data`` packs its edges: x
    [N, D], edge_index [2, E] (global ids), edge_attr [E], pos [N, dp], batch [N] (segment id per row), ptr [S + 1], and
    pooled_feature [S, D] (the mean of every segment's rows) when use_pooling — all on `device` (None: the features' device)."""
    what = "build_topk_hypergraph_data_fast"
    p = _inputs(features, positions, k, ptr, batch, precision, 0, what)
    if device is None:
        device = features.device
    features = features.to(device)
    positions = positions.to(device)
    edge_index, edge_weights, _ = build_topk_weighted_hypergraph_fast_segmented(features, positions, lambda_h, lambda_g, k, device, ptr=p,
                                                                                precision=precision)
    result = {"x": features, "edge_index": edge_index, "edge_attr": edge_weights, "pos": positions,
              "batch": ragged.segment_ids(p).to(device), "ptr": p.to(device)}
    if use_pooling:
        result["pooled_feature"] = segment_mean_pool(features, p)
    return result
