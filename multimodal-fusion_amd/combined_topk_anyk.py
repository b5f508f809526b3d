"""The top-k of the combined similarity K = K_h * K_g for ANY k (mmf_simtopk_combined_anyk / mmf_simtopk_combined_xy_anyk,
include/ext/mmf_hg_topk_anyk.h).  ``combined_topk``, ``segmented_exact`` and ``combined_topk_xy`` stop at
k + self = 44, what one pass of the exact scan's lists holds; the functions here take any k: up to 44 they call what serves the
shape today (so those bits), above it the entries that run the exact scan in passes of at most 44 - self entries, each behind the
per-row floor where the previous one ended.  64 or 128 combined-similarity neighbours per patch are a sparser stand-in for the
reference's median-threshold graph, which keeps half of all pairs.

Contract of every function: per row the first k entries of the total order (key = eh + eg descending, id ascending) over the
admissible columns, values bitwise ``ops.sim_dense_combined``'s entries, -1 / -inf behind a row's last real entry; for k' >= k the
first k columns of the k' result are the k result.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib, combined_topk, combined_topk_xy, ops, ragged, segmented_exact
from .build_hypergraph._common import compute_device, result_device_like_kernel, to_gpu
from .weighted_hypergraph import segment_mean_pool

ONE_PASS_MAX = 44   # k + self one pass of the exact lists holds (scan_f32_cap, csrc/mmf_scan_f32.hip)


def anyk_route(k: int, exclude_self: bool, segmented: bool) -> str:
    """What serves (k, exclude_self) for one graph (``segmented=False``) or a batch: up to k + self = 44 the existing function
    ("combined_topk.simtopk_combined" / "segmented_exact.simtopk_combined_exact"), above it "mmf_simtopk_combined_anyk"."""
    if int(k) < 1:
        raise ValueError(f"anyk_route: k must be >= 1 (got {k})")
    if int(k) + (1 if exclude_self else 0) <= ONE_PASS_MAX:
        return "segmented_exact.simtopk_combined_exact" if segmented else "combined_topk.simtopk_combined"
    return "mmf_simtopk_combined_anyk"


def simtopk_combined_any_k(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *,
                           ptr=None, batch=None, exclude_self: bool = True, col_splits: int = 0, return_stats: bool = False,
                           profile: bool = False):
    """``combined_topk.simtopk_combined`` (one graph) / ``segmented_exact.simtopk_combined_exact`` (``ptr`` or ``batch``) without
    their limit on k: (idx [N, k] int64 global row ids, val [N, k] f32[, stats dict]).  With a batch ``col_splits`` is 0 or a
    power of two.  CPU tensors are computed on the current GPU and the result moved back."""
    what = "simtopk_combined_any_k"
    p = combined_topk._inputs(features, positions, k, ptr, batch, what)
    segmented = ptr is not None or batch is not None
    if int(col_splits) < 0:
        raise ValueError(f"{what}: col_splits must be >= 0 (got {col_splits})")
    if segmented:
        col_splits = segmented_exact._col_splits(col_splits, what)
    route = anyk_route(k, exclude_self, segmented)
    kw = dict(exclude_self=exclude_self, col_splits=col_splits, return_stats=return_stats, profile=profile)
    if route == "combined_topk.simtopk_combined":
        return combined_topk.simtopk_combined(features, positions, lambda_h, lambda_g, k, **kw)
    if route == "segmented_exact.simtopk_combined_exact":
        return segmented_exact.simtopk_combined_exact(features, positions, lambda_h, lambda_g, k, ptr=p, **kw)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    n, d = F.shape
    idx = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    if n > 0:
        opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        ops._call(route, dev, ops._p(F), ops._p(P), n, d, P.shape[1], float(lambda_h), float(lambda_g), int(k),
                  int(bool(exclude_self)), ops._hp(p if segmented else None), p.numel() - 1 if segmented else 0, ops._p(idx), ops._p(val),
                  ctypes.byref(opts), ctypes.byref(stats), what=what)
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def _run_xy(what, Fq, Pq, Fc, Pc, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, col_splits, profile):
    """mmf_simtopk_combined_xy_anyk on device tensors (f32, contiguous rows): (idx, val, stats)."""
    dev = Fq.device
    nq, d = Fq.shape
    idx = torch.empty((nq, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((nq, int(k)), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    if nq > 0:
        opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        ops._call("mmf_simtopk_combined_xy_anyk", dev, ops._p(Fq), ops._p(Pq), nq, ops._p(Fc), ops._p(Pc), Fc.shape[0], d, Pq.shape[1],
                  float(lambda_h), float(lambda_g), int(k), int(bool(exclude_self)), int(row_offset), int(col_offset), ops._p(idx), ops._p(val),
                  ctypes.byref(opts), ctypes.byref(stats), what=what)
    return idx, val, stats


def simtopk_combined_xy_any_k(q_features: torch.Tensor, q_positions: torch.Tensor, c_features: torch.Tensor, c_positions: torch.Tensor,
                              lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *, exclude_self: bool = False, row_offset: int = 0,
                              col_offset: int = 0, col_splits: int = 0, return_stats: bool = False, profile: bool = False):
    """``combined_topk_xy.simtopk_combined_xy(precision="exact")`` for any k: per query the k best candidates, reported as
    ``col_offset + candidate row``; ``exclude_self`` drops the pair whose ids agree; a query with fewer than k admissible
    candidates gets them first, then -1 / -inf.  Queries that are a row view of the candidates are recognised as a row slice."""
    what = "simtopk_combined_xy_any_k"
    combined_topk_xy._inputs(q_features, q_positions, c_features, c_positions, k, "exact", col_splits, row_offset, col_offset, what)
    home = q_features.device
    dev = compute_device(q_features, q_positions, c_features, c_positions)
    Fq, Pq, Fc, Pc = (to_gpu(t, dev) for t in (q_features, q_positions, c_features, c_positions))
    idx, val, stats = _run_xy(what, Fq, Pq, Fc, Pc, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, col_splits, profile)
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def simtopk_combined_rows_any_k(features: torch.Tensor, positions: torch.Tensor, lo: int, hi: int, lambda_h: float = 1.0,
                                lambda_g: float = 1.0, k: int = 5, *, exclude_self: bool = True, col_offset: int = 0, col_splits: int = 0,
                                return_stats: bool = False, profile: bool = False):
    """Rows [lo, hi) of ``simtopk_combined_any_k(features, positions, ...)`` (one graph), bit for bit, without computing the other
    rows: (idx [hi - lo, k], val [hi - lo, k][, stats dict]), ids shifted by ``col_offset``.  The library is handed views of the
    two arrays, so it sees a row slice."""
    what = "simtopk_combined_rows_any_k"
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= features.shape[0]:
        raise ValueError(f"{what}: rows [{lo}, {hi}) are no range of the {features.shape[0]} rows")
    combined_topk_xy._inputs(features[lo:hi], positions[lo:hi], features, positions, k, "exact", col_splits, 0, col_offset, what)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    idx, val, stats = _run_xy(what, F[lo:hi], P[lo:hi], F, P, lambda_h, lambda_g, k, exclude_self, int(col_offset) + lo, col_offset,
                              col_splits, profile)
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def build_topk_weighted_hypergraph_any_k(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                         k: int = 5, device: Optional[torch.device] = None, *, ptr=None,
                                         batch=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``combined_topk.build_topk_weighted_hypergraph`` for any k, in its layout: (edge_index [2, E] int64 global row ids,
    edge_weights [E] f32, edge_ptr [S + 1] int64) on `device` (None: the features' device).  Edge (i, idx[i, r]) with weight
    val[i, r]; rows ascend and r ascends within a row; a segment of n_s rows gives n_s * min(k, n_s - 1) edges."""
    what = "build_topk_weighted_hypergraph_any_k"
    p = combined_topk._inputs(features, positions, k, ptr, batch, what)
    out_dev = result_device_like_kernel(features, device)
    dev = compute_device(features, positions) if out_dev.type != "cuda" else out_dev
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    one = ptr is None and batch is None
    idx, val = simtopk_combined_any_k(F, P, lambda_h, lambda_g, k, ptr=None if one else p)
    keep = idx >= 0
    rows = torch.arange(idx.shape[0], dtype=torch.int64, device=dev).unsqueeze(1).expand_as(idx)
    edge_index = torch.stack([rows[keep], idx[keep]])
    sizes = p[1:] - p[:-1]
    edge_ptr = torch.zeros(p.numel(), dtype=torch.int64)
    edge_ptr[1:] = torch.cumsum(sizes * torch.clamp(sizes - 1, min=0, max=int(k)), 0)
    return edge_index.to(out_dev).contiguous(), val[keep].to(out_dev), edge_ptr.to(out_dev)


def build_topk_hypergraph_data_any_k(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                     k: int = 5, use_pooling: bool = True, device: Optional[torch.device] = None, *, ptr=None,
                                     batch=None) -> dict:
    """``combined_topk.build_topk_hypergraph_data`` for any k: x, edge_index (global ids), edge_attr, pos, batch, ptr and (with
    use_pooling) pooled_feature, all on `device` (None: the features' device)."""
    what = "build_topk_hypergraph_data_any_k"
    p = combined_topk._inputs(features, positions, k, ptr, batch, what)
    if device is None:
        device = features.device
    features = features.to(device)
    positions = positions.to(device)
    one = ptr is None and batch is None
    edge_index, edge_weights, _ = build_topk_weighted_hypergraph_any_k(features, positions, lambda_h, lambda_g, k, device,
                                                                       ptr=None if one else p)
    result = {"x": features, "edge_index": edge_index, "edge_attr": edge_weights, "pos": positions,
              "batch": ragged.segment_ids(p).to(device), "ptr": p.to(device)}
    if use_pooling:
        result["pooled_feature"] = segment_mean_pool(features, p)
    return result
