"""The cross-segment top-k (include/ext/mmf_hg_cross_seg.h): for every row of a ragged batch, the k best columns
among the rows of all OTHER segments — the complement of every block-diagonal cohort entry.  Leave-one-slide-out nearest
neighbours, the inter-slide edges of a cohort hypergraph, a bank that already holds sections of the same patients.

    simtopk_cross_segments(X, Y, ptr=...)          the exact k-NN of every row outside its own segment, any k
    cross_segments_table(ptr, ...)                 the host work table of the launch (no GPU)
    cross_segment_knn_edges(X, ptr=..., k=5)       the inter-slide counterpart of the reference's k-NN edges (rows a8 / a9)
    cohort.link_slides(out, k=5)                   those edges among the super patches of build_cohort_hypergraphs' result

The bits are those of one exact ``ops.simtopk`` per segment against the rest of Y, ids mapped back.  One scan launch and one re-rank
per pass of 44 entries; the 16-bit scan of the same answer, and the router between the two, are cross_segments16.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, ops, ragged
from .build_hypergraph._common import compute_device
from .ops import _DT, _call, _feat, _hp, _metric, _need_gpu, _p


def checked_col_splits(col_splits, what: str) -> int:
    col_splits = int(col_splits)
    if col_splits < 0 or col_splits & (col_splits - 1):
        raise ValueError(f"{what}: col_splits must be 0 or a power of two (got {col_splits})")
    return col_splits


def checked_offsets(n: int, m: Optional[int], ptr, batch, y_ptr, y_batch, k: int, what: str):
    """Host offsets (x side, y side; the same tensor for a self call, m None) of n rows of X and m of Y, every segment with rows
    checked for k admissible columns: the ValueErrors of this module's calls, raised before any device work."""
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if m is None:
        if y_ptr is not None or y_batch is not None:
            raise ValueError(f"{what}: y_ptr / y_batch need Y")
        xp = yp = ragged.offsets(ptr, batch, n, what=what, allow_no_segments=True)
        m = n
    else:
        xp, yp = ragged.two_sided(n, m, ptr, batch, y_ptr, y_batch, xs="", ys="y_", what=what, allow_no_segments=True)
    nx, own = xp[1:] - xp[:-1], yp[1:] - yp[:-1]
    short = torch.nonzero((nx > 0) & (m - own < int(k))).reshape(-1)
    if short.numel():
        s = int(short[0])
        raise ValueError(f"{what}: segment {s} has {m - int(own[s])} admissible columns (m = {m} minus its own {int(own[s])} rows of Y), "
                         f"k = {int(k)} needs at least {int(k)}")
    return xp, yp


def simtopk_cross_segments(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                           metric="cosine", lam: float = 1.0, k: int = 5, col_splits: int = 0, return_stats: bool = False,
                           profile: bool = False):
    """(idx int64 [n, k], val f32 [n, k][, stats]) of mmf_simtopk_cross_segments: row i of segment s ranked against every row of
    Y (Y None: of X, with y_ptr = ptr) OUTSIDE rows y_ptr[s]:y_ptr[s + 1]; ids are rows of all of Y, order is key descending then
    id ascending, bits are the exact ``ops.simtopk``'s.  Segments per side as ``ops.simtopk_segmented`` takes them (ptr / batch,
    y_ptr / y_batch).  There is no exclude_self (a row's self lies inside its segment) and no -1 / -inf fill: a segment with rows
    and fewer than k admissible columns is a ValueError.  ``col_splits``: 0 (automatic) or a power of two.  Every refusal is raised
    on the host before any device work."""
    what = "simtopk_cross_segments"
    X = _feat(X, f"{what} X")
    if Y is not None:
        Y = _feat(Y, f"{what} Y")
        if Y.device != X.device or Y.dtype != X.dtype or Y.shape[1] != X.shape[1]:
            raise ValueError(f"{what}: X and Y must share device, dtype and feature dim")
    xp, yp = checked_offsets(X.shape[0], None if Y is None else Y.shape[0], ptr, batch, y_ptr, y_batch, k, what)
    col_splits = checked_col_splits(col_splits, what)
    mt = _metric(metric)
    _need_gpu(X, what)
    n, d = X.shape
    k = int(k)
    idx = torch.empty((n, k), dtype=torch.int64, device=X.device)
    val = torch.empty((n, k), dtype=torch.float32, device=X.device)
    opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], int(profile), col_splits, _lib.QUERY_ORDERS["off"], None)
    stats = _lib.SimtopkStats()
    _call("mmf_simtopk_cross_segments", X.device, _p(X), n, _p(Y), n if Y is None else Y.shape[0], d, _DT[X.dtype], mt, float(lam), k,
          _hp(xp), _hp(yp), xp.numel() - 1, _p(idx), _p(val), ctypes.byref(opts), ctypes.byref(stats))
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def cross_segments_table(ptr, y_ptr=None, *, k: int = 5, col_splits: int = 0):
    """(table [entries, 8] int64, lists): the work table of mmf_simtopk_cross_segments for host offsets ``ptr`` (``y_ptr``: the other
    side of a two-sided call) and the list slots per row, 2 x the largest range count of a row block.  Columns: segment, first row of
    X, real queries, first excluded row of Y, first / end tile (of 128 rows of all of Y), number of the column range, end of the
    excluded rows.  Host only: no GPU is touched."""
    L = _lib.lib()
    xp = torch.as_tensor(ptr, dtype=torch.int64).contiguous()
    yp = None if y_ptr is None else torch.as_tensor(y_ptr, dtype=torch.int64).contiguous()
    if xp.dim() != 1 or xp.numel() < 1 or (yp is not None and yp.shape != xp.shape):
        raise ValueError("cross_segments_table: offsets [S + 1] (the same S on both sides)")
    lists = ctypes.c_int(0)
    args = (_hp(xp), _hp(yp), xp.numel() - 1, int(k), int(col_splits))
    grid = L.mmf_cross_segments_table(*args, None, 0, ctypes.byref(lists))
    if grid < 0:
        _lib.check(int(grid), "mmf_cross_segments_table")
    table = torch.empty((int(grid), 8), dtype=torch.int64)
    grid = L.mmf_cross_segments_table(*args, _hp(table), int(grid), ctypes.byref(lists))
    if grid < 0:
        _lib.check(int(grid), "mmf_cross_segments_table")
    return table, int(lists.value)


def cross_segment_knn_edges(X: torch.Tensor, *, ptr=None, batch=None, k: int = 5):
    """(edge_index int64 [2, E], edge_weights f32 [E]): the inter-slide counterpart of the reference's k-NN edges
    (build_hypergraph_knn_kmeans, rows a8 / a9).  Every row's k Euclidean nearest rows OUTSIDE its own segment (``neg_sq_l2``
    through ``simtopk_cross_segments``), the undirected dedup of ``ops.knn_pairs`` (a pair both rows emit appears once, lower id
    first), sorted by (lower, higher) id, and the max(0, cosine) weights of ``ops.edge_cosine``.  Every edge joins two segments."""
    return knn_edges_over(X, ptr, batch, k, simtopk_cross_segments)


def knn_edges_over(X, ptr, batch, k, topk):
    """cross_segment_knn_edges over the neighbours of ``topk`` (this module's exact call, or cross_segments16's router)."""
    what = "cross_segment_knn_edges"
    if ptr is None and batch is None:
        raise ValueError(f"{what}: needs ptr or batch (without segments every row is admissible: ops.simtopk)")
    X = _feat(X, f"{what} X")
    checked_offsets(X.shape[0], None, ptr, batch, None, None, k, what)
    _need_gpu(X, what)
    n = X.shape[0]
    if n == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=X.device), torch.empty((0,), dtype=torch.float32, device=X.device)
    nbr, _ = topk(X, ptr=ptr, batch=batch, metric="neg_sq_l2", k=k)
    lo, hi = ops.knn_pairs(nbr)
    code = torch.sort(lo * n + hi).values
    edge_index = torch.stack([code // n, code % n], dim=0).contiguous()
    return edge_index, ops.edge_cosine(X, edge_index)


def link_slides(out: dict, k: int = 5):
    """``cohort.link_slides`` (defined here, beside the call it is made of; the cohort module exports it).  (edge_index int64
    [2, E], edge_weights f32 [E]): the inter-slide edges of a cohort.  ``out`` is the dict of
    build_cohort_hypergraphs; its super_features rows, cut per slide by group_ptr, are linked by
    cross_segment_knn_edges (every super patch's k Euclidean nearest super patches of OTHER slides, undirected dedup,
    max(0, cosine) weights) and the edges are returned in the cohort's node numbering: super patch c of slide s is node
    node_ptr[s] + c, so they can be concatenated with out["edge_index"].  The result lives where out["super_features"] does; the
    arithmetic runs on the GPU."""
    return link_slides_over(out, k, cross_segment_knn_edges)


def link_slides_over(out, k, knn_edges):
    """link_slides over the edges of ``knn_edges`` (cross_segment_knn_edges of this module or of cross_segments16)."""
    what = "link_slides"
    if not isinstance(out, dict) or any(key not in out for key in ("super_features", "group_ptr", "node_ptr")):
        raise ValueError(f"{what}: needs the dict of build_cohort_hypergraphs (super_features, group_ptr, node_ptr)")
    sf = out["super_features"]
    gp = torch.as_tensor(out["group_ptr"], dtype=torch.int64).cpu()
    node_ptr = torch.as_tensor(out["node_ptr"], dtype=torch.int64).cpu()
    if sf.dim() != 2 or gp.dim() != 1 or gp.shape != node_ptr.shape:
        raise ValueError(f"{what}: super_features [S * C, D] with group_ptr and node_ptr [S + 1]")
    if gp.numel() < 3:
        raise ValueError(f"{what}: a cohort of {gp.numel() - 1} slide(s) has no other slide to link to")
    gp = ragged.offsets(gp, None, sf.shape[0], what=what, unit="slide")
    if bool(((node_ptr[1:] - node_ptr[:-1]) < (gp[1:] - gp[:-1])).any()):
        raise ValueError(f"{what}: node_ptr leaves a slide fewer nodes than it has super patches")
    checked_offsets(sf.shape[0], None, gp, None, None, None, k, what)      # k >= 1 and k admissible super patches for every slide
    home = sf.device
    dev = compute_device(sf)
    ei, ew = knn_edges(sf.detach().to(dev), ptr=gp, k=k)
    shift = (node_ptr[:-1] - gp[:-1]).to(dev)                       # row -> node: slide s's rows move by node_ptr[s] - group_ptr[s]
    seg = ragged.segment_ids(gp).to(dev)
    ei = ei + shift[seg][ei]
    return ei.to(home), ew.to(home)
