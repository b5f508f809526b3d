"""The cross-segment top-k on the WIDE 16-bit scan (include/ext/mmf_hg_cross_segw.h): what
``cross_segments.simtopk_cross_segments`` answers — every row's k best columns among the rows of all OTHER segments — for feature
dims above 1024, where ``cross_segments16`` stops.  Candidates from the wide scan of the 16-bit matrix cores, exact re-rank: bit for
bit the exact entry's ids and values.

    simtopk_cross_segments_wide(X, Y, ptr=...)     the wide 16-bit call (f16 or bf16 operands), 1024 < d <= 4096 with k <= 20
    simtopk_cross_segments(X, Y, ptr=..., precision="auto")   the three-way router: narrow 16-bit, wide 16-bit, exact
    cross_segments_wide_table(ptr, d=..., k=...)   the host work table of the wide launch (no GPU)

    cross_segment_knn_edges(X, ptr=..., k=5, precision="auto")    ``cross_segments.cross_segment_knn_edges`` with a precision
    link_slides(out, k=5, precision="auto")        ``cohort.link_slides`` with a precision

``cross_segments16`` keeps its own two-way router (narrow 16-bit or exact); the one here adds the wide call, so "auto" and "fast"
reach d > 1024.  The result is the same bits on every route.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, cross_segments, cross_segments16, ops, wide_scan
from .cross_segments import checked_col_splits, checked_offsets
from .ops import _DT, _call, _feat, _hp, _metric, _need_gpu, _p

_FAST = ("fast", "fast_bf16")


def _operands(X, Y, what: str):
    X = _feat(X, f"{what} X")
    if Y is not None:
        Y = _feat(Y, f"{what} Y")
        if Y.device != X.device or Y.dtype != X.dtype or Y.shape[1] != X.shape[1]:
            raise ValueError(f"{what}: X and Y must share device, dtype and feature dim")
    return X, Y


def _edge_precision(precision, what: str) -> str:
    if precision not in ("exact", "auto"):
        raise ValueError(f"{what}: precision must be 'exact' or 'auto' (got {precision!r})")
    return precision

# What "auto" does where only the wide scan serves (d, k): it takes it.  Measured (DESIGN.md §4.26,
# profiles/cross_segments_wide_timing.txt; cosine, k = 5): the whole call is 4.06x / 4.08x / 4.98x faster than the exact call at
# d = 1536 (64 x 1024, 512 x 128, 250 ragged slides), 4.22x at d = 2560 (16 x 4096) and 2.38x at 8 x 1024 — 111, 45, 159, 264 and 28
# times the exact arm's spread, where the project's rule asks for more than three at every measured shape.
AUTO_TAKES_WIDE = True


def simtopk_cross_segments_wide(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                                metric="cosine", lam: float = 1.0, k: int = 5, precision: str = "fast", col_splits: int = 0,
                                return_stats: bool = False, profile: bool = False):
    """(idx int64 [n, k], val f32 [n, k][, stats]) of mmf_simtopk_cross_segments_wide: the contract of
    ``cross_segments.simtopk_cross_segments`` (ids are rows of all of Y, key descending then id ascending, no -1 / -inf fill), bit
    for bit its result, from the wide 16-bit scan: ``precision`` "fast" (f16 operands) or "fast_bf16".  Served where
    ``wide_scan.wide_scan_supported(d, k, False)`` holds — 1024 < d <= 4096 with k <= 20; elsewhere a ValueError (the router below
    takes the narrow 16-bit call or the exact one there).  ``col_splits``: 0 (automatic) or a power of two.  Every refusal is a
    ValueError raised on the host before any device work."""
    what = "simtopk_cross_segments_wide"
    if precision not in _FAST:
        raise ValueError(f"{what}: precision must be 'fast' or 'fast_bf16' (got {precision!r}); "
                         "cross_segments_wide.simtopk_cross_segments routes 'auto' and 'exact'")
    X, Y = _operands(X, Y, what)
    xp, yp = checked_offsets(X.shape[0], None if Y is None else Y.shape[0], ptr, batch, y_ptr, y_batch, k, what)
    col_splits = checked_col_splits(col_splits, what)
    mt = _metric(metric)
    n, d = X.shape
    k = int(k)
    if not wide_scan.wide_scan_supported(d, k, False):
        raise ValueError(f"{what}: the wide 16-bit scan does not serve d = {d}, k = {k} (1024 < d <= 4096 with k <= 20); "
                         "cross_segments_wide.simtopk_cross_segments routes the other shapes")
    _need_gpu(X, what)
    idx = torch.empty((n, k), dtype=torch.int64, device=X.device)
    val = torch.empty((n, k), dtype=torch.float32, device=X.device)
    opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], int(profile), col_splits, _lib.QUERY_ORDERS["off"], None)
    stats = _lib.SimtopkStats()
    _call("mmf_simtopk_cross_segments_wide", X.device, _p(X), n, _p(Y), n if Y is None else Y.shape[0], d, _DT[X.dtype], mt, float(lam), k,
          _hp(xp), _hp(yp), xp.numel() - 1, _p(idx), _p(val), ctypes.byref(opts), ctypes.byref(stats))
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def cross_segments_route(d: int, k: int, precision: str) -> str:
    """Where the router below sends (d, k, precision): "exact", "narrow" (``cross_segments16.simtopk_cross_segments_fast``) or
    "wide" (``simtopk_cross_segments_wide``).  "fast" / "fast_bf16" on a shape neither scan serves go to "narrow", whose
    ValueError names the shape."""
    if precision == "exact":
        return "exact"
    narrow = int(k) >= 1 and ops.fast_scan_supported(int(d), int(k), False)
    wide = int(k) >= 1 and not narrow and wide_scan.wide_scan_supported(int(d), int(k), False)
    if precision == "auto":
        return "narrow" if narrow else "wide" if wide and AUTO_TAKES_WIDE else "exact"
    return "wide" if wide else "narrow"


def simtopk_cross_segments(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                           metric="cosine", lam: float = 1.0, k: int = 5, precision: str = "auto", col_splits: int = 0,
                           return_stats: bool = False, profile: bool = False):
    """The three-way router.  ``precision`` "exact": ``cross_segments.simtopk_cross_segments``, unchanged.  "fast" / "fast_bf16":
    ``cross_segments16.simtopk_cross_segments_fast`` where ``ops.fast_scan_supported(d, k, False)`` holds, the wide call above where
    ``wide_scan.wide_scan_supported(d, k, False)`` holds, else the narrow call's ValueError.  "auto": the narrow call where it
    serves; where only the wide scan serves, what ``AUTO_TAKES_WIDE`` records of the measurement; the exact
    call elsewhere.  The result is the same bits on every route."""
    what = "simtopk_cross_segments"
    if precision not in ("auto", "exact") + _FAST:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    kw = dict(ptr=ptr, batch=batch, y_ptr=y_ptr, y_batch=y_batch, metric=metric, lam=lam, k=k, col_splits=col_splits,
              return_stats=return_stats, profile=profile)
    where = "exact" if precision == "exact" else cross_segments_route(_feat(X, f"{what} X").shape[1], int(k), precision)
    if where == "exact":
        return cross_segments.simtopk_cross_segments(X, Y, **kw)
    if precision == "auto":
        precision = "fast"
    if where == "wide":
        return simtopk_cross_segments_wide(X, Y, precision=precision, **kw)
    return cross_segments16.simtopk_cross_segments_fast(X, Y, precision=precision, **kw)


def cross_segments_wide_table(ptr, y_ptr=None, *, d: int, k: int = 5, col_splits: int = 0):
    """(table [entries, 8] int32, lists): the work table mmf_simtopk_cross_segments_wide launches for host offsets ``ptr``
    (``y_ptr``: the other side of a two-sided call), feature dim ``d`` and ``k``, and the list slots per row (2 x the largest entry
    count of a row block).  Columns: first row of the 128-row block (twice: operand position and list row), real queries, first /
    end tile (of 128 rows of the plain image of Y), first tile of the entry's mask window, first list slot (2 x the entry's number
    in its block), end tile of the mask window.  Host only: no GPU is touched."""
    L = _lib.lib()
    xp = torch.as_tensor(ptr, dtype=torch.int64).contiguous()
    yp = None if y_ptr is None else torch.as_tensor(y_ptr, dtype=torch.int64).contiguous()
    if xp.dim() != 1 or xp.numel() < 1 or (yp is not None and yp.shape != xp.shape):
        raise ValueError("cross_segments_wide_table: offsets [S + 1] (the same S on both sides)")
    lists = ctypes.c_int(0)
    args = (_hp(xp), _hp(yp), xp.numel() - 1, int(d), int(k), int(col_splits))
    grid = L.mmf_cross_segments_wide_table(*args, None, 0, ctypes.byref(lists))
    if grid < 0:
        _lib.check(int(grid), "mmf_cross_segments_wide_table")
    table = torch.empty((int(grid), 8), dtype=torch.int32)
    grid = L.mmf_cross_segments_wide_table(*args, _hp(table), int(grid), ctypes.byref(lists))
    if grid < 0:
        _lib.check(int(grid), "mmf_cross_segments_wide_table")
    return table, int(lists.value)


def cross_segment_knn_edges(X: torch.Tensor, *, ptr=None, batch=None, k: int = 5, precision: str = "exact"):
    """``cross_segments.cross_segment_knn_edges`` with a keyword-only ``precision``: "exact" (the default) is that function, "auto"
    takes every row's neighbours from the three-way router above.  The neighbours are the same bits, so the edges and weights are
    equal."""
    precision = _edge_precision(precision, "cross_segment_knn_edges")
    if precision == "exact":
        return cross_segments.cross_segment_knn_edges(X, ptr=ptr, batch=batch, k=k)
    return cross_segments.knn_edges_over(X, ptr, batch, k, lambda X_, **kw: simtopk_cross_segments(X_, precision="auto", **kw))


def link_slides(out: dict, k: int = 5, *, precision: str = "exact"):
    """``cohort.link_slides`` with a keyword-only ``precision``, as ``cross_segment_knn_edges`` above takes it."""
    precision = _edge_precision(precision, "link_slides")
    return cross_segments.link_slides_over(out, k, lambda X_, **kw: cross_segment_knn_edges(X_, precision=precision, **kw))
