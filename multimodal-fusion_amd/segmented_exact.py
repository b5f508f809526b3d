"""The exact f32 top-k of every segment of a ragged batch from ONE table-driven launch of the exact scan
(include/ext/mmf_hg_seg_exact.h): what a cohort gets where no 16-bit scan applies — ``precision="exact"``,
k + self > 20 above d = 512, d > 4096, k + self > 44 — without the launch loop of ``ops.simtopk_segmented``.

    simtopk_segmented_exact(X, Y, ptr=...)         the exact k-NN of every segment, any k
    simtopk_combined_exact(F, P, ..., ptr=...)     the exact top-k of K_h * K_g of every graph of a batch
    simtopk_segmented(..., precision="auto")       the router: a 16-bit scan where one applies, the exact entry elsewhere
    segmented_exact_table(ptr, ...)                the host work table of the launch (no GPU)

The bits are those of one ``ops.simtopk(precision="exact")`` (``combined_topk.simtopk_combined``) per segment.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, ops, ragged, wide_scan
from .build_hypergraph._common import compute_device, to_gpu
from .ops import _feat, _hp, _need_gpu, _simtopk_entry


def _col_splits(col_splits, what: str) -> int:
    col_splits = int(col_splits)
    if col_splits < 0 or col_splits & (col_splits - 1):
        raise ValueError(f"{what}: col_splits must be 0 or a power of two (got {col_splits})")
    return col_splits


def _sides(X, Y, ptr, batch, y_ptr, y_batch, k, what: str):
    """X, Y as the entries take them and the host offsets of both sides, checked before any device work."""
    X = _feat(X, f"{what} X")
    if Y is not None:
        Y = _feat(Y, f"{what} Y")
        if Y.device != X.device or Y.dtype != X.dtype or Y.shape[1] != X.shape[1]:
            raise ValueError(f"{what}: X and Y must share device, dtype and feature dim")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if Y is None:
        if y_ptr is not None or y_batch is not None:
            raise ValueError(f"{what}: y_ptr / y_batch need Y")
        xp = yp = ragged.offsets(ptr, batch, X.shape[0], what=what, allow_no_segments=True)
    else:
        xp, yp = ragged.two_sided(X.shape[0], Y.shape[0], ptr, batch, y_ptr, y_batch, xs="", ys="y_", what=what, allow_no_segments=True)
    return X, Y, xp, yp


def simtopk_segmented_exact(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                            metric="cosine", lam: float = 1.0, k: int = 5, exclude_self: Optional[bool] = None,
                            col_splits: int = 0, return_stats: bool = False, profile: bool = False):
    """``ops.simtopk_segmented(..., precision="exact")`` from one scan launch and one re-rank (mmf_simtopk_segmented_exact): the
    same arguments, the same (idx, val[, stats]) and the same bits — those of one exact ``ops.simtopk`` per segment.  Any k:
    k + self > 44, which ``ops.simtopk_segmented`` refuses, runs passes of at most 44 entries.  ``col_splits``: 0 (automatic: a few
    large segments are split until the call makes about 1024 workgroups) or a power of two, the column ranges every segment is
    scanned in (at most one per 128 columns)."""
    what = "simtopk_segmented_exact"
    X, Y, xp, yp = _sides(X, Y, ptr, batch, y_ptr, y_batch, k, what)
    col_splits = _col_splits(col_splits, what)
    if exclude_self is None:
        exclude_self = Y is None
    _need_gpu(X, what)
    opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], int(profile), col_splits, _lib.QUERY_ORDERS["off"], None)
    return _simtopk_entry("mmf_simtopk_segmented_exact", X, Y, metric, lam, int(k), exclude_self, (_hp(xp), _hp(yp), xp.numel() - 1),
                          opts, return_stats)


def simtopk_combined_exact(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *,
                           ptr=None, batch=None, exclude_self: bool = True, col_splits: int = 0, return_stats: bool = False,
                           profile: bool = False):
    """``combined_topk.simtopk_combined`` of a batch (``ptr`` or ``batch`` required) from one scan launch and one re-rank
    (mmf_simtopk_combined_segmented_exact): the same (idx, val[, stats]), bit for bit; k + self <= 44."""
    what = "simtopk_combined_exact"
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if ptr is None and batch is None:
        raise ValueError(f"{what}: needs ptr or batch (one graph is combined_topk.simtopk_combined's)")
    col_splits = _col_splits(col_splits, what)
    p = ragged.offsets(ptr, batch, features.shape[0], what=what, allow_no_segments=True)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    n, d = F.shape
    idx = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    if n > 0:
        opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], int(profile), col_splits, _lib.QUERY_ORDERS["off"], None)
        ops._call("mmf_simtopk_combined_segmented_exact", dev, ops._p(F), ops._p(P), n, d, P.shape[1], float(lambda_h), float(lambda_g),
                  int(k), int(bool(exclude_self)), _hp(p), p.numel() - 1, ops._p(idx), ops._p(val), ctypes.byref(opts),
                  ctypes.byref(stats))
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def simtopk_segmented(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                      metric="cosine", lam: float = 1.0, k: int = 5, exclude_self: Optional[bool] = None,
                      precision: str = "auto", col_splits: int = 0, return_stats: bool = False, profile: bool = False):
    """The router: ``wide_scan.simtopk_segmented`` wherever a 16-bit scan applies (``ops.fast_scan_supported`` or
    ``wide_scan.wide_scan_supported``) and ``precision`` is not ``"exact"``, ``simtopk_segmented_exact`` elsewhere.  Same
    arguments, same (idx, val[, stats]), same bits either way."""
    what = "segmented_exact.simtopk_segmented"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    if X.dim() != 2:
        raise ValueError(f"{what} X: expected a 2-D [N, D] tensor, got shape {tuple(X.shape)}")
    self_ex = (Y is None) if exclude_self is None else bool(exclude_self)
    d = int(X.shape[1])
    if precision != "exact" and int(k) >= 1 and (ops.fast_scan_supported(d, int(k), self_ex) or wide_scan.wide_scan_supported(d, int(k), self_ex)):
        return wide_scan.simtopk_segmented(X, Y, ptr=ptr, batch=batch, y_ptr=y_ptr, y_batch=y_batch, metric=metric, lam=lam, k=k,
                                           exclude_self=exclude_self, precision=precision, col_splits=col_splits,
                                           return_stats=return_stats, profile=profile)
    if precision not in ("auto", "exact"):
        raise ValueError(f"{what}: precision {precision!r} needs a 16-bit scan, and none serves d = {d}, k = {k}")
    return simtopk_segmented_exact(X, Y, ptr=ptr, batch=batch, y_ptr=y_ptr, y_batch=y_batch, metric=metric, lam=lam, k=k,
                                   exclude_self=exclude_self, col_splits=col_splits, return_stats=return_stats, profile=profile)


def segmented_exact_table(ptr, y_ptr=None, *, k: int = 5, exclude_self: bool = True, col_splits: int = 0):
    """(table [entries, 8] int64, lists): the work table of the two entries for host offsets ``ptr`` (``y_ptr``: the other side of
    a cross call) and the list slots per row, 2 x the largest range count.  Columns: segment, first row of X, real queries, first
    row of the segment in Y, first / end tile, number of the column range, columns of the segment.  Host only: no GPU is touched."""
    L = _lib.lib()
    xp = torch.as_tensor(ptr, dtype=torch.int64).contiguous()
    yp = None if y_ptr is None else torch.as_tensor(y_ptr, dtype=torch.int64).contiguous()
    if xp.dim() != 1 or xp.numel() < 1 or (yp is not None and yp.shape != xp.shape):
        raise ValueError("segmented_exact_table: offsets [S + 1] (the same S on both sides)")
    lists = ctypes.c_int(0)
    args = (_hp(xp), _hp(yp), xp.numel() - 1, int(k), int(bool(exclude_self)), int(col_splits))
    grid = L.mmf_segmented_exact_table(*args, None, 0, ctypes.byref(lists))
    if grid < 0:
        _lib.check(int(grid), "mmf_segmented_exact_table")
    table = torch.empty((int(grid), 8), dtype=torch.int64)
    grid = L.mmf_segmented_exact_table(*args, _hp(table), int(grid), ctypes.byref(lists))
    if grid < 0:
        _lib.check(int(grid), "mmf_segmented_exact_table")
    return table, int(lists.value)
