"""The wide 16-bit top-k for any k (include/ext/mmf_hg_wide_anyk.h): what ``ops.simtopk`` answers, for any k at
1024 < d <= 4096, with the candidates of every pass taken from the wide 16-bit scan.  One pass of that scan holds k + self <= 20
entries per row; beyond that ``ops.simtopk`` refuses "fast", "auto" takes the exact scan and ``fast_anyk.simtopk_fast_any_k``
refuses (it serves d <= 1024).  Here the later passes scan under a per-row ceiling derived from the last entry the row has emitted
and the wide scan's margin.  Bit for bit the ids and values of ``ops.simtopk(..., precision="exact")``.

    simtopk_wide_any_k(X, Y, k=32)            the multi-pass wide call (f16 or bf16 operands); a single wide fast call where one pass serves
    wide_anyk_plan(d, k, exclude_self)        how the call serves (d, k): depth of a pass, first yield, least number of passes (no GPU)
    simtopk(X, Y, k=32, precision="auto")     the router between the call above, ``fast_anyk.simtopk`` and ``ops.simtopk``
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, fast_anyk, ops
from .ops import _DT, _feat, _metric, _need_gpu, _p

_FAST = ("fast", "fast_bf16")


def wide_anyk_plan(d: int, k: int, exclude_self: bool):
    """dict(multi_pass, scan_kk, first_yield, min_passes) of mmf_wide_anyk_plan: whether ``simtopk_wide_any_k`` runs more than one
    pass for (d, k, exclude_self), the depth of a pass (self's slot included: 20, or k + self where one pass serves), the entries
    per row the first pass emits and the least number of passes.  A ValueError where the call refuses (d <= 1024: that is
    ``fast_anyk.fast_anyk_plan``'s ground; d > 4096, d < 1, k < 1).  Host only: no GPU is touched."""
    kk, fy, mp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mmf_wide_anyk_plan(int(d), int(k), int(bool(exclude_self)), ctypes.byref(kk), ctypes.byref(fy), ctypes.byref(mp))
    if rc < 0:
        msg = _lib.lib().mmf_last_error().decode("utf-8", "replace")
        raise ValueError(f"mmf_wide_anyk_plan: {msg}")
    return {"multi_pass": bool(rc), "scan_kk": kk.value, "first_yield": fy.value, "min_passes": mp.value}


def simtopk_wide_any_k(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, metric="cosine", lam: float = 1.0, k: int = 5,
                       exclude_self: Optional[bool] = None, row_offset: int = 0, col_offset: int = 0, precision: str = "fast",
                       col_splits: int = 0, return_stats: bool = False, return_info: bool = False):
    """(idx int64 [n, k], val f32 [n, k][, stats][, info]) of mmf_simtopk_wide_anyk: the contract and the bits of
    ``ops.simtopk(..., precision="exact")`` for any k >= 1 at 1024 < d <= 4096, from the wide 16-bit scan — ``precision`` "fast"
    (f16 operands) or "fast_bf16"; "auto" means "fast", "exact" forwards to the exact scan.  ``info`` (``return_info``): passes, and
    per pass the yield (entries emitted for every row), ghost_max (the most already-emitted columns the re-rank dropped for a row)
    and exact_rows (rows that took the exact rescan).  d <= 1024 is refused (RuntimeError, before any device work: call
    ``fast_anyk.simtopk_fast_any_k``), and so is d > 4096 under a fast precision.  ``MMF_ANYK_SHORT_DIV`` (environment, default 64):
    a pass's yield may leave n / that many rows to the exact rescan; the result does not depend on it."""
    what = "simtopk_wide_any_k"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    X = _feat(X, f"{what} X")
    _need_gpu(X, what)
    if Y is not None:
        Y = _feat(Y, f"{what} Y")
        if Y.device != X.device or Y.dtype != X.dtype or Y.shape[1] != X.shape[1]:
            raise ValueError(f"{what}: X and Y must share device, dtype and feature dim")
    if exclude_self is None:
        exclude_self = Y is None
    n, d = X.shape
    k = int(k)
    idx = torch.empty((n, max(k, 0)), dtype=torch.int64, device=X.device)
    val = torch.empty((n, max(k, 0)), dtype=torch.float32, device=X.device)
    opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], 0, int(col_splits), _lib.QUERY_ORDERS["auto"], None)
    stats, info = _lib.SimtopkStats(), _lib.FastAnykInfo()
    lib = _lib.lib()
    dev = X.device
    rc = lib.mmf_simtopk_wide_anyk(_p(X), n, _p(Y), n if Y is None else Y.shape[0], d, _DT[X.dtype], _metric(metric), float(lam), k,
                                   int(bool(exclude_self)), int(row_offset), int(col_offset), _p(idx), _p(val), ctypes.byref(opts),
                                   ctypes.byref(stats), dev.index or 0, ops._stream(dev), ctypes.byref(info))
    _lib.check(rc, "mmf_simtopk_wide_anyk")
    out = (idx, val)
    if return_stats:
        out += (stats.as_dict(),)
    if return_info:
        out += (info.as_dict(),)
    return out


# Where "auto" takes the multi-pass wide call (f16 operands).  The rule is the project's three-spreads rule over whole-call times
# (profiles/wide_anyk_timing.txt, written by scripts/wide_anyk_timing.py): a shape class is in this table only where that file shows
# the new call ahead of the exact call by more than three times the exact arm's spread.  Measured ahead (cosine, f32 rows, X against
# itself; A / B): d = 1536 with k = 32 at N = 16384 / 65536 / 262144 (0.59 / 0.43 / 0.39), d = 1536 with k = 64 at N = 65536
# (0.67), d = 2560 with k = 32 at N = 65536 (0.62).  Measured BEHIND: bf16 operands everywhere (2.3 - 4.7 times the exact call).
# Not measured, so not taken: d > 2560, k > 64, N < 16384, k > 32 at d > 1536 or below N = 65536.  Entries: (d_lo, d_hi, k_lo, k_hi,
# n_lo) — d in [d_lo, d_hi], k in [k_lo, k_hi], n >= n_lo; the multi-pass condition (k + self > 20) is checked beside the table.
# Without that file the table would be empty.
_AUTO_SHAPES: tuple = ((1025, 1536, 20, 32, 16384), (1025, 1536, 33, 64, 65536), (1537, 2560, 20, 32, 65536))


def _auto_takes(n: int, d: int, k: int) -> bool:
    return any(dl <= d <= dh and kl <= k <= kh and n >= nl for dl, dh, kl, kh, nl in _AUTO_SHAPES)


def simtopk(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, metric="cosine", lam: float = 1.0, k: int = 5,
            exclude_self: Optional[bool] = None, row_offset: int = 0, col_offset: int = 0, precision: str = "auto",
            col_splits: int = 0, return_stats: bool = False):
    """The router.  "exact": ``ops.simtopk``, unchanged.  "fast" / "fast_bf16": ``simtopk_wide_any_k`` for d > 1024,
    ``fast_anyk.simtopk`` for d <= 1024.  "auto": the multi-pass wide call (f16 operands) on the shapes of ``_AUTO_SHAPES`` — those
    profiles/wide_anyk_timing.txt shows ahead of the exact call by the three-spreads rule: 1024 < d <= 1536 with k <= 32 from
    N = 16384 on and k <= 64 from N = 65536 on, 1536 < d <= 2560 with k <= 32 from N = 65536 on — and
    ``fast_anyk.simtopk(precision="auto")`` everywhere else: the same bits either way."""
    what = "wide_anyk.simtopk"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    kw = dict(metric=metric, lam=lam, k=k, exclude_self=exclude_self, row_offset=row_offset, col_offset=col_offset,
              col_splits=col_splits, return_stats=return_stats)
    if precision == "exact":
        return ops.simtopk(X, Y, precision=precision, **kw)
    Xc = _feat(X, f"{what} X")
    d = Xc.shape[1]
    if precision in _FAST:
        if d > 1024:
            return simtopk_wide_any_k(X, Y, precision=precision, **kw)
        return fast_anyk.simtopk(X, Y, precision=precision, **kw)
    self1 = 1 if (exclude_self if exclude_self is not None else Y is None) else 0
    if 1024 < d <= 4096 and int(k) + self1 > 20 and _auto_takes(Xc.shape[0], d, int(k)):
        return simtopk_wide_any_k(X, Y, precision="fast", **kw)
    return fast_anyk.simtopk(X, Y, precision="auto", **kw)
