"""The 16-bit top-k for any k (include/ext/mmf_hg_fast_anyk.h): what ``ops.simtopk`` answers, for any k at
d <= 1024, with the candidates of every pass taken from the 16-bit matrix cores.  One pass of the 16-bit scan holds k + self <= 44
entries per row at d <= 512 and k + self <= 20 at d <= 1024; beyond that ``ops.simtopk`` refuses "fast" and "auto" takes the exact
scan.  Here the later passes scan under a per-row ceiling derived from the last entry the row has emitted.  Bit for bit the ids
and values of ``ops.simtopk(..., precision="exact")``.

    simtopk_fast_any_k(X, Y, k=64)            the multi-pass 16-bit call (f16 or bf16 operands); a single fast call where one pass serves
    fast_anyk_plan(d, k, exclude_self)        how the call serves (d, k): depth of a pass, first yield, least number of passes (no GPU)
    simtopk(X, Y, k=64, precision="auto")     the router between the call above and ``ops.simtopk``
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, ops
from .ops import _DT, _feat, _metric, _need_gpu, _p

_FAST = ("fast", "fast_bf16")


def fast_anyk_plan(d: int, k: int, exclude_self: bool):
    """dict(multi_pass, scan_kk, first_yield, min_passes) of mmf_fast_anyk_plan: whether ``simtopk_fast_any_k`` runs more than one
    pass for (d, k, exclude_self), the depth of a pass (self's slot included: 44 at d <= 512, 20 at d <= 1024), the entries per
    row the first pass emits and the least number of passes.  A ValueError where the call refuses (d > 1024 beyond one pass of
    the wide scan, d > 4096, d < 1, k < 1).  Host only: no GPU is touched."""
    kk, fy, mp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mmf_fast_anyk_plan(int(d), int(k), int(bool(exclude_self)), ctypes.byref(kk), ctypes.byref(fy), ctypes.byref(mp))
    if rc < 0:
        msg = _lib.lib().mmf_last_error().decode("utf-8", "replace")
        raise ValueError(f"mmf_fast_anyk_plan: {msg}")
    return {"multi_pass": bool(rc), "scan_kk": kk.value, "first_yield": fy.value, "min_passes": mp.value}


def simtopk_fast_any_k(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, metric="cosine", lam: float = 1.0, k: int = 5,
                       exclude_self: Optional[bool] = None, row_offset: int = 0, col_offset: int = 0, precision: str = "fast",
                       col_splits: int = 0, return_stats: bool = False, return_info: bool = False):
    """(idx int64 [n, k], val f32 [n, k][, stats][, info]) of mmf_simtopk_fast_anyk: the contract and the bits of
    ``ops.simtopk(..., precision="exact")`` for any k >= 1 at d <= 1024, from the 16-bit scan — ``precision`` "fast" (f16
    operands) or "fast_bf16"; "auto" means "fast", "exact" forwards to the exact scan.  ``info`` (``return_info``): passes, and per
    pass the yield (entries emitted for every row), ghost_max (the most already-emitted columns the re-rank dropped for a row) and
    exact_rows (rows that took the exact rescan).  d > 1024 with k + self > 20 is refused (RuntimeError, before any device work).
    ``MMF_ANYK_SHORT_DIV`` (environment, default 64): a pass's yield may leave n / that many rows to the exact rescan; the result
    does not depend on it."""
    what = "simtopk_fast_any_k"
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
    rc = lib.mmf_simtopk_fast_anyk(_p(X), n, _p(Y), n if Y is None else Y.shape[0], d, _DT[X.dtype], _metric(metric), float(lam), k,
                                   int(bool(exclude_self)), int(row_offset), int(col_offset), _p(idx), _p(val), ctypes.byref(opts),
                                   ctypes.byref(stats), dev.index or 0, ops._stream(dev), ctypes.byref(info))
    _lib.check(rc, "mmf_simtopk_fast_anyk")
    out = (idx, val)
    if return_stats:
        out += (stats.as_dict(),)
    if return_info:
        out += (info.as_dict(),)
    return out


# Where "auto" takes the multi-pass call (f16 operands).  The rule is the project's three-spreads rule over whole-call times
# (profiles/fast_anyk_timing.txt, written by scripts/fast_anyk_timing.py): a shape class is in this table only where that file shows
# the new call ahead of the exact call by more than three times the exact arm's spread.  Measured ahead: d = 768 / 1024 with k = 32
# and d = 1024 with k = 64 at N = 65536 (A / B 0.50 / 0.42 / 0.58); d = 512 with k = 64 at N = 65536 and 262144 (0.85 / 0.48) and
# with k = 128 at N = 262144 (0.74).  Measured BEHIND: d = 512, k = 128 at N = 65536 (1.24), and bf16 operands everywhere.  Not
# measured, so not taken: d <= 256, N < 65536, k > 128.  Entries: (d_lo, d_hi, k_lo, k_hi, n_lo) — d in [d_lo, d_hi], k in
# [k_lo, k_hi], n >= n_lo; the multi-pass condition (k + self beyond one pass) is checked beside the table.
_AUTO_SHAPES: tuple = ((513, 1024, 20, 64, 65536), (257, 512, 44, 64, 65536), (257, 512, 65, 128, 262144))


def _auto_takes(n: int, d: int, k: int) -> bool:
    return any(dl <= d <= dh and kl <= k <= kh and n >= nl for dl, dh, kl, kh, nl in _AUTO_SHAPES)


def simtopk(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, metric="cosine", lam: float = 1.0, k: int = 5,
            exclude_self: Optional[bool] = None, row_offset: int = 0, col_offset: int = 0, precision: str = "auto",
            col_splits: int = 0, return_stats: bool = False):
    """The router.  "exact": ``ops.simtopk``, unchanged.  "fast" / "fast_bf16": ``simtopk_fast_any_k``.  "auto": the multi-pass
    call on the shapes where profiles/fast_anyk_timing.txt shows it ahead of the exact call by the three-spreads rule
    (``_AUTO_SHAPES``: 512 < d <= 1024 with k <= 64 and 256 < d <= 512 with k <= 64 from N = 65536 on, k <= 128 at d <= 512 from
    N = 262144 on; always with f16 operands), ``ops.simtopk(precision="auto")`` everywhere else — the same bits either way.  Without
    that file the table would be empty and "auto" would equal ``ops.simtopk``."""
    what = "fast_anyk.simtopk"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    kw = dict(metric=metric, lam=lam, k=k, exclude_self=exclude_self, row_offset=row_offset, col_offset=col_offset,
              col_splits=col_splits, return_stats=return_stats)
    if precision in _FAST:
        return simtopk_fast_any_k(X, Y, precision=precision, **kw)
    if precision == "auto":
        Xc = _feat(X, f"{what} X")
        self1 = 1 if (exclude_self if exclude_self is not None else Y is None) else 0
        d = Xc.shape[1]
        if int(k) >= 1 and d <= 1024 and not ops.fast_scan_supported(d, int(k), bool(self1)) and _auto_takes(Xc.shape[0], d, int(k)):
            return simtopk_fast_any_k(X, Y, precision="fast", **kw)
    return ops.simtopk(X, Y, precision=precision, **kw)
