"""The segmented 16-bit top-k for any k (include/ext/mmf_hg_seg_anyk.h): what
``segmented_exact.simtopk_segmented_exact`` answers for a ragged batch, for any k at d <= 1024, with the candidates of every pass
taken from the 16-bit matrix cores.  ``ops.simtopk_segmented`` stops at one pass (k + self <= 44 at d <= 512, <= 20 at d <= 1024);
here the later passes scan the same work table under a per-row ceiling derived from the last entry the row has emitted
(``fast_anyk``, DESIGN.md §4.27, is the same for one matrix).  Bit for bit the ids and values of the exact call.

    simtopk_segmented_fast_any_k(X, Y, ptr=..., k=32)   the multi-pass 16-bit call of a cohort; one segmented fast call where one pass serves
    segmented_anyk_plan(d, k, exclude_self)              how the call serves (d, k): depth of a pass, first yield, least number of passes (no GPU)
    simtopk_segmented(..., precision="auto")             the router between the call above and ``segmented_exact.simtopk_segmented``
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, ops, ragged, segmented_exact, wide_scan
from .ops import _DT, _feat, _hp, _metric, _need_gpu, _p

_FAST = ("fast", "fast_bf16")


def segmented_anyk_plan(d: int, k: int, exclude_self: bool):
    """dict(multi_pass, scan_kk, first_yield, min_passes) of mmf_segmented_anyk_plan: whether ``simtopk_segmented_fast_any_k`` runs
    more than one pass for (d, k, exclude_self), the depth of a pass (self's slot included: 44 at d <= 512, 20 at d <= 1024), the
    entries per row the first pass emits and the least number of passes — ``fast_anyk.fast_anyk_plan``'s answers for d <= 1024.  A
    ValueError where the call refuses (d > 1024 beyond one pass of the wide segmented scan, d < 1, k < 1).  Host only."""
    kk, fy, mp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mmf_segmented_anyk_plan(int(d), int(k), int(bool(exclude_self)), ctypes.byref(kk), ctypes.byref(fy), ctypes.byref(mp))
    if rc < 0:
        msg = _lib.lib().mmf_last_error().decode("utf-8", "replace")
        raise ValueError(f"mmf_segmented_anyk_plan: {msg}")
    return {"multi_pass": bool(rc), "scan_kk": kk.value, "first_yield": fy.value, "min_passes": mp.value}


def simtopk_segmented_fast_any_k(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                                 metric="cosine", lam: float = 1.0, k: int = 5, exclude_self: Optional[bool] = None,
                                 precision: str = "fast", return_stats: bool = False, return_info: bool = False):
    """(idx int64 [n, k] GLOBAL row ids of Y, val f32 [n, k][, stats][, info]) of mmf_simtopk_segmented_fast_anyk: the contract and
    the bits of ``segmented_exact.simtopk_segmented_exact`` for any k >= 1 at d <= 1024, from the 16-bit scan — ``precision``
    "fast" (f16 operands) or "fast_bf16"; "auto" means "fast", "exact" forwards to the exact scan.  Segments as in
    ``ops.simtopk_segmented`` (``ptr`` / ``batch``, ``y_ptr`` / ``y_batch``); a segment with fewer than k admissible columns gets them
    first, then -1 / -inf.  ``info`` (``return_info``): passes, and per pass the yield (entries emitted for every row of the call),
    ghost_max and exact_rows (rows of served segments that took the exact rescan).  d > 1024 with k + self > 20 is refused
    (RuntimeError, before any device work).  ``MMF_ANYK_SHORT_DIV`` as in ``fast_anyk.simtopk_fast_any_k``."""
    what = "simtopk_segmented_fast_any_k"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
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
    if exclude_self is None:
        exclude_self = Y is None
    _need_gpu(X, what)
    n, d = X.shape
    k = int(k)
    idx = torch.empty((n, k), dtype=torch.int64, device=X.device)
    val = torch.empty((n, k), dtype=torch.float32, device=X.device)
    opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], 0, 0, _lib.QUERY_ORDERS["off"], None)
    stats, info = _lib.SimtopkStats(), _lib.FastAnykInfo()
    dev = X.device
    rc = _lib.lib().mmf_simtopk_segmented_fast_anyk(_p(X), n, _p(Y), n if Y is None else Y.shape[0], d, _DT[X.dtype], _metric(metric),
                                                    float(lam), k, int(bool(exclude_self)), _hp(xp), _hp(yp), xp.numel() - 1, _p(idx),
                                                    _p(val), ctypes.byref(opts), ctypes.byref(stats), dev.index or 0, ops._stream(dev),
                                                    ctypes.byref(info))
    _lib.check(rc, "mmf_simtopk_segmented_fast_anyk")
    out = (idx, val)
    if return_stats:
        out += (stats.as_dict(),)
    if return_info:
        out += (info.as_dict(),)
    return out


# Where "auto" takes the multi-pass call (f16 operands).  The rule is the project's three-spreads rule over whole-call times
# (profiles/segmented_anyk_timing.txt, written by scripts/segmented_anyk_timing.py): a shape class enters this table only where that
# file shows the new call ahead of ``segmented_exact.simtopk_segmented_exact`` by more than three times the exact arm's spread.
# Measured ahead (262144 rows, cosine): 16 segments of 16384 rows with k = 32 at d = 768 and d = 1024 (A / B 0.92 / 0.81, 19 and 130
# spreads of B).  Measured BEHIND: the same cohort at d = 512, k = 64 (1.21); 64 segments of 4096 rows at all three (d, k) (1.36 -
# 1.78); 1000 ragged slides of 100 .. 300 rows and 2048 slides of 128 rows at d = 768, k = 32 (2.2 / 2.3); bf16 operands (4.4).  Not
# measured, so not taken: k > 32 above d = 512, fewer than 262144 rows, d <= 256.
# Entries: (d_lo, d_hi, k_lo, k_hi, n_lo, rows_per_segment_lo) — d in [d_lo, d_hi], k in [k_lo, k_hi], n >= n_lo rows in segments
# that average at least rows_per_segment_lo rows; the multi-pass condition is checked beside the table.
_AUTO_SHAPES: tuple = ((513, 1024, 20, 32, 262144, 16384),)


def _auto_takes(n: int, d: int, k: int, n_segments: int) -> bool:
    per = n / max(int(n_segments), 1)
    return any(dl <= d <= dh and kl <= k <= kh and n >= nl and per >= pl for dl, dh, kl, kh, nl, pl in _AUTO_SHAPES)


def _n_segments(ptr, batch) -> int:
    if ptr is not None:
        return max(int(torch.as_tensor(ptr).numel()) - 1, 0)
    if batch is not None and torch.as_tensor(batch).numel() > 0:
        return int(torch.as_tensor(batch)[-1]) + 1
    return 0


def simtopk_segmented(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                      metric="cosine", lam: float = 1.0, k: int = 5, exclude_self: Optional[bool] = None, precision: str = "auto",
                      return_stats: bool = False):
    """The router.  "exact": ``segmented_exact.simtopk_segmented``, unchanged.  "fast" / "fast_bf16": that router where one pass of a
    16-bit scan serves (d, k), ``simtopk_segmented_fast_any_k`` where d <= 1024 needs several; d > 1024 beyond one pass raises the
    entry's refusal.  "auto": the multi-pass call (f16 operands) on the shape classes profiles/segmented_anyk_timing.txt shows
    ahead of the exact call by the three-spreads rule (``_AUTO_SHAPES``: 512 < d <= 1024 with k <= 32 from 262144 rows on, in
    segments of 16384 rows or more on average), ``segmented_exact.simtopk_segmented`` everywhere else — small slides lose to the
    exact table-driven scan.  The same bits either way."""
    what = "segmented_anyk.simtopk_segmented"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    if X.dim() != 2:
        raise ValueError(f"{what} X: expected a 2-D [N, D] tensor, got shape {tuple(X.shape)}")
    kw = dict(ptr=ptr, batch=batch, y_ptr=y_ptr, y_batch=y_batch, metric=metric, lam=lam, k=k, exclude_self=exclude_self,
              return_stats=return_stats)
    self_ex = (Y is None) if exclude_self is None else bool(exclude_self)
    d = int(X.shape[1])
    one_pass = int(k) < 1 or ops.fast_scan_supported(d, int(k), self_ex) or (d > 1024 and wide_scan.wide_scan_supported(d, int(k), self_ex))
    if precision in _FAST and not one_pass:
        return simtopk_segmented_fast_any_k(X, Y, precision=precision, **kw)      # (d > 1024: the entry refuses)
    if precision == "auto" and not one_pass and d <= 1024 and _auto_takes(int(X.shape[0]), d, int(k), _n_segments(ptr, batch)):
        return simtopk_segmented_fast_any_k(X, Y, precision="fast", **kw)
    return segmented_exact.simtopk_segmented(X, Y, precision=precision, **kw)
