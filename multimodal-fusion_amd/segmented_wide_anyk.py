"""The segmented wide 16-bit top-k for any k (include/ext/mmf_hg_segw_anyk.h): what
``segmented_exact.simtopk_segmented_exact`` answers for a ragged batch, for any k at 1024 < d <= 4096, with the candidates of every
pass taken from the wide 16-bit scan.  ``wide_scan.simtopk_segmented`` stops at one pass (k + self <= 20) and ``segmented_anyk`` at
d = 1024; here the later passes scan the wide segmented call's work table under a ceiling per operand position derived from the last
entry the row has emitted (``wide_anyk``, DESIGN.md §4.28, is the same for one matrix).  Bit for bit the ids and values of the exact
call.  bf16 operands are served and lose: their margin is eight times f16's, so more already-emitted columns per row slip under the
ceiling and most rows' margin bands outgrow a 32-entry list on a schedule without overflow lists (counted on the CPU in
tests/test_segmented_wide_anyk_cpu.py).

    simtopk_segmented_wide_any_k(X, Y, ptr=..., k=32)    the multi-pass wide call of a cohort; the one-pass wide call where one pass serves
    segmented_wide_anyk_plan(d, k, exclude_self)          how the call serves (d, k): depth of a pass, first yield, least number of passes (no GPU)
    simtopk_segmented(..., precision="auto")              the router between the call above and ``segmented_anyk.simtopk_segmented``
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, ops, ragged, segmented_anyk, wide_scan
from .ops import _DT, _feat, _hp, _metric, _need_gpu, _p

_FAST = ("fast", "fast_bf16")


def segmented_wide_anyk_plan(d: int, k: int, exclude_self: bool):
    """dict(multi_pass, scan_kk, first_yield, min_passes) of mmf_segmented_wide_anyk_plan: whether ``simtopk_segmented_wide_any_k``
    runs more than one pass for (d, k, exclude_self), the depth of a pass (self's slot included: 20), the entries per row the first
    pass emits and the least number of passes — ``wide_anyk.wide_anyk_plan``'s answers.  A ValueError where the call refuses
    (d <= 1024, d > 4096, d < 1, k < 1).  Host only."""
    kk, fy, mp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mmf_segmented_wide_anyk_plan(int(d), int(k), int(bool(exclude_self)), ctypes.byref(kk), ctypes.byref(fy), ctypes.byref(mp))
    if rc < 0:
        msg = _lib.lib().mmf_last_error().decode("utf-8", "replace")
        raise ValueError(f"mmf_segmented_wide_anyk_plan: {msg}")
    return {"multi_pass": bool(rc), "scan_kk": kk.value, "first_yield": fy.value, "min_passes": mp.value}


def simtopk_segmented_wide_any_k(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                                 metric="cosine", lam: float = 1.0, k: int = 5, exclude_self: Optional[bool] = None,
                                 precision: str = "fast", return_stats: bool = False, return_info: bool = False, col_splits: int = 0):
    """(idx int64 [n, k] GLOBAL row ids of Y, val f32 [n, k][, stats][, info]) of mmf_simtopk_segmented_wide_anyk: the contract and
    the bits of ``segmented_exact.simtopk_segmented_exact`` for any k >= 1 at 1024 < d <= 4096, from the wide 16-bit scan —
    ``precision`` "fast" (f16 operands) or "fast_bf16" (served, but it loses: more ghosts per row, smaller yields, more rescans);
    "auto" means "fast", "exact" forwards to the exact scan.  The arguments of ``segmented_anyk.simtopk_segmented_fast_any_k``, and
    ``col_splits``: 0 (one column range per segment) or a power of two, the ranges every segment is scanned in (at most one per 128
    columns of the segment); the work table is built once and every pass launches it.  A segment with fewer than k admissible columns
    gets them first, then -1 / -inf.  ``info`` (``return_info``): passes, and per pass the yield (entries emitted for every row of
    the call), ghost_max and exact_rows (rows of served segments that took the exact rescan).  d <= 1024 is refused
    (``segmented_anyk.simtopk_segmented_fast_any_k`` serves it), d > 4096 under a fast precision too (RuntimeError, before any device
    work).  ``MMF_ANYK_SHORT_DIV`` as in ``fast_anyk.simtopk_fast_any_k``."""
    what = "simtopk_segmented_wide_any_k"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    X = _feat(X, f"{what} X")
    if Y is not None:
        Y = _feat(Y, f"{what} Y")
        if Y.device != X.device or Y.dtype != X.dtype or Y.shape[1] != X.shape[1]:
            raise ValueError(f"{what}: X and Y must share device, dtype and feature dim")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    col_splits = int(col_splits)
    if col_splits < 0 or col_splits & (col_splits - 1):
        raise ValueError(f"{what}: col_splits must be 0 or a power of two (got {col_splits})")
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
    opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], 0, col_splits, _lib.QUERY_ORDERS["off"], None)
    stats, info = _lib.SimtopkStats(), _lib.FastAnykInfo()
    dev = X.device
    rc = _lib.lib().mmf_simtopk_segmented_wide_anyk(_p(X), n, _p(Y), n if Y is None else Y.shape[0], d, _DT[X.dtype], _metric(metric),
                                                    float(lam), k, int(bool(exclude_self)), _hp(xp), _hp(yp), xp.numel() - 1, _p(idx),
                                                    _p(val), ctypes.byref(opts), ctypes.byref(stats), dev.index or 0, ops._stream(dev),
                                                    ctypes.byref(info))
    _lib.check(rc, "mmf_simtopk_segmented_wide_anyk")
    out = (idx, val)
    if return_stats:
        out += (stats.as_dict(),)
    if return_info:
        out += (info.as_dict(),)
    return out


# Where "auto" takes the multi-pass wide call (f16 operands).  The rule is the project's three-spreads rule over whole-call times
# (profiles/segmented_wide_anyk_timing.txt, written by scripts/segmented_wide_anyk_timing.py): a shape class enters this table only
# where that file shows the new call ahead of ``segmented_exact.simtopk_segmented_exact`` by more than three times the exact arm's
# spread.  Measured ahead (MI355X, 262144 rows, cosine, f32 Gaussian rows, X against itself, k = 32; A / B, B − A in spreads of B):
# 4 segments of 65536 rows at d = 1536 (0.46, 342), 16 segments of 16384 rows at d = 1536 (0.73, 83) and at d = 2560 (0.72, 201).
# Measured BEHIND: 64 segments of 4096 rows (1.98) and 2048 slides of 128 rows (1.80) at d = 1536, k = 32 — the exact table-driven
# scan of a small segment costs little, two wide passes and their bookkeeping do not shrink with it; 16 x 16384 at d = 1536, k = 64
# (1.09: five passes, ghosts grow from pass to pass); bf16 operands (7.7 at 64 x 4096: yields 19, 7, 4, 2 and a third to two thirds of
# the rows rescanned per pass), so "auto" never takes them.  Not measured, so not taken: fewer than 262144 rows, segments that average
# between 4096 and 16384 rows (where the break-even lies), d > 2560, k > 32, X against another Y, other metrics.
# Entries: (d_lo, d_hi, k_lo, k_hi, n_lo, rows_per_segment_lo) — d in [d_lo, d_hi], k in [k_lo, k_hi], n >= n_lo rows in
# segments that average at least rows_per_segment_lo rows; the multi-pass condition is checked beside the table.
_AUTO_SHAPES: tuple = ((1025, 2560, 20, 32, 262144, 16384),)


def _auto_takes(n: int, d: int, k: int, n_segments: int) -> bool:
    per = n / max(int(n_segments), 1)
    return any(dl <= d <= dh and kl <= k <= kh and n >= nl and per >= pl for dl, dh, kl, kh, nl, pl in _AUTO_SHAPES)


def simtopk_segmented(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                      metric="cosine", lam: float = 1.0, k: int = 5, exclude_self: Optional[bool] = None, precision: str = "auto",
                      return_stats: bool = False):
    """The router.  "fast" / "fast_bf16": ``simtopk_segmented_wide_any_k`` where 1024 < d <= 4096 needs several passes
    (k + self > 20), ``segmented_anyk.simtopk_segmented`` (the narrow any-k call, the one-pass narrow or wide 16-bit call, or their
    refusal) elsewhere.  "auto": the multi-pass wide call (f16 operands) on the shape classes of ``_AUTO_SHAPES`` — those
    profiles/segmented_wide_anyk_timing.txt shows ahead of the exact call by the three-spreads rule: 1024 < d <= 2560 with k <= 32
    from 262144 rows on, in segments of 16384 rows or more on average; cohorts of smaller slides lose to the exact scan — and
    ``segmented_anyk.simtopk_segmented(..., precision="auto")`` everywhere else.  "exact": that router, unchanged.  The same bits
    on every route."""
    what = "segmented_wide_anyk.simtopk_segmented"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    if X.dim() != 2:
        raise ValueError(f"{what} X: expected a 2-D [N, D] tensor, got shape {tuple(X.shape)}")
    kw = dict(ptr=ptr, batch=batch, y_ptr=y_ptr, y_batch=y_batch, metric=metric, lam=lam, k=k, exclude_self=exclude_self,
              return_stats=return_stats)
    if precision != "exact":
        self_ex = (Y is None) if exclude_self is None else bool(exclude_self)
        n, d = int(X.shape[0]), int(X.shape[1])
        several = int(k) >= 1 and 1024 < d <= 4096 and not wide_scan.wide_scan_supported(d, int(k), self_ex)
        if several and precision in _FAST:
            return simtopk_segmented_wide_any_k(X, Y, precision=precision, **kw)
        if several and precision == "auto" and _auto_takes(n, d, int(k), segmented_anyk._n_segments(ptr, batch)):
            return simtopk_segmented_wide_any_k(X, Y, precision="fast", **kw)
    return segmented_anyk.simtopk_segmented(X, Y, precision=precision, **kw)
