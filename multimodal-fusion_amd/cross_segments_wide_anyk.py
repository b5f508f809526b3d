"""The wide 16-bit cross-segment top-k for any k (include/ext/mmf_hg_cross_segw_anyk.h): what
``cross_segments.simtopk_cross_segments`` answers — every row's k best columns among the rows of all OTHER segments — for any k at
1024 < d <= 4096, with the candidates of every pass taken from the wide 16-bit scan.
``cross_segments_wide.simtopk_cross_segments_wide`` stops at one pass (k <= 20) and ``cross_segments_anyk`` at d = 1024; here the
later passes scan the wide call's work table, under the same per-row column mask, below a per-row ceiling derived from the last
entry the row has emitted (``wide_anyk``, DESIGN.md §4.28, is the same for one matrix).  Bit for bit the ids and values of the
exact call.  bf16 operands are served and lose: their margin is eight times f16's, so about six already-emitted columns per row
slip under the ceiling (against one or two) and shrink every later pass's yield, and most rows' margin bands outgrow a 32-entry
list on a schedule without overflow lists (counted on the CPU in tests/test_cross_segments_wide_anyk_cpu.py).

    simtopk_cross_segments_wide_any_k(X, Y, ptr=..., k=32)   the multi-pass wide call; the one-pass wide call where one pass serves
    cross_segments_wide_anyk_plan(d, k)                    how the call serves (d, k): depth of a pass, first yield, least number of passes (no GPU)
    simtopk_cross_segments(..., precision="auto")          the router between the call above and ``cross_segments_anyk.simtopk_cross_segments``

    cross_segment_knn_edges(X, ptr=..., k=5, precision="auto")    ``cross_segments.cross_segment_knn_edges`` with a precision
    link_slides(out, k=5, precision="auto")                ``cohort.link_slides`` with a precision
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, cross_segments, cross_segments_anyk, ops, wide_scan
from .cross_segments import checked_col_splits, checked_offsets
from .ops import _DT, _feat, _hp, _metric, _need_gpu, _p

_FAST = ("fast", "fast_bf16")


def cross_segments_wide_anyk_plan(d: int, k: int):
    """dict(multi_pass, scan_kk, first_yield, min_passes) of mmf_cross_segments_wide_anyk_plan: whether
    ``simtopk_cross_segments_wide_any_k`` runs more than one pass for (d, k), the depth of a pass (20; no slot goes to self, a row's
    own segment is masked), the entries per row the first pass emits and the least number of passes —
    ``wide_anyk.wide_anyk_plan(d, k, False)``'s answers.  A ValueError where the call refuses (d <= 1024, d > 4096, k < 1).  Host
    only."""
    kk, fy, mp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mmf_cross_segments_wide_anyk_plan(int(d), int(k), ctypes.byref(kk), ctypes.byref(fy), ctypes.byref(mp))
    if rc < 0:
        msg = _lib.lib().mmf_last_error().decode("utf-8", "replace")
        raise ValueError(f"mmf_cross_segments_wide_anyk_plan: {msg}")
    return {"multi_pass": bool(rc), "scan_kk": kk.value, "first_yield": fy.value, "min_passes": mp.value}


def simtopk_cross_segments_wide_any_k(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None,
                                      y_batch=None, metric="cosine", lam: float = 1.0, k: int = 5, precision: str = "fast",
                                      col_splits: int = 0, return_stats: bool = False, return_info: bool = False):
    """(idx int64 [n, k], val f32 [n, k][, stats][, info]) of mmf_simtopk_cross_segments_wide_anyk: the contract and the bits of
    ``cross_segments.simtopk_cross_segments`` (ids are rows of all of Y, key descending then id ascending, never a column of the
    row's own segment, no -1 / -inf fill) for any k >= 1 at 1024 < d <= 4096, from the wide 16-bit scan — ``precision`` "fast" (f16
    operands) or "fast_bf16" (served, but it loses: more ghosts per row, smaller yields, more passes and rescans); "auto" means "fast", "exact" forwards
    to the exact scan.  ``col_splits``: 0 (automatic) or a power of two; the work table is built once and every pass launches it.
    ``info`` (``return_info``): passes, and per pass the yield (entries emitted for every row of the call), ghost_max and exact_rows
    (rows that took the exact rescan).  d <= 1024 is refused (``cross_segments_anyk.simtopk_cross_segments_fast_any_k`` serves it),
    d > 4096 under a fast precision too.  Every refusal is a ValueError raised on the host before any device work.
    ``MMF_ANYK_SHORT_DIV`` as in ``fast_anyk.simtopk_fast_any_k``."""
    what = "simtopk_cross_segments_wide_any_k"
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    X = _feat(X, f"{what} X")
    if Y is not None:
        Y = _feat(Y, f"{what} Y")
        if Y.device != X.device or Y.dtype != X.dtype or Y.shape[1] != X.shape[1]:
            raise ValueError(f"{what}: X and Y must share device, dtype and feature dim")
    xp, yp = checked_offsets(X.shape[0], None if Y is None else Y.shape[0], ptr, batch, y_ptr, y_batch, k, what)
    col_splits = checked_col_splits(col_splits, what)
    mt = _metric(metric)
    n, d = X.shape
    k = int(k)
    # the entry's refusals of an unserved d, as ValueErrors
    if d <= 1024:
        raise ValueError(f"{what}: d = {d} is not above 1024: cross_segments_anyk.simtopk_cross_segments_fast_any_k "
                         "(mmf_simtopk_cross_segments_fast_anyk) serves d <= 1024 for any k")
    if precision != "exact" and d > 4096:
        raise ValueError(f"{what}: d = {d} is beyond the wide 16-bit scan (1024 < d <= 4096; precision='exact' serves it)")
    _need_gpu(X, what)
    idx = torch.empty((n, k), dtype=torch.int64, device=X.device)
    val = torch.empty((n, k), dtype=torch.float32, device=X.device)
    opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], 0, col_splits, _lib.QUERY_ORDERS["off"], None)
    stats, info = _lib.SimtopkStats(), _lib.FastAnykInfo()
    dev = X.device
    rc = _lib.lib().mmf_simtopk_cross_segments_wide_anyk(_p(X), n, _p(Y), n if Y is None else Y.shape[0], d, _DT[X.dtype], mt, float(lam),
                                                         k, _hp(xp), _hp(yp), xp.numel() - 1, _p(idx), _p(val), ctypes.byref(opts),
                                                         ctypes.byref(stats), dev.index or 0, ops._stream(dev), ctypes.byref(info))
    _lib.check(rc, "mmf_simtopk_cross_segments_wide_anyk")
    out = (idx, val)
    if return_stats:
        out += (stats.as_dict(),)
    if return_info:
        out += (info.as_dict(),)
    return out


# Where "auto" takes the multi-pass wide call (f16 operands).  The rule is the project's three-spreads rule over whole-call times
# (profiles/cross_segments_wide_anyk_timing.txt, written by scripts/cross_segments_wide_anyk_timing.py): a shape class enters this
# table only where that file shows the new call ahead of ``cross_segments.simtopk_cross_segments`` by at least three times the exact
# arm's spread.  Measured ahead (MI355X, cosine, f32 Gaussian rows, X against itself; A / B, B − A in spreads of B): at d = 1536,
# k = 32, 64 segments of 1024 rows (0.43, 76), 512 slides of 128 rows (0.42, 271) and 250 ragged slides of 100 .. 300 rows, 47943
# rows (0.38, 304); 16 segments of 4096 rows at d = 2560, k = 32 (0.43, 330); 64 x 1024 at d = 1536, k = 64 (0.68, 135).  Measured
# BEHIND: bf16 operands (3.14 at 64 x 1024, d = 1536, k = 32: yields 20, 7, 3, 2 and 5512 .. 35316 of 65536 rows rescanned per pass),
# so "auto" never takes them.  Not measured, so not taken: fewer than 47943 rows (65536 above d = 1536 and above k = 32), d > 2560,
# k > 32 above d = 1536, k > 64, X against another Y, other metrics.
# Entries: (d_lo, d_hi, k_lo, k_hi, n_lo) — d in [d_lo, d_hi], k in [k_lo, k_hi], n >= n_lo rows; the multi-pass condition is checked
# beside the table.
_AUTO_SHAPES: tuple = ((1025, 1536, 21, 32, 47943), (1025, 1536, 33, 64, 65536), (1537, 2560, 21, 32, 65536))


def _auto_takes(n: int, d: int, k: int) -> bool:
    return any(dl <= d <= dh and kl <= k <= kh and n >= nl for dl, dh, kl, kh, nl in _AUTO_SHAPES)


def simtopk_cross_segments(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                           metric="cosine", lam: float = 1.0, k: int = 5, precision: str = "auto", col_splits: int = 0,
                           return_stats: bool = False, profile: bool = False):
    """The router.  "exact": ``cross_segments.simtopk_cross_segments``, unchanged.  "fast" / "fast_bf16":
    ``simtopk_cross_segments_wide_any_k`` where 1024 < d <= 4096 needs several passes (k > 20),
    ``cross_segments_anyk.simtopk_cross_segments`` (the narrow any-k call, the one-pass narrow or wide 16-bit call, or their
    refusal) elsewhere.  "auto": the multi-pass wide call (f16 operands) on the shape classes of ``_AUTO_SHAPES`` — those
    profiles/cross_segments_wide_anyk_timing.txt shows ahead of the exact call by the three-spreads rule: 1024 < d <= 1536 with
    20 < k <= 32 from 47943 rows on and with 32 < k <= 64 from 65536 rows on, 1536 < d <= 2560 with 20 < k <= 32 from 65536 rows on — and
    ``cross_segments_anyk.simtopk_cross_segments(..., precision="auto")`` everywhere else.  The same bits on every route.
    (``profile`` reaches the one-pass and exact calls only.)"""
    what = "cross_segments_wide_anyk.simtopk_cross_segments"
    if precision not in ("auto", "exact") + _FAST:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    kw = dict(ptr=ptr, batch=batch, y_ptr=y_ptr, y_batch=y_batch, metric=metric, lam=lam, k=k, col_splits=col_splits,
              return_stats=return_stats)
    if precision != "exact":
        Xc = _feat(X, f"{what} X")
        n, d = int(Xc.shape[0]), int(Xc.shape[1])
        several = int(k) >= 1 and 1024 < d <= 4096 and not wide_scan.wide_scan_supported(d, int(k), False)
        if several and precision in _FAST:
            return simtopk_cross_segments_wide_any_k(X, Y, precision=precision, **kw)
        if several and precision == "auto" and _auto_takes(n, d, int(k)):
            return simtopk_cross_segments_wide_any_k(X, Y, precision="fast", **kw)
    return cross_segments_anyk.simtopk_cross_segments(X, Y, precision=precision, profile=profile, **kw)


def _edge_precision(precision, what: str) -> str:
    if precision not in ("exact", "auto"):
        raise ValueError(f"{what}: precision must be 'exact' or 'auto' (got {precision!r})")
    return precision


def cross_segment_knn_edges(X: torch.Tensor, *, ptr=None, batch=None, k: int = 5, precision: str = "exact"):
    """``cross_segments.cross_segment_knn_edges`` with a keyword-only ``precision``: "exact" (the default) is that function, "auto"
    takes every row's neighbours from the router above.  The neighbours are the same bits, so the edges and weights are equal."""
    precision = _edge_precision(precision, "cross_segment_knn_edges")
    if precision == "exact":
        return cross_segments.cross_segment_knn_edges(X, ptr=ptr, batch=batch, k=k)
    return cross_segments.knn_edges_over(X, ptr, batch, k, lambda X_, **kw: simtopk_cross_segments(X_, precision="auto", **kw))


def link_slides(out: dict, k: int = 5, *, precision: str = "exact"):
    """``cohort.link_slides`` with a keyword-only ``precision``, as ``cross_segment_knn_edges`` above takes it."""
    precision = _edge_precision(precision, "link_slides")
    return cross_segments.link_slides_over(out, k, lambda X_, **kw: cross_segment_knn_edges(X_, precision=precision, **kw))
