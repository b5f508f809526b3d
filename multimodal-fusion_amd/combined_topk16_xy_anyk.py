"""The 16-bit top-k of the combined similarity K = K_h * K_g for TWO node sets and ANY k (mmf_simtopk_combined_xy_fast_anyk,
include/ext/mmf_hg_topk16_xy_anyk.h): what ``combined_topk_anyk.simtopk_combined_xy_any_k`` /
``simtopk_combined_rows_any_k`` answer, bit for bit, with the candidates of every pass taken from the 16-bit scan of the combined key.
``combined_topk_xy`` stops at one pass (k + self <= 20) and ``combined_topk16_anyk`` serves one graph or a batch against itself; here
queries and candidates are apart (or the queries are rows [lo, hi) of the candidates), a later pass scans the same work table under a
ceiling per query derived from the last entry the query has emitted, the exact re-rank drops the already-emitted candidates that slip
under it, and the queries a pass cannot finish are gathered into the exact two-set scan from their floors.  Feature dim <= 4096,
position dim <= 8, f32 inputs.

    simtopk_combined_xy_fast_any_k(Fq, Pq, Fc, Pc, lh, lg, k=32)     the multi-pass 16-bit call; the one-pass call where one pass serves
    simtopk_combined_rows_fast_any_k(F, P, lo, hi, lh, lg, k=32)     rows [lo, hi) of one graph against all of it (the library sees a row slice)
    simtopk_combined_xy_any_k / simtopk_combined_rows_any_k(..., precision="auto")   the routers between those and ``combined_topk_anyk``
    ``distributed.sharded_simtopk_combined_fast_any_k``              the row-sharded driver on the rows call
``combined_topk16_anyk.combined_fast_anyk_plan(d, k, exclude_self)`` says how the calls serve (d, k): depth of a pass, first yield,
least passes.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, combined_topk_anyk, combined_topk_xy, ops
from .build_hypergraph._common import compute_device, to_gpu
from .ops import _need_gpu

ONE_PASS_MAX = 20   # k + self one pass of the 16-bit combined scan's lists holds (scan_b16c_supported, csrc/mmf_scan_b16c.hip)
_FAST = ("fast", "fast_bf16")


def _inputs(qf, qp, cf, cp, k: int, precision: str, col_splits: int, row_offset: int, col_offset: int, what: str) -> None:
    """``combined_topk_xy``'s checks, and col_splits 0 or a power of two: before any device work or library call."""
    combined_topk_xy._inputs(qf, qp, cf, cp, k, precision, col_splits, row_offset, col_offset, what)
    cs = int(col_splits)
    if cs & (cs - 1) != 0:
        raise ValueError(f"{what}: col_splits must be 0 or a power of two (got {col_splits})")


def _run(what, Fq, Pq, Fc, Pc, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, precision, col_splits, profile):
    """The entry on device tensors (f32, contiguous rows): (idx, val, stats, info)."""
    dev = Fq.device
    nq, d = Fq.shape
    idx = torch.empty((nq, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((nq, int(k)), dtype=torch.float32, device=dev)
    stats, info = _lib.SimtopkStats(), _lib.FastAnykInfo()
    if nq > 0:
        opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        rc = _lib.lib().mmf_simtopk_combined_xy_fast_anyk(ops._p(Fq), ops._p(Pq), nq, ops._p(Fc), ops._p(Pc), Fc.shape[0], d, Pq.shape[1],
                                                          float(lambda_h), float(lambda_g), int(k), int(bool(exclude_self)), int(row_offset),
                                                          int(col_offset), ops._p(idx), ops._p(val), ctypes.byref(opts), ctypes.byref(stats),
                                                          dev.index or 0, ops._stream(dev), ctypes.byref(info))
        _lib.check(rc, what)
    return idx, val, stats, info


def _result(idx, val, stats, info, return_stats, return_info):
    out = (idx, val)
    if return_stats:
        out += (stats.as_dict(),)
    if return_info:
        out += (info.as_dict(),)
    return out


def simtopk_combined_xy_fast_any_k(q_features: torch.Tensor, q_positions: torch.Tensor, c_features: torch.Tensor, c_positions: torch.Tensor,
                                   lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *, exclude_self: bool = False, row_offset: int = 0,
                                   col_offset: int = 0, precision: str = "fast", col_splits: int = 0, return_stats: bool = False,
                                   return_info: bool = False, profile: bool = False):
    """(idx [Nq, k] int64, val [Nq, k] f32[, stats][, info]) of mmf_simtopk_combined_xy_fast_anyk: the contract and the bits of
    ``combined_topk_anyk.simtopk_combined_xy_any_k`` for any k >= 1 at D <= 4096, from the 16-bit scan of the combined key —
    ``precision`` "fast" (f16 images of the features) or "fast_bf16"; "auto" means "fast", "exact" forwards to the exact passes (any
    D).  Per query the k best candidates, reported as ``col_offset + candidate row``; ``exclude_self`` drops the pair whose ids agree
    (``row_offset + i == col_offset + j``); a query with fewer than k admissible candidates gets them first, then -1 / -inf.  Where
    k + self <= 20 the call is ``combined_topk_xy.simtopk_combined_xy`` at that precision; with fewer than k + self candidates it is
    served exactly.  Queries that are a row view of the candidates (features and positions alike) are recognised by the library as
    a row slice: one operand image.  ``col_splits``: 0 (automatic) or a power of two.  ``info`` (``return_info``): passes, and per
    pass the yield (entries emitted for every query), ghost_max (the most already-emitted candidates the re-rank dropped for a
    query) and exact_rows (queries that took the exact rescan).  The tensors must be on the GPU (RuntimeError otherwise).
    ``MMF_ANYK_SHORT_DIV`` as in ``fast_anyk.simtopk_fast_any_k``."""
    what = "simtopk_combined_xy_fast_any_k"
    _inputs(q_features, q_positions, c_features, c_positions, k, precision, col_splits, row_offset, col_offset, what)
    _need_gpu(q_features, what)
    dev = q_features.device
    if any(t.device != dev for t in (q_positions, c_features, c_positions)):
        raise ValueError(f"{what}: the four tensors must share a device")
    Fq, Pq, Fc, Pc = (to_gpu(t, dev) for t in (q_features, q_positions, c_features, c_positions))
    idx, val, stats, info = _run(what, Fq, Pq, Fc, Pc, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, precision, col_splits, profile)
    return _result(idx, val, stats, info, return_stats, return_info)


def simtopk_combined_rows_fast_any_k(features: torch.Tensor, positions: torch.Tensor, lo: int, hi: int, lambda_h: float = 1.0,
                                     lambda_g: float = 1.0, k: int = 5, *, exclude_self: bool = True, col_offset: int = 0,
                                     precision: str = "fast", col_splits: int = 0, return_stats: bool = False, return_info: bool = False,
                                     profile: bool = False):
    """Rows [lo, hi) of ``combined_topk16_anyk.simtopk_combined_fast_any_k(features, positions, ...)`` (one graph) — so of
    ``combined_topk_anyk.simtopk_combined_any_k`` — bit for bit, without computing the other rows: (idx [hi - lo, k],
    val [hi - lo, k][, stats][, info]), ids shifted by ``col_offset``.  The library is handed views of the two arrays, so it sees a
    row slice: one operand image and one set of chains for all N rows, whatever the panel.  Device tensors only."""
    what = "simtopk_combined_rows_fast_any_k"
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= features.shape[0]:
        raise ValueError(f"{what}: rows [{lo}, {hi}) are no range of the {features.shape[0]} rows")
    _inputs(features[lo:hi], positions[lo:hi], features, positions, k, precision, col_splits, 0, col_offset, what)
    _need_gpu(features, what)
    if positions.device != features.device:
        raise ValueError(f"{what}: features and positions must share a device")
    dev = features.device
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    idx, val, stats, info = _run(what, F[lo:hi], P[lo:hi], F, P, lambda_h, lambda_g, k, exclude_self, int(col_offset) + lo, col_offset, precision,
                                 col_splits, profile)
    return _result(idx, val, stats, info, return_stats, return_info)


# Where "auto" takes the multi-pass 16-bit call (f16 operands).  The rule is the project's three-spreads rule over whole-call times
# (profiles/simtopk_combined_xy_fast_anyk_timing.txt, written by scripts/simtopk_combined_xy_fast_anyk_timing.py): a shape class
# enters this table only where that file shows the new call ahead of mmf_simtopk_combined_xy_anyk by more than three times the exact
# arm's spread at EVERY measured shape of the class.  Measured ahead (MI355X, dp = 2, pixel positions; A / B, B - A in spreads of B,
# at k = 32 and k = 64): the row panel of one eighth of N = 65536 at d = 512 — 0.52 (120) and 0.76 (68) — and at d = 1536 — 0.43 (156)
# and 0.55 (149); of N = 262144 at d = 512 — 0.47 (229) and 0.57 (326); 16384 queries against 65536 distinct candidates at d = 512 —
# 0.54 (26) and 0.70 (49) — and at d = 1536 — 0.46 (106) and 0.61 (99).  Between the two measured dims the scan's share only grows,
# as in the one-pass entries' rule.  bf16 operands pass the same rule at every shape but are not ahead of f16 (at
# d = 1536, k = 64 on the panel they are 24 % behind it), so "auto" never takes them.  Not measured, so not taken: fewer than 8192
# queries or 65536 candidates, d < 512 or d > 1536, k > 64.
# Entries: (d_lo, d_hi, k_lo, k_hi, nq_lo, nc_lo) — d in [d_lo, d_hi], k in [k_lo, k_hi], at least nq_lo queries against at least
# nc_lo candidates; the multi-pass condition is checked beside the table.
_AUTO_SHAPES: tuple = ((512, 1536, 20, 64, 8192, 65536),)


def _auto_takes(nq: int, nc: int, d: int, k: int) -> bool:
    return any(dl <= d <= dh and kl <= k <= kh and nq >= ql and nc >= cl for dl, dh, kl, kh, ql, cl in _AUTO_SHAPES)


def xy_anyk_route(nq: int, nc: int, d: int, k: int, exclude_self: bool, precision: str = "auto") -> str:
    """What the routers of this module call for nq queries against nc candidates: "fast" (this module's 16-bit calls) or "exact"
    (``combined_topk_anyk``'s).  Host only."""
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"xy_anyk_route: unknown precision {precision!r}")
    if int(k) < 1:
        raise ValueError(f"xy_anyk_route: k must be >= 1 (got {k})")
    if precision in _FAST:
        return "fast"
    kk = int(k) + (1 if exclude_self else 0)
    several = kk > ONE_PASS_MAX and 1 <= int(d) <= 4096 and int(nc) >= kk
    if precision == "auto" and several and _auto_takes(int(nq), int(nc), int(d), int(k)):
        return "fast"
    return "exact"


def simtopk_combined_xy_any_k(q_features: torch.Tensor, q_positions: torch.Tensor, c_features: torch.Tensor, c_positions: torch.Tensor,
                              lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *, exclude_self: bool = False, row_offset: int = 0,
                              col_offset: int = 0, precision: str = "auto", col_splits: int = 0, return_stats: bool = False,
                              profile: bool = False):
    """The router: (idx, val[, stats]), the same bits on every route.  "fast" / "fast_bf16": ``simtopk_combined_xy_fast_any_k``.
    "auto": that call (f16 operands) on the shape classes of ``_AUTO_SHAPES`` — those
    profiles/simtopk_combined_xy_fast_anyk_timing.txt shows ahead of the exact passes by the three-spreads rule at every measured
    shape: 8192 queries or more against 65536 candidates or more at 512 <= D <= 1536 with k <= 64 (beyond one pass) — and ``combined_topk_anyk.simtopk_combined_xy_any_k`` everywhere else.  "exact": the latter, unchanged.  CPU tensors are
    computed on the current GPU and the result moved back."""
    what = "combined_topk16_xy_anyk.simtopk_combined_xy_any_k"
    combined_topk_xy._inputs(q_features, q_positions, c_features, c_positions, k, precision, col_splits, row_offset, col_offset, what)
    kw = dict(exclude_self=exclude_self, row_offset=row_offset, col_offset=col_offset, col_splits=col_splits, return_stats=return_stats,
              profile=profile)
    if xy_anyk_route(q_features.shape[0], c_features.shape[0], q_features.shape[1], k, exclude_self, precision) == "exact":
        return combined_topk_anyk.simtopk_combined_xy_any_k(q_features, q_positions, c_features, c_positions, lambda_h, lambda_g, k, **kw)
    home = q_features.device
    dev = compute_device(q_features, q_positions, c_features, c_positions)
    Fq, Pq, Fc, Pc = (to_gpu(t, dev) for t in (q_features, q_positions, c_features, c_positions))
    out = simtopk_combined_xy_fast_any_k(Fq, Pq, Fc, Pc, lambda_h, lambda_g, k, precision="fast" if precision == "auto" else precision, **kw)
    return (out[0].to(home), out[1].to(home)) + tuple(out[2:])


def simtopk_combined_rows_any_k(features: torch.Tensor, positions: torch.Tensor, lo: int, hi: int, lambda_h: float = 1.0,
                                lambda_g: float = 1.0, k: int = 5, *, exclude_self: bool = True, col_offset: int = 0,
                                precision: str = "auto", col_splits: int = 0, return_stats: bool = False, profile: bool = False):
    """The router for rows [lo, hi) of one graph: ``simtopk_combined_rows_fast_any_k`` under "fast" / "fast_bf16" and, under "auto",
    on the shape classes of ``_AUTO_SHAPES`` (hi - lo >= 8192 queries against all N >= 65536 rows at 512 <= D <= 1536 with k <= 64
    beyond one pass); ``combined_topk_anyk.simtopk_combined_rows_any_k``
    everywhere else and under "exact".  The same bits on every route."""
    what = "combined_topk16_xy_anyk.simtopk_combined_rows_any_k"
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= features.shape[0]:
        raise ValueError(f"{what}: rows [{lo}, {hi}) are no range of the {features.shape[0]} rows")
    combined_topk_xy._inputs(features[lo:hi], positions[lo:hi], features, positions, k, precision, col_splits, 0, col_offset, what)
    kw = dict(exclude_self=exclude_self, col_offset=col_offset, col_splits=col_splits, return_stats=return_stats, profile=profile)
    if xy_anyk_route(hi - lo, features.shape[0], features.shape[1], k, exclude_self, precision) == "exact":
        return combined_topk_anyk.simtopk_combined_rows_any_k(features, positions, lo, hi, lambda_h, lambda_g, k, **kw)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    out = simtopk_combined_rows_fast_any_k(F, P, lo, hi, lambda_h, lambda_g, k, precision="fast" if precision == "auto" else precision, **kw)
    return (out[0].to(home), out[1].to(home)) + tuple(out[2:])
