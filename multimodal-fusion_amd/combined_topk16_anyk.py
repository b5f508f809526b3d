"""The 16-bit top-k of the combined similarity K = K_h * K_g for ANY k (mmf_simtopk_combined_fast_anyk,
include/ext/mmf_hg_topk16_anyk.h): what ``combined_topk_anyk.simtopk_combined_any_k`` answers for one graph or a
ragged batch, bit for bit, with the candidates of every pass taken from the 16-bit scan of the combined key.  ``combined_topk16`` and
``combined_topk16_segmented`` stop at one pass (k + self <= 20); here a later pass scans the same work table under a ceiling per row
derived from the last entry the row has emitted, the exact re-rank drops the already-emitted columns that slip under it, and the rows
a pass cannot finish are gathered into the exact scan of the combined key from their floors.  Feature dim <= 4096, position dim <= 8,
f32 inputs.

    simtopk_combined_fast_any_k(F, P, lh, lg, k=32)            the multi-pass 16-bit call; the one-pass call where one pass serves
    combined_fast_anyk_plan(d, k, exclude_self)                how the call serves (d, k): depth of a pass, first yield, least passes (no GPU)
    simtopk_combined_any_k(..., precision="auto")              the router between the call above and ``combined_topk_anyk``
    build_topk_weighted_hypergraph_fast_any_k / build_topk_hypergraph_data_fast_any_k   ``combined_topk_anyk``'s builders on the router
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib, combined_topk, combined_topk_anyk, ops, ragged
from .build_hypergraph._common import compute_device, result_device_like_kernel, to_gpu
from .ops import _need_gpu
from .weighted_hypergraph import segment_mean_pool

ONE_PASS_MAX = 20   # k + self one pass of the 16-bit combined scan's lists holds (scan_b16c_supported, csrc/mmf_scan_b16c.hip)
_FAST = ("fast", "fast_bf16")


def combined_fast_anyk_plan(d: int, k: int, exclude_self: bool):
    """dict(multi_pass, scan_kk, first_yield, min_passes) of mmf_combined_fast_anyk_plan: whether ``simtopk_combined_fast_any_k``
    runs more than one pass for (d, k, exclude_self), the depth of its first scan (self's slot included: k + self, or 20 beyond one
    pass), the entries per row the first pass emits and the least number of passes (every later pass emits at most 20 - self).  A
    ValueError where the call refuses (d > 4096, d < 1, k < 1).  Host only."""
    kk, fy, mp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mmf_combined_fast_anyk_plan(int(d), int(k), int(bool(exclude_self)), ctypes.byref(kk), ctypes.byref(fy), ctypes.byref(mp))
    if rc < 0:
        msg = _lib.lib().mmf_last_error().decode("utf-8", "replace")
        raise ValueError(f"mmf_combined_fast_anyk_plan: {msg}")
    return {"multi_pass": bool(rc), "scan_kk": kk.value, "first_yield": fy.value, "min_passes": mp.value}


def _inputs(features: torch.Tensor, positions: torch.Tensor, k: int, ptr, batch, precision: str, col_splits: int, what: str) -> torch.Tensor:
    """Host offsets ([0, N] for one graph), checked before any device work or library call: shapes, k, the precision's name,
    col_splits, ptr / batch.  The entry refuses what it does not support (D > 4096, dp > 8) with its own words."""
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    cs = int(col_splits)
    if cs < 0 or (cs & (cs - 1)) != 0:
        raise ValueError(f"{what}: col_splits must be 0 or a power of two (got {col_splits})")
    return combined_topk._inputs(features, positions, k, ptr, batch, what)


def simtopk_combined_fast_any_k(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *,
                                ptr=None, batch=None, exclude_self: bool = True, precision: str = "fast", col_splits: int = 0,
                                return_stats: bool = False, return_info: bool = False, profile: bool = False):
    """(idx [N, k] int64 global row ids, val [N, k] f32[, stats][, info]) of mmf_simtopk_combined_fast_anyk: the contract and the bits
    of ``combined_topk_anyk.simtopk_combined_any_k`` for any k >= 1 at D <= 4096, from the 16-bit scan of the combined key —
    ``precision`` "fast" (f16 images of the features) or "fast_bf16"; "auto" means "fast", "exact" forwards to the exact passes.
    Without ``ptr`` / ``batch`` the rows are one graph.  Where k + self <= 20 the call is ``combined_topk16.simtopk_combined_fast`` /
    ``combined_topk16_segmented.simtopk_combined_fast_segmented`` at that precision.  ``col_splits``: 0 (automatic) or a power of two,
    the column ranges every segment is scanned in at most.  A segment with fewer than k admissible columns gets them first, then
    -1 / -inf.  ``info`` (``return_info``): passes, and per pass the yield (entries emitted for every row of the call), ghost_max
    (the most already-emitted columns the re-rank dropped for a row) and exact_rows (rows of served segments that took the exact
    rescan).  The tensors must be on the GPU (RuntimeError otherwise).  ``MMF_ANYK_SHORT_DIV`` as in ``fast_anyk.simtopk_fast_any_k``."""
    what = "simtopk_combined_fast_any_k"
    p = _inputs(features, positions, k, ptr, batch, precision, col_splits, what)
    _need_gpu(features, what)
    if positions.device != features.device:
        raise ValueError(f"{what}: features and positions must share a device")
    dev = features.device
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    n, d = F.shape
    idx = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
    stats, info = _lib.SimtopkStats(), _lib.FastAnykInfo()
    if n > 0:
        one = ptr is None and batch is None
        opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        rc = _lib.lib().mmf_simtopk_combined_fast_anyk(ops._p(F), ops._p(P), n, d, P.shape[1], float(lambda_h), float(lambda_g), int(k),
                                                       int(bool(exclude_self)), ops._hp(None if one else p), 0 if one else p.numel() - 1,
                                                       ops._p(idx), ops._p(val), ctypes.byref(opts), ctypes.byref(stats), dev.index or 0,
                                                       ops._stream(dev), ctypes.byref(info))
        _lib.check(rc, what)
    out = (idx, val)
    if return_stats:
        out += (stats.as_dict(),)
    if return_info:
        out += (info.as_dict(),)
    return out


# Where "auto" takes the multi-pass 16-bit call (f16 operands).  The rule is the project's three-spreads rule over whole-call times
# (profiles/simtopk_combined_fast_anyk_timing.txt, written by scripts/simtopk_combined_fast_anyk_timing.py): a shape class enters
# this table only where that file shows the new call ahead of ``combined_topk_anyk.simtopk_combined_any_k`` by more than three times
# the exact arm's spread at EVERY measured size of the class.  Measured ahead (MI355X, dp = 2, pixel positions, self excluded; A / B,
# B - A in spreads of B): one graph at d = 512 with N = 16384 / 65536 / 262144 — k = 32: 0.57 / 0.53 / 0.50 (66 / 251 / 2989), k = 64:
# 0.71 / 0.60 / 0.53 (40 / 126 / 487); one graph of 65536 rows at d = 1536 — 0.45 (247) and 0.51 (207); 16 segments of 16384 rows,
# k = 32 — 0.79 (33) at d = 512, 0.61 (148) at d = 1536; 64 segments of 4096 rows at d = 1536, k = 32 — 0.88 (17).  Between the two
# measured dims the scan's share only grows, as in the one-pass entries' rule.  Measured BEHIND: 64 x 4096 at
# d = 512 (1.10) and 2048 slides of 128 rows (2.22) — the exact table-driven scan of a small segment costs little, two 16-bit passes
# and their bookkeeping do not shrink with it.  bf16 operands time like f16 within a spread or two and are not ahead of it, so
# "auto" never takes them.  Not measured, so not taken: fewer than 16384 rows, d < 512 or d > 1536, k > 64 (batches: k > 32),
# batches of fewer than 262144 rows, other segment sizes, ragged batches with unserved segments.
# Entries: (d_lo, d_hi, k_lo, k_hi, n_lo, rows_per_segment_lo, segments_hi) — d in [d_lo, d_hi], k in [k_lo, k_hi], n >= n_lo rows in
# at most segments_hi segments (one graph: one segment) that average at least rows_per_segment_lo rows; the multi-pass condition is
# checked beside the table.
_AUTO_SHAPES: tuple = ((512, 1536, 20, 64, 16384, 16384, 1),
                       (512, 1536, 20, 32, 262144, 16384, 16),
                       (1536, 1536, 20, 32, 262144, 4096, 64))


def _auto_takes(n: int, d: int, k: int, n_segments: int) -> bool:
    segs = max(int(n_segments), 1)
    per = n / segs
    return any(dl <= d <= dh and kl <= k <= kh and n >= nl and per >= pl and segs <= sh for dl, dh, kl, kh, nl, pl, sh in _AUTO_SHAPES)


def anyk_route(n: int, d: int, k: int, exclude_self: bool, n_segments: int, precision: str = "auto") -> str:
    """What ``simtopk_combined_any_k`` of this module calls: "combined_topk16_anyk.simtopk_combined_fast_any_k" or
    "combined_topk_anyk.simtopk_combined_any_k".  Host only."""
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"anyk_route: unknown precision {precision!r}")
    if int(k) < 1:
        raise ValueError(f"anyk_route: k must be >= 1 (got {k})")
    fast, exact = "combined_topk16_anyk.simtopk_combined_fast_any_k", "combined_topk_anyk.simtopk_combined_any_k"
    if precision in _FAST:
        return fast
    several = int(k) + (1 if exclude_self else 0) > ONE_PASS_MAX and 1 <= int(d) <= 4096
    if precision == "auto" and several and _auto_takes(int(n), int(d), int(k), n_segments):
        return fast
    return exact


def simtopk_combined_any_k(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *,
                           ptr=None, batch=None, exclude_self: bool = True, precision: str = "auto", col_splits: int = 0,
                           return_stats: bool = False, profile: bool = False):
    """The router: (idx, val[, stats]), the same bits on every route.  "fast" / "fast_bf16": ``simtopk_combined_fast_any_k``.
    "auto": that call (f16 operands) on the shape classes of ``_AUTO_SHAPES`` — those profiles/simtopk_combined_fast_anyk_timing.txt
    shows ahead of the exact passes by the three-spreads rule at every measured size: one graph of 16384 rows or more at
    512 <= D <= 1536 with k <= 64, and batches of 262144 rows or more in at most 16 segments of 16384 rows or more (at D = 1536: at
    most 64 segments of 4096 or more) with k <= 32 — and
    ``combined_topk_anyk.simtopk_combined_any_k`` everywhere else.  "exact": the latter, unchanged.  CPU tensors are computed on
    the current GPU and the result moved back."""
    what = "combined_topk16_anyk.simtopk_combined_any_k"
    p = _inputs(features, positions, k, ptr, batch, precision, col_splits, what)
    one = ptr is None and batch is None
    route = anyk_route(features.shape[0], features.shape[1], k, exclude_self, p.numel() - 1, precision)
    kw = dict(ptr=None if one else p, exclude_self=exclude_self, col_splits=col_splits, return_stats=return_stats, profile=profile)
    if route == "combined_topk_anyk.simtopk_combined_any_k":
        return combined_topk_anyk.simtopk_combined_any_k(features, positions, lambda_h, lambda_g, k, **kw)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    out = simtopk_combined_fast_any_k(F, P, lambda_h, lambda_g, k, precision="fast" if precision == "auto" else precision, **kw)
    return (out[0].to(home), out[1].to(home)) + tuple(out[2:])


def build_topk_weighted_hypergraph_fast_any_k(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                              k: int = 5, device: Optional[torch.device] = None, *, ptr=None, batch=None,
                                              precision: str = "auto") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``combined_topk_anyk.build_topk_weighted_hypergraph_any_k`` on this module's router, in its layout: (edge_index [2, E] int64
    global row ids, edge_weights [E] f32, edge_ptr [S + 1] int64) on `device` (None: the features' device).  Edge (i, idx[i, r]) with
    weight val[i, r]; rows ascend and r ascends within a row; a segment of n_s rows gives n_s * min(k, n_s - 1) edges."""
    what = "build_topk_weighted_hypergraph_fast_any_k"
    p = _inputs(features, positions, k, ptr, batch, precision, 0, what)
    out_dev = result_device_like_kernel(features, device)
    dev = compute_device(features, positions) if out_dev.type != "cuda" else out_dev
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    one = ptr is None and batch is None
    idx, val = simtopk_combined_any_k(F, P, lambda_h, lambda_g, k, ptr=None if one else p, precision=precision)
    keep = idx >= 0
    rows = torch.arange(idx.shape[0], dtype=torch.int64, device=dev).unsqueeze(1).expand_as(idx)
    edge_index = torch.stack([rows[keep], idx[keep]])
    sizes = p[1:] - p[:-1]
    edge_ptr = torch.zeros(p.numel(), dtype=torch.int64)
    edge_ptr[1:] = torch.cumsum(sizes * torch.clamp(sizes - 1, min=0, max=int(k)), 0)
    return edge_index.to(out_dev).contiguous(), val[keep].to(out_dev), edge_ptr.to(out_dev)


def build_topk_hypergraph_data_fast_any_k(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                          k: int = 5, use_pooling: bool = True, device: Optional[torch.device] = None, *, ptr=None,
                                          batch=None, precision: str = "auto") -> dict:
    """``combined_topk_anyk.build_topk_hypergraph_data_any_k`` on this module's router: x, edge_index (global ids), edge_attr, pos,
    batch, ptr and (with use_pooling) pooled_feature, all on `device` (None: the features' device)."""
    what = "build_topk_hypergraph_data_fast_any_k"
    p = _inputs(features, positions, k, ptr, batch, precision, 0, what)
    if device is None:
        device = features.device
    features = features.to(device)
    positions = positions.to(device)
    one = ptr is None and batch is None
    edge_index, edge_weights, _ = build_topk_weighted_hypergraph_fast_any_k(features, positions, lambda_h, lambda_g, k, device,
                                                                            ptr=None if one else p, precision=precision)
    result = {"x": features, "edge_index": edge_index, "edge_attr": edge_weights, "pos": positions,
              "batch": ragged.segment_ids(p).to(device), "ptr": p.to(device)}
    if use_pooling:
        result["pooled_feature"] = segment_mean_pool(features, p)
    return result
