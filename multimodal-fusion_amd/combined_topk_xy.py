"""The k best candidates per query of the combined similarity K = K_h * K_g for TWO node sets (mmf_simtopk_combined_xy,
include/ext/mmf_hg_topk_xy.h): what ``combined_topk.simtopk_combined`` / ``combined_topk16.simtopk_combined_fast``
compute for one graph against itself, with queries and candidates apart and an id offset on each side — new patches against an
existing slide, two registered sections in one coordinate frame, or rows [lo, hi) of one graph against all of it
(``simtopk_combined_rows``; ``distributed.sharded_simtopk_combined`` shards a graph over ranks with it).  The nq x nc matrix is
never formed.  "exact": any feature dim, k + self <= 44; "fast" / "fast_bf16": k + self <= 20, feature dim <= 4096; position dim
<= 8, f32 inputs.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ops
from .build_hypergraph._common import compute_device, to_gpu


def _inputs(qf: torch.Tensor, qp: torch.Tensor, cf: torch.Tensor, cp: torch.Tensor, k: int, precision: str, col_splits: int, row_offset: int,
            col_offset: int, what: str) -> None:
    """Checked before any device work or library call: shapes, k, the precision's name, col_splits and the offsets.  The entry
    refuses what it does not support (k + self, D, dp beyond its limits) with its own words."""
    if qf.dim() != 2 or qp.dim() != 2 or qp.shape[0] != qf.shape[0]:
        raise ValueError(f"{what}: query features [Nq, D] and positions [Nq, dp] must share Nq")
    if cf.dim() != 2 or cp.dim() != 2 or cp.shape[0] != cf.shape[0]:
        raise ValueError(f"{what}: candidate features [Nc, D] and positions [Nc, dp] must share Nc")
    if cf.shape[1] != qf.shape[1] or cp.shape[1] != qp.shape[1]:
        raise ValueError(f"{what}: queries and candidates must share D and dp (got D {qf.shape[1]} / {cf.shape[1]}, dp {qp.shape[1]} / {cp.shape[1]})")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
    if int(col_splits) < 0:
        raise ValueError(f"{what}: col_splits must be >= 0 (got {col_splits})")
    if int(row_offset) < 0 or int(col_offset) < 0:
        raise ValueError(f"{what}: row_offset and col_offset must be >= 0 (got {row_offset}, {col_offset})")


def _run(what, Fq, Pq, Fc, Pc, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, precision, col_splits, profile):
    """The entry on device tensors (f32, contiguous rows): (idx, val, stats)."""
    dev = Fq.device
    nq, d = Fq.shape
    idx = torch.empty((nq, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((nq, int(k)), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    if nq > 0:
        opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        ops._call("mmf_simtopk_combined_xy", dev, ops._p(Fq), ops._p(Pq), nq, ops._p(Fc), ops._p(Pc), Fc.shape[0], d, Pq.shape[1],
                  float(lambda_h), float(lambda_g), int(k), int(bool(exclude_self)), int(row_offset), int(col_offset), ops._p(idx), ops._p(val),
                  ctypes.byref(opts), ctypes.byref(stats), what=what)
    return idx, val, stats


def simtopk_combined_xy(q_features: torch.Tensor, q_positions: torch.Tensor, c_features: torch.Tensor, c_positions: torch.Tensor,
                        lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *, exclude_self: bool = False, row_offset: int = 0,
                        col_offset: int = 0, precision: str = "auto", col_splits: int = 0, return_stats: bool = False, profile: bool = False):
    """(idx [Nq, k] int64, val [Nq, k] f32[, stats dict]): per query the k best candidates by key = eh + eg (descending, then id
    ascending), reported as ``col_offset + candidate row``, with val = K_h * K_g — ``combined_topk.simtopk_combined``'s keys and
    values, the same bits.  ``exclude_self`` drops the pair whose ids agree (``row_offset + i == col_offset + j``); a query with
    fewer than k admissible candidates gets them first, then -1 / -inf.  ``precision``: "exact" runs the exact f32 scan, "fast" /
    "fast_bf16" an f16 / bf16 candidate scan with an exact re-rank (stats["fallback_rows"]: queries it handed to the exact scan),
    "auto" the f16 scan in the measured range (512 <= D <= 1536, k + self <= 11) and the exact scan elsewhere;
    stats["precision_used"] says which ran.  Queries that are a row view of the candidates (``c[lo:hi]``, features and positions alike) are recognised by the
    library as a row slice: one operand image, and the bits of the self entries for those rows.  CPU tensors are computed on the
    current GPU and the result moved back."""
    what = "simtopk_combined_xy"
    _inputs(q_features, q_positions, c_features, c_positions, k, precision, col_splits, row_offset, col_offset, what)
    home = q_features.device
    dev = compute_device(q_features, q_positions, c_features, c_positions)
    Fq, Pq, Fc, Pc = (to_gpu(t, dev) for t in (q_features, q_positions, c_features, c_positions))
    idx, val, stats = _run(what, Fq, Pq, Fc, Pc, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, precision, col_splits, profile)
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def simtopk_combined_rows(features: torch.Tensor, positions: torch.Tensor, lo: int, hi: int, lambda_h: float = 1.0, lambda_g: float = 1.0,
                          k: int = 5, *, exclude_self: bool = True, col_offset: int = 0, precision: str = "auto", col_splits: int = 0,
                          return_stats: bool = False, profile: bool = False):
    """Rows [lo, hi) of ``combined_topk.simtopk_combined(features, positions, ...)`` (``precision="exact"``) or of
    ``combined_topk16.simtopk_combined_fast`` ("fast" / "fast_bf16"), bit for bit, without computing the other rows: (idx
    [hi - lo, k], val [hi - lo, k][, stats dict]), ids shifted by ``col_offset``.  The library is handed views of the two arrays,
    so it sees a row slice: one operand image and one set of chains for all N rows, whatever the panel."""
    what = "simtopk_combined_rows"
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= features.shape[0]:
        raise ValueError(f"{what}: rows [{lo}, {hi}) are no range of the {features.shape[0]} rows")
    _inputs(features[lo:hi], positions[lo:hi], features, positions, k, precision, col_splits, 0, col_offset, what)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    idx, val, stats = _run(what, F[lo:hi], P[lo:hi], F, P, lambda_h, lambda_g, k, exclude_self, int(col_offset) + lo, col_offset, precision,
                           col_splits, profile)
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)
