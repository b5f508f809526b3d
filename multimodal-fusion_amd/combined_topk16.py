"""The k best columns per row of the combined similarity K = K_h * K_g of ONE graph from the 16-bit matrix cores
(mmf_simtopk_combined_fast, include/mmf_hg_topk16.h): the result of ``combined_topk.simtopk_combined``, bit for
bit, from an f16 / bf16 candidate scan of the combined key, an exact re-rank, and the exact scan for the rows the 16-bit scan
could not certify.  k + self <= 20, feature dim <= 4096, position dim <= 8, f32 inputs; ragged batches stay on
``combined_topk.simtopk_combined``.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib, ops
from .build_hypergraph._common import compute_device, result_device_like_kernel, to_gpu


def _inputs(features: torch.Tensor, positions: torch.Tensor, k: int, precision: str, what: str) -> None:
    """Checked before any device work or library call: shapes, k and the precision's name.  The entry refuses what it does not
    support (k + self > 20, D > 4096, dp > 8) with its own words."""
    if features.dim() != 2 or positions.dim() != 2 or positions.shape[0] != features.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")


def simtopk_combined_fast(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0, k: int = 5, *,
                          exclude_self: bool = True, precision: str = "auto", col_splits: int = 0, return_stats: bool = False,
                          profile: bool = False):
    """(idx [N, k] int64, val [N, k] f32[, stats dict]) of one graph: ``combined_topk.simtopk_combined``'s result, the same bits.
    ``precision``: "fast" scans f16 images of the features, "fast_bf16" bf16 images, "exact" runs the exact f32 scan, "auto"
    takes the f16 scan in the measured range (512 <= D <= 1536, k + self <= 11) and the exact scan elsewhere; stats
    ["precision_used"] says which ran and stats["fallback_rows"] how many rows the 16-bit scan handed to the exact pass.
    ``col_splits``: 0 (automatic) or the column ranges every row block is scanned in (rounded up to a power of two).  CPU
    tensors are computed on the current GPU and the result moved back."""
    what = "simtopk_combined_fast"
    _inputs(features, positions, k, precision, what)
    home = features.device
    dev = compute_device(features, positions)
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    n, d = F.shape
    idx = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
    val = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    if n > 0:
        opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], int(profile), int(col_splits), _lib.QUERY_ORDERS["off"], None)
        ops._call("mmf_simtopk_combined_fast", dev, ops._p(F), ops._p(P), n, d, P.shape[1], float(lambda_h), float(lambda_g), int(k),
                  int(bool(exclude_self)), None, 0, ops._p(idx), ops._p(val), ctypes.byref(opts), ctypes.byref(stats))
    idx, val = idx.to(home), val.to(home)
    return (idx, val, stats.as_dict()) if return_stats else (idx, val)


def build_topk_weighted_hypergraph_fast(features: torch.Tensor, positions: torch.Tensor, lambda_h: float = 1.0, lambda_g: float = 1.0,
                                        k: int = 5, device: Optional[torch.device] = None, *,
                                        precision: str = "auto") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The directed top-k edges of one graph in ``combined_topk.build_topk_weighted_hypergraph``'s layout: (edge_index [2, E]
    int64, edge_weights [E] f32, edge_ptr = [0, E]) on `device` (None: the features' device).  Edge (i, idx[i, r]) with weight
    val[i, r]; rows ascend and r ascends within a row; N rows give N * min(k, N - 1) edges."""
    what = "build_topk_weighted_hypergraph_fast"
    _inputs(features, positions, k, precision, what)
    out_dev = result_device_like_kernel(features, device)
    dev = compute_device(features, positions) if out_dev.type != "cuda" else out_dev
    F, P = to_gpu(features, dev), to_gpu(positions, dev)
    idx, val = simtopk_combined_fast(F, P, lambda_h, lambda_g, k, precision=precision)
    keep = idx >= 0
    rows = torch.arange(idx.shape[0], dtype=torch.int64, device=dev).unsqueeze(1).expand_as(idx)
    edge_index = torch.stack([rows[keep], idx[keep]])
    edge_ptr = torch.tensor([0, int(edge_index.shape[1])], dtype=torch.int64)
    return edge_index.to(out_dev).contiguous(), val[keep].to(out_dev), edge_ptr.to(out_dev)
