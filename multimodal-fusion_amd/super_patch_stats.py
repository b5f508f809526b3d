"""The statistics aggregate_wsi_super_patches takes from a slide's similarity matrix K = K_h * K_g, for a slide whose K does not
fit (include/mmf_hg_stream.h): the mean off-diagonal similarity inside every cluster and mean, std, min, max and
lower median of K, from row panels of K that are recomputed and never stored.  Bit for bit what ops.segment_offdiag_mean and
mmf_array_stats return on ops.sim_dense_combined(F, P), for every panel height.

    seg = ops.segment_sort(labels, C)
    intra, k_stats = super_patch_stats_streamed(F, P, seg.order, seg.offsets, C, lambda_h, lambda_g)
    streamed_workspace_bytes(n, d, dp, C)          # what that call keeps on the device: no term in n^2 but the median's 5 %

Every argument error is raised on the host before the device is touched.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, ops


def _check_shape(n: int, d: int, dp: int, what: str) -> None:
    if n < 2:
        raise ValueError(f"{what}: need at least 2 rows (got {n})")
    if d < 1 or dp < 1:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] need D >= 1 and dp >= 1 (got {d} and {dp})")


def streamed_workspace_bytes(n: int, d: int, dp: int, n_clusters: int, panel_rows: int = 0) -> int:
    """Bytes of device workspace super_patch_stats_streamed asks for with these sizes in the current environment
    (mmf_super_patch_stats_streamed_bytes): the panel, the f32 image of the features, the median's scratch, the carried lane sums
    and O(n) row tables.  Pure host arithmetic."""
    what = "streamed_workspace_bytes"
    n, d, dp = int(n), int(d), int(dp)
    _check_shape(n, d, dp, what)
    if int(panel_rows) < 0:
        raise ValueError(f"{what}: panel_rows must be >= 0 (got {panel_rows})")
    got = int(_lib.lib().mmf_super_patch_stats_streamed_bytes(n, d, dp, int(n_clusters), int(panel_rows)))
    if got < 0:
        _lib.check(got, "mmf_super_patch_stats_streamed_bytes")
    return got


def super_patch_stats_streamed(F: torch.Tensor, P: torch.Tensor, order: Optional[torch.Tensor], offsets: Optional[torch.Tensor],
                               n_clusters: int, lambda_h: float = 1.0, lambda_g: float = 1.0, *,
                               panel_rows: int = 0) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """(intra_mean f64 [n_clusters], k_stats f64 [5]) on the device (mmf_super_patch_stats_streamed).  order int64 [N] / offsets
    int64 [n_clusters + 1]: the members of every cluster as ops.segment_sort leaves them; order None: no cluster means (None is
    returned for them).  intra_mean is NaN for a cluster of fewer than two rows; k_stats is mean, unbiased std, min, max, lower
    median of K.  panel_rows: rows of K per panel (0: about 1 GiB).  The call may wait for the stream once (the median's verdict)."""
    what = "super_patch_stats_streamed"
    if F.dim() != 2 or P.dim() != 2 or P.shape[0] != F.shape[0]:
        raise ValueError(f"{what}: features [N, D] and positions [N, dp] must share N")
    n, C = F.shape[0], int(n_clusters)
    _check_shape(n, F.shape[1], P.shape[1], what)
    if int(panel_rows) < 0:
        raise ValueError(f"{what}: panel_rows must be >= 0 (got {panel_rows})")
    if order is not None:
        if C < 1:
            raise ValueError(f"{what}: bad n_clusters {C}")
        if offsets is None or order.numel() != n or offsets.numel() != C + 1:
            raise ValueError(f"{what}: order must hold {n} rows and offsets {C + 1} entries "
                             f"(got {order.numel()} and {None if offsets is None else offsets.numel()})")
    dev = F.device
    if P.device != dev or (order is not None and (order.device != dev or offsets.device != dev)):
        raise ValueError(f"{what}: all tensors must share a device")
    ops._need_gpu(F, what)
    F, P = F.float().contiguous(), P.float().contiguous()
    intra = None
    if order is not None:
        order, offsets = order.to(torch.int64).contiguous(), offsets.to(torch.int64).contiguous()
        intra = torch.empty((C,), dtype=torch.float64, device=dev)
    k_stats = torch.empty((5,), dtype=torch.float64, device=dev)
    ops._call("mmf_super_patch_stats_streamed", dev, ops._p(F), ops._p(P), n, F.shape[1], P.shape[1], float(lambda_h), float(lambda_g),
              ops._p(order), ops._p(offsets if order is not None else None), C, int(panel_rows), ops._p(intra), ops._p(k_stats))
    return intra, k_stats
