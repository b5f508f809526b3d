"""What the wide 16-bit scan covers (include/mmf_hg_wide.h): ``ops.simtopk(..., precision="fast" | "fast_bf16")``
for feature dims above 1024, where the register-resident scan stops.  Host-only queries: no GPU is touched.

``simtopk_segmented`` is the segmented form (include/mmf_hg_wide_seg.h): the k-NN of every segment of a ragged
batch in one call, with the wide scan behind it where it applies.

Flagged rows (``fallback_rows`` of the call's stats).  A row's candidate lists hold ``list_capacity`` entries each; what a crowded
list of ``ops.simtopk``'s wide scan cannot hold goes to the row's ``OVERFLOW_SLOTS`` overflow slots and is re-ranked exactly with
the lists.  A row is flagged, and answered by the exact f32 rescan, only when a column of its error-margin
band found neither a list nor a free overflow slot: near-duplicate clusters of up to about ``OVERFLOW_SLOTS`` rows stay on the
fast path.  ``MMF_WIDE_SINK=0`` in the environment (read per call) switches the overflow lists off: every row whose band
exceeds a list is then flagged, as in the segmented form, which has no overflow lists.  The results are the same bits either way.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ragged
from .ops import _feat, _hp, _need_gpu, _simtopk_entry


OVERFLOW_SLOTS = 192   # overflow slots per row of the wide scan (kSpillCap, csrc/mmf_api.hip)


def wide_scan_supported(d: int, k: int, exclude_self: bool = True) -> bool:
    """True when ``ops.simtopk`` serves ``precision="fast"`` / ``"fast_bf16"`` at feature dim ``d`` through the wide scan:
    1024 < d <= 4096 and k + self <= 20 (d <= 1024 is ``ops.fast_scan_supported``'s)."""
    return bool(_lib.lib().mmf_wide_scan_supported(int(d), int(k), int(bool(exclude_self))))


def list_capacity(k: int, exclude_self: bool = True) -> int:
    """Entries of one candidate list of the wide scan (0: k + self beyond 20).  A row with at most this many columns inside
    its error-margin band is never sent to the exact rescan."""
    return int(_lib.lib().mmf_wide_scan_list_capacity(int(k), int(bool(exclude_self))))


def simtopk_segmented(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, ptr=None, batch=None, y_ptr=None, y_batch=None,
                      metric="cosine", lam: float = 1.0, k: int = 5, exclude_self: Optional[bool] = None,
                      precision: str = "auto", col_splits: int = 0, return_stats: bool = False, profile: bool = False):
    """``ops.simtopk_segmented`` with the wide scan behind it (mmf_simtopk_segmented_wide): the same arguments, the same
    (idx, val[, stats]) and the same bits — those of one ``ops.simtopk`` per segment.  For 1024 < d <= 4096 and k + self <= 20
    (``wide_scan_supported``) the candidates of every segment come from ONE launch of the wide 16-bit scan: ``precision="fast"``
    and ``"fast_bf16"`` are accepted and ``"auto"`` takes ``"fast"``, where ``ops.simtopk_segmented`` refuses the former and sends
    every segment through the exact pass.  ``col_splits``: 0 (automatic) or a power of two, the column ranges every segment is
    scanned in (at most one per 128 columns of the segment); outside the wide scan's shapes it must stay 0, and the call is
    ``ops.simtopk_segmented``'s."""
    what = "wide_scan.simtopk_segmented"
    X = _feat(X, f"{what} X")
    if Y is not None:
        Y = _feat(Y, f"{what} Y")
        if Y.device != X.device or Y.dtype != X.dtype or Y.shape[1] != X.shape[1]:
            raise ValueError(f"{what}: X and Y must share device, dtype and feature dim")
    if int(k) < 1:
        raise ValueError(f"{what}: k must be >= 1 (got {k})")
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"{what}: unknown precision {precision!r}")
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
    opts = _lib.SimtopkOpts(_lib.PRECISIONS[precision], int(profile), col_splits, _lib.QUERY_ORDERS["off"], None)
    return _simtopk_entry("mmf_simtopk_segmented_wide", X, Y, metric, lam, k, exclude_self, (_hp(xp), _hp(yp), xp.numel() - 1), opts,
                          return_stats)
