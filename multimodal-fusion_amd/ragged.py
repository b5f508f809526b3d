"""Host-side description of a ragged batch, shared by ops.py and every cohort module: offsets from ptr / batch, the two-sided
description, block offsets, budget groups and the per-segment size checks of scikit-learn.  Pure host code that imports nothing
from the package.  Every message reads ``{what}: {unit} {index}: ...`` and names the first bad segment; `unit` is the caller's word
for a segment ("segment", "slide")."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch


def _cumulative(sizes: torch.Tensor) -> torch.Tensor:
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)]).contiguous()


def offsets(ptr, batch, rows: Optional[int], *, side: str = "", what: str, unit: str = "segment", min_rows: int = 0,
            allow_no_segments: bool = False) -> torch.Tensor:
    """Host int64 offsets [S + 1] from exactly one of ptr (offsets) / batch (sorted segment id per row, PyG's convention), every
    segment with at least min_rows rows.  rows None: the row count is what ptr / batch say.  `side` prefixes the argument names
    in the messages ("wsi_").  allow_no_segments accepts ptr = [0] and an empty batch: S = 0.  A ptr or batch on the device costs
    one device -> host copy."""
    if (ptr is None) == (batch is None):
        raise ValueError(f"{what}: give exactly one of {side}ptr / {side}batch")
    if ptr is not None:
        p = torch.as_tensor(ptr).detach().to("cpu", torch.int64).reshape(-1).contiguous()
        if p.numel() < (1 if allow_no_segments else 2):
            raise ValueError(f"{what}: {unit} 0: {side}ptr describes no {unit} (it needs S + 1 >= 2 offsets)")
        if int(p[0]) != 0:
            raise ValueError(f"{what}: {unit} 0: {side}ptr must start at 0 (got {int(p[0])})")
        sizes = p[1:] - p[:-1]
        bad = torch.nonzero(sizes < min_rows).reshape(-1)
        if bad.numel():
            s = int(bad[0])
            if int(sizes[s]) < 0:
                raise ValueError(f"{what}: {unit} {s}: {side}ptr decreases ({int(p[s])} -> {int(p[s + 1])})")
            raise ValueError(f"{what}: {unit} {s} has {int(sizes[s])} rows in {side}ptr, need at least {min_rows}")
        if rows is not None and int(p[-1]) != rows:
            raise ValueError(f"{what}: {unit} {max(p.numel() - 2, 0)}: {side}ptr must end at {rows} (got {int(p[-1])}): "
                             f"a {side}ptr must start at 0 and end at {rows}, the number of rows")
        return p
    b = torch.as_tensor(batch)
    if b.dim() != 1 or (rows is not None and b.numel() != rows):
        raise ValueError(f"{what}: {unit} 0: {side}batch must hold one {unit} id per row ({rows})")
    b = b.detach().to("cpu", torch.int64)           # the one device -> host copy of a batch vector
    if b.numel() == 0:
        if allow_no_segments:
            return torch.zeros(1, dtype=torch.int64)
        raise ValueError(f"{what}: {unit} 0: {side}batch describes no {unit} (it is empty)")
    if int(b[0]) < 0:
        raise ValueError(f"{what}: {unit} {int(b[0])}: {side}batch must be non-negative")
    down = torch.nonzero(b[1:] < b[:-1]).reshape(-1)
    if down.numel():
        r = int(down[0]) + 1
        raise ValueError(f"{what}: {unit} {int(b[r])}: {side}batch must be sorted (row {r} follows {unit} {int(b[r - 1])})")
    counts = torch.bincount(b)
    bad = torch.nonzero(counts < min_rows).reshape(-1)
    if bad.numel():
        s = int(bad[0])
        raise ValueError(f"{what}: {unit} {s} has {int(counts[s])} rows in {side}batch, need at least {min_rows}")
    return _cumulative(counts)


def two_sided(n_x: Optional[int], n_y: Optional[int], x_ptr, x_batch, y_ptr, y_batch, *, xs: str, ys: str, what: str,
              unit: str = "segment", min_rows: Tuple[int, int] = (0, 0),
              allow_no_segments: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x offsets, y offsets) of a two-sided description: segment s pairs x[xp[s]:xp[s+1]] with y[yp[s]:yp[s+1]], so both sides
    must describe the same number of segments (a batch vector ends at its last id: trailing segments without rows need ptr).
    xs / ys: the sides' argument prefixes ("wsi_", "tma_"); min_rows per side."""
    xp = offsets(x_ptr, x_batch, n_x, side=xs, what=what, unit=unit, min_rows=min_rows[0], allow_no_segments=allow_no_segments)
    yp = offsets(y_ptr, y_batch, n_y, side=ys, what=what, unit=unit, min_rows=min_rows[1], allow_no_segments=allow_no_segments)
    if xp.numel() != yp.numel():
        sx, sy = xp.numel() - 1, yp.numel() - 1
        raise ValueError(f"{what}: {unit} {min(sx, sy)}: {xs.rstrip('_') or 'x'} describes {sx} {unit}s, "
                         f"{ys.rstrip('_') or 'y'} {sy}")
    return xp, yp


def block_offsets(xp: torch.Tensor, yp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Host int64 [S + 1]: where block s ([n_s, m_s] row-major; [n_s, n_s] without yp) starts in one flat buffer."""
    n = xp[1:] - xp[:-1]
    return _cumulative(n * (n if yp is None else yp[1:] - yp[:-1]))


def segment_ids(p: torch.Tensor) -> torch.Tensor:
    """Host int64 [rows]: the segment of every row (the batch vector that has the offsets p)."""
    return torch.repeat_interleave(torch.arange(p.numel() - 1, dtype=torch.int64), p[1:] - p[:-1])


def budget_groups(sizes: Sequence[int], budget: int) -> List[Tuple[int, int, bool]]:
    """Consecutive segments [a, b) whose blocks (n_s^2 f32 each) fit `budget` bytes together; (s, s + 1, True) for a segment
    whose block alone is larger."""
    out, a, acc = [], 0, 0
    for s, n_s in enumerate(sizes):
        b = n_s * n_s * 4
        if b > budget:
            if s > a:
                out.append((a, s, False))
            out.append((s, s + 1, True))
            a, acc = s + 1, 0
            continue
        if acc + b > budget and s > a:
            out.append((a, s, False))
            a, acc = s, 0
        acc += b
    if len(sizes) > a:
        out.append((a, len(sizes), False))
    return out


def _kmeans_size(s: int, n_s: int, n_clusters: int, what: str, unit: str) -> None:
    if not (1 <= n_clusters <= n_s):
        raise ValueError(f"{what}: {unit} {s}: n_samples={n_s} should be >= n_clusters={n_clusters}.")


def check_kmeans_sizes(sizes: Sequence[int], n_clusters: int, what: str, unit: str = "segment") -> None:
    """What scikit-learn's KMeans raises for the first segment with fewer rows than clusters (or for n_clusters < 1)."""
    for s, n_s in enumerate(sizes):
        _kmeans_size(s, n_s, n_clusters, what, unit)


def check_knn_sizes(sizes: Sequence[int], k: int, what: str, unit: str = "segment", n_clusters: Optional[int] = None) -> None:
    """What scikit-learn's kneighbors raises for the first segment with fewer than k + 1 rows (k neighbours besides the row
    itself).  n_clusters given: check_kmeans_sizes' test as well, segment by segment and after the neighbours, which is the order
    the plain mirror fails in on each slide."""
    for s, n_s in enumerate(sizes):
        if k + 1 > n_s:
            raise ValueError(f"{what}: {unit} {s}: Expected n_neighbors <= n_samples_fit, but n_neighbors = {k + 1}, "
                             f"n_samples_fit = {n_s}, n_samples = {n_s}")
        if n_clusters is not None:
            _kmeans_size(s, n_s, n_clusters, what, unit)
