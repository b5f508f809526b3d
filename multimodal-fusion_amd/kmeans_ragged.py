"""Ragged-width segmented KMeans (include/ext/mmf_hg_kmeans_ragged.h): scikit-learn's fit for every block of a
flat buffer in ONE call, where block s is ``rows[s] x widths[s]`` — each block with a feature width of its own.

This is the shape of the cohort's grouping step: slide s clusters the n_s rows of its [n_s, m_s] WSI x TMA similarity block, and
m_s (the slide's TMA patch count) differs from slide to slide, while ``kmeans_fit_predict_segmented`` takes one feature dimension.
Every block gets, bit for bit, what ``kmeans.kmeans_fit_predict`` returns on it: the means, the variances, scikit-learn's
tolerance ``tol * mean(var)`` and the centring are taken over the block's own columns; only the internal mean-centred copy is padded
(with zeros, behind the centring) to the width of the widest block of a lockstep group, where a zero column adds an exact 0.0.

    labels, centres, inertia = kmeans_fit_predict_ragged(S_flat, k, rows=n_sizes, widths=m_sizes)     # blocks back to back
    bounds, ds = ragged_groups(n_sizes, m_sizes, k)                                                   # host only: the lockstep groups
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops, ragged
from .kmeans import segment_streams


def _i64(v, what: str, name: str, n: Optional[int] = None) -> np.ndarray:
    """A host table column as the C entries read it: C-contiguous int64 [n_seg]."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    a = np.ascontiguousarray(v, dtype=np.int64)
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise ValueError(f"{what}: {name} must be a 1-D sequence" + ("" if n is None else f" of {n} entries (one per segment)"))
    return a


def _table(what: str, n_values: int, rows, widths, xoff, n_clusters: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(xoff, rows, widths) checked on the host: the first bad segment raises ValueError.  xoff None: the blocks back to back."""
    r = _i64(rows, what, "rows")
    if r.shape[0] < 1:
        raise ValueError(f"{what}: at least one segment is needed")
    w = _i64(widths, what, "widths", r.shape[0])
    x = np.concatenate([[0], np.cumsum(r * w)[:-1]]).astype(np.int64) if xoff is None else _i64(xoff, what, "xoff", r.shape[0])
    k = int(n_clusters)
    for s in range(r.shape[0]):
        ragged._kmeans_size(s, int(r[s]), k, what, "segment")
        if w[s] < 1:
            raise ValueError(f"{what}: segment {s}: width {int(w[s])} must be >= 1")
        if x[s] < 0 or int(x[s]) + int(r[s]) * int(w[s]) > n_values:
            raise ValueError(f"{what}: segment {s}: block [{int(x[s])}, {int(x[s])} + {int(r[s])} x {int(w[s])}) outside the "
                             f"{n_values} values of V")
    return x, r, w


def _hptr(a: Optional[np.ndarray]) -> Optional[ctypes.c_void_p]:
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def ragged_groups(rows, widths, n_clusters: int, n_init: int = 10) -> Tuple[List[int], List[int]]:
    """The lockstep groups one ragged call makes of these segments, in the order given (mmf_kmeans_ragged_groups; no GPU):
    (bounds: group g is the segments bounds[g] .. bounds[g+1] - 1; ds: per segment, the internal width of its group).  A group
    holds at most 16384 / (n_init * n_clusters) segments, and closes before a segment that would make sum rows * ds exceed twice
    the sum of rows * (own width rounded up to 32)."""
    what = "ragged_groups"
    k = int(n_clusters)
    r = _i64(rows, what, "rows")
    w = _i64(widths, what, "widths", r.shape[0])
    import math
    trials = 2 + int(math.log(k)) if k >= 1 else 1
    bounds = np.zeros(r.shape[0] + 1, dtype=np.int64)
    ds = np.zeros(max(r.shape[0], 1), dtype=np.int64)
    L = _lib.lib()
    g = L.mmf_kmeans_ragged_groups(_hptr(r), _hptr(w), r.shape[0], k, int(n_init), trials, _hptr(bounds), _hptr(ds))
    if g < 0:
        _lib.check(int(g), what)
    return bounds[:g + 1].tolist(), ds[:r.shape[0]].tolist()


def kmeans_fit_ragged(V: torch.Tensor, xoff, rows, widths, n_clusters: int, first_centres, uniforms, *, max_iter: int = 300,
                      tol: float = 1e-4, return_seeds: bool = False):
    """The thin binding of mmf_kmeans_fit_ragged.  V: flat f32 device tensor; segment s is rows[s] x widths[s], row-major, at
    element xoff[s] (host sequences; blocks need not be adjacent or in memory order).  first_centres: int64 [n_seg, n_init], rows
    local to each segment; uniforms: float64 [n_init, n_clusters - 1, trials], shared (HOST numpy arrays: kmeans.segment_streams
    draws them).  Consecutive segments run as one lockstep group (ragged_groups).  Returns (labels int64 [sum rows] in call order,
    0 .. k-1 within each segment; centres: flat f32 [k * sum widths], segment s is [k, widths[s]] at k * sum of the widths before
    it; info: one dict per segment with ops.kmeans_fit's keys[, seeds int64 [n_seg, n_init, k], rows local to the segment])."""
    what = "kmeans_fit_ragged"
    if V.dim() != 1:
        raise ValueError(f"{what}: V must be the flat 1-D buffer of the blocks, got shape {tuple(V.shape)}")
    k = int(n_clusters)
    x, r, w = _table(what, V.numel(), rows, widths, xoff, k)
    n_seg = r.shape[0]
    first, u, n_init, trials = ops._kmeans_stream(what, k, first_centres, uniforms, n_seg)
    for s in range(n_seg):
        bad = np.nonzero((first[s] < 0) | (first[s] >= r[s]))[0]
        if bad.size:
            raise ValueError(f"{what}: segment {s}: first_centres[{int(bad[0])}] outside [0, n_samples)")
    ops._need_gpu(V, what)
    V = V.detach().float().contiguous()
    labels = torch.empty(int(r.sum()), dtype=torch.int64, device=V.device)
    centres = torch.empty(k * int(w.sum()), dtype=torch.float32, device=V.device)
    seeds = torch.empty((n_seg, n_init, k), dtype=torch.int64, device=V.device) if return_seeds else None
    info = np.zeros((n_seg, 7 + 2 * n_init), dtype=np.float64)
    ops._call("mmf_kmeans_fit_ragged", V.device, ops._p(V), V.numel(), _hptr(x), _hptr(r), _hptr(w), n_seg, k, n_init, trials, _hptr(first),
              _hptr(u) if k > 1 else None, int(max_iter), float(tol), ops._p(labels), ops._p(centres), ops._p(seeds), _hptr(info))
    out_info = [ops._kmeans_info(row) for row in info]
    if return_seeds:
        return labels, centres, out_info, seeds
    return labels, centres, out_info


def kmeans_fit_predict_ragged(V_flat: torch.Tensor, n_clusters: int, *, rows, widths, xoff=None, n_init: int = 10, max_iter: int = 300,
                              tol: float = 1e-4, seed: int = 42, return_info: bool = False):
    """kmeans.kmeans_fit_predict for every block of a flat buffer in one call: block s is V_flat[xoff[s] : xoff[s] + rows[s] *
    widths[s]].view(rows[s], widths[s]) (xoff None: the blocks back to back, the layout of compute_wsi_tma_similarity_segmented's
    S_flat).  Returns (labels int64 [sum rows], segment after segment in the caller's order, 0 .. k-1 within each; centres: a list
    of f32 [k, widths[s]] views; inertia f64 numpy [n_seg]), bit for bit the per-block calls.

    The random stream depends on the row counts only (kmeans.segment_streams).  The segments are handed to the library stably
    sorted by their width rounded up to 32, so that lockstep groups hold blocks of one internal width where they can; the labels
    return to the caller's order in one indexed store.  Bad segments raise ValueError on the host, before the device is touched
    (and before the "needs a ROCm device" RuntimeError), and name the segment."""
    what = "kmeans_fit_predict_ragged"
    if V_flat.dim() != 1:
        raise ValueError(f"{what}: V_flat must be the flat 1-D buffer of the blocks, got shape {tuple(V_flat.shape)}")
    k = int(n_clusters)
    x, r, w = _table(what, V_flat.numel(), rows, widths, xoff, k)
    ops._need_gpu(V_flat, what)
    n_seg = r.shape[0]
    first, u = segment_streams(int(seed), int(n_init), k, r.tolist())
    order = np.argsort((w + 31) // 32, kind="stable")
    labels_sorted, cen_flat, info_sorted = kmeans_fit_ragged(V_flat, x[order], r[order], w[order], k, first[order], u, max_iter=max_iter, tol=tol)
    in_order = bool((order == np.arange(n_seg)).all())
    if in_order:
        labels = labels_sorted
    else:
        labels = torch.empty_like(labels_sorted)
        labels[_scatter_index(r, order).to(labels.device)] = labels_sorted
    coff = np.concatenate([[0], np.cumsum(k * w[order])])
    centres: List[Optional[torch.Tensor]] = [None] * n_seg
    info: List[Optional[dict]] = [None] * n_seg
    for i, s in enumerate(order.tolist()):
        centres[s] = cen_flat[int(coff[i]):int(coff[i + 1])].view(k, int(w[s]))
        info[s] = info_sorted[i]
    inertia = np.array([i["inertia"] for i in info], dtype=np.float64)
    if return_info:
        return labels, centres, inertia, info
    return labels, centres, inertia


def _scatter_index(rows: np.ndarray, order: np.ndarray) -> torch.Tensor:
    """dest[j] = the row of the caller's order that row j of the call order (segments in `order`) is: labels[dest] = labels_sorted."""
    start = np.concatenate([[0], np.cumsum(rows)[:-1]])
    dest = np.concatenate([np.arange(start[s], start[s] + rows[s]) for s in order.tolist()]) if len(order) else np.zeros(0, np.int64)
    return torch.from_numpy(dest.astype(np.int64))
