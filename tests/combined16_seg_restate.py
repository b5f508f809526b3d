"""Numpy restatement of the SEGMENTED 16-bit scan of the combined key (helper module, not a test file): the
batches of the tests and the margin band of a row inside its own segment.

The segmented scan (scan_b16c_kernel<.., SEG>, multimodal-fusion_amd/csrc/mmf_scan_b16c.hip) forms the approximate key and the
margin exactly as the one-graph scan does (tests/combined16_restate.py), with two differences that this module restates:

  * the power-of-two scale, the four maxima and the largest position chain are those of the WHOLE batch — a superset of any one
    segment, so m0_i is at least what a call on the segment alone would use;
  * a row's columns are those of its own segment: T_i is the min(k + self, n_s)-th best A among them and the band the columns of
    the segment with A_ij >= T_i - margin_i(T_i).
A row whose band holds at most `combined16_restate.capacity(k + self)` columns is never sent to the exact pass.
"""
from __future__ import annotations

import numpy as np

import combined16_restate as cr
from oracle import scan16_restate as rs


def batch(sizes, d: int, dp: int, seed: int):
    """(F [N, d], P [N, dp], ptr [S + 1] int64): make_data(n_s, d, dp, seed + s) per non-empty segment s, concatenated."""
    Fs, Ps = [np.zeros((0, d), np.float32)], [np.zeros((0, dp), np.float32)]
    for s, n_s in enumerate(sizes):
        if n_s > 0:
            F, P = cr.make_data(n_s, d, dp, seed + s)
            Fs.append(F)
            Ps.append(P)
    ptr = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(Fs)), np.ascontiguousarray(np.concatenate(Ps)), ptr


def bands_segmented(F: np.ndarray, P: np.ndarray, ptr, lh: float, lg: float, kk: int, operand: str):
    """Per row: (T, margin_i(T), number of columns of the row's segment in the band).  Image, m0 and the approximate keys are
    taken on the whole batch; kk = k + self entries, the row itself among the columns."""
    n = F.shape[0]
    img = cr.image(F, operand)
    pn = rs.sq_norms(np.ascontiguousarray(P, np.float32))
    m0 = cr.m0_of(img, pn, P.shape[1], lh, lg)
    T = np.full(n, -np.inf, np.float32)
    cnt = np.zeros(n, np.int64)
    for s in range(len(ptr) - 1):
        a, b = int(ptr[s]), int(ptr[s + 1])
        if b == a:
            continue
        rows = slice(a, b)
        A = cr.approx_keys(img, P, lh, lg, rows)[:, a:b]
        kth = min(kk, b - a) - 1
        t = -np.partition(-A, kth, axis=1)[:, kth]
        T[rows] = t
        cnt[rows] = (A >= (t - cr.margin(m0[rows], t))[:, None]).sum(axis=1)
    return T, cr.margin(m0, T), cnt
