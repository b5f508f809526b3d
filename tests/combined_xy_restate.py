"""Helpers of the two-set top-k tests (not a test file): the cases of the capacity test, the reference composed from the oracle,
and the margin band of tests/combined16_restate.py restated for queries that are not the candidates (mmf_simtopk_combined_xy,
DESIGN.md §4.19).

A case names row ranges of ONE data set `combined16_restate.make_data(total, d, dp, total % 7 + d % 5)`: the queries are rows
[q0, q1), the candidates rows [c0, c1), and the ids are the rows' numbers in the data set (row_offset = q0, col_offset = c0), so
"self" is the same row of the data.  `slice` says how the test hands them to the library: as views of one device array (the
library then sees a row slice of the candidates) or as two arrays of their own.

The band: image, common scale, the four maxima and the largest position chain over the rows the library is given — the union of
both ranges — and a query's band taken among the candidate columns only: the columns with A_ij >= T_i - margin_i(T_i), T_i the
(k + self)-th best A of the query among the candidates.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import combined16_restate as cr
from oracle import scan16_restate as rs

LH, LG = 0.5, 2e-7
Case = namedtuple("Case", "name total d dp q c slice")
CASES = [
    Case("R1", 390, 40, 2, (0, 130), (130, 390), False),
    Case("R2", 400, 64, 3, (100, 300), (50, 350), False),
    Case("R3", 258, 130, 8, (0, 129), (129, 258), False),
    Case("R4", 600, 512, 2, (0, 300), (300, 600), False),
    Case("R5", 700, 96, 2, (175, 350), (0, 700), True),
    Case("R6", 300, 1536, 2, (0, 150), (150, 300), False),
]

_DATA = {}


def case_data(case: Case):
    key = (case.total, case.d, case.dp)
    if key not in _DATA:
        _DATA[key] = cr.make_data(case.total, case.d, case.dp, case.total % 7 + case.d % 5)
    return _DATA[key]


def reference(F, P, q, c, k, lh=LH, lg=LG, exclude_self=False, K=None):
    """(idx [nq, k] int64 padded with -1, oracle values [nq, k] padded with -inf) of rows [q0, q1) against rows [c0, c1) of the
    data set, ids = row numbers: key = lh * -sq(features) + lg * -sq(positions) in f32, np.lexsort by (-key, id), the values
    the block of oracle.sim_dense_combined of the whole set (K: that matrix, when the caller already has it)."""
    import oracle
    (q0, q1), (c0, c1) = q, c
    nq, nc = q1 - q0, c1 - c0
    idx = np.full((nq, k), -1, dtype=np.int64)
    val = np.full((nq, k), -np.inf, dtype=np.float32)
    if nq == 0 or nc == 0:
        return idx, val
    A = oracle.sim_dense(F[q0:q1], F[c0:c1], metric="neg_sq_l2")
    B = oracle.sim_dense(P[q0:q1], P[c0:c1], metric="neg_sq_l2")
    key = (np.float32(lh) * A + np.float32(lg) * B).astype(np.float32)
    if K is None:
        K = oracle.sim_dense_combined(F, P, lh, lg)
    ids = np.arange(c0, c1)
    for i in range(nq):
        ki = key[i].copy()
        if exclude_self and c0 <= q0 + i < c1:
            ki[q0 + i - c0] = -np.inf
        take = min(k, nc - (1 if exclude_self and c0 <= q0 + i < c1 else 0))
        order = np.lexsort((ids, -ki))[:take]
        idx[i, :take] = ids[order]
        val[i, :take] = K[q0 + i, ids[order]]
    return idx, val


def bands_xy(F, P, q, c, lh, lg, kk, operand):
    """Per query: (T, margin_i(T), columns in the band) with everything the margin uses taken over the union of both ranges."""
    (q0, q1), (c0, c1) = q, c
    seen = np.union1d(np.arange(c0, c1), np.arange(q0, q1))
    Fs, Ps = np.ascontiguousarray(F[seen]), np.ascontiguousarray(P[seen])
    img = cr.image(Fs, operand)
    pn = rs.sq_norms(Ps)
    m0 = cr.m0_of(img, pn, P.shape[1], lh, lg)
    qi = np.searchsorted(seen, np.arange(q0, q1))
    ci = np.searchsorted(seen, np.arange(c0, c1))
    A = cr.approx_keys(img, Ps, lh, lg, qi)[:, ci]
    kth = min(kk, c1 - c0) - 1
    T = -np.partition(-A, kth, axis=1)[:, kth]
    mg = cr.margin(m0[qi], T)
    cnt = (A >= (T - mg)[:, None]).sum(axis=1)
    return T, mg, cnt


def oracle_op(q_features, q_positions, c_features, c_positions, lambda_h, lambda_g, k, *, exclude_self, row_offset, col_offset):
    """The composition above as a stand-in for the device op of distributed.sharded_simtopk_combined (CPU torch tensors)."""
    import oracle
    import torch
    Fq, Pq, Fc, Pc = (np.ascontiguousarray(t.numpy(), np.float32) for t in (q_features, q_positions, c_features, c_positions))
    nq, nc = Fq.shape[0], Fc.shape[0]
    key = (np.float32(lambda_h) * oracle.sim_dense(Fq, Fc, metric="neg_sq_l2") +
           np.float32(lambda_g) * oracle.sim_dense(Pq, Pc, metric="neg_sq_l2")).astype(np.float32)
    K = oracle.sim_dense_combined(np.vstack([Fq, Fc]), np.vstack([Pq, Pc]), lambda_h, lambda_g)[:nq, nq:]
    ids = col_offset + np.arange(nc)
    idx = np.full((nq, k), -1, dtype=np.int64)
    val = np.full((nq, k), -np.inf, dtype=np.float32)
    for i in range(nq):
        ki = key[i].copy()
        me = row_offset + i - col_offset
        hit = exclude_self and 0 <= me < nc
        if hit:
            ki[me] = -np.inf
        take = min(k, nc - (1 if hit else 0))
        order = np.lexsort((ids, -ki))[:take]
        idx[i, :take] = ids[order]
        val[i, :take] = K[i, order]
    return torch.from_numpy(idx), torch.from_numpy(val)
