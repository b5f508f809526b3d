"""Numpy restatement of the passes of mmf_simtopk_combined_xy_fast_anyk (helper module, not a test file): the
ceiling per QUERY and the pass loop of combined_xy_fast_anyk_run (mmf_api.hip) for queries that are not the candidates, or only some
of them — tests/combined16_anyk_restate.py's ceiling, yield rule and plan over tests/combined_xy_restate.py's two-sided image.

Why the ceiling carries over.  The derivation of the ceiling (mmf_scan_b16c.hip, "Ceilings") is per row: it uses
|A_ij - key_ij| <= e0_i + 3 u' |A_ij| and e0_i <= m0_i / 2 and nothing else.  For two sets the scale, the four maxima and the largest
position chain are taken over the UNION of both sides (combined_xy_restate.bands_xy), a superset of the candidates — all the bound of
query i needs — so the inequality holds pair by pair with m0_i at least what a self call over the union would use, and
ceiling_i = the float above fl(hf + fl(6 u |hf|)), hf = fl(fk_i + m0_i / 2), never masks a candidate that ranks after the floor.

A pass p >= 1 (`done` entries emitted, K = 20 - self deep), per query i (ids: q0 + i for the queries, c0 + j for the candidates):
  * S_i: the admissible candidates (all but the one whose id is the query's, when self is excluded) that rank after the floor;
  * the unmasked candidates: A_ij <= ceiling_i;  ghosts: already-emitted candidates that are unmasked — a prefix of the re-ranked row,
    which holds the K best unmasked admissible candidates in the exact order;
  * certified_i = K - min(ghosts_i, K);  the band under the ceiling, among the CANDIDATE columns only: the unmasked candidates (the
    query's own row among them, when it is one) with A_ij >= T_i - margin_i(T_i), T_i the 20th best unmasked A;  a band of at most
    32 columns is never flagged by the scan;
  * the yield t: the largest t <= min(K, k - done) that leaves at most nq / short_div unflagged queries short of it.
Every query then has done + t entries (the short and the flagged ones from the exact rescan): the next floor is entry done + t - 1 of
the query's exact order.
"""
from __future__ import annotations

import numpy as np

import combined16_anyk_restate as ar
import combined16_restate as cr
import combined_xy_restate as xr
from oracle import scan16_restate as rs

DEPTH, LIST_CAP, UP = ar.DEPTH, ar.LIST_CAP, ar.UP


def setup(F, P, q, c, lh, lg, operand):
    """(A [nq, nc] f64 approximate keys, key [nq, nc] f64 canonical keys (NaN: -inf), m0 [nq] f32) with the image, the scale, the maxima
    and the largest position chain over the union of both ranges, as combined_xy_restate.bands_xy takes them."""
    (q0, q1), (c0, c1) = q, c
    seen = np.union1d(np.arange(c0, c1), np.arange(q0, q1))
    Fs, Ps = np.ascontiguousarray(F[seen], np.float32), np.ascontiguousarray(P[seen], np.float32)
    img = cr.image(Fs, operand)
    pn = rs.sq_norms(Ps)
    m0 = cr.m0_of(img, pn, P.shape[1], lh, lg)
    qi = np.searchsorted(seen, np.arange(q0, q1))
    ci = np.searchsorted(seen, np.arange(c0, c1))
    A = cr.approx_keys(img, Ps, lh, lg, qi)[:, ci].astype(np.float64)
    key = cr.canonical_keys(Fs, Ps, lh, lg)[np.ix_(qi, ci)].astype(np.float64)
    key = np.where(np.isnan(key), -np.inf, key)
    return A, key, m0[qi]


def passes(F, P, q, c, lh, lg, k, operand, *, exclude_self=False, short_div=64, max_passes=15):
    """The later passes of the call on rows [q0, q1) against rows [c0, c1) of (F, P), ids = row numbers: a list of dicts, one per
    pass p >= 1, with per query `excess` = max over S_i of A_ij - ceiling_i (-inf for an empty S_i), `ghosts`, `ghost_slack` = min
    over the ghosts of (ceiling_i + m0_i / 2 + 3 u' |A_ij|) - key_ij (+inf without ghosts), `prefix` (the ghosts lead the re-ranked
    row), `band`, `flagged` (band over 32, or fewer than K candidates left), and the pass's `yield`, `short` queries, `done` before
    it.  The call must be one the passes serve: c1 - c0 >= k + self."""
    (q0, q1), (c0, c1) = q, c
    nq, nc = q1 - q0, c1 - c0
    self1 = 1 if exclude_self else 0
    K = DEPTH - self1
    assert nc >= k + self1 > DEPTH, "served exactly, or by one pass"
    A, key, m0 = setup(F, P, q, c, lh, lg, operand)
    ids = np.arange(nc)
    order = []
    for i in range(nq):
        rk = key[i].copy()
        me = q0 + i - c0
        hit = bool(self1 and 0 <= me < nc)
        if hit:
            rk[me] = -np.inf
        o = np.lexsort((ids, -rk))
        order.append(o[o != me] if hit else o)           # the exact order over the admissible candidates
    out, done = [], K
    while done < k and len(out) + 1 < max_passes:
        rec = {name: [] for name in ("excess", "ghosts", "ghost_slack", "prefix", "band", "flagged")}
        for i in range(nq):
            o = order[i]
            fk = np.float32(key[i, o[done - 1]])
            cl = float(ar.ceiling(np.array([fk]), m0[i:i + 1])[0])
            open_ = A[i] <= cl                             # unmasked candidates, the query's own row among them
            after = o[done:]
            rec["excess"].append(float((A[i, after] - cl).max()) if after.size else -np.inf)
            emitted = o[:done]
            gh = emitted[open_[emitted]]
            rec["ghosts"].append(int(gh.size))
            slack = (cl + 0.5 * float(m0[i]) + 3.0 * UP * np.abs(A[i, gh])) - key[i, gh]
            rec["ghost_slack"].append(float(slack.min()) if gh.size else np.inf)
            staged = o[open_[o]][:K]                        # the K best unmasked admissible candidates in the exact order
            is_ghost = np.isin(staged, gh)
            g = int(is_ghost.sum())
            rec["prefix"].append(bool(is_ghost[:g].all() and not is_ghost[g:].any()))
            vals = np.sort(A[i, open_])[::-1]
            if vals.size >= DEPTH:
                T = np.float32(vals[DEPTH - 1])
                band = int((vals >= np.float64(T) - np.float64(cr.margin(m0[i], T))).sum())
            else:
                band = int(vals.size)
            rec["band"].append(band)
            rec["flagged"].append(bool(band > LIST_CAP or staged.size < K))
        rec = {name: np.asarray(v) for name, v in rec.items()}
        cert = K - np.minimum(rec["ghosts"], K)
        hist = np.bincount(cert[~rec["flagged"]], minlength=K + 1)
        t, short = ar.anyk_yield(hist, min(K, k - done), nq // short_div)
        rec.update(done=done, short=short)
        rec["yield"] = t if t >= 1 else k - done            # a yield below 1: the exact scan finishes every query
        rec["finished_exact"] = t < 1
        out.append(rec)
        done += rec["yield"]
    return out


# ---- the seeded inputs the GPU tests (tests/test_gpu_simtopk_combined_xy_fast_anyk.py) share with the restatement --------------------
LH, LG = xr.LH, xr.LG
# The "clean" two-set input is combined_xy_restate's R1 itself (130 queries against 260 candidates of 390 rows, d = 40, dp = 2: a
# partial query block, a partial candidate tile): every band under a ceiling holds at most 32 columns in every pass, for both operand
# types (asserted on the CPU, tests/test_simtopk_combined_xy_fast_anyk_cpu.py), so no query may be flagged by the scan.
CLEAN_CASE = xr.CASES[0]


def clean_case():
    """((F, P), q, c) of the clean input."""
    return xr.case_data(CLEAN_CASE), CLEAN_CASE.q, CLEAN_CASE.c


def gaussian_inputs(seed: int = 21):
    """R1's shape on combined16_anyk_restate.clean_inputs' kind of data: Gaussian rows scaled to a squared norm of about 8 (every
    pair far apart) on pixel positions — the background of the tie input."""
    case = CLEAN_CASE
    rng = np.random.RandomState(7400 + seed)
    F = (rng.randn(case.total, case.d) * np.sqrt(8.0 / case.d)).astype(np.float32)
    P = (rng.randint(0, 48, (case.total, case.dp)) * 224).astype(np.float32)
    return np.ascontiguousarray(F), np.ascontiguousarray(P)


def ghost_case():
    """combined16_anyk_restate.ghost_inputs() split into its first 200 rows as queries against all 600: ((F, P), q, c)."""
    return ar.ghost_inputs(), (0, 200), (0, ar.GHOST_N)


TIE_QUERIES = (0, 1, 2)                       # identical queries (rows of the data set)
TIE_NEAR = np.arange(140, 155)                # 15 candidates nearer to them than the tie group: ranks 0 .. 14
TIE_GROUP = np.arange(200, 230)               # 30 identical candidates at one position: ranks 15 .. 44, ordered by id alone


def tie_inputs():
    """The Gaussian input with a planted neighbourhood for queries 0 .. 2 (made identical): 15 candidates at distinct small distances
    (rows TIE_NEAR) and 30 identical candidates a little further away (rows TIE_GROUP), all at the queries' position — every other
    candidate is far (squared distance about 16, and another position).  Ranks 15 .. 44 of those queries tie in every bit of the key
    across the first floor (entry 19 or 20)."""
    F, P = gaussian_inputs()
    rng = np.random.RandomState(7500)
    for r in TIE_QUERIES[1:]:
        F[r], P[r] = F[0], P[0]
    for t, r in enumerate(TIE_NEAR):
        F[r] = F[0] + np.float32(0.002 * (t + 1)) * rng.randn(F.shape[1]).astype(np.float32)
        P[r] = P[0]
    F[TIE_GROUP] = F[0] + np.float32(0.06) * rng.randn(F.shape[1]).astype(np.float32)
    P[TIE_GROUP] = P[0]
    return np.ascontiguousarray(F), np.ascontiguousarray(P)
