"""Numpy restatement of the passes of mmf_simtopk_combined_fast_anyk (helper module, not a test file): the
per-row ceiling of multimodal-fusion_amd/csrc/mmf_scan_b16c.hip ("Ceilings", comb_ceil_kernel) and the pass loop of
combined_fast_anyk_run (mmf_api.hip) with its yield rule, on top of tests/combined16_restate.py (image, approximate key A, m0,
margin) and tests/combined16_seg_restate.py (the batch-wide scale and maxima of a ragged batch).

The ceiling.  |A_ij - key_ij| <= e0_i + 3 u' |A_ij| with e0_i <= m0_i / 2.  A column that ranks strictly after the
row's floor (fk_i, fid_i) has key_ij <= fk_i, so with h = fk_i + e0_i:  A_ij >= 0 gives A_ij (1 - 3 u') <= h;  h < A_ij < 0 gives
|A_ij| < |h|;  either way A_ij <= h + 3.1 u' |h|.  In f32:  hf = fl(fk_i + m0_i / 2),  ceiling = the float above
fl(hf + fl(6 u |hf|)),  -inf for a floor of -inf.

A pass p >= 1 (`done` entries emitted, K = 20 - self deep), per row of a served segment:
  * S_i: the columns of the segment that rank after the floor (the row itself never among them when self is excluded);
  * the unmasked columns: A_ij <= ceiling_i;  ghosts: already-emitted columns that are unmasked — a prefix of the re-ranked row,
    which holds the K best unmasked columns in the exact order (the row itself dropped by identity);
  * certified_i = K - min(ghosts_i, K);  the band under the ceiling: the unmasked columns (the row itself among them) with
    A_ij >= T_i - margin_i(T_i), T_i the 20th best unmasked A;  a band of at most 32 columns is never flagged by the scan;
  * the yield t: the largest t <= min(K, k - done) that leaves at most n_served / short_div unflagged rows short of it.
Every row then has done + t entries (the short and the flagged ones from the exact rescan): the next floor is entry done + t - 1 of
the row's exact order.
"""
from __future__ import annotations

import numpy as np

import combined16_restate as cr
from oracle import scan16_restate as rs

DEPTH = 20
LIST_CAP = 32
U24 = cr.U24
UP = 1.01 * 2.0 ** -24          # u'


def ceiling(fk: np.ndarray, m0: np.ndarray) -> np.ndarray:
    """comb_ceil_kernel in numpy f32."""
    f = np.float32
    fk, m0 = np.asarray(fk, f), np.asarray(m0, f)
    with np.errstate(invalid="ignore"):
        hf = (fk + f(0.5) * m0).astype(f)
        c = (hf + ((f(6.0) * U24) * np.abs(hf)).astype(f)).astype(f)
        c = np.nextafter(c, f(np.inf)).astype(f)
    return np.where(np.isneginf(fk), f(-np.inf), c).astype(f)


def anyk_yield(hist, t_max: int, budget: int):
    """mmf_api.hip's anyk_yield: (t, rows short of t)."""
    t, below, short = 0, 0, 0
    for tq in range(1, t_max + 1):
        below += int(hist[tq - 1])
        if below > budget:
            break
        t, short = tq, below
    return t, short


def plan(k: int, exclude_self: bool):
    """(scan_kk, first_yield, min_passes) of mmf_combined_fast_anyk_plan."""
    self1 = 1 if exclude_self else 0
    kk, per = k + self1, DEPTH - self1
    if kk <= DEPTH:
        return kk, k, 1
    return DEPTH, per, 1 + -(-(k - per) // per)


def passes(F: np.ndarray, P: np.ndarray, lh: float, lg: float, k: int, operand: str, *, exclude_self: bool = True, ptr=None,
           short_div: int = 64, max_passes: int = 15):
    """The later passes of the call on (F, P): a list of dicts, one per pass p >= 1, with per served row (arrays over the served
    rows, in row order) `excess` = max over S_i of A_ij - ceiling_i (-inf for an empty S_i), `ghosts`, `ghost_slack` = min over the
    ghosts of (ceiling_i + m0_i / 2 + 3 u' |A_ij|) - key_ij (+inf without ghosts), `prefix` (the ghosts lead the re-ranked row),
    `band`, `flagged` (band over 32, or fewer than K columns left), and the pass's `yield`, `short` rows, `done` before it."""
    F = np.ascontiguousarray(F, np.float32)
    P = np.ascontiguousarray(P, np.float32)
    n = F.shape[0]
    self1 = 1 if exclude_self else 0
    K = DEPTH - self1
    ptr = np.array([0, n], np.int64) if ptr is None else np.asarray(ptr, np.int64)
    img = cr.image(F, operand)
    pn = rs.sq_norms(P)
    m0 = cr.m0_of(img, pn, P.shape[1], lh, lg)
    segs = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        a, b = int(a), int(b)
        if b - a == 0 or b - a - self1 < k:
            continue                                         # not served: the exact launch loop answers it
        A = cr.approx_keys(img, P, lh, lg, slice(a, b))[:, a:b].astype(np.float64)
        key = cr.canonical_keys(F[a:b], P[a:b], lh, lg).astype(np.float64)
        key = np.where(np.isnan(key), -np.inf, key)
        rank_key = key.copy()
        if self1:
            np.fill_diagonal(rank_key, -np.inf)
        ids = np.broadcast_to(np.arange(b - a), key.shape)
        order = np.lexsort((ids, -rank_key), axis=1)[:, :b - a - self1]      # the exact order without the row itself
        segs.append((a, b, A, key, order))
    n_served = sum(b - a for a, b, *_ in segs)
    out, done = [], K
    while done < k and len(out) + 1 < max_passes:
        rec = {name: [] for name in ("excess", "ghosts", "ghost_slack", "prefix", "band", "flagged")}
        for a, b, A, key, order in segs:
            ns = b - a
            rows = np.arange(ns)
            fl = order[:, done - 1]
            fk = key[rows, fl].astype(np.float32)
            cl = ceiling(fk, m0[a:b]).astype(np.float64)
            open_ = A <= cl[:, None]                          # unmasked columns, the row itself among them
            for i in range(ns):
                after = order[i, done:]
                rec["excess"].append(float((A[i, after] - cl[i]).max()) if after.size else -np.inf)
                emitted = order[i, :done]
                gh = emitted[open_[i, emitted]]
                rec["ghosts"].append(int(gh.size))
                slack = (cl[i] + 0.5 * float(m0[a + i]) + 3.0 * UP * np.abs(A[i, gh])) - key[i, gh]
                rec["ghost_slack"].append(float(slack.min()) if gh.size else np.inf)
                staged = order[i][open_[i, order[i]]][:K]     # the K best unmasked columns in the exact order
                is_ghost = np.array([c in set(gh.tolist()) for c in staged], bool) if gh.size else np.zeros(staged.size, bool)
                g = int(is_ghost.sum())
                rec["prefix"].append(bool(is_ghost[:g].all() and not is_ghost[g:].any()))
                vals = np.sort(A[i, open_[i]])[::-1]
                if vals.size >= DEPTH:
                    T = np.float32(vals[DEPTH - 1])
                    band = int((vals >= np.float64(T) - np.float64(cr.margin(m0[a + i], T))).sum())
                else:
                    band = int(vals.size)
                rec["band"].append(band)
                rec["flagged"].append(bool(band > LIST_CAP or staged.size < K))
        rec = {name: np.asarray(v) for name, v in rec.items()}
        cert = K - np.minimum(rec["ghosts"], K)
        hist = np.bincount(cert[~rec["flagged"]], minlength=K + 1)
        t, short = anyk_yield(hist, min(K, k - done), n_served // short_div)
        rec.update(done=done, short=short)
        rec["yield"] = t if t >= 1 else k - done             # a yield below 1: the exact scan finishes every row
        rec["finished_exact"] = t < 1
        out.append(rec)
        done += rec["yield"]
    return out


# ---- the seeded inputs the GPU tests (tests/test_gpu_simtopk_combined_fast_anyk.py) share with the restatement ---------------------
LH, LG = 0.5, 2e-7
CLEAN = {"n300": (300, 40, 2, 11), "n700": (700, 130, 3, 12), "n260": (260, 1536, 2, 13)}     # name -> (n, d, dp, seed)


def clean_inputs(name: str):
    """Gaussian rows scaled to a squared norm of about 8 (no near-duplicates) on distinct-ish pixel positions: the inputs the GPU
    tests call "clean" — every band under a ceiling holds at most 32 columns in every pass (asserted on the CPU)."""
    n, d, dp, seed = CLEAN[name]
    rng = np.random.RandomState(7000 + seed)
    F = (rng.randn(n, d) * np.sqrt(8.0 / d)).astype(np.float32)
    P = (rng.randint(0, 48, (n, dp)) * 224).astype(np.float32)
    return np.ascontiguousarray(F), np.ascontiguousarray(P)


GHOST_N, GHOST_D, GHOST_CLUSTER = 600, 64, 10


def ghost_inputs():
    """60 clusters of 10 near-duplicate rows (a centre + 1e-3 noise), every position equal: a row's first pass emits its 9
    cluster mates and the 10 rows of the nearest other cluster, its floor is the last of them, and that cluster's rows — all within
    the margin of the floor — pass under the next ceiling: ghosts in pass 1.  The band of pass 1 stays within two clusters."""
    rng = np.random.RandomState(7100)
    centres = rng.randn(GHOST_N // GHOST_CLUSTER, GHOST_D).astype(np.float32)
    F = (np.repeat(centres, GHOST_CLUSTER, axis=0) + np.float32(1e-3) * rng.randn(GHOST_N, GHOST_D).astype(np.float32)).astype(np.float32)
    F = F[rng.permutation(GHOST_N)]
    P = np.full((GHOST_N, 2), 448.0, np.float32)
    return np.ascontiguousarray(F), np.ascontiguousarray(P)


GHOST_LH, GHOST_LG = 0.05, 2e-7


def adversarial_inputs(operand: str, d: int):
    """tests/adversarial16.py's worst-case rounding rows for the RBF key (every component of the A columns rounds one way, of the
    B columns the other, the q rows are exact) as ONE set scanned against itself, with pixel positions added: the 2048 columns of
    the rectangular family, then its three q rows.  Returns (F, P, lambda_h, rows of q)."""
    import adversarial16 as adv
    fam = adv.rect_family("cand", "rbf", operand, "ba", d, 5, adv.DIM_COLS)
    F = np.ascontiguousarray(np.concatenate([fam.Y, fam.X[fam.q_rows]]).astype(np.float32))
    rng = np.random.RandomState(7200 + d)
    P = (rng.randint(0, 48, (F.shape[0], 2)) * 224).astype(np.float32)
    return F, np.ascontiguousarray(P), float(fam.lam), np.arange(fam.Y.shape[0], F.shape[0])
