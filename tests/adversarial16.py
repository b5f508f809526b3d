"""Worst-case rounding data for the 16-bit scan's error margin (helper module, not a test file).

A *family* is a few query rows `q`, k columns `A` that are their true top-k, kk + 3 columns `B` (kk = k + self) whose
APPROXIMATE values beat A's, and fillers that matter to neither: the scan keeps A only because its margin says so.  On
Gaussian data the rounding error of z_i . z_j is a random walk far inside the Cauchy-Schwarz bound; here every component
rounds the same way, so the error of a (q, A) and of a (q, B) pair each come close to the bound, with opposite signs.

Candidate-side families (the `un * RB` term; `candidate_side`): q is exactly representable in the 16-bit format (rn = 0);
every component of B lies just above a rounding midpoint and every component of A just below it.
  dot / neg_sq_l2 / rbf: B = (b - h + delta) on d - 1 components, 0 on the last; A_i = (b - h - delta) there and a small
    exactly representable c_i on the last, which is what makes A truly better; q = b/2 (dot) or b (L2) on every component.
    h = half an ulp of the format at b, delta = h / (padded d).
  cosine: q = 63 ones and a one on the last component, B = the same 63 ones and t on component 63, A_i = B + eps_i on the
    last; t puts 256 / |B| just above a midpoint and eps_i pushes 256 / |A_i| just below it.
Query-side family (the `rn * ZB` term; `query_side`, dot): q_k = b + s_k (h - delta) with a balanced sign pattern s, so q
  rounds to b on every component; B = b - w s and A_i = b + w s - tau_i are exactly representable (RB = 0: the candidate
  fillers are exact too).  The truth prefers A by 2 w d (h - delta) - sum(q tau), the approximation prefers B by
  b sum(tau).

Positions: every builder takes the rows of q and the columns of A and B, so a test decides which workgroup, column split,
panel or super-block meets which.  (A row's threshold is the kk-th best of the union of its two lane lists, so which of
the two a column falls into does not matter.)

Fillers matter to neither and must not send ordinary rows to the exact rescan, which the GPU tests require to stay idle.
Three kinds, each used where the device run showed it flags no row:
  * "gauss": Gaussian rows, the columns (and, when X is scanned against itself, all rows) rounded to bf16 so that they carry no
    residual.  Used at d = 128, k = 5.  With bf16 operands the margin of ANY query row is at least 2 |u_i| RB with RB the
    family's residual; at d = 500 .. 1000 or k = 15 .. 30 that is so much of the spread of a row's Gaussian values that the
    band below the k-th best overflows the row's lists.
  * "ladder" (`ladder`): rows c e_p with c = 250, 245, ..., 60, exactly representable, norms below the family's; an ordinary
    query row 30 e_p (a ladder row itself when X is scanned against itself) sees the values 30 c of its own component, 5 apart
    in c where its margin covers less than 3, and an exact 0 everywhere else.  Used at the larger d and k — not for the L2
    metrics (equal-norm columns tie) and not with a single list pair per row when X is scanned against itself (the ties at 0
    crowd it): both flag rows.
  * "signs" (cosine): +-1 on 16 components, which normalise exactly.
The four maxima of the candidate side are the family's own, and an ordinary query row of a rectangular call has less than half
a q row's margin.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Optional, Sequence

import numpy as np

import oracle
from oracle import scan16_restate as rs
from oracle.scan16_restate import DOT

BASE = {128: 24.0, 512: 16.5, 1024: 8.5}      # b per padded dim: the largest norm b sqrt(d) stays in [256, 512) at d = 128, 500, 1000


@dataclasses.dataclass
class Family:
    name: str
    metric: str
    operand: str                  # "f16" / "bf16"
    k: int
    kk: int                       # k + self
    lam: float
    X: np.ndarray                 # query rows (all rows for a scan of X against itself)
    Y: Optional[np.ndarray]       # columns; None: X against itself
    q_rows: np.ndarray
    a_cols: np.ndarray
    b_cols: np.ndarray
    ref: Optional[tuple] = None

    @property
    def precision(self) -> str:
        return "fast" if self.operand == "f16" else "fast_bf16"

    @property
    def cols(self) -> np.ndarray:
        return self.X if self.Y is None else self.Y


def columns(start: int, count: int) -> np.ndarray:
    return np.arange(start, start + count, dtype=np.int64)


def half_ulp(operand: str, v: float) -> float:
    """Half an ulp of the 16-bit format in the binade of v."""
    e = int(np.floor(np.log2(abs(v))))
    return float(2.0 ** (e - (10 if operand == "f16" else 7) - 1))


def representable(operand: str, v) -> bool:
    v = np.atleast_1d(np.asarray(v, np.float32))
    if operand == "f16":
        return bool(np.array_equal(v.astype(np.float16).astype(np.float32), v))
    return bool(np.array_equal(rs.bf16_to_f32(rs.round_bf16(v)), v))


RUNGS = 39                                        # filler magnitudes 250, 245, ..., 60: exact in f16 and bf16


def ladder(n: int, d: int) -> np.ndarray:
    """n filler rows c e_p: one non-zero component each, row j on component j mod C (C = ceil(n / RUNGS)) with magnitude
    250 - 5 (j div C)."""
    C = -(-n // RUNGS)
    assert C <= d
    j = np.arange(n)
    f = np.zeros((n, d), np.float32)
    f[j, j % C] = 250.0 - 5.0 * (j // C)
    return f


def gauss(rng, n: int, d: int, norm: float, pre_round: bool) -> np.ndarray:
    """n Gaussian filler rows of the given norm, optionally rounded to bf16 (exact in f16 too at these magnitudes)."""
    f = rng.randn(n, d)
    f *= norm / np.linalg.norm(f, axis=1, keepdims=True)
    f = f.astype(np.float32)
    return rs.bf16_to_f32(rs.round_bf16(f)) if pre_round else f


def _signs(rng, n: int, d: int) -> np.ndarray:
    """+-1 on 16 components: normalises to +-64 exactly, no residual at all (cosine: every un is the same 256)."""
    f = np.zeros((n, d), np.float32)
    for i in range(n):
        f[i, rng.choice(d, 16, replace=False)] = rng.choice([-1.0, 1.0], 16)
    return f


def _place(fam_name, metric, operand, k, kk, lam, q, A, B, n_rows, n_cols, q_pos, a_pos, b_pos, self_scan, seed, d, fill,
           c_norm=200.0):
    """fill: "signs" (cosine), "gauss" (query rows of norm 30, columns of norm c_norm rounded to bf16; X against itself: norm
    100, rounded) or "ladder" (columns `ladder`, query rows 30 e_p on the ladder's components)."""
    q_pos, a_pos, b_pos = (np.asarray(p, np.int64) for p in (q_pos, a_pos, b_pos))
    assert len(q_pos) == len(q) and len(a_pos) == len(A) == k and len(b_pos) == len(B) == kk + 3
    rng = np.random.RandomState(seed)
    if self_scan:
        X = {"ladder": lambda: ladder(n_rows, d), "gauss": lambda: gauss(rng, n_rows, d, 100.0, True)}[fill]()
        assert len(set(q_pos) | set(a_pos) | set(b_pos)) == len(q_pos) + len(a_pos) + len(b_pos)
        X[q_pos], X[a_pos], X[b_pos] = q, A, B
        Y = None
    else:
        if fill == "signs":
            X, Y = _signs(rng, n_rows, d), _signs(rng, n_cols, d)
        elif fill == "gauss":
            X, Y = gauss(rng, n_rows, d, 30.0, False), gauss(rng, n_cols, d, c_norm, True)
        else:
            X = np.zeros((n_rows, d), np.float32)
            X[np.arange(n_rows), np.arange(n_rows) % (-(-n_cols // RUNGS))] = 30.0
            Y = ladder(n_cols, d)
        X[q_pos] = q
        Y[a_pos], Y[b_pos] = A, B
    return Family(fam_name, metric, operand, k, kk, lam, X, Y, q_pos, a_pos, b_pos)


def candidate_side(metric: str, operand: str, d: int, k: int, *, n_rows: int, n_cols: int = 0, q_pos: Sequence[int],
                   a_pos: Sequence[int], b_pos: Sequence[int], self_scan: bool = False, seed: int = 0, fill: str = "ladder") -> Family:
    """The `un * RB` family.  len(q_pos) query rows, len(a_pos) == k, len(b_pos) == k + self + 3."""
    kk = k + (1 if self_scan else 0)
    nq = len(q_pos)
    name = f"cand-{metric}-{operand}-d{d}-k{k}" + ("-self" if self_scan else "")
    if metric == rs.COSINE:
        assert d == 128 and not self_scan
        q, A, B = _cosine_rows(operand, k, kk, nq)
        return _place(name, metric, operand, k, kk, 1.0, q, A, B, n_rows, n_cols, q_pos, a_pos, b_pos, False, seed, d, "signs")
    b = BASE[rs.padded_dim(d)]
    h = half_ulp(operand, b)
    delta = h / rs.padded_dim(d)
    l2 = metric in (rs.NEG_SQ_L2, rs.RBF)
    assert not (l2 and self_scan), "identical q rows would be each other's nearest rows"
    qv = b if l2 else b / 2
    # Q(A) - Q(B) wanted: above the f32 chain's noise, which grows with the chain's length
    gap = 1.1 * np.sqrt(d / 128.0)
    if l2:      # Q_A - Q_B = (2 b c - c^2 - 4 h delta (d - 1)) / 2
        c0 = (2 * gap + 4 * h * delta * (d - 1)) / (2 * b - 1.0)
    else:       # Q_A - Q_B = (b / 2) (c - 2 delta (d - 1))
        c0 = gap / qv + 2 * delta * (d - 1)
    step = 2.0 ** -7
    c0 = np.ceil(c0 / step) * step
    q = np.full((nq, d), qv, np.float32)
    B = np.full((kk + 3, d), b - h + delta, np.float32)
    B[:, -1] = 0.0
    A = np.full((k, d), b - h - delta, np.float32)
    A[:, -1] = c0 + step * np.arange(k)
    assert representable(operand, A[:, -1]) and representable(operand, q)
    assert float(B[0, 0]) == b - h + delta and float(A[0, 0]) == b - h - delta, "b - h +- delta must be exact in f32"
    lam = 1e-3 if metric == rs.RBF else 1.0
    return _place(name, metric, operand, k, kk, lam, q, A, B, n_rows, n_cols, q_pos, a_pos, b_pos, self_scan, seed, d, fill)


def _unit_component(v: np.ndarray) -> np.float32:
    """u of a component that is 1.0 in the row v, as prep computes it for cosine: (1 / clamped_norm) * 256."""
    sc = rs.row_scalars(v[None, :], rs.COSINE)[0]
    return np.float32(np.float32(1.0) / sc) * np.float32(256.0)


def _cosine_rows(operand: str, k: int, kk: int, nq: int):
    d = 128
    ulp = 2.0 * half_ulp(operand, 31.0)
    mid = 32.0 - ulp / 2                                  # the highest midpoint below 32
    q = np.zeros((nq, d), np.float32)
    q[:, :63] = 1.0
    q[:, -1] = 1.0                                        # norm 8: 32 on every component, exactly
    B = np.zeros(d, np.float32)
    B[:63] = 1.0
    t = np.float32(np.sqrt((256.0 / mid) ** 2 - 63.0))
    # walk t down until 256 / |B| is the smallest f32 above the midpoint
    B[63] = t
    while _unit_component(B) <= mid:
        t = np.nextafter(t, np.float32(0)); B[63] = t
    while True:
        t2 = np.nextafter(t, np.float32(2)); B[63] = t2
        if _unit_component(B) <= mid:
            break
        t = t2
    B[63] = t
    assert _unit_component(B) > mid
    # the smallest eps (in steps of 2^-12) that takes 256 / |A| below the midpoint
    step = 2.0 ** -12
    A = np.repeat(B[None, :], k, axis=0)
    e = step
    while True:
        A[0, -1] = e
        if _unit_component(A[0]) < mid:
            break
        e += step
    A[:, -1] = e * (1.0 + np.arange(k) / 16.0)
    return q, A, np.repeat(B[None, :], kk + 3, axis=0)


def query_side(operand: str, k: int, *, n_rows: int, n_cols: int, q_pos: Sequence[int], a_pos: Sequence[int],
               b_pos: Sequence[int], d: int = 128, seed: int = 0) -> Family:
    """The `rn * ZB` family (dot, X against separate columns)."""
    assert d == 128
    kk = k
    b, w = 10.0, 30.0
    h = half_ulp(operand, b)
    delta = h / d
    s = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    q = np.repeat((b + s * (h - delta))[None, :], len(q_pos), axis=0).astype(np.float32)
    assert float(q[0, 0]) == b + h - delta and float(q[0, 1]) == b - h + delta
    B = np.repeat((b - w * s)[None, :], kk + 3, axis=0).astype(np.float32)
    ulp = 2.0 * half_ulp(operand, b + w)
    gap = 1.1
    T = int(np.floor((2 * w * (h - delta) * d - gap) / ((b + h - delta) * ulp)))     # ulps taken off the +w components
    plus = np.flatnonzero(s > 0)
    A = np.repeat((b + w * s)[None, :], k, axis=0)
    for i in range(k):
        t = T - i
        A[i, plus] -= ulp * (t // len(plus))
        A[i, plus[: t % len(plus)]] -= ulp
    A = A.astype(np.float32)
    assert representable(operand, A) and representable(operand, B)
    name = f"query-dot-{operand}-d{d}-k{k}"
    return _place(name, rs.DOT, operand, k, kk, 1.0, q, A, B, n_rows, n_cols, q_pos, a_pos, b_pos, False, seed, d, "gauss", 50.0)


# ---------------------------------------------------------------------------------------------------------------------
# what a family is worth: oracle, restated operands, sharpness
# ---------------------------------------------------------------------------------------------------------------------
def restated(fam: Family):
    """(query side, candidate side, margins of the query rows) of the family's call, restated."""
    nx = rs.sq_norms(fam.X)
    mx = float(nx.max())
    if fam.Y is not None:
        mx = max(mx, float(rs.sq_norms(fam.Y).max()))
    qs = rs.operands(fam.X, fam.metric, fam.operand, mx)
    cs = qs if fam.Y is None else rs.operands(fam.Y, fam.metric, fam.operand, mx)
    return qs, cs, rs.margins(qs, cs["maxima"], fam.metric, fam.kk)


def reference(fam: Family):
    """The oracle's (idx, val) for every query row; computed once per family."""
    if fam.ref is None:
        fam.ref = oracle.simtopk(fam.X, fam.Y, metric=fam.metric, lam=fam.lam, k=fam.k, exclude_self=fam.Y is None)
    return fam.ref


def analyse(fam: Family) -> dict:
    """Per q row: the sharpness rho = (kk-th best G - min over A of G) / margin, whether the kk best G avoid A, and
    max |G - Q| / e1 over the family's (q, column) pairs; plus whose the four maxima are."""
    qs, cs, mg = restated(fam)
    sub = {key: (v[fam.q_rows] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == len(fam.X) else v) for key, v in qs.items()}
    G = rs.approx_values(sub, cs)
    Q = rs.target_values(sub, cs)
    if fam.Y is None:
        G[np.arange(len(fam.q_rows)), fam.q_rows] = -np.inf           # self is excluded
    order = np.argsort(-G, axis=1, kind="stable")
    top = order[:, : fam.kk]
    kth = np.take_along_axis(G, top[:, -1:], axis=1)[:, 0]
    margin = mg["margin"][fam.q_rows].astype(np.float64)
    rho = (kth - G[:, fam.a_cols].min(axis=1)) / margin
    fam_cols = np.concatenate([fam.a_cols, fam.b_cols])
    err = np.abs(G[:, fam_cols] - Q[:, fam_cols]).max(axis=1) / mg["e1"][fam.q_rows].astype(np.float64)
    members = np.zeros(len(fam.cols), bool)
    members[fam_cols] = True
    if fam.Y is None:
        members[fam.q_rows] = True
    # the candidate side's maxima are the family's own: no filler reaches them (zn / un of unit rows differ by rounding only)
    own = [cs[key][~members].max(initial=0.0) <= cs[key][members].max() * (1 + 1e-6) for key in ("zn", "rn", "un")]
    other = np.setdiff1d(np.arange(len(fam.X)), fam.q_rows if fam.Y is not None else np.concatenate([fam.q_rows, fam_cols]))
    return dict(rho=rho, top_avoids_a=not np.isin(top, fam.a_cols).any(), err_over_e1=err, maxima_own=all(own),
                margin=margin, other_margin_max=float(mg["margin"][other].max()) if len(other) else 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the families the GPU tests use (tests/test_gpu_scan16_adversarial.py); tests/test_scan16_margin_cpu.py certifies each
# ---------------------------------------------------------------------------------------------------------------------
RECT_ROWS, RECT_COLS = 300, 4096
RECT_Q = (5, 130, 290)                 # two waves of the first row block and one row of the second
KINDS = [("cand", "dot"), ("cand", "neg_sq_l2"), ("cand", "rbf"), ("cand", "cosine"), ("query", "dot")]
OPERANDS = ["f16", "bf16"]
DIM_K = [(d, k) for d in (128, 500, 1000) for k in (5, 15, 30) if (d, k) != (1000, 30)]   # no 32-entry lists at padded dim 1024
# X against itself: q rows 5, 130, 600, 1450 = row blocks (and super-blocks of one row block) 0, 0, 2 and 5; B from row 300 (block 1),
# A from row 1030 (block 4).  The scan never drops anything in the first 32 tiles (1024 columns) of a column range, while its
# thresholds form, so A lies behind them — as in the rectangular families.
SELF_ROWS = 1500
DIM_COLS = 2048


def rect_family(kind: str, metric: str, operand: str, order: str = "ba", d: int = 128, k: int = 5, n_cols: int = RECT_COLS) -> Family:
    """q rows among RECT_ROWS query rows; order "ba": B in the first eighth of the columns and A in the last, "ab": the reverse.
    Built once per argument set."""
    return _rect_family(kind, metric, operand, order, d, k, n_cols)


@functools.lru_cache(maxsize=None)
def _rect_family(kind, metric, operand, order, d, k, n_cols) -> Family:
    lo, hi = 64, n_cols - 496
    a0, b0 = (hi, lo) if order == "ba" else (lo, hi)
    kw = dict(n_rows=RECT_ROWS, n_cols=n_cols, q_pos=RECT_Q, a_pos=columns(a0, k), b_pos=columns(b0, k + 3))
    if kind == "query":
        return query_side(operand, k, d=d, **kw)
    return candidate_side(metric, operand, d, k, fill="gauss" if (d, k) == (128, 5) and n_cols == RECT_COLS else "ladder", **kw)


def self_family(operand: str, d: int = 128, k: int = 5, n_rows: int = SELF_ROWS, fill: str = "ladder") -> Family:
    """X against itself (dot): q, A and B rows in different row blocks of 256.  Built once per argument set."""
    return _self_family(operand, d, k, n_rows, fill)


@functools.lru_cache(maxsize=None)
def _self_family(operand, d, k, n_rows, fill) -> Family:
    q_pos = (5, 130, 600, n_rows - 50)
    return candidate_side(DOT, operand, d, k, n_rows=n_rows, q_pos=q_pos, a_pos=columns(1030, k),
                          b_pos=columns(300, k + 4), self_scan=True, fill=fill)


def all_families():
    """(family, floor of its sharpness) for every family a GPU test uses.  Floors: 0.85 for the candidate-side dot / L2 / rbf
    families at padded dim 128 and 0.6 for cosine; elsewhere 0.9 x the sharpness the construction reaches in the restatement
    (the reached values are listed in tests/test_scan16_margin_cpu.py)."""
    out = []
    for op in OPERANDS:
        for kind, metric in KINDS:
            for order in ("ba", "ab"):
                out.append(rect_family(kind, metric, op, order))
        for d, k in DIM_K:
            out.append(rect_family("cand", DOT, op, "ba", d, k, DIM_COLS))
        for k in (5, 30):
            out.append(self_family(op, 128, k))
        out.append(self_family(op, 500, 5))
        out.append(self_family(op, 128, 5, SELF_ROWS, "gauss"))
    return out
