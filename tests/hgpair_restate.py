"""numpy restatement of pair-weighted hypergraph propagation and of the softmax over the pairs of a row
(include/ext/mmf_hg_hgpair.h), bit for bit, and the float64 references they are compared with.

The plan is hgconv_restate's with the columns remembered: the valid pairs sorted by (row, member) with a STABLE sort, so that the
copies of a repeated pair keep their column order; pos[j] is the column of edge_index that slot j came from.  Every chain loops over
the MEMBER POSITION p and adds, for every row that has a p-th slot, that slot's term — one rounded float32 multiply and one rounded
float32 add per row and step (numpy neither fuses nor reorders them).

The bounds.  eps = 2^-24 is the relative error of one rounded float32 operation; B = the largest number of slots of a hyperedge,
D = that of a node.  A[v, e] is the sum of a over the columns (v, e); P_a = diag(Dinv) A diag(w Binv) A^T.

  propagation, "count":  a term a_p x_v of Y_e carries one rounding (the product) and meets at most B adds; the scale multiplies are
      two more roundings (Binv_e itself is a rounded reciprocal of an exact count: one; w_e: one).  A term of out_v then carries one
      rounding (the product a_p Y_e), at most D adds, and the scale (Dinv_v: the chain of w has at most D roundings relative for
      positive w, the reciprocal one, the multiply one).  First order, with |P_a| built from |a|:
          |out - P_a x| <= (B + 2 D + 8) eps (|P_a| |x|) (1 + 2^-10)
      (hgconv_restate.bound's count with the two products and the weighted degree's chain written out; second-order terms are below
      2^-10 of the first for B + 2 D + 8 < 2^14, which `bound` checks).
  propagation, "weight":  B_e and D_v are chains of a (resp. a w): for NON-NEGATIVE a each is within (B + 1) eps, resp. (D + 2) eps,
      relatively; `bound` refuses a negative weight in this mode:
          |out - P_a x| <= (2 B + 2 D + 10) eps (|P_a| |x|) (1 + 2^-10)
  grad_a ("count"):  grad_a[p] = dot64(g'_v, Y_e) + dot64(x_v, T_e) with g' = Dinv . G (two roundings per element against the exact
      Dinv G: D + 2 with the degree's chain).  dot64 of C terms: K = ceil(C / 64) + 7 roundings per term (the product, the lane
      chain, six tree levels), plus the last add.  Y and T carry the errors of their own chains:
      |Y - Y64| <= (B + 4) eps |Y|_abs,  |T - T64| <= (B + D + 7) eps |T|_abs  (|.|_abs: the same sums over absolute values), so
          |grad_a - grad_a64| <= ((K + 1 + D + 2 + B + 4) (|g'| . |Y|_abs) + (K + 1 + B + D + 7) (|x| . |T|_abs)) eps (1 + 2^-10)
  softmax:  readout_restate's derivation with one chain level of n_r slots in place of the two levels of chunks: t = score - m is
      off by |t| eps, cexp by 2 CEXP_ULPS eps relatively, the denominator's chain by n_r eps, the divide by one:
          |alpha - alpha64| <= (2 (2 CEXP_ULPS + T_r) + n_r + 2) eps alpha64 (1 + 2^-10) + (n_r + 1) 2^-125
      (T_r = min(max - min of the row's scores, 87); the last term is the flush of rows below -87, as in readout_restate).
  softmax backward:  grad = alpha (g - c), c the chain of alpha g: with rho_r the relative error of alpha above,
          |grad - grad64| <= alpha64 ((rho_r + 3 eps) |g| + (2 rho_r + (n_r + 4) eps) S_r) (1 + 2^-10) + (n_r + 1) 2^-125 (|g| + G_r)
      with S_r = sum over the row of alpha64 |g| and G_r the row's largest |g|.

A plain helper module like the other tests/*_restate.py, not a conftest."""
from __future__ import annotations

import numpy as np

import hgconv_restate as hr
import readout_restate as rr

F32 = np.float32
EPS = 2.0 ** -24
FLUSH = 2.0 ** -125
bits = hr.bits


# ---- the plan with positions ----------------------------------------------------------------------------------------------------------
def csr_pos(rows, cols, columns, R):
    """ptr [R + 1], col [E'], pos [E']: the pairs sorted by (row, col), stable, and the column of edge_index of every slot."""
    order = np.lexsort((cols, rows))                 # stable: equal (row, col) keep their order, which is the column order
    return np.searchsorted(rows[order], np.arange(R + 1), side="left").astype(np.int64), cols[order], columns[order]


def plan(edge_index, N, M, w=None):
    """hgconv_restate.plan plus epos / npos (int64 here; the device holds int32)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    ok = (ei[0] >= 0) & (ei[0] < N) & (ei[1] >= 0) & (ei[1] < M)
    columns = np.nonzero(ok)[0].astype(np.int64)
    v, e = ei[0][ok], ei[1][ok]
    pl = hr.plan(ei, N, M, w)
    eptr, emem, epos = csr_pos(e, v, columns, M)
    nptr, nmem, npos = csr_pos(v, e, columns, N)
    assert np.array_equal(eptr, pl["eptr"]) and np.array_equal(emem, pl["emem"]) and np.array_equal(nptr, pl["nptr"]) and np.array_equal(nmem, pl["nmem"])
    pl.update(epos=epos, npos=npos, E=ei.shape[1], valid=ok)
    return pl


def chain_weighted(ptr, col, pos, a, src):
    """acc[r] = the float32 chain of (a[pos[j]] * src[col[j]]) over j in [ptr[r], ptr[r + 1]); src [S] or [S, C]."""
    src = np.asarray(src, dtype=F32)
    a = np.asarray(a, dtype=F32)
    R = ptr.size - 1
    deg = np.diff(ptr)
    acc = np.zeros((R,) + src.shape[1:], dtype=F32)
    for p in range(int(deg.max()) if R else 0):
        m = np.nonzero(deg > p)[0]
        j = ptr[m] + p
        wt = a[pos[j]]
        term = (wt[:, None] * src[col[j]]) if src.ndim == 2 else (wt * src[col[j]])
        acc[m] = acc[m] + term.astype(F32)
    return acc


def scales(pl, a, normalization):
    """(edge_scale [M], node_scale [N]) float32 of the mode."""
    if normalization == "count":
        return pl["binv"], pl["dinv"]
    assert normalization == "weight"
    a = np.asarray(a, dtype=F32)
    B = chain_weighted(pl["eptr"], pl["emem"], pl["epos"], a, np.ones(pl["N"], dtype=F32))
    D = chain_weighted(pl["nptr"], pl["nmem"], pl["npos"], a, np.ones(pl["M"], dtype=F32) if pl["w"] is None else pl["w"])
    with np.errstate(divide="ignore"):
        es = np.where(B != 0, F32(1.0) / B, F32(0.0)).astype(F32)
        ns = np.where(D != 0, F32(1.0) / D, F32(0.0)).astype(F32)
    return es, ns


def propagate(x, a, edge_index, M, w=None, normalization="count", transpose=False, pl=None):
    """(out [N, C], Y [M, C]) float32.  transpose: x is G, the pre-scale g' = node_scale . G one float32 multiply, no node scale at the
    end; Y is then T."""
    x = np.asarray(x, dtype=F32)
    pl = plan(edge_index, x.shape[0], M, w) if pl is None else pl
    es, ns = scales(pl, a, normalization)
    if transpose:
        x = x * ns[:, None]
    Y = chain_weighted(pl["eptr"], pl["emem"], pl["epos"], a, x) * es[:, None]
    if pl["w"] is not None:
        Y = Y * pl["w"][:, None]
    out = chain_weighted(pl["nptr"], pl["nmem"], pl["npos"], a, Y)
    if not transpose:
        out = out * ns[:, None]
    return out.astype(F32), Y.astype(F32)


def grad_a(x, a, G, edge_index, M, w=None, pl=None):
    """grad_a [E] float32 of the count mode: dot64(g'_v, Y_e) + dot64(x_v, T_e) for the valid columns, 0 for the others."""
    x, G = np.asarray(x, dtype=F32), np.asarray(G, dtype=F32)
    pl = plan(edge_index, x.shape[0], M, w) if pl is None else pl
    _, Y = propagate(x, a, edge_index, M, w, "count", pl=pl)
    _, T = propagate(G, a, edge_index, M, w, "count", transpose=True, pl=pl)
    gp = G * pl["dinv"][:, None]
    ei = np.asarray(edge_index, dtype=np.int64)
    cols = np.nonzero(pl["valid"])[0]
    v, e = ei[0][cols], ei[1][cols]
    out = np.zeros(ei.shape[1], dtype=F32)
    if cols.size:
        out[cols] = rr.dot64(gp[v], Y[e]) + rr.dot64(x[v], T[e])
    return out


# ---- softmax over the slots of a row --------------------------------------------------------------------------------------------------
def softmax(score, ptr, pos, E):
    """alpha [E] float32: per row the exact maximum (-0 < +0), e = cexp(score - max), Z the chain of e in slot order, e / Z."""
    score = np.asarray(score, dtype=F32)
    R = ptr.size - 1
    deg = np.diff(ptr)
    n = int(ptr[-1])
    row = np.repeat(np.arange(R), deg)
    cols = pos[:n]
    keys = np.zeros(R, dtype=np.uint32)
    np.maximum.at(keys, row, rr._key(score[cols]))
    m = rr._unkey(keys)
    e = rr.cexp(score[cols] - m[row]) if n else np.zeros(0, dtype=F32)
    Z = np.zeros(R, dtype=F32)
    for p in range(int(deg.max()) if R else 0):
        k = np.nonzero(deg > p)[0]
        Z[k] = Z[k] + e[ptr[k] + p]
    alpha = np.zeros(E, dtype=F32)
    if n:
        alpha[cols] = e / Z[row]
    return alpha


def softmax_backward(alpha, g, ptr, pos, E):
    alpha, g = np.asarray(alpha, dtype=F32), np.asarray(g, dtype=F32)
    R = ptr.size - 1
    deg = np.diff(ptr)
    n = int(ptr[-1])
    row = np.repeat(np.arange(R), deg)
    cols = pos[:n]
    t = alpha[cols] * g[cols]
    c = np.zeros(R, dtype=F32)
    for p in range(int(deg.max()) if R else 0):
        k = np.nonzero(deg > p)[0]
        c[k] = c[k] + t[ptr[k] + p]
    out = np.zeros(E, dtype=F32)
    if n:
        out[cols] = alpha[cols] * (g[cols] - c[row])
    return out


def group_of(pl, group):
    return (pl["eptr"], pl["epos"]) if group == "edge" else (pl["nptr"], pl["npos"])


# ---- float64 --------------------------------------------------------------------------------------------------------------------------
def dense64(edge_index, a, N, M, w=None, normalization="count", absolute=False):
    """dict(A [N, M], es [M], ns [N], wv [M], P [N, N], B, D): the float64 operator P_a = diag(ns) A diag(wv es) A^T; B, D the largest
    slot counts.  absolute: A from |a| (the bound's |P_a|; the scales stay those of a)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    a = np.asarray(a, dtype=np.float64)
    ok = (ei[0] >= 0) & (ei[0] < N) & (ei[1] >= 0) & (ei[1] < M)
    v, e, av = ei[0][ok], ei[1][ok], a[ok]
    A = np.zeros((N, M))
    np.add.at(A, (v, e), av)
    H = np.zeros((N, M))
    np.add.at(H, (v, e), 1.0)
    wv = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    Bd, Dd = (H.sum(0), H @ wv) if normalization == "count" else (A.sum(0), A @ wv)
    with np.errstate(divide="ignore", invalid="ignore"):
        es = np.where(Bd != 0, 1.0 / Bd, 0.0)
        ns = np.where(Dd != 0, 1.0 / Dd, 0.0)
    if absolute:
        A = np.zeros((N, M))
        np.add.at(A, (v, e), np.abs(av))
        es, ns = np.abs(es), np.abs(ns)
    P = (ns[:, None] * A) @ ((wv * es)[:, None] * A.T)
    return dict(A=A, es=es, ns=ns, wv=wv, P=P, B=int(H.sum(0).max()) if M and N else 0, D=int(H.sum(1).max()) if M and N else 0)


def bound(edge_index, a, x, N, M, w=None, normalization="count", transpose=False):
    """Per element of out (transpose: of grad_x against P_a^T G): the docstring's bound."""
    if normalization == "weight" and (np.asarray(a) < 0).any():
        raise ValueError("bound: the weight mode's bound is derived for non-negative pair weights")
    d = dense64(edge_index, a, N, M, w, normalization, absolute=True)
    k = (d["B"] + 2 * d["D"] + 8) if normalization == "count" else (2 * d["B"] + 2 * d["D"] + 10)
    if k >= 2 ** 14:
        raise ValueError("bound: derived for fewer than 2^14 roundings per term")
    P = d["P"].T if transpose else d["P"]
    return k * EPS * (1 + 2.0 ** -10) * (P @ np.abs(np.asarray(x, dtype=np.float64)))


def grad_a64(edge_index, a, x, G, N, M, w=None):
    """(grad_a64 [E], bound [E]) of the count mode in float64: dL/da_p = g'_v . Y_e + x_v . T_e with L = sum(G * out)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    x, G = np.asarray(x, dtype=np.float64), np.asarray(G, dtype=np.float64)
    d = dense64(ei, a, N, M, w, "count")
    da = dense64(ei, a, N, M, w, "count", absolute=True)
    gp = d["ns"][:, None] * G
    sc = (d["wv"] * d["es"])[:, None]
    Y, T = sc * (d["A"].T @ x), sc * (d["A"].T @ gp)
    Ya, Ta = sc * (da["A"].T @ np.abs(x)), sc * (da["A"].T @ np.abs(gp))
    ok = (ei[0] >= 0) & (ei[0] < N) & (ei[1] >= 0) & (ei[1] < M)
    cols = np.nonzero(ok)[0]
    v, e = ei[0][cols], ei[1][cols]
    want = np.zeros(ei.shape[1])
    tol = np.zeros(ei.shape[1])
    want[cols] = (gp[v] * Y[e]).sum(1) + (x[v] * T[e]).sum(1)
    K = (x.shape[1] + 63) // 64 + 7
    B, D = d["B"], d["D"]
    tol[cols] = ((K + 1 + D + 2 + B + 4) * (np.abs(gp[v]) * Ya[e]).sum(1) + (K + 1 + B + D + 7) * (np.abs(x[v]) * Ta[e]).sum(1)) * EPS * (1 + 2.0 ** -10)
    return want, tol


def softmax64(score, ptr, pos, E):
    """(alpha64 [E], bound [E], rho per slot's column [E]) in float64 on the float32 scores."""
    score = np.asarray(score, dtype=np.float64)
    alpha, tol, rho = np.zeros(E), np.zeros(E), np.zeros(E)
    for r in range(ptr.size - 1):
        c = pos[int(ptr[r]):int(ptr[r + 1])]
        if c.size:
            s = score[c]
            wgt = np.exp(s - s.max())
            al = wgt / wgt.sum()
            T = min(float(s.max() - s.min()), 87.0)
            rel = (2 * (2 * rr.CEXP_ULPS + T) + c.size + 2) * EPS * (1 + 2.0 ** -10)
            alpha[c], rho[c] = al, rel
            tol[c] = rel * al + (c.size + 1) * FLUSH
    return alpha, tol, rho


def softmax_backward64(score, g, ptr, pos, E):
    """(grad64 [E], bound [E]) of alpha = softmax64(score) under L = sum(g * alpha)."""
    g = np.asarray(g, dtype=np.float64)
    alpha, _, rho = softmax64(score, ptr, pos, E)
    grad, tol = np.zeros(E), np.zeros(E)
    for r in range(ptr.size - 1):
        c = pos[int(ptr[r]):int(ptr[r + 1])]
        if c.size:
            cr = float((alpha[c] * g[c]).sum())
            S = float((alpha[c] * np.abs(g[c])).sum())
            grad[c] = alpha[c] * (g[c] - cr)
            tol[c] = alpha[c] * ((rho[c] + 3 * EPS) * np.abs(g[c]) + (2 * rho[c] + (c.size + 4) * EPS) * S) * (1 + 2.0 ** -10) + \
                (c.size + 1) * FLUSH * (np.abs(g[c]) + float(np.abs(g[c]).max()))
    return grad, tol


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------
def pair_weights(E, seed, signed=False):
    rng = np.random.RandomState(seed)
    a = (0.05 + rng.rand(E)).astype(F32)
    if signed:
        a = (a * rng.choice([-1.0, 1.0], size=E)).astype(F32)
    return a


def scores(E, seed, scale=3.0):
    return (scale * np.random.RandomState(seed).randn(E)).astype(F32)


def row_sizes_incidence(sizes=(0, 1, 7, 8, 9, 63, 64, 65, 1000)):
    """Hyperedge i has sizes[i] nodes (0 .. sizes[i] - 1): edge_index [2, sum], N = max size, M = len(sizes)."""
    v, e = [], []
    for i, d in enumerate(sizes):
        v += list(range(d))
        e += [i] * d
    return np.array([v, e], dtype=np.int64), max(sizes), len(sizes)
