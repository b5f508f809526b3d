"""numpy restatement of the attention readout over a ragged batch (include/ext/mmf_hg_readout.h), bit for bit, and
the float64 reference it is compared with.

The operator is torch_geometric's GlobalAttention: inside every segment s (rows ptr[s] .. ptr[s + 1]) a softmax of the gate, then
the gate-weighted sum of the rows of x.  The rule of the header, restated: every product a rounded float32 multiply, every sum a
rounded float32 add (numpy neither fuses nor reorders them), in this order:

    m_s      = max of the segment's gates (-0 < +0)         t_i = gate_i - m_s         e_i = cexp(t_i)
    z_{s,q}  = chain of e_i over the rows of chunk q (CHUNK = 64 rows), ascending;  u_{s,q}[c] = chain of (e_i * x[i, c])
    Z_s      = chain of z_{s,q} over q ascending;                                   U_s[c]     = chain of u_{s,q}[c]
    out[s]   = U_s / Z_s      alpha_i = e_i / Z_s      seg_max[s] = m_s      seg_sum[s] = Z_s

The loops below go over the POSITION inside a chunk (then over the chunk number inside a segment) and add, for every chunk that has
such a row, that row's term: one rounded add per chunk and step, so each chain is sequential by construction.

The bound.  With eps = 2^-24 (the relative error of one rounded float32 operation), per segment with n_s rows in Q_s chunks:
  * t_i = fl(gate_i - m_s) is off by at most |t_i| eps, which e_i sees as a relative error of at most min(|t_i|, 87) eps =: T eps
    (rows with t_i < -87 are flushed: below);
  * cexp is within CEXP_ULPS ulps of exp; an ulp of y is at most 2 eps y, so that is a relative error of at most 2 CEXP_ULPS eps;
  * the product e_i * x is one rounding; a term of the numerator then meets at most 63 adds inside its chunk and Q_s on the second
    level (the add that takes the chunk's partial in, and Q_s - 1 after it), a term of the denominator the same;
  * the divide is one rounding.
To first order a term of the numerator is off by (2 CEXP_ULPS + T + 1 + 63 + Q_s) eps relatively, the denominator by
(2 CEXP_ULPS + T + 63 + Q_s) eps, the quotient by their sum plus one:

    |out - out64| <= 2 (2 CEXP_ULPS + T_s + 64 + Q_s + 4) eps (alpha64 @ |x|) (1 + 2^-10)  +  2 n_s 2^-125 max|x|

(the 4 rounds the constants up; 1 + 2^-10 covers the terms of second order, which are below 2^-12 of the first for every Q_s < 2^10
and are checked to be so: `bound` refuses a larger Q_s).  The last term is the flush: a row with t_i < -87 gets e_i = +0 where
exp(t_i) <= exp(-87) < 2^-125, and Z_s >= 1 (the row of the maximum has e = 1), so the rows left out change the numerator by at most
n_s 2^-125 max|x| and the denominator by at most n_s 2^-125 relatively.

A plain helper module like the other tests/*_restate.py, not a conftest."""
from __future__ import annotations

import numpy as np

F32 = np.float32
CHUNK = 64
# The largest error of cexp over EVERY float32 in [-87, 0] against float64 exp, in ulps of the correctly rounded result, rounded up
# to the next half ulp (scripts/readout_exp_sweep.py; DESIGN.md §4.36 has the figure of the sweep).
CEXP_ULPS = 1.5

LOG2E = F32(1.4426950408889634)
LN2_HI = F32(0.693145751953125)
LN2_LO = F32(1.428606765330187e-06)
COEF = [F32(1.0), F32(1.0), F32(1.0 / 2), F32(1.0 / 6), F32(1.0 / 24), F32(1.0 / 120), F32(1.0 / 720), F32(1.0 / 5040)]


def cexp(t):
    """The header's canonical exponential for finite t <= 0, float32 in and out."""
    t = np.asarray(t, dtype=F32)
    tt = np.maximum(t, F32(-87.0))                     # the flushed rows are overwritten below; this keeps the shift in range
    n = np.rint(tt * LOG2E).astype(F32)
    r = (tt - n * LN2_HI) - n * LN2_LO
    p = np.full(t.shape, COEF[7], dtype=F32)
    for k in range(6, -1, -1):
        p = p * r
        p = p + COEF[k]
    scale = ((n.astype(np.int32) + 127) << 23).astype(np.int32).view(F32)
    return np.where(t < F32(-87.0), F32(0.0), p * scale).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _key(g):
    """The order-preserving unsigned key of a float32 (-0 < +0)."""
    u = bits(g).astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def chunk_table(ptr):
    """(segment id, first row) of every chunk, segments ascending, chunks ascending inside a segment: int32 [num_chunks, 2]."""
    ptr = np.asarray(ptr, dtype=np.int64)
    recs = [(s, r) for s in range(ptr.size - 1) for r in range(int(ptr[s]), int(ptr[s + 1]), CHUNK)]
    return np.array(recs, dtype=np.int32).reshape(-1, 2)


def forward(x, gate, ptr):
    """(out [S, C], alpha [N], seg_max [S], seg_sum [S]) float32, with the bits of the header's rule."""
    x = np.asarray(x, dtype=F32)
    gate = np.asarray(gate, dtype=F32).reshape(-1)
    ptr = np.asarray(ptr, dtype=np.int64)
    N, C = x.shape
    S = ptr.size - 1
    n = np.diff(ptr)
    seg = np.repeat(np.arange(S), n)
    keys = np.zeros(S, dtype=np.uint32)
    np.maximum.at(keys, seg, _key(gate))
    m = np.where(n > 0, _unkey(keys), F32(-np.inf)).astype(F32)
    e = cexp(gate - m[seg]) if N else np.zeros(0, dtype=F32)
    tab = chunk_table(ptr)
    Q = tab.shape[0]
    cseg, crow = tab[:, 0].astype(np.int64), tab[:, 1].astype(np.int64)
    cnt = np.minimum(ptr[cseg + 1] - crow, CHUNK) if Q else np.zeros(0, dtype=np.int64)
    z = np.zeros(Q, dtype=F32)
    u = np.zeros((Q, C), dtype=F32)
    for j in range(int(cnt.max()) if Q else 0):
        k = np.nonzero(cnt > j)[0]
        i = crow[k] + j
        z[k] = z[k] + e[i]
        u[k] = u[k] + e[i][:, None] * x[i]
    nq = (n + CHUNK - 1) // CHUNK
    first = np.concatenate([[0], np.cumsum(nq)])[:-1]
    Z = np.zeros(S, dtype=F32)
    U = np.zeros((S, C), dtype=F32)
    for q in range(int(nq.max()) if S else 0):
        k = np.nonzero(nq > q)[0]
        Z[k] = Z[k] + z[first[k] + q]
        U[k] = U[k] + u[first[k] + q]
    out = np.zeros((S, C), dtype=F32)
    live = n > 0
    out[live] = U[live] / Z[live][:, None]
    alpha = (e / Z[seg]).astype(F32) if N else np.zeros(0, dtype=F32)
    return out, alpha, m, Z


def dot64(a, b):
    """The header's dot64 of the rows of a and b [R, C]: 64 lane partials (chains over c = l, l + 64, ...), then the halving tree."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    R, C = a.shape
    p = np.zeros((R, 64), dtype=F32)
    for c0 in range(0, C, 64):
        w = min(64, C - c0)
        p[:, :w] = p[:, :w] + a[:, c0:c0 + w] * b[:, c0:c0 + w]
    h = 32
    while h >= 1:
        p[:, :h] = p[:, :h] + p[:, h:2 * h]
        h //= 2
    return p[:, 0].copy()


def backward(x, ptr, alpha, out, grad_out):
    """(grad_x [N, C], grad_gate [N]) float32 from the forward's alpha and out and G = grad_out [S, C]."""
    x, alpha, out, G = (np.asarray(v, dtype=F32) for v in (x, alpha, out, grad_out))
    ptr = np.asarray(ptr, dtype=np.int64)
    seg = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    Gi = G[seg]
    gx = alpha[:, None] * Gi
    d = dot64(Gi, x)
    r = dot64(G, out)
    return gx.astype(F32), (alpha * (d - r[seg])).astype(F32)


# ---- float64: torch_geometric's formula -----------------------------------------------------------------------------------------------
def reference64(x, gate, ptr):
    """(out64 [S, C], alpha64 [N]): softmax(gate, batch) and scatter-add of alpha * x, in float64 on the float32 inputs."""
    x = np.asarray(x, dtype=np.float64)
    gate = np.asarray(gate, dtype=np.float64).reshape(-1)
    ptr = np.asarray(ptr, dtype=np.int64)
    S = ptr.size - 1
    out = np.zeros((S, x.shape[1]))
    alpha = np.zeros(x.shape[0])
    for s in range(S):
        a, b = int(ptr[s]), int(ptr[s + 1])
        if b > a:
            w = np.exp(gate[a:b] - gate[a:b].max())
            alpha[a:b] = w / w.sum()
            out[s] = alpha[a:b] @ x[a:b]
    return out, alpha


def backward64(x, gate, ptr, grad_out):
    """The analytic gradient of reference64 in float64: (grad_x, grad_gate)."""
    x = np.asarray(x, dtype=np.float64)
    G = np.asarray(grad_out, dtype=np.float64)
    ptr = np.asarray(ptr, dtype=np.int64)
    out, alpha = reference64(x, gate, ptr)
    seg = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    gx = alpha[:, None] * G[seg]
    gg = alpha * ((G[seg] * x).sum(1) - (G * out).sum(1)[seg])
    return gx, gg


EPS = 2.0 ** -24
FLUSH = 2.0 ** -125


def _segment_terms(gate, ptr):
    """Per segment: rows, chunks, T_s = the largest min(|t_i|, 87)."""
    gate = np.asarray(gate, dtype=np.float64).reshape(-1)
    ptr = np.asarray(ptr, dtype=np.int64)
    n = np.diff(ptr)
    q = (n + CHUNK - 1) // CHUNK
    if int(q.max(initial=0)) >= 2 ** 10:
        raise ValueError("bound: derived for fewer than 2^10 chunks per segment")
    T = np.zeros(ptr.size - 1)
    for s in range(ptr.size - 1):
        g = gate[int(ptr[s]):int(ptr[s + 1])]
        if g.size:
            T[s] = min(float(g.max() - g.min()), 87.0)
    return n, q, T


def alpha_rel(gate, ptr):
    """Per segment: the relative error of alpha_i = e_i / Z_s (a row that is not flushed) — numerator one e, no chain."""
    n, q, T = _segment_terms(gate, ptr)
    return (2 * (2 * CEXP_ULPS + T) + 64 + q + 4) * EPS * (1 + 2.0 ** -10)


def bound(x, gate, ptr):
    """Per element of out [S, C]: the docstring's bound."""
    x = np.asarray(x, dtype=np.float64)
    n, q, T = _segment_terms(gate, ptr)
    _, alpha = reference64(x, gate, ptr)
    ax = np.zeros((ptr.size - 1, x.shape[1]))
    np.add.at(ax, np.repeat(np.arange(ptr.size - 1), n), alpha[:, None] * np.abs(x))
    xmax = float(np.abs(x).max(initial=0.0))
    return 2 * (2 * CEXP_ULPS + T + 64 + q + 4)[:, None] * EPS * (1 + 2.0 ** -10) * ax + (2 * n * FLUSH * xmax)[:, None]


def bound_backward(x, gate, ptr, grad_out):
    """(per element of grad_x, per element of grad_gate), derived the same way.
    grad_x[i, c] = alpha_i * G[s, c]: alpha's relative error rho_s (alpha_rel) and one multiply, plus 2^-125 |G| for a flushed row.
    grad_gate_i = alpha_i * (d_i - r_s): dot64 of C terms is a chain of ceil(C / 64) adds and 6 tree levels on rounded products,
    K = ceil(C / 64) + 7 roundings per term; r_s also carries the error of out (bound); the subtract and the multiply are two more
    roundings on |d_i| + |r_s| <= |G_s| . |x_i| + |G_s| . |out_s|; alpha_i adds rho_s on the same magnitude."""
    x = np.asarray(x, dtype=np.float64)
    G = np.abs(np.asarray(grad_out, dtype=np.float64))
    ptr = np.asarray(ptr, dtype=np.int64)
    n = np.diff(ptr)
    seg = np.repeat(np.arange(ptr.size - 1), n)
    out, alpha = reference64(x, gate, ptr)
    rho = alpha_rel(gate, ptr)[seg]
    tol_x = (rho + 2 * EPS)[:, None] * alpha[:, None] * G[seg] + FLUSH * (n[seg][:, None] + 1) * G[seg]
    K = (x.shape[1] + 63) // 64 + 7
    mag = (G[seg] * np.abs(x)).sum(1) + (G * np.abs(out)).sum(1)[seg]
    err_out = (G * bound(x, gate, ptr)).sum(1)[seg]
    tol_g = alpha * (1 + rho) * ((K + 2) * EPS * mag * (1 + 2.0 ** -10) + err_out) + rho * alpha * mag + FLUSH * (n[seg] + 1) * mag
    return tol_x, tol_g


# ---- the seeded inputs of tests/test_readout_cpu.py and tests/test_gpu_readout.py -----------------------------------------------------
EDGE_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 0, 1000, 7)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def features(N, C, seed):
    return np.random.RandomState(seed).randn(N, C).astype(F32)


def gates(N, seed, scale=3.0):
    return (scale * np.random.RandomState(seed).randn(N)).astype(F32)


def ragged_sizes(S, total, seed):
    """S sizes that add up to `total`, some of them 0."""
    rng = np.random.RandomState(seed)
    sizes = np.diff(np.concatenate([[0], np.sort(rng.randint(0, total + 1, size=S - 1)), [total]])).astype(np.int64)
    for s in (3, S - 1):                                                      # two empty segments, their rows go to segment 0
        sizes[0] += sizes[s]
        sizes[s] = 0
    return sizes
