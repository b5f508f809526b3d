"""numpy restatement of hypergraph propagation out = D^-1 H W B^-1 H^T x (include/ext/mmf_hg_hgconv.h), bit for bit.

Every sum runs over the pairs of its row sorted by the other id ascending (a stable sort; duplicates adjacent) as a sequential float32
chain: the loop below goes over the MEMBER POSITION p and adds, for every row that has a p-th member, that member's term — one
rounded float32 add per row and step, so the chain is sequential by construction (numpy neither fuses nor reorders it).

A plain helper module like the other tests/*_restate.py, not a conftest."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def valid_pairs(edge_index, N, M):
    """The columns whose node id lies in [0, N) and whose hyperedge id lies in [0, M): (nodes, edges)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    ok = (ei[0] >= 0) & (ei[0] < N) & (ei[1] >= 0) & (ei[1] < M)
    return ei[0][ok], ei[1][ok]


def csr(rows, cols, R):
    """ptr int64 [R + 1], col int64 [E]: the pairs sorted by (row, col) — the members of a row ascending, duplicates adjacent."""
    order = np.lexsort((cols, rows))                 # stable, last key first
    rows, cols = rows[order], cols[order]
    return np.searchsorted(rows, np.arange(R + 1), side="left").astype(np.int64), cols


def chain_sum(ptr, col, src):
    """acc[r] = the float32 chain of src[col[j]] over j in [ptr[r], ptr[r + 1]); src [S] or [S, C]."""
    src = np.asarray(src, dtype=F32)
    R = ptr.size - 1
    deg = np.diff(ptr)
    acc = np.zeros((R,) + src.shape[1:], dtype=F32)
    for p in range(int(deg.max()) if R else 0):
        m = np.nonzero(deg > p)[0]
        acc[m] = acc[m] + src[col[ptr[m] + p]]
    return acc


def plan(edge_index, N, M, w=None):
    v, e = valid_pairs(edge_index, N, M)
    eptr, emem = csr(e, v, M)
    nptr, nmem = csr(v, e, N)
    B = np.diff(eptr)
    with np.errstate(divide="ignore"):
        binv = np.where(B > 0, F32(1.0) / B.astype(F32), F32(0.0)).astype(F32)
        D = chain_sum(nptr, nmem, np.ones(M, dtype=F32) if w is None else np.asarray(w, dtype=F32))
        dinv = np.where(D != 0, F32(1.0) / D, F32(0.0)).astype(F32)
    return dict(eptr=eptr, emem=emem, nptr=nptr, nmem=nmem, binv=binv, dinv=dinv, w=None if w is None else np.asarray(w, dtype=F32),
                N=N, M=M)


def propagate(x, edge_index, M, w=None, transpose=False):
    """(out [N, C], Y [M, C]) float32.  transpose: P^T x = H (W Binv) H^T (Dinv . x), the pre-scale one float32 multiply."""
    x = np.asarray(x, dtype=F32)
    pl = plan(edge_index, x.shape[0], M, w)
    if transpose:
        x = x * pl["dinv"][:, None]
    Y = chain_sum(pl["eptr"], pl["emem"], x) * pl["binv"][:, None]
    if w is not None:
        Y = Y * pl["w"][:, None]
    out = chain_sum(pl["nptr"], pl["nmem"], Y)
    if not transpose:
        out = out * pl["dinv"][:, None]
    return out.astype(F32), Y.astype(F32)


def dense_operator(edge_index, N, M, w=None):
    """P = Dinv H W Binv H^T in float64, [N, N]; H counts a pair as often as it occurs.  Also (max B_e, max node degree)."""
    v, e = valid_pairs(edge_index, N, M)
    H = np.zeros((N, M), dtype=np.float64)
    np.add.at(H, (v, e), 1.0)
    wv = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    B = H.sum(0)
    D = H @ wv
    with np.errstate(divide="ignore", invalid="ignore"):
        binv = np.where(B > 0, 1.0 / B, 0.0)
        dinv = np.where(D != 0, 1.0 / D, 0.0)
    P = (dinv[:, None] * H) @ ((wv * binv)[:, None] * H.T)
    return P, int(B.max()) if M else 0, int(H.sum(1).max()) if N else 0


def bound(P, x, max_b, max_deg):
    """Per element: (max B_e + max D-degree + 4) 2^-24 (|P| @ |x|) — two sequential chains plus the roundings of the two reciprocals
    and the two scales; P is non-negative for non-negative weights."""
    return (max_b + max_deg + 4) * 2.0 ** -24 * (np.abs(P) @ np.abs(np.asarray(x, dtype=np.float64)))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- the inputs of tests/test_gpu_hgconv.py (seeded; built once per process) ---------------------------------------------------------
def random_incidence(N, M, E, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, N, size=E), rng.randint(0, M, size=E)]).astype(np.int64)


def features(N, C, seed):
    return np.random.RandomState(seed).randn(N, C).astype(F32)


def weights(M, seed):
    return (0.25 + np.random.RandomState(seed).rand(M)).astype(F32)


def hub_incidence(N=1200, M=1100):
    """Hyperedge 0 holds nodes 0 .. 999 (degree 1000); node 5 sits in hyperedges 0 .. 1001 (degree 1002); every other node i has
    the hyperedge i % M of its own next to it: rows of degree 1 and 2 beside the two hubs."""
    v = list(range(1000)) + [5] * 1001 + list(range(1000, N))
    e = [0] * 1000 + list(range(1, 1002)) + [i % M for i in range(1000, N)]
    return np.array([v, e], dtype=np.int64)


def degree_incidence(degrees=(7, 8, 9, 63, 64, 65)):
    """Hyperedge i has degrees[i] nodes; node j then sits in the hyperedges with degree > j: node degrees 6 .. 1."""
    v, e = [], []
    for i, d in enumerate(degrees):
        v += list(range(d))
        e += [i] * d
    # and the same degrees on the node side: node 100 + i sits in degrees[i] hyperedges of their own
    for i, d in enumerate(degrees):
        v += [100 + i] * d
        e += list(range(10 + 70 * i, 10 + 70 * i + d))
    return np.array([v, e], dtype=np.int64)
