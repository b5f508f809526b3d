"""numpy restatement of the 16-bit hypergraph branch (include/ext/mmf_hg_hg16.h), bit for bit: 16-bit storage,
float32 arithmetic, one round-to-nearest-even per stored tensor.  Every operation is a composition of tests/hgconv_restate.py,
tests/hgpair_restate.py and tests/readout_restate.py (imported, not edited) with ``r16``.

A 16-bit tensor is held here as a float32 array whose every value is representable in the 16-bit type (``r16`` returns such an
array; ``r16_bits`` the uint16 patterns, ``widen`` the way back).  kind is "bf16" or "f16".

    r16, bf16   on the bits u of the float32:  (u + 0x7fff + ((u >> 16) & 1)) >> 16
    r16, f16    on the bits too: for |f| >= 2^-14 the same add-and-shift on the rebased exponent (the carry runs into the exponent
                and into infinity; anything past it is infinity), below 2^-14 the 24-bit significand shifted right by 126 - e with
                round-to-nearest-even: subnormals are kept

The bounds against float64.  u16 = 2^-8 (bf16) or 2^-11 (f16) is the relative error of one r16 of a value in the type's normal range;
eta = 2^-25 is the absolute error of one r16 into f16's subnormal range (half the spacing 2^-24), 0 for bf16 on data kept in the
normal range.  With P the dense operator, S2 the matrix of the second step (Dinv H, or H for the transposed form; with pair weights
|ns| |A| or |A|) and b32 the float32 bound of the restatement underneath (hgconv_restate.bound / hgpair_restate.bound):
    Y16 = Y32 (1 + d1) + e1,  |d1| <= u16, |e1| <= eta.  The second step on Y16 makes float32 errors relative to |Y16| <= |Y| (1 + u16),
    and carries d1 and e1 through S2; out16 = out32' (1 + d2) + e2.  So
        |out16 - P x| <= b32 (1 + u16)^2 + ((1 + u16)^2 - 1) |P| |x| + eta ((1 + u16) rowsum|S2| + 1)
    — to first order b32 + 2 u16 |P||x| + eta (rowsum|S2| + 1).  A bias adds one float32 rounding of (|out| + |bias|) before the r16:
        + 2^-24 (|P||x| + |bias|) (1 + u16) + u16 |bias|
    grad_a: Y16 and T16 each carry one r16, the two dot64 are float32 on the widened rows (hgpair_restate.grad_a64's tolerance t32):
        |grad_a16 - grad_a64| <= t32 (1 + u16) + u16 (|g'| . |Y|_abs + |x| . |T|_abs) + eta (sum |g'| + sum |x|)
    readout: out and alpha are float32 results on the widened x — readout_restate's own bounds; grad_x16 = r16(alpha G):
        |grad_x16 - grad_x64| <= t32 (1 + u16) + u16 |grad_x64| + eta

A plain helper module like the other tests/*_restate.py, not a conftest."""
from __future__ import annotations

import numpy as np

import hgconv_restate as hr
import hgpair_restate as hp
import readout_restate as rr

F32 = np.float32
KINDS = ("bf16", "f16")
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
ETA = {"bf16": 0.0, "f16": 2.0 ** -25}
bits = hr.bits


# ---- widen, r16 -----------------------------------------------------------------------------------------------------------------------
def r16_bits(f, kind):
    """uint16 patterns of round-to-nearest-even of the finite float32 array f."""
    u = bits(f).astype(np.uint64)                    # 64-bit so that no add below wraps
    if kind == "bf16":
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert kind == "f16"
    sign = ((u >> 16) & 0x8000).astype(np.uint64)
    au = u & 0x7FFFFFFF
    e = (au >> 23).astype(np.int64)
    # normal results: rebase the exponent (127 -> 15), round the 13 bits that fall off, the carry runs on; past infinity is infinity
    normal = np.minimum(((au - 0x38000000 + 0xFFF + ((au >> 13) & 1)) >> 13) if au.size else au, 0x7C00)
    # subnormal results (|f| < 2^-14): the significand with its hidden bit, shifted right by s = 126 - e, ties to even
    s = np.clip(126 - e, 14, 25).astype(np.uint64)   # s = 25 (e < 102): everything rounds to 0 (the significand is below half)
    m = (au & 0x7FFFFF) | 0x800000
    m = np.where(e == 0, 0, m)                       # float32 zero and subnormals: far below half of 2^-24
    q = m >> s
    rem = m & ((np.uint64(1) << s) - 1)
    half = np.uint64(1) << (s - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1))).astype(np.uint64)
    h = np.where(au >= 0x38800000, normal, q)
    return (sign | h).astype(np.uint16)


def widen(b, kind):
    """The float32 array of the uint16 patterns b: exact."""
    b = np.asarray(b, dtype=np.uint16)
    if kind == "bf16":
        return (b.astype(np.uint32) << 16).view(F32)
    return b.view(np.float16).astype(F32)


def r16(f, kind):
    """f rounded to the 16-bit type, as a float32 array."""
    f = np.ascontiguousarray(f, dtype=F32)
    return widen(r16_bits(f, kind), kind).reshape(f.shape)


# ---- propagation ----------------------------------------------------------------------------------------------------------------------
def propagate16(x, edge_index, M, kind, w=None, bias=None, transpose=False):
    """(out [N, C], Y [M, C]): hgconv_restate.propagate with Y rounded once before the node step reads it and out rounded once, after
    the bias.  transpose: x is G as it is (16-bit); the product with Dinv is the float32 multiply of the hyperedge step."""
    x = np.asarray(x, dtype=F32)
    pl = hr.plan(edge_index, x.shape[0], M, w)
    src = x * pl["dinv"][:, None] if transpose else x
    Y = hr.chain_sum(pl["eptr"], pl["emem"], src) * pl["binv"][:, None]
    if w is not None:
        Y = Y * pl["w"][:, None]
    Y = r16(Y, kind)
    out = hr.chain_sum(pl["nptr"], pl["nmem"], Y)
    if not transpose:
        out = out * pl["dinv"][:, None]
        if bias is not None:
            out = out + np.asarray(bias, dtype=F32)[None, :]
    return r16(out, kind), Y


def propagate_pairs16(x, a, edge_index, M, kind, w=None, normalization="count", bias=None, transpose=False, pl=None):
    """(out, Y): hgpair_restate.propagate with the same two roundings."""
    x = np.asarray(x, dtype=F32)
    pl = hp.plan(edge_index, x.shape[0], M, w) if pl is None else pl
    es, ns = hp.scales(pl, a, normalization)
    src = x * ns[:, None] if transpose else x
    Y = hp.chain_weighted(pl["eptr"], pl["emem"], pl["epos"], a, src) * es[:, None]
    if pl["w"] is not None:
        Y = Y * pl["w"][:, None]
    Y = r16(Y, kind)
    out = hp.chain_weighted(pl["nptr"], pl["nmem"], pl["npos"], a, Y)
    if not transpose:
        out = out * ns[:, None]
        if bias is not None:
            out = out + np.asarray(bias, dtype=F32)[None, :]
    return r16(out, kind), Y


def grad_a16(x, a, G, edge_index, M, kind, w=None):
    """grad_a [E] float32 of the count mode from the 16-bit x and G: dot64(g'_v, Y16_e) + dot64(x_v, T16_e), g' = G * Dinv."""
    x, G = np.asarray(x, dtype=F32), np.asarray(G, dtype=F32)
    pl = hp.plan(edge_index, x.shape[0], M, w)
    _, Y = propagate_pairs16(x, a, edge_index, M, kind, w, "count", pl=pl)
    _, T = propagate_pairs16(G, a, edge_index, M, kind, w, "count", transpose=True, pl=pl)
    gp = G * pl["dinv"][:, None]
    ei = np.asarray(edge_index, dtype=np.int64)
    cols = np.nonzero(pl["valid"])[0]
    v, e = ei[0][cols], ei[1][cols]
    out = np.zeros(ei.shape[1], dtype=F32)
    if cols.size:
        out[cols] = rr.dot64(gp[v], Y[e]) + rr.dot64(x[v], T[e])
    return out


# ---- readout --------------------------------------------------------------------------------------------------------------------------
def readout16(x, gate, ptr):
    """(out, alpha, seg_max, seg_sum) float32: readout_restate.forward on the widened x (x holds 16-bit values already)."""
    return rr.forward(x, gate, ptr)


def readout_backward16(x, ptr, alpha, out, grad_out, kind):
    """(grad_x in the 16-bit type, grad_gate float32)."""
    gx, gg = rr.backward(x, ptr, alpha, out, grad_out)
    return r16(gx, kind), gg


# ---- bounds against float64 -----------------------------------------------------------------------------------------------------------
def _wrap(b32, mag, s2_rowsum, kind, bias=None):
    u, eta = U16[kind], ETA[kind]
    tol = b32 * (1 + u) ** 2 + ((1 + u) ** 2 - 1) * mag + eta * ((1 + u) * s2_rowsum[:, None] + 1)
    if bias is not None:
        ab = np.abs(np.asarray(bias, dtype=np.float64))[None, :]
        tol = tol + 2.0 ** -24 * (mag + ab) * (1 + u) + u * ab
    return tol


def bound16(edge_index, x, N, M, kind, w=None, bias=None, transpose=False):
    """(P x [+ bias] in float64, bound) of propagate16's out — transpose: of P^T x."""
    P, B, D = hr.dense_operator(edge_index, N, M, w)
    v, e = hr.valid_pairs(edge_index, N, M)
    H = np.zeros((N, M))
    np.add.at(H, (v, e), 1.0)
    x64 = np.asarray(x, dtype=np.float64)
    if transpose:
        P = P.T
        s2 = H.sum(1)
    else:
        wv = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
        Dd = H @ wv
        with np.errstate(divide="ignore"):
            s2 = np.where(Dd != 0, 1.0 / Dd, 0.0) * H.sum(1)
    want = P @ x64 + (0.0 if bias is None else np.asarray(bias, dtype=np.float64)[None, :])
    return want, _wrap(hr.bound(P, x, B, D), np.abs(P) @ np.abs(x64), s2, kind, bias)


def bound_pairs16(edge_index, a, x, N, M, kind, w=None, normalization="count", bias=None, transpose=False):
    d = hp.dense64(edge_index, a, N, M, w, normalization)
    da = hp.dense64(edge_index, a, N, M, w, normalization, absolute=True)
    x64 = np.asarray(x, dtype=np.float64)
    P, Pa = (d["P"].T, da["P"].T) if transpose else (d["P"], da["P"])
    s2 = da["A"].sum(1) * (1.0 if transpose else da["ns"])
    want = P @ x64 + (0.0 if bias is None else np.asarray(bias, dtype=np.float64)[None, :])
    return want, _wrap(hp.bound(edge_index, a, x, N, M, w, normalization, transpose), Pa @ np.abs(x64), s2, kind, bias)


def grad_a_bound16(edge_index, a, x, G, N, M, kind, w=None):
    """(grad_a64, bound) of grad_a16."""
    u, eta = U16[kind], ETA[kind]
    want, t32 = hp.grad_a64(edge_index, a, x, G, N, M, w)
    ei = np.asarray(edge_index, dtype=np.int64)
    x64, G64 = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(G, dtype=np.float64))
    da = hp.dense64(ei, a, N, M, w, "count", absolute=True)
    gp = da["ns"][:, None] * G64
    sc = (da["wv"] * da["es"])[:, None]
    Ya, Ta = sc * (da["A"].T @ x64), sc * (da["A"].T @ gp)
    ok = (ei[0] >= 0) & (ei[0] < N) & (ei[1] >= 0) & (ei[1] < M)
    cols = np.nonzero(ok)[0]
    v, e = ei[0][cols], ei[1][cols]
    tol = t32 * (1 + u)
    tol[cols] += u * ((gp[v] * Ya[e]).sum(1) + (x64[v] * Ta[e]).sum(1)) + eta * (gp[v].sum(1) + x64[v].sum(1))
    return want, tol


def readout_grad_x_bound16(x, gate, ptr, grad_out, kind):
    """(grad_x64, bound) of readout_backward16's grad_x."""
    gx64, _ = rr.backward64(x, gate, ptr, grad_out)
    t32, _ = rr.bound_backward(x, gate, ptr, grad_out)
    return gx64, t32 * (1 + U16[kind]) + U16[kind] * np.abs(gx64) + ETA[kind]


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------
def features16(N, C, seed, kind):
    """hgconv_restate.features rounded to the 16-bit type (float32 array)."""
    return r16(hr.features(N, C, seed), kind)


def rounding_values():
    """Finite float32 values at every tie and boundary of both types: halfway points with even and odd neighbours, the bf16 pairs of
    the GPU test, the f16 subnormal range (ties, the smallest subnormal, half of it, just above half), the largest f16 and the
    overflow threshold 65520, the carry into the next binade, both zeros."""
    v = [0.0, -0.0, 1.0, 1.00390625, 1.01171875, 1.0078125, 1.015625, 1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -9, 1.0 + 2.0 ** -12, 1.0 + 3 * 2.0 ** -12,
         1.0 + 2.0 ** -9 + 2.0 ** -20, 1.0 + 2.0 ** -12 - 2.0 ** -23, 1.99609375, 1.998046875, 1.9999, 2.0 - 2.0 ** -12, 2.0 - 2.0 ** -9,
         65504.0, 65519.99, 65520.0, 65520.01, 65536.0, 60000.0, 1.0e5, 3.0e38, 3.3895313892515355e38, 3.3961775292304e38,
         2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 2.0 ** -25 - 2.0 ** -40, 3 * 2.0 ** -25,
         5 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -20 + 2.0 ** -25, 2.0 ** -20 + 3 * 2.0 ** -25, 1023.5 * 2.0 ** -24, 1022.5 * 2.0 ** -24, 2.0 ** -100, 1.5 * 2.0 ** -100,
         2.0 ** -126]
    v = np.array(v, dtype=F32)
    return np.concatenate([v, -v])
