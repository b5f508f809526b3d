"""TEST INFRASTRUCTURE ONLY — numpy restatement of the 16-bit scan's operand image and error margin.

What is restated is the contract of ``prep_half_kernel`` and of the margin block at the top of ``scan_b16x_kernel``
(multimodal-fusion_amd/csrc/mmf_scan_bf16.hip), the way ``oracle/kmeans_restate.py`` restates KMeans:

  * canonical row scalars: n_i = k-ordered f32 fmaf chain of x_i with itself (csrc/mmf_prep.hip), the clamped norm
    ``max(sqrtf(n_i), 1e-8)`` for cosine;
  * the common power-of-two scale that puts the largest norm of BOTH operands into [256, 512) (256 for cosine);
  * u = x * scale (cosine: ``(x / clamped_norm) * scale``, two f32 operations in that order), z = round_16(u) to f16, or to
    bf16 with round-to-nearest-even;
  * zn, rn, un = (1 + 1e-4) * norms of z, of z - u and of u; cb = -n_i scale^2 / 2 for the L2 metrics, 0 otherwise;
  * the four maxima of a side: max zn, max rn, max un, max |cb|;
  * per query row e1, e2 and margin = 2 (e1 + e2) * 1.001 + 1e-30 with the candidate side's maxima.

The kernel takes the three norms from lane-striped f32 fmaf sums and a butterfly; here the sums are float64 and rounded
once, so zn / rn / un and everything derived from them agree with the device to rounding (1e-5 relative is what
tests/test_gpu_scan16_adversarial.py pins), while z and cb are the same bits.

`approx_values` (G) and `target_values` (Q) are the two quantities the header's argument relates, in float64.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

DOT, COSINE, NEG_SQ_L2, RBF = "dot", "cosine", "neg_sq_l2", "rbf"
UP = np.float32(1.0) + np.float32(1e-4)
EPS24 = np.float32(5.9604645e-8)          # 2^-24


def padded_dim(d: int) -> int:
    for dp in (128, 256, 512, 1024):
        if d <= dp:
            return dp
    raise ValueError(f"d = {d} is not supported by the 16-bit scan")


def list_capacity(kk: int) -> int:
    """Entries of a lane list for kk = k + self: 15 up to 11, 16 up to 20, 32 (5 slot bits) up to 44."""
    if kk <= 11:
        return 15
    if kk <= 20:
        return 16
    if kk <= 44:
        return 32
    raise ValueError(f"k + self = {kk} is not supported by the 16-bit scan")


def sq_norms(X: np.ndarray) -> np.ndarray:
    """n_i: the canonical k-ordered f32 fmaf chain (the product of two f32 is exact in float64; one rounding per step)."""
    X = np.ascontiguousarray(X, np.float32)
    acc = np.zeros(X.shape[0], np.float32)
    X64 = X.astype(np.float64)
    for k in range(X.shape[1]):
        acc = (X64[:, k] * X64[:, k] + acc.astype(np.float64)).astype(np.float32)
    return acc


def row_scalars(X: np.ndarray, metric: str) -> np.ndarray:
    n = sq_norms(X)
    if metric != COSINE:
        return n
    a = np.sqrt(n)                       # f32 in, f32 out: correctly rounded
    return np.where(a > np.float32(1e-8), a, np.float32(1e-8)).astype(np.float32)


def common_scale(max_sq_norm: float, metric: str) -> np.float32:
    mx = np.float32(1.0) if metric == COSINE else np.sqrt(np.float32(max_sq_norm))
    if mx > 0 and np.isfinite(mx):
        ex = int(np.frexp(mx)[1])
    else:
        ex = 9
    e = min(max(9 - ex, -100), 100)
    return np.float32(np.ldexp(np.float32(1.0), e))


def round_bf16(u: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even to bf16; returns the uint16 patterns."""
    b = np.ascontiguousarray(u, np.float32).view(np.uint32)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    r = np.where(nan, (b >> np.uint32(16)) | np.uint32(0x0040), r)
    return r.astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def operands(X: np.ndarray, metric: str, operand: str, max_sq_norm: Optional[float] = None) -> Dict[str, np.ndarray]:
    """One side's image.  operand: "f16" / "bf16".  max_sq_norm: the largest n_i over BOTH operands of the call (default:
    this side's own).  Returns scal, scale, u, z (f32 values), zbits (uint16 [n, padded dim]), zn, rn, un, cb, maxima."""
    X = np.ascontiguousarray(X, np.float32)
    n, d = X.shape
    dp = padded_dim(d)
    scal = row_scalars(X, metric)
    if max_sq_norm is None:
        max_sq_norm = float(sq_norms(X).max()) if n else 0.0
    scale = common_scale(max_sq_norm, metric)
    u = X / scal[:, None] if metric == COSINE else X
    u = (u.astype(np.float32) * scale).astype(np.float32)
    if operand == "f16":
        h = u.astype(np.float16)
        z, bits = h.astype(np.float32), h.view(np.uint16)
    elif operand == "bf16":
        bits = round_bf16(u)
        z = bf16_to_f32(bits)
    else:
        raise ValueError(operand)
    zbits = np.zeros((n, dp), np.uint16)
    zbits[:, :d] = bits
    z64, u64 = z.astype(np.float64), u.astype(np.float64)
    r64 = (z - u).astype(np.float64)          # the kernel's f32 subtraction (exact: z and u share a binade or z is coarser)

    def norm(v):
        return np.sqrt((v * v).sum(axis=1).astype(np.float32)) * UP

    zn, rn, un = norm(z64), norm(r64), norm(u64)
    if metric in (NEG_SQ_L2, RBF):
        cb = (np.float32(-0.5) * scal * scale * scale).astype(np.float32)
    else:
        cb = np.zeros(n, np.float32)
    maxima = np.array([zn.max(initial=0), rn.max(initial=0), un.max(initial=0), np.abs(cb).max(initial=0)], np.float32)
    return dict(scal=scal, scale=scale, u=u, z=z, zbits=zbits, zn=zn, rn=rn, un=un, cb=cb, maxima=maxima, d=d, dp=dp)


def margins(q: Dict[str, np.ndarray], cand_maxima: np.ndarray, metric: str, kk: int) -> Dict[str, np.ndarray]:
    """e1, e2 and margin of every query row of `q` against a candidate side with the maxima `cand_maxima`, in the kernel's f32
    operation order."""
    f = np.float32
    ZB, RB, UB, CB = (f(v) for v in cand_maxima)
    zn, rn, un = q["zn"].astype(f), q["rn"].astype(f), q["un"].astype(f)
    g_acc = f(q["dp"] + 8) * EPS24
    g_chain = f(q["d"] + 2) * EPS24
    slot_eps = f(1.9073486e-6) if list_capacity(kk) <= 16 else f(3.8146973e-6)
    e1 = rn * ZB + un * RB + (g_acc + slot_eps) * (zn * ZB + CB)
    if metric == DOT:
        e2 = g_chain * un * UB
    elif metric == COSINE:
        e2 = (g_chain + f(4.7683716e-7)) * un * UB * f(1.01)
    else:
        e2 = g_chain * un * UB + f(2.3841858e-7) * (un * un + UB * UB)
    margin = f(2.0) * (e1 + e2) * f(1.001) + f(1e-30)
    return dict(e1=e1.astype(f), e2=e2.astype(f), margin=margin.astype(f), slot_eps=slot_eps, g_acc=g_acc, g_chain=g_chain)


def approx_values(q: Dict[str, np.ndarray], c: Dict[str, np.ndarray]) -> np.ndarray:
    """G[i, j] = cb_j + z_i . z_j in float64: what the scan ranks, without the MFMA chain's own rounding."""
    return c["cb"].astype(np.float64)[None, :] + q["z"].astype(np.float64) @ c["z"].astype(np.float64).T


def target_values(q: Dict[str, np.ndarray], c: Dict[str, np.ndarray]) -> np.ndarray:
    """Q[i, j] = cb_j + u_i . u_j in float64: the real-number target the margin is measured against."""
    return c["cb"].astype(np.float64)[None, :] + q["u"].astype(np.float64) @ c["u"].astype(np.float64).T
