"""The 16-bit top-k for any k (include/ext/mmf_hg_fast_anyk.h) without a GPU: the header and the export list, the
Python signatures, the host-only plan, the entry's host checks in their order, and a numpy restatement of the ceiling argument
on the inputs tests/test_gpu_fast_anyk.py uses (which imports them from here)."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the GPU test's shapes: n = 2001 rows (off every tile edge), against themselves or against m = 1500 others.  (d, k) covers the padded
# dims 128 / 256 / 512 (depth 44) and 1024 (depth 20), two to seven passes; metrics and row dtypes rotate over the cases.
N, M = 2001, 1500
CASES = [(40, 45, "cosine", "f32"), (40, 128, "dot", "f16"), (200, 64, "neg_sq_l2", "bf16"), (300, 64, "rbf", "f32"),
         (300, 128, "cosine", "f16"), (600, 21, "dot", "bf16"), (600, 32, "neg_sq_l2", "f32"), (600, 64, "rbf", "f16")]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def lam_for(d):
    return 0.5 / d                       # unit Gaussian rows are sqrt(2 d) apart: RBF values stay inside f32


@functools.lru_cache(maxsize=None)
def case_inputs(d, dtype, two_sided):
    """(X, Y or None) on the host: seeded Gaussian rows in the case's dtype.  Computed once per shape, never written."""
    X = torch.from_numpy(np.random.RandomState(300 + d).randn(N, d).astype(np.float32)).to(DTYPES[dtype])
    Y = torch.from_numpy(np.random.RandomState(400 + d).randn(M, d).astype(np.float32)).to(DTYPES[dtype]) if two_sided else None
    return X, Y


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, exports, signatures -------------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(os.path.join(ROOT, "include", "ext", "mmf_hg_fast_anyk.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.FAST_ANYK_EXPORTS) == {"mmf_simtopk_fast_anyk", "mmf_fast_anyk_plan"}
    assert f"#define MMF_FAST_ANYK_MAX_PASSES {mmf._lib.FAST_ANYK_MAX_PASSES}" in hdr
    L = mmf._lib.lib()
    for name in mmf._lib.FAST_ANYK_EXPORTS:
        assert getattr(L, name).restype is ctypes.c_int
    assert len(L.mmf_simtopk_fast_anyk.argtypes) == len(L.mmf_simtopk_ex.argtypes) + 1
    # passes, yield[16], ghost_max[16] (int32), exact_rows[16] (int64, 8-aligned)
    assert ctypes.sizeof(mmf._lib.FastAnykInfo) == 8 * ((4 + 64 + 64 + 7) // 8) + 128
    build = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py")).read()
    assert "mmf_fast_anyk.hip" in build and "mmf_hg_fast_anyk.h" in build


def test_python_signatures(mmf):
    assert mmf.simtopk_fast_any_k is mmf.fast_anyk.simtopk_fast_any_k and mmf.fast_anyk_plan is mmf.fast_anyk.fast_anyk_plan
    sig = inspect.signature(mmf.fast_anyk.simtopk_fast_any_k)
    assert list(sig.parameters) == ["X", "Y", "metric", "lam", "k", "exclude_self", "row_offset", "col_offset", "precision", "col_splits",
                                    "return_stats", "return_info"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("X", "Y"))
    assert sig.parameters["precision"].default == "fast" and sig.parameters["Y"].default is None
    assert list(inspect.signature(mmf.fast_anyk.fast_anyk_plan).parameters) == ["d", "k", "exclude_self"]
    rsig = inspect.signature(mmf.fast_anyk.simtopk)
    assert rsig.parameters["precision"].default == "auto"
    # until profiles/fast_anyk_timing.txt shows a shape ahead by the three-spreads rule, "auto" is ops.simtopk
    assert mmf.fast_anyk._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "fast_anyk_timing.txt"))
    with pytest.raises(ValueError, match="unknown precision"):
        mmf.fast_anyk.simtopk(torch.zeros(4, 4), k=2, precision="fastest")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmf.simtopk_fast_any_k(torch.zeros(4, 4), k=2)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def test_plan(mmf):
    assert mmf.fast_anyk_plan(40, 44, False) == {"multi_pass": False, "scan_kk": 44, "first_yield": 44, "min_passes": 1}
    for (d, k, ex), kk in {(40, 45, False): 44, (300, 64, True): 44, (600, 20, True): 20, (600, 21, False): 20, (600, 128, True): 20}.items():
        p = mmf.fast_anyk_plan(d, k, ex)
        assert p["multi_pass"] and p["scan_kk"] == kk and p["first_yield"] == kk - int(ex), (d, k, ex, p)
        per = kk - int(ex)
        assert p["min_passes"] == -(-k // per), (d, k, ex, p)
    with pytest.raises(ValueError, match="d = 1100, k = 21"):
        mmf.fast_anyk_plan(1100, 21, False)
    assert not mmf.fast_anyk_plan(1100, 20, False)["multi_pass"]          # one pass of the wide scan
    for bad in [(0, 5, False), (40, 0, False), (5000, 5, False)]:
        with pytest.raises(ValueError):
            mmf.fast_anyk_plan(*bad)


# ---- the entry's host checks, in mmf_simtopk_ex's order --------------------------------------------------------------------------------------
def _entry(mmf, *, X=1, n=8, Y=None, m=0, d=40, dtype=0, metric=1, lam=1.0, k=50, ex=0, out=(1, 1), prec=2, event=None, device=0):
    L = mmf._lib.lib()
    buf = ctypes.create_string_buffer(64)                     # a non-NULL host address: no check before the first device call reads it
    ptr = lambda on: ctypes.addressof(buf) if on else None    # noqa: E731
    opts = mmf._lib.SimtopkOpts(prec, 0, 0, 0, ptr(event))
    rc = L.mmf_simtopk_fast_anyk(ptr(X), n, ptr(Y), m, d, dtype, metric, lam, k, ex, 0, 0, ptr(out[0]), ptr(out[1]), ctypes.byref(opts), None,
                                 device, None, None)
    return rc, L.mmf_last_error().decode()


def test_entry_checks_in_order(mmf):
    INV, UNS = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    # the device comes first, whatever else is wrong
    rc, msg = _entry(mmf, device=-1, n=-1, k=0, metric=9)
    assert rc == UNS and msg.startswith("simtopk_fast_anyk: device_id -1")
    steps = [(dict(n=-1, dtype=9, metric=9, lam=0.0, k=0), INV, "bad shape"),
             (dict(dtype=9, X=0, metric=9, k=0), INV, "bad in_dtype"),
             (dict(X=0, metric=9, k=0), INV, "X is NULL"),
             (dict(metric=9, k=0, prec=7), INV, "simtopk_fast_anyk: bad metric 9"),
             (dict(metric=3, lam=0.0, k=0, prec=7), INV, "simtopk_fast_anyk: MMF_RBF needs lambda > 0"),
             (dict(k=0, prec=7, event=1), INV, "simtopk_fast_anyk: k must be >= 1"),
             (dict(prec=7, event=1, out=(0, 1)), INV, "simtopk_fast_anyk: bad precision 7"),
             (dict(event=1, d=1100, out=(0, 1)), UNS, "simtopk_fast_anyk: select_wait_event"),
             (dict(d=1100, k=21, out=(0, 1)), UNS, "simtopk_fast_anyk: d = 1100, k = 21"),
             (dict(out=(0, 1), k=9), INV, "simtopk_fast_anyk: NULL output"),
             (dict(out=(1, 0), k=9), INV, "simtopk_fast_anyk: NULL output"),
             (dict(k=9), INV, "simtopk_fast_anyk: k = 9 exceeds the 8 admissible columns"),
             (dict(k=8, ex=1), INV, "simtopk_fast_anyk: k = 8 exceeds the 7 admissible columns (m = 8, self excluded)")]
    for kw, want, text in steps:
        rc, msg = _entry(mmf, **kw)
        assert rc == want and text in msg, (kw, rc, msg)
    assert _entry(mmf, n=0, X=0, out=(0, 0))[0] == mmf._lib.MMF_OK          # no rows: a no-op
    assert _entry(mmf, d=1100, k=21, prec=1, out=(0, 1))[1].startswith("simtopk_fast_anyk: NULL output")   # EXACT is not refused for (d, k)


# ---- the ceiling argument, restated in numpy on the GPU test's inputs ----------------------------------------------------------------------------
def _round16(u, f16):
    if f16:
        return u.astype(np.float16).astype(np.float64)
    b = u.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def _ceiling_case(d, k, metric, dtype, two_sided, f16, depth):
    """Per row: the largest scanned value G over the columns that rank after the floor minus the row's ceiling (must be <= 0), and
    the number of already-emitted columns at or below the ceiling (the ghosts).  E1, E2 and the map are those of
    mmf_scan_bf16.hip's header and ceil_kernel, evaluated in float64."""
    X, Y = case_inputs(d, dtype, two_sided)
    x = X.double().numpy()
    y = x if Y is None else Y.double().numpy()
    self1 = 0 if two_sided else 1
    lam = lam_for(d)
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    dot = x @ y.T
    if metric == "dot":
        key = dot
    elif metric == "cosine":
        key = dot / (np.maximum(np.sqrt(nx), 1e-8)[:, None] * np.maximum(np.sqrt(ny), 1e-8)[None, :])
    else:
        key = -(nx[:, None] + ny[None, :] - 2.0 * dot) * (lam if metric == "rbf" else 1.0)
    if self1:
        np.fill_diagonal(key, -np.inf)                      # self is dropped by identity, wherever it ranks
    # operands: normalised for cosine, scaled by the power of two that puts the largest norm into [256, 512)
    ux = x / np.maximum(np.sqrt(nx), 1e-8)[:, None] if metric == "cosine" else x
    uy = y / np.maximum(np.sqrt(ny), 1e-8)[:, None] if metric == "cosine" else y
    mx = 1.0 if metric == "cosine" else np.sqrt(max(nx.max(), ny.max()))
    s = 2.0 ** (9 - np.frexp(mx)[1])
    ux, uy = ux * s, uy * s
    zx, zy = _round16(ux, f16), _round16(uy, f16)
    biased = metric in ("neg_sq_l2", "rbf")
    cb = -0.5 * ny * s * s if biased else np.zeros(len(y))
    G = zx @ zy.T + cb[None, :]
    norm = lambda a: np.sqrt((a * a).sum(1))      # noqa: E731
    zn, rn, un = norm(zx), norm(zx - ux), norm(ux)
    ZB, RB, UB, CB = norm(zy).max(), norm(zy - uy).max(), norm(uy).max(), np.abs(cb).max()
    dp = 128 if d <= 128 else 256 if d <= 256 else 512 if d <= 512 else 1024
    eps = 2.0 ** -24
    cap = 32 if depth == 44 else 15
    e1 = rn * ZB + un * RB + ((dp + 8) * eps + (2.0 ** -19 if cap <= 16 else 2.0 ** -18)) * (zn * ZB + CB)
    g_chain = (d + 2) * eps
    e2 = g_chain * un * UB if metric == "dot" else (g_chain + 8 * eps) * un * UB * 1.01 if metric == "cosine" else \
        g_chain * un * UB + 4 * eps * (un * un + UB * UB)
    first = depth - self1                                   # entries the first pass emits
    order = np.lexsort((np.broadcast_to(np.arange(key.shape[1]), key.shape), -key), axis=1)
    emitted, after = order[:, :first], order[:, first:key.shape[1] - self1]
    fk = np.take_along_axis(key, emitted[:, -1:], 1)[:, 0]
    mapped = s * s * fk if not biased else 0.5 * s * s * ((fk / lam if metric == "rbf" else fk) + nx)
    ceil = mapped + e1 + e2
    excess = np.take_along_axis(G, after, 1).max(1) - ceil
    ghosts = (np.take_along_axis(G, emitted, 1) <= ceil[:, None]).sum(1)
    return excess, ghosts, first


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_no_column_after_the_floor_exceeds_its_ceiling(d, k, metric, dtype, two_sided):
    depth = 44 if d <= 512 else 20
    for f16 in (True, False):
        excess, ghosts, first = _ceiling_case(d, k, metric, dtype, two_sided, f16, depth)
        print(f"d={d} {metric} {dtype} two_sided={two_sided} {'f16' if f16 else 'bf16'} operands, after {first}: "
              f"ghosts mean {ghosts.mean():.2f} max {ghosts.max()}, largest G - ceiling {excess.max():.3g}")
        assert excess.max() <= 0.0, "a column that ranks after the floor lies above the row's ceiling"
        if f16:
            # the GPU test's cap on exact_rows (f16 operands): a pass yields at least one entry while at most n / 64 rows have
            # depth - self or more ghosts — here every row but that many has fewer, by a wide berth
            short = np.sort(ghosts)[::-1][N // 64]
            assert short <= first // 2, f"more than n / 64 rows with over {first // 2} ghosts"
