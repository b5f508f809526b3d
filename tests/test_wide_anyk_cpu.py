"""The wide 16-bit top-k for any k (include/ext/mmf_hg_wide_anyk.h) without a GPU: the header and the export
list, the Python signatures, the host-only plan, the entry's host checks in their order, and a numpy restatement of the ceiling
argument with the WIDE scan's margin on the inputs tests/test_gpu_wide_anyk.py uses (which imports them from here)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fast_anyk_cpu import M, N, _round16, case_inputs, lam_for  # noqa: E402,F401  (seeded Gaussian rows: seeds 300 + d / 400 + d)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the GPU test's shapes: n = 2001 rows (off every tile edge), against themselves or against m = 1500 others; d = 1100 and 1536
# (padded dims 1152 and 1536), depth 20, two to four passes; metrics and row dtypes rotate over the cases
CASES = [(1100, 21, "dot", "bf16"), (1100, 32, "cosine", "f32"), (1536, 32, "neg_sq_l2", "f16"), (1536, 64, "rbf", "f32")]
DEPTH = 20
BAND_CAP = 32 + 192          # what a row keeps for certain: a 32-entry list's worth of columns, and its 192 overflow slots


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, exports, signatures -------------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(os.path.join(ROOT, "include", "ext", "mmf_hg_wide_anyk.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.WIDE_ANYK_EXPORTS) == {"mmf_simtopk_wide_anyk", "mmf_wide_anyk_plan"}
    assert '#include "mmf_hg_fast_anyk.h"' in hdr and "typedef struct" not in hdr          # the info struct is reused, not redeclared
    L = mmf._lib.lib()
    for name in mmf._lib.WIDE_ANYK_EXPORTS:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.mmf_simtopk_wide_anyk.argtypes == L.mmf_simtopk_fast_anyk.argtypes
    assert len(L.mmf_simtopk_wide_anyk.argtypes) == len(L.mmf_simtopk_ex.argtypes) + 1
    assert L.mmf_wide_anyk_plan.argtypes == L.mmf_fast_anyk_plan.argtypes
    build = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py")).read()
    assert "mmf_hg_wide_anyk.h" in build and "mmf_scan_b16w.hip" in build


def test_python_signatures(mmf):
    assert mmf.simtopk_wide_any_k is mmf.wide_anyk.simtopk_wide_any_k and mmf.wide_anyk_plan is mmf.wide_anyk.wide_anyk_plan
    sig = inspect.signature(mmf.wide_anyk.simtopk_wide_any_k)
    assert sig.parameters.keys() == inspect.signature(mmf.fast_anyk.simtopk_fast_any_k).parameters.keys()
    assert list(sig.parameters) == ["X", "Y", "metric", "lam", "k", "exclude_self", "row_offset", "col_offset", "precision", "col_splits",
                                    "return_stats", "return_info"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("X", "Y"))
    assert sig.parameters["precision"].default == "fast" and sig.parameters["Y"].default is None
    assert list(inspect.signature(mmf.wide_anyk.wide_anyk_plan).parameters) == ["d", "k", "exclude_self"]
    rsig = inspect.signature(mmf.wide_anyk.simtopk)
    assert list(rsig.parameters) == list(inspect.signature(mmf.fast_anyk.simtopk).parameters)
    assert rsig.parameters["precision"].default == "auto"
    # until profiles/wide_anyk_timing.txt shows a shape ahead by the three-spreads rule, "auto" is fast_anyk.simtopk
    assert mmf.wide_anyk._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "wide_anyk_timing.txt"))
    with pytest.raises(ValueError, match="unknown precision"):
        mmf.wide_anyk.simtopk(torch.zeros(4, 1100), k=2, precision="fastest")
    with pytest.raises(ValueError, match="unknown precision"):
        mmf.simtopk_wide_any_k(torch.zeros(4, 1100), k=2, precision="fastest")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmf.simtopk_wide_any_k(torch.zeros(4, 1100), k=2)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def test_plan(mmf):
    assert mmf.wide_anyk_plan(1100, 21, False) == {"multi_pass": True, "scan_kk": 20, "first_yield": 20, "min_passes": 2}
    assert mmf.wide_anyk_plan(1536, 64, True) == {"multi_pass": True, "scan_kk": 20, "first_yield": 19, "min_passes": 4}    # ceil(64 / 19)
    assert mmf.wide_anyk_plan(1100, 20, False) == {"multi_pass": False, "scan_kk": 20, "first_yield": 20, "min_passes": 1}
    assert mmf.wide_anyk_plan(4096, 5, True) == {"multi_pass": False, "scan_kk": 6, "first_yield": 5, "min_passes": 1}
    for (d, k, ex) in [(1025, 20, True), (2560, 40, False), (4096, 128, True)]:
        p = mmf.wide_anyk_plan(d, k, ex)
        per = 20 - int(ex)
        assert p == {"multi_pass": True, "scan_kk": 20, "first_yield": per, "min_passes": -(-k // per)}, (d, k, ex, p)
    with pytest.raises(ValueError, match="mmf_fast_anyk_plan"):
        mmf.wide_anyk_plan(1024, 21, False)
    for bad in [(600, 50, False), (4097, 5, False), (5000, 30, True), (0, 5, False), (1100, 0, False)]:
        with pytest.raises(ValueError):
            mmf.wide_anyk_plan(*bad)
    # the narrow plan keeps refusing what this one serves
    with pytest.raises(ValueError, match="d = 1100, k = 21"):
        mmf.fast_anyk_plan(1100, 21, False)


# ---- the entry's host checks, in mmf_simtopk_ex's order --------------------------------------------------------------------------------------
def _entry(mmf, *, X=1, n=8, Y=None, m=0, d=1100, dtype=0, metric=1, lam=1.0, k=50, ex=0, out=(1, 1), prec=2, event=None, device=0):
    L = mmf._lib.lib()
    buf = ctypes.create_string_buffer(64)                     # a non-NULL host address: no check before the first device call reads it
    ptr = lambda on: ctypes.addressof(buf) if on else None    # noqa: E731
    opts = mmf._lib.SimtopkOpts(prec, 0, 0, 0, ptr(event))
    rc = L.mmf_simtopk_wide_anyk(ptr(X), n, ptr(Y), m, d, dtype, metric, lam, k, ex, 0, 0, ptr(out[0]), ptr(out[1]), ctypes.byref(opts), None,
                                 device, None, None)
    return rc, L.mmf_last_error().decode()


def test_entry_checks_in_order(mmf):
    INV, UNS = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    # the device comes first, whatever else is wrong
    rc, msg = _entry(mmf, device=-1, n=-1, k=0, metric=9)
    assert rc == UNS and msg.startswith("simtopk_wide_anyk: device_id -1")
    steps = [(dict(n=-1, dtype=9, metric=9, lam=0.0, k=0), INV, "bad shape"),
             (dict(dtype=9, X=0, metric=9, k=0), INV, "bad in_dtype"),
             (dict(X=0, metric=9, k=0), INV, "X is NULL"),
             (dict(metric=9, k=0, prec=7), INV, "simtopk_wide_anyk: bad metric 9"),
             (dict(metric=3, lam=0.0, k=0, prec=7), INV, "simtopk_wide_anyk: MMF_RBF needs lambda > 0"),
             (dict(k=0, prec=7, event=1), INV, "simtopk_wide_anyk: k must be >= 1"),
             (dict(prec=7, event=1, d=600, out=(0, 1)), INV, "simtopk_wide_anyk: bad precision 7"),
             (dict(event=1, d=600, out=(0, 1)), UNS, "simtopk_wide_anyk: select_wait_event"),
             (dict(d=600, out=(0, 1)), UNS, "simtopk_wide_anyk: d = 600 is not above 1024: call mmf_simtopk_fast_anyk"),
             (dict(d=1024, k=5, prec=1, out=(0, 1)), UNS, "mmf_simtopk_fast_anyk"),
             (dict(d=5000, out=(0, 1)), UNS, "simtopk_wide_anyk: d = 5000 is beyond the wide 16-bit scan"),
             (dict(d=5000, prec=3, out=(0, 1)), UNS, "simtopk_wide_anyk: d = 5000 is beyond the wide 16-bit scan"),
             (dict(out=(0, 1), k=9), INV, "simtopk_wide_anyk: NULL output"),
             (dict(out=(1, 0), k=9), INV, "simtopk_wide_anyk: NULL output"),
             (dict(k=9), INV, "simtopk_wide_anyk: k = 9 exceeds the 8 admissible columns"),
             (dict(k=8, ex=1), INV, "simtopk_wide_anyk: k = 8 exceeds the 7 admissible columns (m = 8, self excluded)")]
    for kw, want, text in steps:
        rc, msg = _entry(mmf, **kw)
        assert rc == want and text in msg, (kw, rc, msg)
    assert _entry(mmf, n=0, X=0, out=(0, 0))[0] == mmf._lib.MMF_OK          # no rows: a no-op
    assert _entry(mmf, d=5000, prec=1, out=(0, 1))[1].startswith("simtopk_wide_anyk: NULL output")   # EXACT is not refused for d > 4096
    # the narrow entry keeps its refusal of what this one serves, in its wording
    L = mmf._lib.lib()
    buf = ctypes.create_string_buffer(64)
    opts = mmf._lib.SimtopkOpts(2, 0, 0, 0, None)
    rc = L.mmf_simtopk_fast_anyk(ctypes.addressof(buf), 8, None, 0, 1100, 0, 1, 1.0, 21, 0, 0, 0, None, None, ctypes.byref(opts), None, 0, None, None)
    assert rc == UNS and "simtopk_fast_anyk: d = 1100, k = 21 is beyond one pass of the wide 16-bit scan" in L.mmf_last_error().decode()


# ---- the ceiling argument, restated in numpy with the wide scan's margin on the GPU test's inputs ---------------------------------------------------
def _wide_ceiling_case(d, metric, dtype, two_sided, f16):
    """Per row, from the reference alone (float64): the largest scanned value G over the columns that rank after the floor of the
    first pass minus the row's ceiling (must be <= 0); the already-emitted columns at or below the ceiling (the ghosts); and the
    margin band — the columns with G >= (20th best G) - margin — of pass 0 (all columns) and of pass 1 (the columns at or below
    the ceiling).  E1, E2 and the map are those of mmf_scan_b16w.hip's header and wide_ceil_kernel: dp = d rounded up to 128, no
    slot-bit term."""
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
    dp = 128 * -(-d // 128)
    eps = 2.0 ** -24
    e1 = rn * ZB + un * RB + (dp + 8) * eps * (zn * ZB + CB)
    g_chain = (d + 2) * eps
    e2 = g_chain * un * UB if metric == "dot" else (g_chain + 8 * eps) * un * UB * 1.01 if metric == "cosine" else \
        g_chain * un * UB + 4 * eps * (un * un + UB * UB)
    margin = 2.0 * (e1 + e2)
    first = DEPTH - self1                                   # entries the first pass emits
    order = np.lexsort((np.broadcast_to(np.arange(key.shape[1]), key.shape), -key), axis=1)
    emitted, after = order[:, :first], order[:, first:key.shape[1] - self1]
    fk = np.take_along_axis(key, emitted[:, -1:], 1)[:, 0]
    mapped = s * s * fk if not biased else 0.5 * s * s * ((fk / lam if metric == "rbf" else fk) + nx)
    ceil = mapped + e1 + e2
    excess = np.take_along_axis(G, after, 1).max(1) - ceil
    ghosts = (np.take_along_axis(G, emitted, 1) <= ceil[:, None]).sum(1)

    def band(Gv):     # columns at or above (DEPTH-th best value of the row) - margin
        t = -np.partition(-Gv, DEPTH - 1, axis=1)[:, DEPTH - 1]
        return (Gv >= (t - margin)[:, None]).sum(1)
    band0 = band(G)
    band1 = band(np.where(G <= ceil[:, None], G, -np.inf))
    return excess, ghosts, first, band0, band1


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_no_column_after_the_floor_exceeds_its_ceiling(d, k, metric, dtype, two_sided):
    for f16 in (True, False):
        excess, ghosts, first, band0, band1 = _wide_ceiling_case(d, metric, dtype, two_sided, f16)
        short = np.sort(ghosts)[::-1][N // 64]
        print(f"d={d} {metric} {dtype} two_sided={two_sided} {'f16' if f16 else 'bf16'} operands, after {first}: "
              f"ghosts mean {ghosts.mean():.2f} max {ghosts.max()} (n/64-th largest {short}), largest G - ceiling {excess.max():.3g}, "
              f"largest band {band0.max()} in pass 0, {band1.max()} in pass 1")
        assert excess.max() <= 0.0, "a column that ranks after the floor lies above the row's ceiling"
        if f16:
            # the GPU test's cap on exact_rows (f16 operands): a pass yields at least one entry while at most n / 64 rows have
            # depth - self or more ghosts — here every row but that many has at most half of that; and no row's band outgrows
            # its two 32-entry lists plus its 192 overflow slots, so no row is flagged for a crowd
            assert short <= first // 2, f"more than n / 64 rows with over {first // 2} ghosts"
            assert band0.max() <= BAND_CAP and band1.max() <= BAND_CAP, "a margin band beyond the lists and the overflow list"
