"""The segmented 16-bit top-k for any k (include/ext/mmf_hg_seg_anyk.h) without a GPU: the header and the export
list, the Python signatures, the host-only plan, the entry's host checks in their order, and a numpy restatement of the ceiling
argument per segment on the cohort tests/test_gpu_segmented_anyk.py uses (which imports it from here): the margin's maxima over
ALL candidates of the call, the order and the floor inside the row's own segment."""
import ctypes
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fast_anyk_cpu import CASES, M, N, _round16, case_inputs, lam_for  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the deep cohort: the rows of test_fast_anyk_cpu's inputs cut into six segments whose sizes straddle the 256-row and 128-row block
# edges; every segment keeps at least a pass depth of unemitted columns in every pass of every case (k <= 128, depth <= 44)
X_SIZES = [700, 301, 257, 256, 255, 232]
Y_SIZES = [500, 260, 200, 190, 175, 175]
assert sum(X_SIZES) == N and sum(Y_SIZES) == M


def offsets(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, exports, signatures -------------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(os.path.join(ROOT, "include", "ext", "mmf_hg_seg_anyk.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.SEG_ANYK_EXPORTS) == {"mmf_simtopk_segmented_fast_anyk", "mmf_segmented_anyk_plan"}
    assert not [n for n in dir(mmf._lib) if n.startswith("EXPORTS") and "SEG_ANYK" in n]
    L = mmf._lib.lib()
    for name in mmf._lib.SEG_ANYK_EXPORTS:
        assert getattr(L, name).restype is ctypes.c_int
    assert len(L.mmf_simtopk_segmented_fast_anyk.argtypes) == len(L.mmf_simtopk_segmented.argtypes) + 1
    assert len(L.mmf_segmented_anyk_plan.argtypes) == len(L.mmf_fast_anyk_plan.argtypes)
    build = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py")).read()
    assert "mmf_hg_seg_anyk.h" in build


def test_python_signatures(mmf):
    sa = mmf.segmented_anyk
    assert mmf.simtopk_segmented_fast_any_k is sa.simtopk_segmented_fast_any_k and mmf.segmented_anyk_plan is sa.segmented_anyk_plan
    for name in ("segmented_anyk", "simtopk_segmented_fast_any_k", "segmented_anyk_plan"):
        assert name in mmf.__all__
    assert "mmf.segmented_anyk.*" in mmf.__doc__
    sig = inspect.signature(sa.simtopk_segmented_fast_any_k)
    assert list(sig.parameters) == ["X", "Y", "ptr", "batch", "y_ptr", "y_batch", "metric", "lam", "k", "exclude_self", "precision",
                                    "return_stats", "return_info"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("X", "Y"))
    assert sig.parameters["precision"].default == "fast" and sig.parameters["Y"].default is None
    assert list(inspect.signature(sa.segmented_anyk_plan).parameters) == ["d", "k", "exclude_self"]
    assert inspect.signature(sa.simtopk_segmented).parameters["precision"].default == "auto"
    # until profiles/segmented_anyk_timing.txt shows a shape ahead by the three-spreads rule, "auto" is segmented_exact.simtopk_segmented
    assert sa._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "segmented_anyk_timing.txt"))
    with pytest.raises(ValueError, match="unknown precision"):
        sa.simtopk_segmented(torch.zeros(4, 4), ptr=[0, 4], k=2, precision="fastest")
    with pytest.raises(ValueError, match="unknown precision"):
        sa.simtopk_segmented_fast_any_k(torch.zeros(4, 4), ptr=[0, 4], k=2, precision="fastest")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmf.simtopk_segmented_fast_any_k(torch.zeros(4, 4), ptr=[0, 4], k=2)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def test_plan(mmf):
    for d in (1, 40, 128, 300, 512, 513, 600, 1024):
        for k in (1, 19, 20, 21, 43, 44, 45, 64, 128, 500):
            for ex in (False, True):
                assert mmf.segmented_anyk_plan(d, k, ex) == mmf.fast_anyk_plan(d, k, ex), (d, k, ex)
    assert mmf.segmented_anyk_plan(600, 32, True) == {"multi_pass": True, "scan_kk": 20, "first_yield": 19, "min_passes": 2}
    assert mmf.segmented_anyk_plan(1100, 20, False) == {"multi_pass": False, "scan_kk": 20, "first_yield": 20, "min_passes": 1}
    L = mmf._lib.lib()
    assert L.mmf_segmented_anyk_plan(1100, 21, 0, None, None, None) == mmf._lib.MMF_E_UNSUPPORTED
    assert b"d = 1100, k = 21" in L.mmf_last_error()
    assert L.mmf_segmented_anyk_plan(1100, 20, 1, None, None, None) == mmf._lib.MMF_E_UNSUPPORTED
    assert L.mmf_segmented_anyk_plan(0, 5, 0, None, None, None) == mmf._lib.MMF_E_INVALID
    assert L.mmf_segmented_anyk_plan(40, 0, 0, None, None, None) == mmf._lib.MMF_E_INVALID
    with pytest.raises(ValueError, match="d = 1100, k = 21"):
        mmf.segmented_anyk_plan(1100, 21, False)


# ---- the entry's host checks, in mmf_simtopk_segmented's order -------------------------------------------------------------------------------
def _entry(mmf, *, X=1, n=8, Y=None, m=0, d=40, dtype=0, metric=1, lam=1.0, k=50, ex=0, xptr=(0, 3, 8), yptr=None, nseg=2, out=(1, 1), prec=2,
           splits=0, event=None, device=0):
    L = mmf._lib.lib()
    buf = ctypes.create_string_buffer(64)                     # a non-NULL host address: no check before the first device call reads it
    ptr = lambda on: ctypes.addressof(buf) if on else None    # noqa: E731
    arr = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)    # noqa: E731
    xp, yp = arr(xptr), arr(yptr)
    opts = mmf._lib.SimtopkOpts(prec, 0, splits, 0, ptr(event))
    rc = L.mmf_simtopk_segmented_fast_anyk(ptr(X), n, ptr(Y), m, d, dtype, metric, lam, k, ex,
                                           None if xp is None else ctypes.addressof(xp), None if yp is None else ctypes.addressof(yp), nseg,
                                           ptr(out[0]), ptr(out[1]), ctypes.byref(opts), None, device, None, None)
    return rc, L.mmf_last_error().decode()


def test_entry_checks_in_order(mmf):
    INV, UNS = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    who = "simtopk_segmented_fast_anyk"
    # the device comes first, whatever else is wrong
    rc, msg = _entry(mmf, device=-1, n=-1, k=0, metric=9, xptr=None)
    assert rc == UNS and msg.startswith(f"{who}: device_id -1")
    steps = [(dict(n=-1, dtype=9, metric=9, lam=0.0, k=0, xptr=None), INV, "bad shape"),
             (dict(dtype=9, X=0, metric=9, k=0, xptr=None), INV, "bad in_dtype"),
             (dict(X=0, metric=9, k=0, xptr=None), INV, "X is NULL"),
             (dict(metric=9, k=0, xptr=None), INV, f"{who}: bad metric 9"),
             (dict(metric=3, lam=0.0, k=0, xptr=None), INV, f"{who}: MMF_RBF needs lambda > 0"),
             (dict(k=0, xptr=None), INV, f"{who}: k must be >= 1"),
             (dict(xptr=None, splits=2), INV, f"{who}: need n_seg >= 0 and host offsets x_ptr[n_seg + 1]"),
             (dict(xptr=(1, 3, 8), splits=2), INV, f"{who}: x_ptr must start at 0"),
             (dict(xptr=(0, 5, 3), splits=2), INV, f"{who}: x_ptr decreases at segment 1"),
             (dict(xptr=(0, 3, 7), splits=2), INV, f"{who}: x_ptr must end at 8"),
             (dict(Y=1, m=6, yptr=(0, 3, 7), splits=2), INV, f"{who}: y_ptr must end at 6"),
             (dict(prec=7, splits=2), INV, f"{who}: bad precision 7"),
             (dict(splits=2, d=1100, out=(0, 1)), UNS, f"{who}: col_splits and select_wait_event are not supported"),
             (dict(event=1, d=1100, out=(0, 1)), UNS, f"{who}: col_splits and select_wait_event are not supported"),
             (dict(d=1100, k=21, out=(0, 1)), UNS, f"{who}: d = 1100, k = 21"),
             (dict(d=1100, k=20, ex=1, prec=3, out=(0, 1)), UNS, f"{who}: d = 1100, k = 20"),
             (dict(out=(0, 1)), INV, f"{who}: NULL output"),
             (dict(out=(1, 0)), INV, f"{who}: NULL output")]
    for kw, want, text in steps:
        rc, msg = _entry(mmf, **kw)
        assert rc == want and text in msg, (kw, rc, msg)
    assert "no ceilings" in _entry(mmf, d=1100, k=21, out=(0, 1))[1]
    assert _entry(mmf, n=0, X=0, xptr=(0, 0, 0), out=(0, 0))[0] == mmf._lib.MMF_OK          # no rows: a no-op
    # a segment short of k admissible columns is not refused (it gets what it has): the next refusal is the NULL output
    assert _entry(mmf, k=50, out=(0, 1))[1].startswith(f"{who}: NULL output")
    assert _entry(mmf, d=1100, k=21, prec=1, out=(0, 1))[1].startswith(f"{who}: NULL output")   # EXACT is not refused for (d, k)


# ---- the ceiling argument, restated in numpy per segment -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operands(d, dtype, two_sided, metric, f16):
    """What the scan holds for a case, in float64: scanned values G of every (row, column) pair, canonical keys, the per-row E1 + E2
    with the maxima over ALL candidates, and the key -> G map's pieces.  E1, E2, the map and the scale are _ceiling_case's."""
    X, Y = case_inputs(d, dtype, two_sided)
    x = X.double().numpy()
    y = x if Y is None else Y.double().numpy()
    lam = lam_for(d)
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    dot = x @ y.T
    if metric == "dot":
        key = dot
    elif metric == "cosine":
        key = dot / (np.maximum(np.sqrt(nx), 1e-8)[:, None] * np.maximum(np.sqrt(ny), 1e-8)[None, :])
    else:
        key = -(nx[:, None] + ny[None, :] - 2.0 * dot) * (lam if metric == "rbf" else 1.0)
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
    ZB, RB, UB, CB = norm(zy).max(), norm(zy - uy).max(), norm(uy).max(), np.abs(cb).max()       # the whole candidate image
    dp = 128 if d <= 128 else 256 if d <= 256 else 512 if d <= 512 else 1024
    eps = 2.0 ** -24
    cap = 32 if d <= 512 else 15
    e1 = rn * ZB + un * RB + ((dp + 8) * eps + (2.0 ** -19 if cap <= 16 else 2.0 ** -18)) * (zn * ZB + CB)
    g_chain = (d + 2) * eps
    e2 = g_chain * un * UB if metric == "dot" else (g_chain + 8 * eps) * un * UB * 1.01 if metric == "cosine" else \
        g_chain * un * UB + 4 * eps * (un * un + UB * UB)
    return key, G, e1 + e2, s, nx, lam, biased


def segment_ceiling_case(d, metric, dtype, two_sided, f16):
    """Per row of the deep cohort, after the first pass: the largest scanned value over the columns OF THE ROW'S SEGMENT that rank
    after its floor minus the row's ceiling (must be <= 0), and the already-emitted columns of the segment at or below the ceiling
    (the ghosts); also the entries the first pass emits."""
    key, G, e12, s, nx, lam, biased = _operands(d, dtype, two_sided, metric, f16)
    depth = 44 if d <= 512 else 20
    self1 = 0 if two_sided else 1
    first = depth - self1
    xo = np.concatenate([[0], np.cumsum(X_SIZES)])
    yo = np.concatenate([[0], np.cumsum(Y_SIZES)]) if two_sided else xo
    excess, ghosts = [], []
    for g in range(len(X_SIZES)):
        kg = key[xo[g]:xo[g + 1], yo[g]:yo[g + 1]].copy()
        Gg = G[xo[g]:xo[g + 1], yo[g]:yo[g + 1]]
        if self1:
            np.fill_diagonal(kg, -np.inf)                       # self is dropped by identity, wherever it ranks
        order = np.lexsort((np.broadcast_to(np.arange(kg.shape[1]), kg.shape), -kg), axis=1)
        emitted, after = order[:, :first], order[:, first:kg.shape[1] - self1]
        fk = np.take_along_axis(kg, emitted[:, -1:], 1)[:, 0]
        ni = nx[xo[g]:xo[g + 1]]
        mapped = s * s * fk if not biased else 0.5 * s * s * ((fk / lam if metric == "rbf" else fk) + ni)
        ceil = mapped + e12[xo[g]:xo[g + 1]]
        excess.append(np.take_along_axis(Gg, after, 1).max(1) - ceil)
        ghosts.append((np.take_along_axis(Gg, emitted, 1) <= ceil[:, None]).sum(1))
    return np.concatenate(excess), np.concatenate(ghosts), first


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_no_column_after_the_floor_exceeds_its_ceiling(d, k, metric, dtype, two_sided):
    for f16 in (True, False):
        excess, ghosts, first = segment_ceiling_case(d, metric, dtype, two_sided, f16)
        assert len(excess) == N
        print(f"d={d} {metric} {dtype} two_sided={two_sided} {'f16' if f16 else 'bf16'} operands, after {first}: "
              f"ghosts mean {ghosts.mean():.2f} max {ghosts.max()}, largest G - ceiling {excess.max():.3g}")
        assert excess.max() <= 0.0, "a column that ranks after the floor lies above the row's ceiling"
        if f16:
            # the GPU test's cap on exact_rows (f16 operands): a pass yields at least one entry while at most n / 64 rows have
            # depth - self or more ghosts — here every row but that many has fewer, by a wide berth
            short = np.sort(ghosts)[::-1][N // 64]
            assert short <= first // 2, f"more than n / 64 rows with over {first // 2} ghosts"
