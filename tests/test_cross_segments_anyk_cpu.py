"""The 16-bit cross-segment top-k for any k (include/ext/mmf_hg_cross_seg_anyk.h) without a GPU: the header and the
export list, the Python signatures, the host-only plan, the entry's host checks in their order, and a numpy restatement of the
ceiling argument for the cross form on the cohort tests/test_gpu_cross_segments_anyk.py uses: the margin's maxima over ALL
candidates of the call, the order and the floor over the columns OUTSIDE the row's own segment."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fast_anyk_cpu import CASES, N  # noqa: E402
from test_segmented_anyk_cpu import X_SIZES, Y_SIZES, _operands  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, exports, signatures -------------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(os.path.join(ROOT, "include", "ext", "mmf_hg_cross_seg_anyk.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.CROSS_ANYK_EXPORTS) == {"mmf_simtopk_cross_segments_fast_anyk", "mmf_cross_segments_anyk_plan"}
    assert '#include "mmf_hg_fast_anyk.h"' in hdr
    for name in dir(mmf._lib):                                  # ... and from no other list
        v = getattr(mmf._lib, name)
        if name != "CROSS_ANYK_EXPORTS" and isinstance(v, list) and all(isinstance(e, str) for e in v):
            assert not set(v) & declared, name
    L = mmf._lib.lib()
    for name in mmf._lib.CROSS_ANYK_EXPORTS:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.mmf_simtopk_cross_segments_fast_anyk.argtypes[:-1] == L.mmf_simtopk_cross_segments_fast.argtypes
    assert L.mmf_simtopk_cross_segments_fast_anyk.argtypes[-1] is ctypes.POINTER(mmf._lib.FastAnykInfo)
    assert len(L.mmf_cross_segments_anyk_plan.argtypes) == len(L.mmf_fast_anyk_plan.argtypes) - 1      # no exclude_self
    build = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py")).read()
    assert "mmf_hg_cross_seg_anyk.h" in build


def test_python_signatures(mmf):
    ca = mmf.cross_segments_anyk
    assert mmf.simtopk_cross_segments_fast_any_k is ca.simtopk_cross_segments_fast_any_k
    assert mmf.cross_segments_anyk_plan is ca.cross_segments_anyk_plan
    for name in ("cross_segments_anyk", "simtopk_cross_segments_fast_any_k", "cross_segments_anyk_plan"):
        assert name in mmf.__all__
    assert "mmf.cross_segments_anyk.*" in mmf.__doc__
    assert mmf.simtopk_cross_segments is mmf.cross_segments.simtopk_cross_segments       # the package-level name stays the exact call
    sig = inspect.signature(ca.simtopk_cross_segments_fast_any_k)
    assert list(sig.parameters) == ["X", "Y", "ptr", "batch", "y_ptr", "y_batch", "metric", "lam", "k", "precision", "col_splits",
                                    "return_stats", "return_info"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("X", "Y"))
    want = dict(Y=None, ptr=None, batch=None, y_ptr=None, y_batch=None, metric="cosine", lam=1.0, k=5, precision="fast", col_splits=0,
                return_stats=False, return_info=False)
    assert {n: sig.parameters[n].default for n in want} == want
    assert list(inspect.signature(ca.cross_segments_anyk_plan).parameters) == ["d", "k"]
    assert inspect.signature(ca.simtopk_cross_segments).parameters["precision"].default == "auto"
    for fn in (ca.cross_segment_knn_edges, ca.link_slides):
        p = inspect.signature(fn).parameters["precision"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "exact"
    # until profiles/cross_segments_anyk_timing.txt shows a shape ahead by the three-spreads rule, "auto" is the wide module's router
    assert ca._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "cross_segments_anyk_timing.txt"))
    with pytest.raises(ValueError, match="unknown precision"):
        ca.simtopk_cross_segments(torch.zeros(8, 4), ptr=[0, 4, 8], k=2, precision="fastest")
    with pytest.raises(ValueError, match="unknown precision"):
        ca.simtopk_cross_segments_fast_any_k(torch.zeros(8, 4), ptr=[0, 4, 8], k=2, precision="fastest")
    with pytest.raises(ValueError, match="segment 0 has 4 admissible columns"):
        ca.simtopk_cross_segments_fast_any_k(torch.zeros(8, 4), ptr=[0, 4, 8], k=5)
    with pytest.raises(ValueError, match="col_splits must be 0 or a power of two"):
        ca.simtopk_cross_segments_fast_any_k(torch.zeros(8, 4), ptr=[0, 4, 8], k=2, col_splits=3)
    with pytest.raises(ValueError, match="d = 1100, k = 21"):
        ca.simtopk_cross_segments_fast_any_k(torch.zeros(64, 1100), ptr=[0, 30, 64], k=21)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmf.simtopk_cross_segments_fast_any_k(torch.zeros(8, 4), ptr=[0, 4, 8], k=2)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def test_plan(mmf):
    for d in (1, 40, 128, 300, 512, 513, 600, 1024):
        for k in (1, 19, 20, 21, 43, 44, 45, 64, 128, 500):
            assert mmf.cross_segments_anyk_plan(d, k) == mmf.fast_anyk_plan(d, k, False), (d, k)
    assert mmf.cross_segments_anyk_plan(600, 32) == {"multi_pass": True, "scan_kk": 20, "first_yield": 20, "min_passes": 2}
    assert mmf.cross_segments_anyk_plan(1100, 20) == {"multi_pass": False, "scan_kk": 20, "first_yield": 20, "min_passes": 1}
    L = mmf._lib.lib()
    assert L.mmf_cross_segments_anyk_plan(1100, 21, None, None, None) == mmf._lib.MMF_E_UNSUPPORTED
    assert b"d = 1100, k = 21" in L.mmf_last_error()
    assert L.mmf_cross_segments_anyk_plan(5000, 5, None, None, None) == mmf._lib.MMF_E_UNSUPPORTED
    assert L.mmf_cross_segments_anyk_plan(0, 5, None, None, None) == mmf._lib.MMF_E_INVALID
    assert L.mmf_cross_segments_anyk_plan(40, 0, None, None, None) == mmf._lib.MMF_E_INVALID
    with pytest.raises(ValueError, match="d = 1100, k = 21"):
        mmf.cross_segments_anyk_plan(1100, 21)


# ---- the entry's host checks, in mmf_simtopk_cross_segments_fast's order ---------------------------------------------------------------------
def _entry(mmf, *, X=1, n=8, Y=None, m=0, d=40, dtype=0, metric=1, lam=1.0, k=3, xptr=(0, 3, 8), yptr=None, nseg=2, out=(1, 1), prec=2,
           splits=0, event=None, device=0):
    L = mmf._lib.lib()
    buf = ctypes.create_string_buffer(64)                     # a non-NULL host address: no check before the first device call reads it
    ptr = lambda on: ctypes.addressof(buf) if on else None    # noqa: E731
    arr = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)    # noqa: E731
    xp, yp = arr(xptr), arr(yptr)
    opts = mmf._lib.SimtopkOpts(prec, 0, splits, 0, ptr(event))
    rc = L.mmf_simtopk_cross_segments_fast_anyk(ptr(X), n, ptr(Y), m, d, dtype, metric, lam, k,
                                                None if xp is None else ctypes.addressof(xp), None if yp is None else ctypes.addressof(yp),
                                                nseg, ptr(out[0]), ptr(out[1]), ctypes.byref(opts), None, device, None, None)
    return rc, L.mmf_last_error().decode()


def test_entry_checks_in_order(mmf):
    INV, UNS = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    who = "simtopk_cross_segments_fast_anyk"
    # the device comes first, whatever else is wrong
    rc, msg = _entry(mmf, device=-1, n=-1, k=0, metric=9, xptr=None)
    assert rc == UNS and msg.startswith(f"{who}: device_id -1")
    # each step fixes the first fault of the one before; what follows it in the order is still wrong
    steps = [(dict(n=-1, dtype=9, metric=9, lam=0.0, k=0, xptr=None), INV, "bad shape"),
             (dict(dtype=9, X=0, metric=9, k=0, xptr=None), INV, "bad in_dtype"),
             (dict(X=0, metric=9, k=0, xptr=None), INV, "X is NULL"),
             (dict(metric=9, k=0, xptr=None), INV, f"{who}: bad metric 9"),
             (dict(metric=3, lam=0.0, k=0, xptr=None), INV, f"{who}: MMF_RBF needs lambda > 0"),
             (dict(k=0, xptr=None), INV, f"{who}: k must be >= 1"),
             (dict(xptr=None, splits=3), INV, f"{who}: need n_seg >= 0 and host offsets x_ptr[n_seg + 1]"),
             (dict(xptr=(1, 3, 8), splits=3), INV, f"{who}: x_ptr must start at 0"),
             (dict(xptr=(0, 5, 3), splits=3), INV, f"{who}: x_ptr decreases at segment 1"),
             (dict(xptr=(0, 3, 7), splits=3), INV, f"{who}: x_ptr must end at 8"),
             (dict(Y=1, m=6, yptr=(0, 3, 7), splits=3), INV, f"{who}: y_ptr must end at 6"),
             (dict(splits=3, prec=7), INV, f"{who}: col_splits must be 0 or a power of two (got 3)"),
             (dict(prec=7, event=1), INV, f"{who}: bad precision 7"),
             (dict(event=1, d=1100, k=21, out=(0, 1)), UNS, f"{who}: select_wait_event is not supported"),
             (dict(d=1100, k=21, out=(0, 1)), UNS, f"{who}: d = 1100, k = 21"),
             (dict(d=1100, k=21, prec=3, out=(0, 1)), UNS, f"{who}: d = 1100, k = 21"),
             (dict(d=5000, k=3, out=(0, 1)), UNS, f"{who}: d = 5000, k = 3"),
             (dict(out=(0, 1), k=6), INV, f"{who}: NULL output"),
             (dict(out=(1, 0), k=6), INV, f"{who}: NULL output"),
             (dict(k=6), INV, f"{who}: segment 0 has 5 admissible columns (m = 8 minus its own 3 rows of Y), k = 6 needs at least 6"),
             (dict(k=4, xptr=(0, 3, 8), Y=1, m=9, yptr=(0, 1, 9)), INV, f"{who}: segment 1 has 1 admissible columns")]
    for kw, want, text in steps:
        rc, msg = _entry(mmf, **kw)
        assert rc == want and text in msg, (kw, rc, msg)
    assert "no ceilings" in _entry(mmf, d=1100, k=21, out=(0, 1))[1]
    assert _entry(mmf, n=0, X=0, xptr=(0, 0, 0), out=(0, 0))[0] == mmf._lib.MMF_OK          # no rows: a no-op
    assert _entry(mmf, n=0, X=0, xptr=(0, 0, 0), out=(0, 0), k=500, d=700)[0] == mmf._lib.MMF_OK
    # EXACT is not refused for (d, k), nor is a (d, k) of several passes under FAST: the next refusal is the NULL output
    assert _entry(mmf, d=1100, k=21, prec=1, out=(0, 1))[1].startswith(f"{who}: NULL output")
    assert _entry(mmf, d=600, k=21, out=(0, 1))[1].startswith(f"{who}: NULL output")
    assert _entry(mmf, d=600, k=21, prec=0, out=(0, 1))[1].startswith(f"{who}: NULL output")   # AUTO means FAST


# ---- the ceiling argument, restated in numpy for the cross form ------------------------------------------------------------------------------
def cross_ceiling_case(d, metric, dtype, two_sided, f16):
    """Per row of the deep cohort, after the first pass: the largest scanned value over the columns OUTSIDE THE ROW'S SEGMENT that
    rank after its floor minus the row's ceiling (must be <= 0), and the already-emitted columns at or below the ceiling (the
    ghosts; all of them lie in other segments — a masked column is neither a ghost nor a candidate); also the entries the first pass
    emits.  No self term: a row's self lies inside its masked segment."""
    key, G, e12, s, nx, lam, biased = _operands(d, dtype, two_sided, metric, f16)
    first = 44 if d <= 512 else 20
    xo = np.concatenate([[0], np.cumsum(X_SIZES)])
    yo = np.concatenate([[0], np.cumsum(Y_SIZES)]) if two_sided else xo
    m = key.shape[1]
    excess, ghosts = [], []
    for g in range(len(X_SIZES)):
        kg = key[xo[g]:xo[g + 1]].copy()
        Gg = G[xo[g]:xo[g + 1]]
        kg[:, yo[g]:yo[g + 1]] = -np.inf                         # the mask: the own segment ranks last, behind every real column
        adm = m - (yo[g + 1] - yo[g])
        assert adm >= 1000                                       # no row goes shallow at k <= 128
        order = np.lexsort((np.broadcast_to(np.arange(m), kg.shape), -kg), axis=1)
        emitted, after = order[:, :first], order[:, first:adm]
        fk = np.take_along_axis(kg, emitted[:, -1:], 1)[:, 0]
        ni = nx[xo[g]:xo[g + 1]]
        mapped = s * s * fk if not biased else 0.5 * s * s * ((fk / lam if metric == "rbf" else fk) + ni)
        ceil = mapped + e12[xo[g]:xo[g + 1]]
        excess.append(np.take_along_axis(Gg, after, 1).max(1) - ceil)
        ghosts.append((np.take_along_axis(Gg, emitted, 1) <= ceil[:, None]).sum(1))
    return np.concatenate(excess), np.concatenate(ghosts), first


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_no_unmasked_column_after_the_floor_exceeds_its_ceiling(d, k, metric, dtype, two_sided):
    for f16 in (True, False):
        excess, ghosts, first = cross_ceiling_case(d, metric, dtype, two_sided, f16)
        assert len(excess) == N
        print(f"d={d} {metric} {dtype} two_sided={two_sided} {'f16' if f16 else 'bf16'} operands, after {first}: "
              f"ghosts mean {ghosts.mean():.2f} max {ghosts.max()}, largest G - ceiling {excess.max():.3g}")
        assert excess.max() <= 0.0, "a column outside the row's segment that ranks after the floor lies above the row's ceiling"
        if f16:
            # the GPU test's cap on exact_rows (f16 operands): a pass yields at least one entry while at most n / 64 rows have
            # `first` or more ghosts — here every row but that many has fewer, by a wide berth
            short = np.sort(ghosts)[::-1][N // 64]
            assert short <= first // 2, f"more than n / 64 rows with over {first // 2} ghosts"
