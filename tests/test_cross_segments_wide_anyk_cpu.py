"""The wide 16-bit cross-segment top-k for any k (include/ext/mmf_hg_cross_segw_anyk.h) without a GPU: the header
and the export list, the Python signatures, the host-only plan, the entry's host checks in their order, and a numpy restatement of
the ceiling argument for this form on the cohort tests/test_gpu_cross_segments_wide_anyk.py uses: the WIDE scan's margin (dp = d
rounded up to 128, no slot-bit term; test_wide_anyk_cpu._wide_ceiling_case) with its maxima over ALL candidates of the call, the
order, the floor and the margin bands over the columns OUTSIDE the row's own segment (test_cross_segments_anyk_cpu.cross_ceiling_case).

Counted here (float64, 2001 rows in six segments, the four cases, against themselves and against 1500 others):
    f16 operands:  largest value minus ceiling -9.9 .. -66.6; ghosts per row mean 1.21 .. 2.12, max 4 .. 7, (N / 64)-th largest
                   3 .. 5; largest band 25 .. 31 (pass 0) and 25 .. 34 (pass 1); rows with a band over 32: 0 in pass 0, at most 2
                   of 2001 in pass 1.
    bf16 operands (the three cases whose rows are not bf16 already): largest value minus ceiling -224 .. -362; ghosts per row mean
                   5.94 .. 6.61, max 12 .. 14, (N / 64)-th largest 10 .. 11; largest band 57 .. 59 (pass 0) and 67 .. 76 (pass 1);
                   rows with a band over 32: 1410 .. 1733 of 2001 in pass 0, 1950 .. 1987 in pass 1 — on a schedule without
                   overflow lists the "never flagged" guarantee is gone for nearly every row, and five times the ghosts shrink the
                   yield of every later pass: bf16 operands lose.  No cap on them."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fast_anyk_cpu import N, _round16, case_inputs, lam_for  # noqa: E402
from test_segmented_anyk_cpu import X_SIZES, Y_SIZES  # noqa: E402
from test_wide_anyk_cpu import CASES, DEPTH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST_CAP = 32                # one list's worth of columns: what a row keeps for certain on a schedule without overflow lists


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, exports, signatures -------------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(os.path.join(ROOT, "include", "ext", "mmf_hg_cross_segw_anyk.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.CROSS_WIDE_ANYK_EXPORTS) == {"mmf_simtopk_cross_segments_wide_anyk", "mmf_cross_segments_wide_anyk_plan"}
    assert '#include "mmf_hg_fast_anyk.h"' in hdr and "typedef struct" not in hdr          # the info struct is reused, not redeclared
    for name in dir(mmf._lib):                                  # ... and from no other list
        v = getattr(mmf._lib, name)
        if name != "CROSS_WIDE_ANYK_EXPORTS" and isinstance(v, list) and all(isinstance(e, str) for e in v):
            assert not set(v) & declared, name
    L = mmf._lib.lib()
    for name in mmf._lib.CROSS_WIDE_ANYK_EXPORTS:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.mmf_simtopk_cross_segments_wide_anyk.argtypes == L.mmf_simtopk_cross_segments_fast_anyk.argtypes
    assert L.mmf_simtopk_cross_segments_wide_anyk.argtypes[:-1] == L.mmf_simtopk_cross_segments_wide.argtypes
    assert L.mmf_cross_segments_wide_anyk_plan.argtypes == L.mmf_cross_segments_anyk_plan.argtypes
    build = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py")).read()
    assert "mmf_hg_cross_segw_anyk.h" in build and "mmf_scan_b16w.hip" in build


def test_python_signatures(mmf):
    cw, ca = mmf.cross_segments_wide_anyk, mmf.cross_segments_anyk
    assert mmf.simtopk_cross_segments_wide_any_k is cw.simtopk_cross_segments_wide_any_k
    assert mmf.cross_segments_wide_anyk_plan is cw.cross_segments_wide_anyk_plan
    for name in ("cross_segments_wide_anyk", "simtopk_cross_segments_wide_any_k", "cross_segments_wide_anyk_plan"):
        assert name in mmf.__all__
    assert "mmf.cross_segments_wide_anyk.*" in mmf.__doc__
    assert mmf.simtopk_cross_segments is mmf.cross_segments.simtopk_cross_segments       # the package-level name stays the exact call
    sig, ref = inspect.signature(cw.simtopk_cross_segments_wide_any_k), inspect.signature(ca.simtopk_cross_segments_fast_any_k)
    assert list(sig.parameters) == list(ref.parameters)
    assert {n: (p.kind, p.default) for n, p in sig.parameters.items()} == {n: (p.kind, p.default) for n, p in ref.parameters.items()}
    assert list(inspect.signature(cw.cross_segments_wide_anyk_plan).parameters) == ["d", "k"]
    rsig = inspect.signature(cw.simtopk_cross_segments)
    assert list(rsig.parameters) == list(inspect.signature(ca.simtopk_cross_segments).parameters)
    assert rsig.parameters["precision"].default == "auto"
    for fn in (cw.cross_segment_knn_edges, cw.link_slides):
        p = inspect.signature(fn).parameters["precision"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "exact"
    # until profiles/cross_segments_wide_anyk_timing.txt shows a shape ahead by the three-spreads rule, "auto" is the narrow module's router
    assert cw._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "cross_segments_wide_anyk_timing.txt"))
    for entry in cw._AUTO_SHAPES:
        dl, dh, kl, kh, nl = entry
        assert 1024 < dl <= dh <= 4096 and 21 <= kl <= kh and nl >= 1
    with pytest.raises(ValueError, match="unknown precision"):
        cw.simtopk_cross_segments(torch.zeros(8, 1100), ptr=[0, 4, 8], k=2, precision="fastest")
    with pytest.raises(ValueError, match="unknown precision"):
        cw.simtopk_cross_segments_wide_any_k(torch.zeros(8, 1100), ptr=[0, 4, 8], k=2, precision="fastest")
    with pytest.raises(ValueError, match="segment 0 has 4 admissible columns"):
        cw.simtopk_cross_segments_wide_any_k(torch.zeros(8, 1100), ptr=[0, 4, 8], k=5)
    with pytest.raises(ValueError, match="col_splits must be 0 or a power of two"):
        cw.simtopk_cross_segments_wide_any_k(torch.zeros(8, 1100), ptr=[0, 4, 8], k=2, col_splits=3)
    with pytest.raises(ValueError, match="d = 600 is not above 1024.*mmf_simtopk_cross_segments_fast_anyk"):
        cw.simtopk_cross_segments_wide_any_k(torch.zeros(64, 600), ptr=[0, 30, 64], k=21)
    with pytest.raises(ValueError, match="d = 5000 is beyond the wide 16-bit scan"):
        cw.simtopk_cross_segments_wide_any_k(torch.zeros(64, 5000), ptr=[0, 30, 64], k=21)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmf.simtopk_cross_segments_wide_any_k(torch.zeros(64, 1100), ptr=[0, 30, 64], k=21)
    with pytest.raises(RuntimeError, match="no CPU path"):                  # "exact" is not refused for d > 4096
        mmf.simtopk_cross_segments_wide_any_k(torch.zeros(64, 5000), ptr=[0, 30, 64], k=21, precision="exact")


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def test_plan(mmf):
    plan = mmf.cross_segments_wide_anyk_plan
    assert plan(1100, 21) == {"multi_pass": True, "scan_kk": 20, "first_yield": 20, "min_passes": 2}
    assert plan(1536, 64) == {"multi_pass": True, "scan_kk": 20, "first_yield": 20, "min_passes": 4}
    assert plan(1100, 20) == {"multi_pass": False, "scan_kk": 20, "first_yield": 20, "min_passes": 1}
    for d in (1025, 1100, 1536, 2560, 4096):
        for k in (1, 11, 12, 20, 21, 40, 41, 64, 128, 500):
            assert plan(d, k) == mmf.wide_anyk_plan(d, k, False), (d, k)
    L = mmf._lib.lib()
    UNS, INV = mmf._lib.MMF_E_UNSUPPORTED, mmf._lib.MMF_E_INVALID
    assert L.mmf_cross_segments_wide_anyk_plan(1024, 21, None, None, None) == UNS
    assert L.mmf_cross_segments_wide_anyk_plan(600, 5, None, None, None) == UNS
    assert L.mmf_cross_segments_wide_anyk_plan(4097, 5, None, None, None) == UNS
    assert L.mmf_cross_segments_wide_anyk_plan(0, 5, None, None, None) == INV
    assert L.mmf_cross_segments_wide_anyk_plan(1100, 0, None, None, None) == INV
    for bad in [(600, 50), (1024, 21), (4097, 5), (5000, 30), (0, 5), (1100, 0)]:
        with pytest.raises(ValueError):
            plan(*bad)
    # the narrow form's plan keeps refusing what this one serves, in its wording
    with pytest.raises(ValueError, match="d = 1100, k = 21"):
        mmf.cross_segments_anyk_plan(1100, 21)


# ---- the entry's host checks, in mmf_simtopk_cross_segments_wide's order -------------------------------------------------------------------
def _entry(mmf, *, X=1, n=8, Y=None, m=0, d=1100, dtype=0, metric=1, lam=1.0, k=3, xptr=(0, 3, 8), yptr=None, nseg=2, out=(1, 1), prec=2,
           splits=0, event=None, device=0, fn="mmf_simtopk_cross_segments_wide_anyk"):
    L = mmf._lib.lib()
    buf = ctypes.create_string_buffer(64)                     # a non-NULL host address: no check before the first device call reads it
    ptr = lambda on: ctypes.addressof(buf) if on else None    # noqa: E731
    arr = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)    # noqa: E731
    xp, yp = arr(xptr), arr(yptr)
    opts = mmf._lib.SimtopkOpts(prec, 0, splits, 0, ptr(event))
    rc = getattr(L, fn)(ptr(X), n, ptr(Y), m, d, dtype, metric, lam, k,
                        None if xp is None else ctypes.addressof(xp), None if yp is None else ctypes.addressof(yp),
                        nseg, ptr(out[0]), ptr(out[1]), ctypes.byref(opts), None, device, None, None)
    return rc, L.mmf_last_error().decode()


def test_entry_checks_in_order(mmf):
    INV, UNS = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    who = "simtopk_cross_segments_wide_anyk"
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
             (dict(prec=7, event=1, d=600), INV, f"{who}: bad precision 7"),
             (dict(event=1, d=600, k=21, out=(0, 1)), UNS, f"{who}: select_wait_event is not supported"),
             (dict(d=600, k=21, out=(0, 1)), UNS, f"{who}: d = 600 is not above 1024: call mmf_simtopk_cross_segments_fast_anyk"),
             (dict(d=1024, k=5, prec=1, out=(0, 1)), UNS, "mmf_simtopk_cross_segments_fast_anyk"),
             (dict(d=5000, k=21, out=(0, 1)), UNS, f"{who}: d = 5000 is beyond the wide 16-bit scan"),
             (dict(d=5000, k=3, prec=3, out=(0, 1)), UNS, f"{who}: d = 5000 is beyond the wide 16-bit scan"),
             (dict(out=(0, 1), k=6), INV, f"{who}: NULL output"),
             (dict(out=(1, 0), k=6), INV, f"{who}: NULL output"),
             (dict(k=6), INV, f"{who}: segment 0 has 5 admissible columns (m = 8 minus its own 3 rows of Y), k = 6 needs at least 6"),
             (dict(k=21), INV, f"{who}: segment 0 has 5 admissible columns"),
             (dict(k=4, xptr=(0, 3, 8), Y=1, m=9, yptr=(0, 1, 9)), INV, f"{who}: segment 1 has 1 admissible columns")]
    for kw, want, text in steps:
        rc, msg = _entry(mmf, **kw)
        assert rc == want and text in msg, (kw, rc, msg)
    assert _entry(mmf, n=0, X=0, xptr=(0, 0, 0), out=(0, 0))[0] == mmf._lib.MMF_OK          # no rows: a no-op
    assert _entry(mmf, n=0, X=0, xptr=(0, 0, 0), out=(0, 0), k=500, d=2560)[0] == mmf._lib.MMF_OK
    # EXACT is not refused for d > 4096, nor is a (d, k) of several passes under FAST: the next refusal is the NULL output
    assert _entry(mmf, d=5000, k=21, prec=1, out=(0, 1))[1].startswith(f"{who}: NULL output")
    assert _entry(mmf, d=1100, k=21, out=(0, 1))[1].startswith(f"{who}: NULL output")
    assert _entry(mmf, d=1100, k=21, prec=3, out=(0, 1))[1].startswith(f"{who}: NULL output")
    assert _entry(mmf, d=1100, k=21, prec=0, out=(0, 1))[1].startswith(f"{who}: NULL output")   # AUTO means FAST
    # the one-pass wide entry's refusals up to there, word for word but the name
    for kw in (dict(xptr=(0, 5, 3)), dict(splits=3), dict(prec=7), dict(event=1), dict(out=(0, 1)), dict(k=6), dict(metric=9)):
        rc_w, msg_w = _entry(mmf, fn="mmf_simtopk_cross_segments_wide", **kw)
        rc_a, msg_a = _entry(mmf, **kw)
        assert rc_w == rc_a and msg_w.replace("simtopk_cross_segments_wide", who) == msg_a, kw
    # the narrow any-k entry keeps its refusal of what this one serves, in its wording
    rc, msg = _entry(mmf, fn="mmf_simtopk_cross_segments_fast_anyk", d=1100, k=21, out=(0, 1))
    assert rc == UNS and "simtopk_cross_segments_fast_anyk: d = 1100, k = 21 is beyond one pass of the wide cross-segment 16-bit scan" in msg


# ---- the ceiling argument, restated in numpy for the wide cross form ----------------------------------------------------------------------
def cross_wide_ceiling_case(d, metric, dtype, two_sided, f16):
    """Per row of the cohort, from the reference alone (float64), after the first pass: the largest scanned value G over the columns
    OUTSIDE THE ROW'S SEGMENT that rank after its floor minus the row's ceiling (must be <= 0); the already-emitted columns at or
    below the ceiling (the ghosts; all of them lie in other segments — a masked column is neither a ghost nor a candidate); and the
    margin band — the admissible columns with G >= (20th best admissible G) - margin — of pass 0 (every admissible column) and of
    pass 1 (those at or below the ceiling).  E1, E2 and the map are those of mmf_scan_b16w.hip's header and wide_ceil_kernel: dp = d
    rounded up to 128, no slot-bit term, the maxima over ALL candidates of the call (a superset of any row's admissible columns).
    No self term: a row's self lies inside its masked segment."""
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

    xo = np.concatenate([[0], np.cumsum(X_SIZES)])
    yo = np.concatenate([[0], np.cumsum(Y_SIZES)]) if two_sided else xo
    m = key.shape[1]
    excess, ghosts, band0, band1 = [], [], [], []
    for g in range(len(X_SIZES)):
        rows = slice(xo[g], xo[g + 1])
        kg, Gg = key[rows].copy(), G[rows].copy()
        kg[:, yo[g]:yo[g + 1]] = -np.inf                         # the mask: the own segment ranks last, behind every real column
        Gg[:, yo[g]:yo[g + 1]] = -np.inf                         # ... and is -inf in the accumulators before anything reads them
        adm = m - (yo[g + 1] - yo[g])
        assert adm >= 1000                                       # no row goes shallow at k <= 64
        order = np.lexsort((np.broadcast_to(np.arange(m), kg.shape), -kg), axis=1)
        emitted, after = order[:, :DEPTH], order[:, DEPTH:adm]
        fk = np.take_along_axis(kg, emitted[:, -1:], 1)[:, 0]
        mapped = s * s * fk if not biased else 0.5 * s * s * ((fk / lam if metric == "rbf" else fk) + nx[rows])
        ceil = mapped + e1[rows] + e2[rows]
        excess.append(np.take_along_axis(Gg, after, 1).max(1) - ceil)
        ghosts.append((np.take_along_axis(Gg, emitted, 1) <= ceil[:, None]).sum(1))

        def band(Gv):     # admissible columns at or above (DEPTH-th best value of the row) - margin; -inf never counts
            t = -np.partition(-Gv, DEPTH - 1, axis=1)[:, DEPTH - 1]
            return ((Gv >= (t - margin[rows])[:, None]) & np.isfinite(Gv)).sum(1)
        band0.append(band(Gg))
        band1.append(band(np.where(Gg <= ceil[:, None], Gg, -np.inf)))
    return np.concatenate(excess), np.concatenate(ghosts), np.concatenate(band0), np.concatenate(band1)


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_no_unmasked_column_after_the_floor_exceeds_its_ceiling(d, k, metric, dtype, two_sided):
    for f16 in (True, False):
        excess, ghosts, band0, band1 = cross_wide_ceiling_case(d, metric, dtype, two_sided, f16)
        assert len(excess) == N
        short = np.sort(ghosts)[::-1][N // 64]
        crowded0, crowded1 = int((band0 > LIST_CAP).sum()), int((band1 > LIST_CAP).sum())
        print(f"d={d} {metric} {dtype} two_sided={two_sided} {'f16' if f16 else 'bf16'} operands, after {DEPTH}: "
              f"ghosts mean {ghosts.mean():.2f} max {ghosts.max()} (n/64-th largest {short}), largest G - ceiling {excess.max():.3g}, "
              f"largest band {band0.max()} in pass 0, {band1.max()} in pass 1, rows with a band over {LIST_CAP}: {crowded0} / {crowded1} of {N}")
        assert excess.max() <= 0.0, "a column outside the row's segment that ranks after the floor lies above the row's ceiling"
        if f16:
            # what the GPU test's cap on exact_rows (f16 operands, sum <= passes * ceil(N / 64)) rests on: a pass yields at least
            # DEPTH - 10 entries while at most N / 64 rows have more than 10 ghosts, and — this schedule has no overflow lists — at
            # most N / 64 rows carry a margin band that one 32-entry list cannot hold for certain
            assert short <= 10, "more than N / 64 rows with over 10 ghosts"
            assert crowded0 <= N // 64 and crowded1 <= N // 64, f"more than N / 64 rows with a margin band over {LIST_CAP} columns"
