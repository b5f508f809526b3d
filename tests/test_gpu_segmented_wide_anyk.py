"""The segmented wide 16-bit top-k for any k (segmented_wide_anyk.*, include/ext/mmf_hg_segw_anyk.h): several
passes of the table-driven wide 16-bit scan over a ragged batch at 1024 < d <= 4096, the later ones under ceilings indexed by operand
position, each re-ranked exactly.

The reference is always ``segmented_exact.simtopk_segmented_exact`` on the same inputs (code this feature does not touch), compared
bit for bit, ids and values; one case compares against the CPU oracle, segment by segment.  With f16 operands the test caps the rows
that took the exact rescan at ceil(n_served / 64) per pass, so that a pass cannot come from the rescan:
tests/test_segmented_wide_anyk_cpu.py counts, on these same inputs and from the reference alone, the already-emitted columns that
slip under a row's ceiling and the rows whose margin band outgrows a 32-entry list."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg  # noqa: E402
from test_gpu_segmented import assert_same  # noqa: E402
from test_fast_anyk_cpu import N, case_inputs, lam_for  # noqa: E402
from test_segmented_anyk_cpu import X_SIZES, Y_SIZES, offsets  # noqa: E402
from test_wide_anyk_cpu import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def exact(mmf, X, Y=None, **kw):
    return mmf.segmented_exact.simtopk_segmented_exact(X, Y, **kw)


def check_info(info, k, passes_at_least=2):
    assert info["passes"] >= passes_at_least, info
    assert sum(info["yield"]) == k, info
    assert all(y >= 1 for y in info["yield"]), info


def rows(seed, n, d):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, d).astype(np.float32)).cuda()


_REF = {}


def deep_case(mmf, d, k, metric, dtype, two_sided):
    """The deep cohort of a case on the device, with the exact call's answer: computed once per case, never written."""
    key = (d, k, metric, dtype, two_sided)
    if key not in _REF:
        X, Y = case_inputs(d, dtype, two_sided)
        X = X.cuda()
        Y = None if Y is None else Y.cuda()
        kw = dict(ptr=offsets(X_SIZES), metric=metric, lam=lam_for(d), k=k)
        if two_sided:
            kw["y_ptr"] = offsets(Y_SIZES)
        _REF[key] = (X, Y, kw, exact(mmf, X, Y, **kw))
    return _REF[key]


# ---- 1. the four cases, both operand types, X against itself and against Y ---------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_same_bits_as_the_exact_call(mmf, d, k, metric, dtype, two_sided, precision):
    X, Y, kw, ref = deep_case(mmf, d, k, metric, dtype, two_sided)
    idx, val, st, info = mmf.simtopk_segmented_wide_any_k(X, Y, precision=precision, return_stats=True, return_info=True, **kw)
    print(f"d={d} k={k} {metric} {dtype} two_sided={two_sided} {precision}: {info}")
    assert_same((idx, val), ref)
    assert st["precision_used"] == {"fast": 2, "fast_bf16": 3}[precision]
    check_info(info, k)
    if precision == "fast":      # the 16-bit passes, not the rescan, produced the answer (every segment of the cohort is served)
        assert sum(info["exact_rows"]) <= info["passes"] * -(-N // 64), info


# ---- 2. a cohort of edge segments: empty, short of k (the -1 / -inf fill), adm = k exactly, shallow ---------------------------------------
def test_edge_segments(mmf):
    d, k, sizes = 1100, 21, [0, 1, 20, 21, 22, 23, 128, 129, 300]
    X = rows(23 + d, sum(sizes), d)
    ptr = offsets(sizes)
    kw = dict(ptr=ptr, metric="neg_sq_l2", k=k)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(X, return_info=True, **kw)
    print(f"edge segments d={d} k={k}: {info}")
    assert_same((idx, val), exact(mmf, X, **kw))
    check_info(info, k)
    idx, val = idx.cpu(), val.cpu()
    for g, ng in enumerate(sizes):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        blk = idx[lo:hi]
        assert bool(((blk == -1) | ((blk >= lo) & (blk < hi))).all()), f"segment {g}: an id outside the segment's columns"
        if 0 < ng <= k:                                      # ng - 1 admissible columns, then the fill (21 rows: 20 columns, unserved)
            assert bool((blk[:, :ng - 1] >= 0).all()) and bool((blk[:, ng - 1:] == -1).all())
            assert bool(torch.isinf(val[lo:hi, ng - 1:]).all()) and bool((val[lo:hi, ng - 1:] < 0).all())
        elif ng > k:                                         # 22 rows: exactly k columns; 23: one to spare (shallow, rescanned)
            assert bool((blk >= 0).all())
    served = sum(ng for ng in sizes if ng > k)
    assert all(e <= served for e in info["exact_rows"]), info          # rows of served segments only


def test_no_segment_served_and_the_exact_precision(mmf):
    """Every segment short of k columns: the exact launch loop answers the call (one pass on record).  precision="exact" through
    the entry is the exact segmented call."""
    X = rows(29, 60, 1100)
    kw = dict(ptr=offsets([10, 0, 30, 20]), metric="cosine", k=45)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(X, return_info=True, **kw)
    assert_same((idx, val), exact(mmf, X, **kw))
    assert info["passes"] == 1 and info["yield"] == [45] and info["exact_rows"] == [0]
    X, Y, kw, ref = deep_case(mmf, 1100, 32, "cosine", "f32", True)
    idx, val, st, info = mmf.simtopk_segmented_wide_any_k(X, Y, precision="exact", return_stats=True, return_info=True, **kw)
    assert_same((idx, val), ref)
    assert st["precision_used"] == 1 and info["passes"] == 1


# ---- 3. forced column ranges: several entries per row block, the threshold union under ceilings ------------------------------------------------
@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("col_splits", [2, 4])
def test_forced_col_splits(mmf, col_splits, two_sided):
    X, Y, kw, ref = deep_case(mmf, 1536, 32, "neg_sq_l2", "f16", two_sided)
    idx, val, st, info = mmf.simtopk_segmented_wide_any_k(X, Y, col_splits=col_splits, return_stats=True, return_info=True, **kw)
    print(f"col_splits={col_splits} two_sided={two_sided}: {info}")
    assert_same((idx, val), ref)
    check_info(info, 32)
    # the largest segment has 6 tiles of columns one-sided (700 rows) and 4 two-sided (500): 4 ranges fit both
    assert st["col_splits"] == col_splits, st
    assert sum(info["exact_rows"]) <= info["passes"] * -(-N // 64), info


# ---- 4. a block of ties across the pass boundary, the same repeated rows next door -----------------------------------------------------------
def test_tie_block_across_the_pass_boundary(mmf):
    rs = np.random.RandomState(11)
    d = 1100
    row = rs.randn(1, d).astype(np.float32)
    Y = np.concatenate([rs.randn(300, d).astype(np.float32), np.repeat(row, 100, 0),          # segment 0: columns 0 .. 399
                        rs.randn(100, d).astype(np.float32), np.repeat(row, 100, 0)])         # segment 1: columns 400 .. 599
    X = 3.0 * row + 0.05 * rs.randn(128, d).astype(np.float32)          # near the repeated row: its copies lead every row's order
    Xc, Yc = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    kw = dict(ptr=[0, 64, 128], y_ptr=[0, 400, 600], metric="dot", k=30, exclude_self=False)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(Xc, Yc, return_info=True, **kw)
    print(f"tie block: {info}")
    assert_same((idx, val), exact(mmf, Xc, Yc, **kw))
    check_info(info, 30)
    idx = idx.cpu()
    assert torch.equal(idx[:64], torch.arange(300, 330).expand(64, 30)), "the tie run continues ascending across the pass boundary (column 20)"
    assert torch.equal(idx[64:], torch.arange(500, 530).expand(64, 30)), "no id comes from the neighbouring segment's copies"


# ---- 5. exact duplicates among the queries of a segment; d = 4096; batch= equals ptr= -------------------------------------------------------------
def test_duplicate_queries(mmf):
    base = np.random.RandomState(13).randn(150, 1100).astype(np.float32)
    X = torch.from_numpy(np.concatenate([np.tile(base, (3, 1)), np.tile(base[:90], (2, 1))])).cuda()
    kw = dict(ptr=[0, 450, 630], metric="cosine", k=30, exclude_self=True)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(X, return_info=True, **kw)
    assert_same((idx, val), exact(mmf, X, **kw))
    check_info(info, 30)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_the_widest_dim(mmf, precision):
    X = rows(31, 300, 4096)
    kw = dict(ptr=[0, 170, 300], metric="cosine", k=25)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(X, precision=precision, return_info=True, **kw)
    print(f"d=4096 {precision}: {info}")
    assert_same((idx, val), exact(mmf, X, **kw))
    check_info(info, 25)


def test_batch_equals_ptr(mmf):
    X, _, kw, ref = deep_case(mmf, 1100, 32, "cosine", "f32", False)
    batch = torch.repeat_interleave(torch.arange(len(X_SIZES)), torch.tensor(X_SIZES))
    kwb = {k_: v for k_, v in kw.items() if k_ != "ptr"}
    assert_same(mmf.simtopk_segmented_wide_any_k(X, batch=batch, **kwb), ref)
    assert_same(mmf.simtopk_segmented_wide_any_k(X, batch=batch.cuda(), **kwb), ref)


# ---- 6. the operating point does not change the bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["16", "256"])
def test_operating_points(mmf, monkeypatch, env):
    X, _, kw, ref = deep_case(mmf, 1536, 64, "rbf", "f32", False)
    monkeypatch.setenv("MMF_ANYK_SHORT_DIV", env)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(X, return_info=True, **kw)
    print(f"MMF_ANYK_SHORT_DIV={env}: {info}")
    assert_same((idx, val), ref)
    check_info(info, 64)


# ---- 7. where one pass serves, the call is the wide segmented call ---------------------------------------------------------------------------
@pytest.mark.parametrize("d,k,col_splits", [(1100, 19, 0), (1536, 11, 2)])
def test_single_pass_shapes(mmf, d, k, col_splits):
    X, _ = case_inputs(d, "f32", False)
    X = X.cuda()
    kw = dict(ptr=offsets(X_SIZES), metric="cosine", k=k, exclude_self=True, col_splits=col_splits)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(X, return_info=True, **kw)
    assert_same((idx, val), mmf.wide_scan.simtopk_segmented(X, precision="fast", **kw))
    assert info["passes"] == 1 and info["yield"] == [k]


# ---- 8. the CPU oracle, segment by segment -----------------------------------------------------------------------------------------------------
def test_against_the_oracle(mmf):
    sizes = [120, 70, 110]
    X = np.random.RandomState(7).randn(sum(sizes), 1100).astype(np.float32)
    idx, val, info = mmf.simtopk_segmented_wide_any_k(torch.from_numpy(X).cuda(), ptr=offsets(sizes), metric="cosine", k=50, return_info=True)
    check_info(info, 50)
    o = offsets(sizes).tolist()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for g in range(len(sizes)):
        ridx, rval = oracle.simtopk(X[o[g]:o[g + 1]], metric="cosine", k=50)
        assert np.array_equal(idx[o[g]:o[g + 1]], ridx + o[g])
        assert np.array_equal(val[o[g]:o[g + 1]].view(np.int32), rval.view(np.int32))


# ---- 9. a busy non-default stream -------------------------------------------------------------------------------------------------------------------
def test_behind_a_closed_gate(mmf):
    sizes = [250, 90, 260]

    def make(which):
        rs = np.random.RandomState(17 if which == "truth" else 18)
        return [torch.from_numpy(rs.randn(sum(sizes), 1100).astype(np.float32))]

    def entry(X):
        return list(mmf.simtopk_segmented_wide_any_k(X, ptr=offsets(sizes), metric="cosine", k=40))

    def reference(X):
        o = offsets(sizes).tolist()
        parts = [oracle.simtopk(X[o[g]:o[g + 1]], metric="cosine", k=40) for g in range(len(sizes))]
        return [np.concatenate([p[0] + o[g] for g, p in enumerate(parts)]), np.concatenate([p[1] for p in parts])]
    sg.run_gated(entry, make, reference, name="simtopk_segmented_wide_any_k", calls=2)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mmf):
    with pytest.raises(RuntimeError, match="d = 600 is not above 1024"):
        mmf.simtopk_segmented_wide_any_k(torch.randn(64, 600, device="cuda"), ptr=[0, 30, 64], metric="cosine", k=21, exclude_self=False)
    with pytest.raises(RuntimeError, match="d = 5000 is beyond the wide 16-bit scan"):
        mmf.simtopk_segmented_wide_any_k(torch.randn(64, 5000, device="cuda"), ptr=[0, 30, 64], metric="cosine", k=21, exclude_self=False)
    # the narrow entry keeps refusing what this one serves
    with pytest.raises(RuntimeError, match="d = 1100, k = 21"):
        mmf.simtopk_segmented_fast_any_k(torch.randn(64, 1100, device="cuda"), ptr=[0, 30, 64], metric="cosine", k=21, exclude_self=False)
    L = mmf._lib.lib()
    X = torch.randn(128, 1100, device="cuda")
    idx = torch.empty((128, 30), dtype=torch.int64, device="cuda")
    val = torch.empty((128, 30), dtype=torch.float32, device="cuda")
    ptr = torch.tensor([0, 64, 128], dtype=torch.int64)
    ev = torch.cuda.Event()
    ev.record()
    for opts, want, text in ((mmf._lib.SimtopkOpts(2, 0, 0, 0, ctypes.c_void_p(ev.cuda_event)), mmf._lib.MMF_E_UNSUPPORTED, b"select_wait_event"),
                             (mmf._lib.SimtopkOpts(2, 0, 3, 0, None), mmf._lib.MMF_E_INVALID, b"col_splits")):
        rc = L.mmf_simtopk_segmented_wide_anyk(X.data_ptr(), 128, None, 0, 1100, 0, 1, 1.0, 30, 0, ptr.data_ptr(), None, 2, idx.data_ptr(),
                                               val.data_ptr(), ctypes.byref(opts), None, 0, None, None)
        assert rc == want and text in L.mmf_last_error()


# ---- 11. the router's three arms -------------------------------------------------------------------------------------------------------------------------
def test_router(mmf):
    sw = mmf.segmented_wide_anyk
    X, _, kw, ref = deep_case(mmf, 1100, 32, "cosine", "f32", False)
    # explicit fast precisions: the new call where d > 1024 needs several passes
    for precision, used in (("fast", 2), ("fast_bf16", 3)):
        idx, val, st = sw.simtopk_segmented(X, precision=precision, return_stats=True, **kw)
        assert_same((idx, val), ref)
        assert st["precision_used"] == used
    # "auto": the new call on the shape classes of _AUTO_SHAPES only; N = 2001 rows is on none of them, "exact" never
    assert not sw._auto_takes(N, 1100, 32, len(X_SIZES))
    for precision in ("auto", "exact"):
        idx, val, st = sw.simtopk_segmented(X, precision=precision, return_stats=True, **kw)
        assert_same((idx, val), ref)
        assert st["precision_used"] == 1
    for dl, dh, kl, kh, nl, pl in sw._AUTO_SHAPES:                                     # whatever table was committed (may be empty)
        assert sw._auto_takes(nl, dl, kl, 1) and not sw._auto_takes(nl - 1, dl, kl, 1)
    # everywhere else: segmented_anyk's router — one pass of the wide scan, and the narrow any-k call at d <= 1024
    kw1 = dict(kw, k=19)
    assert_same(sw.simtopk_segmented(X, precision="fast", **kw1), mmf.segmented_anyk.simtopk_segmented(X, precision="fast", **kw1))
    Xn = rows(37, 400, 600)
    kwn = dict(ptr=[0, 150, 400], metric="cosine", k=32)
    idx, val, st = sw.simtopk_segmented(Xn, precision="fast", return_stats=True, **kwn)
    assert_same((idx, val), exact(mmf, Xn, **kwn))
    assert st["precision_used"] == 2
