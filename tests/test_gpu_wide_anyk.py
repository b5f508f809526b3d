"""The wide 16-bit top-k for any k (wide_anyk.*, include/ext/mmf_hg_wide_anyk.h): several passes of the wide
16-bit scan (1024 < d <= 4096), the later ones under per-row ceilings, each re-ranked exactly.

The reference is always ``ops.simtopk(..., precision="exact")`` on the same inputs (code this feature does not touch), compared
bit for bit, ids and values; one case also compares against the CPU oracle.  With f16 operands the test caps the rows that took
the exact rescan at ceil(n / 64) per pass, so that a pass cannot come from the rescan: tests/test_wide_anyk_cpu.py counts, on
these same inputs and from the reference alone, the already-emitted columns that slip under a row's ceiling and the margin bands."""
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
from test_wide_anyk_cpu import CASES, N, ROOT, case_inputs, lam_for  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def exact(mmf, X, Y=None, **kw):
    return mmf.ops.simtopk(X, Y, precision="exact", **kw)


def check_info(info, k, passes_at_least=2):
    assert info["passes"] >= passes_at_least, info
    assert sum(info["yield"]) == k, info
    assert all(y >= 1 for y in info["yield"]), info


def gauss(seed, n, d):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, d).astype(np.float32))


# ---- 1. every CPU case, both operand types, X against itself and against Y -----------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_same_bits_as_the_exact_call(mmf, d, k, metric, dtype, two_sided, precision):
    X, Y = case_inputs(d, dtype, two_sided)
    X = X.cuda()
    Y = None if Y is None else Y.cuda()
    kw = dict(metric=metric, lam=lam_for(d), k=k)
    idx, val, st, info = mmf.simtopk_wide_any_k(X, Y, precision=precision, return_stats=True, return_info=True, **kw)
    print(f"d={d} k={k} {metric} {dtype} two_sided={two_sided} {precision}: {info}")
    assert_same((idx, val), exact(mmf, X, Y, **kw))
    assert st["precision_used"] == {"fast": 2, "fast_bf16": 3}[precision]
    check_info(info, k)
    if precision == "fast":      # the 16-bit passes, not the rescan, produced the answer
        assert sum(info["exact_rows"]) <= info["passes"] * -(-N // 64), info


# ---- 2. the widest widths, bit identity only -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(2560, 21), (4096, 25)])
def test_wider_widths(mmf, d, k):
    X = gauss(500 + d, 300, d).cuda()
    idx, val, info = mmf.simtopk_wide_any_k(X, metric="cosine", k=k, return_info=True)
    print(f"d={d} k={k}: {info}")
    assert_same((idx, val), exact(mmf, X, metric="cosine", k=k))
    check_info(info, k)


# ---- 3. the CPU oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "neg_sq_l2"])
def test_against_the_oracle(mmf, metric):
    X = np.random.RandomState(7).randn(300, 1100).astype(np.float32)
    ridx, rval = oracle.simtopk(X, metric=metric, k=30)
    idx, val, info = mmf.simtopk_wide_any_k(torch.from_numpy(X).cuda(), metric=metric, k=30, return_info=True)
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(val.cpu().numpy().view(np.int32), rval.view(np.int32))
    check_info(info, 30)


# ---- 4. a block of ties across the pass boundary --------------------------------------------------------------------------------------------
def test_tie_block_across_the_pass_boundary(mmf):
    rs = np.random.RandomState(11)
    row = rs.randn(1, 1100).astype(np.float32)
    Y = np.concatenate([rs.randn(300, 1100).astype(np.float32), np.repeat(row, 100, 0)])
    X = 3.0 * row + 0.05 * rs.randn(64, 1100).astype(np.float32)         # near the repeated row: its copies lead every row's order
    Xc, Yc = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    idx, val, info = mmf.simtopk_wide_any_k(Xc, Yc, metric="dot", k=40, exclude_self=False, return_info=True)
    print(f"tie block: {info}")
    assert_same((idx, val), exact(mmf, Xc, Yc, metric="dot", k=40, exclude_self=False))
    check_info(info, 40)
    assert info["yield"][0] == 20
    assert torch.equal(idx.cpu(), torch.arange(300, 340).expand(64, 40)), "the tie run continues ascending across the pass boundary"


# ---- 5. exact duplicates among the queries ------------------------------------------------------------------------------------------------------
def test_duplicate_queries(mmf):
    X = gauss(13, 200, 1100).repeat(4, 1).cuda()
    idx, val, info = mmf.simtopk_wide_any_k(X, metric="cosine", k=30, exclude_self=True, return_info=True)
    assert_same((idx, val), exact(mmf, X, metric="cosine", k=30, exclude_self=True))
    check_info(info, 30)


# ---- 6. id offsets: an overlapping and a disjoint self column ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_offset,col_offset", [(500, 0), (0, 300), (5000, 0)])
def test_offsets(mmf, row_offset, col_offset):
    X, Y = case_inputs(1100, "f32", True)
    X, Y = X[:700].cuda(), Y.cuda()
    kw = dict(metric="neg_sq_l2", k=32, exclude_self=True, row_offset=row_offset, col_offset=col_offset)
    idx, val, info = mmf.simtopk_wide_any_k(X, Y, return_info=True, **kw)
    assert_same((idx, val), exact(mmf, X, Y, **kw))
    check_info(info, 32)


def test_rows_of_the_candidate_block(mmf):
    """X a row slice of Y (the row-sharded call): the query side is a view into the candidate side's images and scalars."""
    Y, _ = case_inputs(1100, "f32", False)
    Y = Y.cuda()
    X = Y[640:1400]
    kw = dict(metric="cosine", k=32, exclude_self=True, row_offset=640)
    idx, val, info = mmf.simtopk_wide_any_k(X, Y, return_info=True, **kw)
    assert_same((idx, val), exact(mmf, X, Y, **kw))
    check_info(info, 32)


# ---- 7. fewer columns left than a pass holds ---------------------------------------------------------------------------------------------------
def test_fewer_columns_left_than_a_pass_holds(mmf):
    """m = 30, k = 26: after the first 19 entries ten columns are left, the lists of the second pass come up short of the depth, and
    every row takes the exact rescan with its floor."""
    X = gauss(19, 30, 1100).cuda()
    idx, val, info = mmf.simtopk_wide_any_k(X, metric="neg_sq_l2", k=26, return_info=True)
    assert_same((idx, val), exact(mmf, X, metric="neg_sq_l2", k=26))
    check_info(info, 26)


# ---- 8. the operating points do not change the bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,col_splits", [(None, 1), (None, 2), (None, 4), (("MMF_ANYK_SHORT_DIV", "16"), 0), (("MMF_ANYK_SHORT_DIV", "256"), 0),
                                            (("MMF_WIDE_SINK", "0"), 0)])
def test_operating_points(mmf, monkeypatch, env, col_splits):
    X, _ = case_inputs(1100, "f32", False)
    X = X.cuda()
    if env is not None:
        monkeypatch.setenv(*env)
    idx, val, st, info = mmf.simtopk_wide_any_k(X, metric="cosine", k=50, col_splits=col_splits, return_stats=True, return_info=True)
    print(f"{env} col_splits={col_splits}: {info}")
    assert_same((idx, val), exact(mmf, X, metric="cosine", k=50))
    check_info(info, 50)
    if col_splits:
        assert st["col_splits"] == col_splits


# ---- 9. rows flagged in the first pass still leave floors -------------------------------------------------------------------------------------------
def test_rows_flagged_in_the_first_pass(mmf, monkeypatch):
    X, _ = case_inputs(1100, "f32", False)
    X = X.cuda()
    ref = exact(mmf, X, metric="cosine", k=50)
    monkeypatch.setenv("MMF_DEBUG_FLAG_ROWS", "100")
    idx, val, info = mmf.simtopk_wide_any_k(X, metric="cosine", k=50, return_info=True)
    assert_same((idx, val), ref)
    check_info(info, 50)
    assert info["exact_rows"][0] >= 100, info


# ---- 10. where one pass serves, the call is the wide fast call -------------------------------------------------------------------------------------
def test_single_pass_shape(mmf):
    X, _ = case_inputs(1100, "f32", False)
    X = X.cuda()
    idx, val, st, info = mmf.simtopk_wide_any_k(X, metric="cosine", k=20, exclude_self=False, return_stats=True, return_info=True)
    assert_same((idx, val), mmf.ops.simtopk(X, metric="cosine", k=20, exclude_self=False, precision="fast"))
    assert info["passes"] == 1 and info["yield"] == [20] and st["precision_used"] == 2


# ---- 11. the router ---------------------------------------------------------------------------------------------------------------------------------
def test_router(mmf):
    X, _ = case_inputs(1100, "f32", False)
    X = X.cuda()
    ref = exact(mmf, X, metric="cosine", k=32)
    for precision, used in (("fast", 2), ("fast_bf16", 3), ("exact", 1), ("auto", 1)):      # n = 2001: not a shape "auto" takes
        idx, val, st = mmf.wide_anyk.simtopk(X, metric="cosine", k=32, precision=precision, return_stats=True)
        assert_same((idx, val), ref)
        assert st["precision_used"] == used, (precision, st)
    # d <= 1024: the narrow call, which serves k + self > 20 there in passes of its own
    Xn = gauss(23, 500, 600).cuda()
    idx, val, st = mmf.wide_anyk.simtopk(Xn, metric="cosine", k=30, precision="fast", return_stats=True)
    assert_same((idx, val), exact(mmf, Xn, metric="cosine", k=30))
    assert st["precision_used"] == 2
    assert mmf.wide_anyk._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "wide_anyk_timing.txt"))
    assert not mmf.wide_anyk._auto_takes(2001, 1100, 32)
    if mmf.wide_anyk._AUTO_SHAPES:      # what the timing file shows ahead, and nothing it does not show
        assert mmf.wide_anyk._auto_takes(65536, 1536, 32) and mmf.wide_anyk._auto_takes(16384, 1536, 32) and mmf.wide_anyk._auto_takes(65536, 2560, 32)
        assert not mmf.wide_anyk._auto_takes(16384, 1536, 64) and not mmf.wide_anyk._auto_takes(65536, 2560, 64) and not mmf.wide_anyk._auto_takes(65536, 4096, 32)


# ---- 12. a busy non-default stream -------------------------------------------------------------------------------------------------------------------
def test_behind_a_closed_gate(mmf):
    def make(which):
        rs = np.random.RandomState(17 if which == "truth" else 18)
        return [torch.from_numpy(rs.randn(600, 1100).astype(np.float32))]

    def entry(X):
        return list(mmf.simtopk_wide_any_k(X, metric="cosine", k=30))

    def reference(X):
        ridx, rval = oracle.simtopk(X, metric="cosine", k=30)
        return [ridx, rval]
    sg.run_gated(entry, make, reference, name="simtopk_wide_any_k", calls=2)


# ---- 13. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mmf):
    X = torch.randn(64, 600, device="cuda")
    with pytest.raises(RuntimeError, match="mmf_simtopk_fast_anyk"):
        mmf.simtopk_wide_any_k(X, metric="cosine", k=50, exclude_self=False)
    X = torch.randn(64, 5000, device="cuda")
    for precision in ("fast", "fast_bf16", "auto"):
        with pytest.raises(RuntimeError, match="d = 5000 is beyond the wide 16-bit scan"):
            mmf.simtopk_wide_any_k(X, metric="cosine", k=30, precision=precision)
    L = mmf._lib.lib()
    X = torch.randn(64, 1100, device="cuda")
    idx = torch.empty((64, 30), dtype=torch.int64, device="cuda")
    val = torch.empty((64, 30), dtype=torch.float32, device="cuda")
    ev = torch.cuda.Event()
    ev.record()
    opts = mmf._lib.SimtopkOpts(2, 0, 0, 0, ctypes.c_void_p(ev.cuda_event))
    rc = L.mmf_simtopk_wide_anyk(X.data_ptr(), 64, None, 0, 1100, 0, 1, 1.0, 30, 0, 0, 0, idx.data_ptr(), val.data_ptr(), ctypes.byref(opts),
                                 None, 0, None, None)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and b"select_wait_event" in L.mmf_last_error()
