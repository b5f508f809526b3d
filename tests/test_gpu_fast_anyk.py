"""The 16-bit top-k for any k (fast_anyk.*, include/ext/mmf_hg_fast_anyk.h): several passes of the 16-bit scan,
the later ones under per-row ceilings, each re-ranked exactly.

The reference is always ``ops.simtopk(..., precision="exact")`` on the same inputs (code this feature does not touch), compared
bit for bit, ids and values; one case also compares against the CPU oracle.  With f16 operands the test caps the rows that took
the exact rescan at ceil(n / 64) per pass, so that a pass cannot come from the rescan: tests/test_fast_anyk_cpu.py counts, on
these same inputs and from the reference alone, the already-emitted columns that slip under a row's ceiling."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg  # noqa: E402
from test_gpu_segmented import assert_same  # noqa: E402
from test_fast_anyk_cpu import CASES, N, case_inputs, lam_for  # noqa: E402

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


# ---- 1. every kernel shape, both operand types, X against itself and against Y ---------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_same_bits_as_the_exact_call_on_every_kernel(mmf, d, k, metric, dtype, two_sided, precision):
    X, Y = case_inputs(d, dtype, two_sided)
    X = X.cuda()
    Y = None if Y is None else Y.cuda()
    kw = dict(metric=metric, lam=lam_for(d), k=k)
    idx, val, st, info = mmf.simtopk_fast_any_k(X, Y, precision=precision, return_stats=True, return_info=True, **kw)
    print(f"d={d} k={k} {metric} {dtype} two_sided={two_sided} {precision}: {info}")
    assert_same((idx, val), exact(mmf, X, Y, **kw))
    assert st["precision_used"] == {"fast": 2, "fast_bf16": 3}[precision]
    check_info(info, k)
    if precision == "fast":      # the 16-bit passes, not the rescan, produced the answer
        assert sum(info["exact_rows"]) <= info["passes"] * -(-N // 64), info


# ---- 2. the CPU oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "neg_sq_l2"])
def test_against_the_oracle(mmf, metric):
    X = np.random.RandomState(7).randn(300, 40).astype(np.float32)
    ridx, rval = oracle.simtopk(X, metric=metric, k=50)
    idx, val, info = mmf.simtopk_fast_any_k(torch.from_numpy(X).cuda(), metric=metric, k=50, return_info=True)
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(val.cpu().numpy().view(np.int32), rval.view(np.int32))
    check_info(info, 50)


# ---- 3. a block of ties across the pass boundary --------------------------------------------------------------------------------------------
def test_tie_block_across_the_pass_boundary(mmf):
    rs = np.random.RandomState(11)
    row = rs.randn(1, 64).astype(np.float32)
    Y = np.concatenate([rs.randn(300, 64).astype(np.float32), np.repeat(row, 100, 0)])
    X = 3.0 * row + 0.05 * rs.randn(64, 64).astype(np.float32)           # near the repeated row: its copies lead every row's order
    Xc, Yc = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    idx, val, info = mmf.simtopk_fast_any_k(Xc, Yc, metric="dot", k=60, exclude_self=False, return_info=True)
    print(f"tie block: {info}")
    assert_same((idx, val), exact(mmf, Xc, Yc, metric="dot", k=60, exclude_self=False))
    check_info(info, 60)
    assert torch.equal(idx.cpu(), torch.arange(300, 360).expand(64, 60)), "the tie run continues ascending across the pass boundary"


# ---- 4. exact duplicates among the queries ------------------------------------------------------------------------------------------------------
def test_duplicate_queries(mmf):
    base = np.random.RandomState(13).randn(200, 96).astype(np.float32)
    X = torch.from_numpy(np.tile(base, (4, 1))).cuda()
    idx, val, info = mmf.simtopk_fast_any_k(X, metric="cosine", k=50, exclude_self=True, return_info=True)
    assert_same((idx, val), exact(mmf, X, metric="cosine", k=50, exclude_self=True))
    check_info(info, 50)


# ---- 5. id offsets: an overlapping and a disjoint self column ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_offset,col_offset", [(500, 0), (0, 300), (5000, 0)])
def test_offsets(mmf, row_offset, col_offset):
    X, Y = case_inputs(300, "f32", True)
    X, Y = X[:700].cuda(), Y.cuda()
    kw = dict(metric="neg_sq_l2", k=64, exclude_self=True, row_offset=row_offset, col_offset=col_offset)
    idx, val, info = mmf.simtopk_fast_any_k(X, Y, return_info=True, **kw)
    assert_same((idx, val), exact(mmf, X, Y, **kw))
    check_info(info, 64)


def test_rows_of_the_candidate_block(mmf):
    """X a row slice of Y (the row-sharded call): the query side is a view into the candidate side's images and scalars."""
    Y, _ = case_inputs(300, "f32", False)
    Y = Y.cuda()
    X = Y[640:1400]
    kw = dict(metric="cosine", k=64, exclude_self=True, row_offset=640)
    idx, val, info = mmf.simtopk_fast_any_k(X, Y, return_info=True, **kw)
    assert_same((idx, val), exact(mmf, X, Y, **kw))
    check_info(info, 64)


def test_fewer_columns_left_than_a_pass_holds(mmf):
    """m = 50, k = 46: after the first 43 entries six columns are left, the lists of the second pass come up short of the depth, and
    every row takes the exact rescan with its floor."""
    X = torch.from_numpy(np.random.RandomState(19).randn(50, 40).astype(np.float32)).cuda()
    idx, val, info = mmf.simtopk_fast_any_k(X, metric="neg_sq_l2", k=46, return_info=True)
    assert_same((idx, val), exact(mmf, X, metric="neg_sq_l2", k=46))
    check_info(info, 46)


def test_query_order_in_the_first_pass(mmf):
    """The scan of the first pass takes its queries in another order (MMF_QUERY_ORDER_ON): the floors are still the rows'."""
    import ctypes
    X, _ = case_inputs(300, "f32", False)
    X = X.cuda()
    n, k = X.shape[0], 64
    idx = torch.empty((n, k), dtype=torch.int64, device="cuda")
    val = torch.empty((n, k), dtype=torch.float32, device="cuda")
    opts = mmf._lib.SimtopkOpts(2, 0, 0, mmf._lib.QUERY_ORDERS["on"], None)
    stats, info = mmf._lib.SimtopkStats(), mmf._lib.FastAnykInfo()
    rc = mmf._lib.lib().mmf_simtopk_fast_anyk(X.data_ptr(), n, None, 0, 300, 0, 1, 1.0, k, 1, 0, 0, idx.data_ptr(), val.data_ptr(), ctypes.byref(opts),
                                              ctypes.byref(stats), 0, mmf.ops._stream(X.device), ctypes.byref(info))
    assert rc == 0 and stats.query_order == 1 and info.passes >= 2
    assert_same((idx, val), exact(mmf, X, metric="cosine", k=k))


def test_router(mmf):
    X, _ = case_inputs(300, "f32", False)
    X = X.cuda()
    ref = exact(mmf, X, metric="cosine", k=64)
    _, _, st = mmf.fast_anyk.simtopk(X, metric="cosine", k=64, return_stats=True)                       # n = 2001: not a shape "auto" takes
    assert st["precision_used"] == 1
    for precision, used in (("fast", 2), ("fast_bf16", 3), ("exact", 1)):
        idx, val, st = mmf.fast_anyk.simtopk(X, metric="cosine", k=64, precision=precision, return_stats=True)
        assert_same((idx, val), ref)
        assert st["precision_used"] == used
    assert mmf.fast_anyk._auto_takes(65536, 1024, 32) and mmf.fast_anyk._auto_takes(262144, 512, 128)
    assert not mmf.fast_anyk._auto_takes(65536, 512, 128) and not mmf.fast_anyk._auto_takes(2001, 300, 64)


# ---- 6. rows flagged in the first pass still leave floors -------------------------------------------------------------------------------------------
def test_rows_flagged_in_the_first_pass(mmf, monkeypatch):
    X, _ = case_inputs(300, "f32", False)
    X = X.cuda()
    ref = exact(mmf, X, metric="cosine", k=64)
    monkeypatch.setenv("MMF_DEBUG_FLAG_ROWS", "100")
    idx, val, info = mmf.simtopk_fast_any_k(X, metric="cosine", k=64, return_info=True)
    assert_same((idx, val), ref)
    check_info(info, 64)
    assert info["exact_rows"][0] >= 100, info


# ---- 7. the operating point and the column splits do not change the bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("env,col_splits", [("16", 0), ("256", 0), (None, 1), (None, 4)])
def test_operating_points(mmf, monkeypatch, env, col_splits):
    X, _ = case_inputs(300, "f32", False)
    X = X.cuda()
    if env is not None:
        monkeypatch.setenv("MMF_ANYK_SHORT_DIV", env)
    idx, val, info = mmf.simtopk_fast_any_k(X, metric="cosine", k=100, col_splits=col_splits, return_info=True)
    print(f"MMF_ANYK_SHORT_DIV={env} col_splits={col_splits}: {info}")
    assert_same((idx, val), exact(mmf, X, metric="cosine", k=100))
    check_info(info, 100)


# ---- 8. where one pass serves, the call is the fast call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(300, 44), (600, 20)])
def test_single_pass_shapes(mmf, d, k):
    X, _ = case_inputs(d, "f32", False)
    X = X.cuda()
    idx, val, info = mmf.simtopk_fast_any_k(X, metric="cosine", k=k, exclude_self=False, return_info=True)
    assert_same((idx, val), mmf.ops.simtopk(X, metric="cosine", k=k, exclude_self=False, precision="fast"))
    assert info["passes"] == 1 and info["yield"] == [k]


# ---- 9. a busy non-default stream -------------------------------------------------------------------------------------------------------------------
def test_behind_a_closed_gate(mmf):
    def make(which):
        rs = np.random.RandomState(17 if which == "truth" else 18)
        return [torch.from_numpy(rs.randn(600, 72).astype(np.float32))]

    def entry(X):
        return list(mmf.simtopk_fast_any_k(X, metric="cosine", k=60))

    def reference(X):
        ridx, rval = oracle.simtopk(X, metric="cosine", k=60)
        return [ridx, rval]
    sg.run_gated(entry, make, reference, name="simtopk_fast_any_k", calls=2)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mmf):
    import ctypes
    X = torch.randn(64, 1100, device="cuda")
    with pytest.raises(RuntimeError, match="d = 1100, k = 21"):
        mmf.simtopk_fast_any_k(X, metric="cosine", k=21, exclude_self=False)
    L = mmf._lib.lib()
    X = torch.randn(64, 40, device="cuda")
    idx = torch.empty((64, 50), dtype=torch.int64, device="cuda")
    val = torch.empty((64, 50), dtype=torch.float32, device="cuda")
    ev = torch.cuda.Event()
    ev.record()
    opts = mmf._lib.SimtopkOpts(2, 0, 0, 0, ctypes.c_void_p(ev.cuda_event))
    rc = L.mmf_simtopk_fast_anyk(X.data_ptr(), 64, None, 0, 40, 0, 1, 1.0, 50, 0, 0, 0, idx.data_ptr(), val.data_ptr(), ctypes.byref(opts),
                                 None, 0, None, None)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and b"select_wait_event" in L.mmf_last_error()
