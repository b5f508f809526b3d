"""The symmetric 16-bit scan (X against itself: every pair of rows multiplied once, DESIGN.md §4.1 "Symmetric scan") against
today's scan (MMF_SYMMETRIC=0) and against the oracle, bit for bit in ids and scores; and calls it does not apply to, which
must not notice the switch."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available()
    return m


@contextmanager
def symmetric(mode, G=None):
    keys = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G")
    old = {k: os.environ.get(k) for k in keys}
    os.environ["MMF_SYMMETRIC"] = str(mode)
    if G is None:
        os.environ.pop("MMF_SYMMETRIC_G", None)
    else:
        os.environ["MMF_SYMMETRIC_G"] = str(G)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make(n, d, seed, unit=True, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    if unit:
        x = x / x.norm(dim=1, keepdim=True)
    return x.to(dtype)


def sym_grid(n, G):
    import multimodal_fusion_amd as m
    nb = (n + 255) // 256
    return 2 * m._lib.lib().mmf_debug_symmetric_schedule(nb, G, 0, None, 0)


def both(mmf, X, G, **kw):
    """(result with the symmetric scan forced, result with it off); asserts which path ran and that the bits agree."""
    n = X.shape[0]
    with symmetric(1, G):
        i1, v1, s1 = mmf.simtopk(X, return_stats=True, query_order="off", **kw)
    with symmetric(0):
        i0, v0, s0 = mmf.simtopk(X, return_stats=True, query_order="off", **kw)
    assert s1["scan_grid"] == sym_grid(n, G), (s1, sym_grid(n, G))
    assert s0["scan_grid"] != s1["scan_grid"]
    assert s1["precision_used"] == s0["precision_used"]
    assert torch.equal(i1, i0) and torch.equal(v1, v0)
    return (i1, v1, s1), (i0, v0, s0)


def check_oracle(X, idx, val, metric, k, exclude_self, rows=None):
    Xh = X.float().cpu().numpy() if X.dtype != torch.float32 else X.cpu().numpy()
    n = X.shape[0]
    if rows is None:
        ri, rv = oracle.simtopk(Xh, metric=metric, k=k, exclude_self=exclude_self)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv)
        return
    for lo in rows:
        hi = min(lo + 32, n)
        ri, rv = oracle.simtopk(Xh[lo:hi], Xh, metric=metric, k=k, exclude_self=exclude_self, row_offset=lo)
        assert np.array_equal(idx[lo:hi].cpu().numpy(), ri) and np.array_equal(val[lo:hi].cpu().numpy(), rv), lo


# (n, G): ns = 2, 3, 4, 5, 8 super-blocks, n never a multiple of 256; (2300, 2) and (1900, 3): left-over row blocks (the last
# super-block takes them: 4 x 2 + 1 and 2 x 3 + 2 row blocks)
@pytest.mark.parametrize("n,G", [(300, 1), (700, 1), (1000, 1), (1100, 1), (2000, 1), (2300, 2), (1900, 3), (2700, 2)])
def test_super_block_counts(mmf, n, G):
    X = make(n, 512, 100 + n)
    (i, v, st), _ = both(mmf, X, G, metric="cosine", k=5)
    assert st["fallback_rows"] == 0
    check_oracle(X, i, v, "cosine", 5, True)


def test_second_launch_without_work_leaves_no_stale_lists(mmf):
    """Two super-blocks: everything is a plain pair and the second launch is idle; its list pair must read as empty whatever an
    earlier call left in the (cached) workspace."""
    with symmetric(0):
        mmf.simtopk(make(3000, 512, 5), metric="cosine", k=5, col_splits=8)        # many lists per row, all of them used
    X = make(500, 512, 6)
    (i, v, st), _ = both(mmf, X, 1, metric="cosine", k=5)
    assert st["fallback_rows"] == 0
    check_oracle(X, i, v, "cosine", 5, True)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("k", [1, 5, 10])
def test_metrics_self_and_k(mmf, metric, exclude_self, k):
    n = 1500
    X = make(n, 500, 7, unit=(metric == "cosine")) * (1.0 if metric == "cosine" else 0.3)
    (i, v, st), _ = both(mmf, X, 2, metric=metric, k=k, exclude_self=exclude_self)
    check_oracle(X, i, v, metric, k, exclude_self)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_row_and_operand_types(mmf, dtype, precision):
    X = make(1300, 512, 11, dtype=dtype)
    (i, v, st), _ = both(mmf, X, 1, metric="cosine", k=5, precision=precision)
    check_oracle(X, i, v, "cosine", 5, True)


def test_exact_duplicate_rows_tie_by_id(mmf):
    X = make(2000, 512, 21)
    X[100:104] = X[50]
    X[900] = X[50]
    X[1999] = X[50]
    X[1200:1203] = X[1700]
    (i, v, st), _ = both(mmf, X, 1, metric="cosine", k=5)
    check_oracle(X, i, v, "cosine", 5, True)
    assert i[50].tolist() == [100, 101, 102, 103, 900]


def test_identical_rows_beyond_the_received_capacity_take_the_exact_rescan(mmf):
    """2048 identical rows spread over all 8 super-blocks: each of them would receive 3/8 of the others (768) from the scans of
    other rows.  With 16 of them among a wave's 32 queries the waves' logs (4096 entries) fill up first; either way the rows are
    flagged and rescanned exactly.  (The next test fills the received lists without filling a log.)"""
    n, G = 4096, 2
    X = make(n, 512, 31)
    X[::2] = X[0]
    (i, v, st), (_, _, s0) = both(mmf, X, G, metric="cosine", k=5)
    assert st["fallback_rows"] > 0
    check_oracle(X, i, v, "cosine", 5, True, rows=[0, 1000, 2048, n - 32])
    assert i[0].tolist() == [2, 4, 6, 8, 10] and i[2].tolist() == [0, 4, 6, 8, 10]


def test_a_full_received_list_takes_the_exact_rescan(mmf):
    """One row copied to every 10th row of 16384 (8 super-blocks): a copy receives 3/8 of the 1638 others, 614 entries — more than
    the 512 its received list holds — while a wave has 3 or 4 copies among its queries, about 2400 log entries of 4096: the
    logs hold everything and the filing of the logs finds the lists full."""
    n, G = 16384, 8
    X = make(n, 512, 71)
    X[::10] = X[0]
    (i, v, st), _ = both(mmf, X, G, metric="cosine", k=5)
    assert st["fallback_rows"] > 0
    check_oracle(X, i, v, "cosine", 5, True, rows=[0, 5000, n - 32])
    assert i[0].tolist() == [10, 20, 30, 40, 50] and i[10].tolist() == [0, 20, 30, 40, 50]


def test_default_path_with_left_over_row_blocks(mmf):
    """The path as a caller gets it (no switch set, default super-block size) at a row count with left-over row blocks and a ragged
    last row block: 131072 + 300 rows are 16 super-blocks, the last of 34 row blocks.  Same bits as the plain scan, no row flagged."""
    n = 131072 + 300
    X = make(n, 512, 81)
    old = {k: os.environ.pop(k, None) for k in ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G")}
    try:
        i1, v1, s1 = mmf.simtopk(X, metric="cosine", k=5, return_stats=True)
    finally:
        for k, val in old.items():
            if val is not None:
                os.environ[k] = val
    with symmetric(0):
        i0, v0, s0 = mmf.simtopk(X, metric="cosine", k=5, return_stats=True)
    assert s1["scan_grid"] == sym_grid(n, 32) and s0["scan_grid"] != s1["scan_grid"]
    assert s1["fallback_rows"] == 0 and s1["query_order"] == 0
    assert torch.equal(i1, i0) and torch.equal(v1, v0)
    check_oracle(X, i1, v1, "cosine", 5, True, rows=[0, 65536, 131072, n - 32])


def same_with_switch(call):
    with symmetric(1, 1):
        a = call()
    with symmetric(0):
        b = call()
    assert a[2]["scan_grid"] == b[2]["scan_grid"] and a[2]["col_splits"] == b[2]["col_splits"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_calls_it_does_not_apply_to_are_unchanged(mmf):
    n = 1500
    X, Y = make(n, 512, 41), make(n, 512, 42)
    same_with_switch(lambda: mmf.simtopk(X, Y, metric="cosine", k=5, return_stats=True))                       # Y != X
    same_with_switch(lambda: mmf.simtopk(X[256:1024], X, metric="cosine", k=5, exclude_self=True, row_offset=256,
                                         return_stats=True))                                                   # X a slice of Y
    same_with_switch(lambda: mmf.simtopk(X, metric="neg_sq_l2", k=5, return_stats=True))                       # an L2 metric
    same_with_switch(lambda: mmf.simtopk(X, metric="rbf", lam=0.5, k=5, return_stats=True))
    same_with_switch(lambda: mmf.simtopk(X, metric="cosine", k=11, return_stats=True))                         # k + self > 11
    same_with_switch(lambda: mmf.simtopk(make(n, 1024, 43), metric="cosine", k=5, precision="fast", return_stats=True))   # d = 1024
    same_with_switch(lambda: mmf.simtopk(make(n, 256, 44), metric="cosine", k=5, return_stats=True))           # d = 256
    same_with_switch(lambda: mmf.simtopk(X, metric="cosine", k=5, col_splits=4, return_stats=True))            # forced col_splits
    same_with_switch(lambda: mmf.simtopk_segmented(X, ptr=[0, 700, n], k=5, precision="fast", return_stats=True))   # segmented entry


def test_panel_entry_is_unchanged(mmf):
    ops = mmf.ops
    N, d, k = 2048, 512, 5
    X = make(N, d, 51)
    maxn = torch.zeros(1, device="cuda")
    scal = torch.empty(N, device="cuda")
    ops.row_scalars(X, "cosine", scal, maxn)
    max4 = torch.zeros(4, device="cuda")
    Z = torch.zeros((N + 256, d), dtype=torch.float16, device="cuda")
    zn, rn, un, cb = (torch.zeros(N + 256, device="cuda") for _ in range(4))
    ops.prep_rows(X, "cosine", "f16", scal, maxn, Z[:N], zn[:N], rn[:N], un[:N], cb[:N], max4)
    cbc = torch.full((N + 256,), float("-inf"), device="cuda")
    cbc[:N] = cb[:N]
    ev = torch.cuda.Event()
    ev.record()
    panels = [dict(Z=Z, cb=cbc, m=N, m_pad=N, seg_len=N, seg_stride=N, id_base=0, event=ev)]
    q = dict(Z=Z, scal=scal, zn=zn, rn=rn, un=un, cb=cb)
    same_with_switch(lambda: ops.simtopk_panels(X, X, q, scal, panels, max4, metric="cosine", k=k, exclude_self=True,
                                                return_stats=True, query_order="off"))


def test_applied_query_order_keeps_todays_path(mmf):
    X = make(1500, 512, 61)
    with symmetric(1, 1):
        i1, v1, s1 = mmf.simtopk(X, metric="cosine", k=5, return_stats=True, query_order="on")
    with symmetric(0):
        i0, v0, s0 = mmf.simtopk(X, metric="cosine", k=5, return_stats=True, query_order="on")
    assert s1["query_order"] == 1 and s1["scan_grid"] == s0["scan_grid"]
    assert torch.equal(i1, i0) and torch.equal(v1, v0)
