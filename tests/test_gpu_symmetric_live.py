"""The symmetric 16-bit scan with thresholds that rise while its second launch runs and a schedule that looks back (DESIGN.md
§4.1, MMF_SYMMETRIC_LIVE unset or 1) against the frozen image and the forward schedule (MMF_SYMMETRIC_LIVE=0), against the plain
scan (MMF_SYMMETRIC=0) and against the oracle: ids and scores bit for bit.  Also the work tables a cached workspace keeps
between calls."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

KEYS = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G", "MMF_SYMMETRIC_LIVE")


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available()
    return m


@contextmanager
def switches(symmetric, G=None, live=None):
    old = {k: os.environ.get(k) for k in KEYS}
    for k, v in zip(KEYS, (symmetric, G, live)):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make(n, d, seed, unit=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True) if unit else x


def sym_grid(mmf, n, G):
    return 2 * mmf._lib.lib().mmf_debug_symmetric_schedule((n + 255) // 256, G, 0, None, 0)


def three(mmf, X, G, **kw):
    """The live symmetric scan's result and stats, after comparing it with the frozen symmetric scan and with the plain scan."""
    n = X.shape[0]
    kw.setdefault("metric", "cosine")
    kw.setdefault("k", 5)
    with switches(1, G, None):
        i1, v1, s1 = mmf.simtopk(X, return_stats=True, query_order="off", **kw)
    with switches(1, G, 0):
        i2, v2, s2 = mmf.simtopk(X, return_stats=True, query_order="off", **kw)
    with switches(0):
        i0, v0, s0 = mmf.simtopk(X, return_stats=True, query_order="off", **kw)
    assert s1["scan_grid"] == sym_grid(mmf, n, G) == s2["scan_grid"] and s0["scan_grid"] != s1["scan_grid"]
    assert torch.equal(i1, i0) and torch.equal(v1, v0), "live symmetric scan differs from the plain scan"
    assert torch.equal(i2, i0) and torch.equal(v2, v0), "frozen symmetric scan differs from the plain scan"
    return i1, v1, s1, s2


def check_oracle(X, idx, val, metric="cosine", k=5, exclude_self=True, rows=None):
    Xh = X.cpu().numpy()
    n = X.shape[0]
    if rows is None:
        ri, rv = oracle.simtopk(Xh, metric=metric, k=k, exclude_self=exclude_self)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv)
        return
    for lo in rows:
        hi = min(lo + 32, n)
        ri, rv = oracle.simtopk(Xh[lo:hi], Xh, metric=metric, k=k, exclude_self=exclude_self, row_offset=lo)
        assert np.array_equal(idx[lo:hi].cpu().numpy(), ri) and np.array_equal(val[lo:hi].cpu().numpy(), rv), lo


@pytest.mark.parametrize("ns", [3, 4, 5, 6, 7, 8, 9])
def test_wrap_of_the_backward_range(mmf, ns):
    """ns super-blocks of one row block, odd and even, the last row block ragged: super-block a scans a - h .. a - 1, which wraps
    below 0 for a < h.  Gaussian rows stay far inside the capacities with frozen thresholds too, so nothing may fall back."""
    n = 256 * ns - 37
    X = make(n, 512, 300 + ns)
    i, v, st, st_frozen = three(mmf, X, 1)
    assert st["fallback_rows"] == 0 and st_frozen["fallback_rows"] == 0
    check_oracle(X, i, v)


@pytest.mark.parametrize("n,G", [(2300, 2), (1900, 3), (2700, 2)])
def test_left_over_row_blocks(mmf, n, G):
    X = make(n, 512, 400 + n)
    i, v, st, _ = three(mmf, X, G)
    assert st["fallback_rows"] == 0
    check_oracle(X, i, v)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_planted_neighbours_across_super_blocks(mmf, precision):
    """Nine super-blocks of one row block; rows i + 256 delta (delta = 1 .. 8) are X[i] plus noise of relative size 0.02: every row's
    top 5 lies in other super-blocks, half of it arrives through the received lists, and the thresholds rise steeply while the
    symmetric launch runs."""
    n = 2304
    X = make(n, 512, 500)
    g = torch.Generator(device="cuda").manual_seed(501)
    for delta in range(1, 9):
        noise = torch.randn((256, 512), generator=g, device="cuda")
        noise = 0.02 * noise / noise.norm(dim=1, keepdim=True)
        X[256 * delta:256 * (delta + 1)] = X[:256] + noise
    X = X / X.norm(dim=1, keepdim=True)
    i, v, st, _ = three(mmf, X, 1, precision=precision)
    check_oracle(X, i, v)
    assert ((i % 256) == (torch.arange(n, device="cuda") % 256)[:, None]).all()      # the planted copies, nothing else


def test_more_workgroups_than_compute_units(mmf):
    """18 super-blocks of 16 row blocks, 289 row blocks: workgroups that have finished, that run and that have not started in one
    launch.  (The frozen thresholds' model gives 24 received entries per row here, well inside 512.)"""
    n = 73728 + 100
    X = make(n, 512, 600)
    i, v, st, st_frozen = three(mmf, X, 16)
    assert st["fallback_rows"] == 0 and st_frozen["fallback_rows"] == 0
    check_oracle(X, i, v, rows=[0, 36864, 73728, n - 32])


def test_dot_with_self(mmf):
    X = make(1500, 512, 700, unit=False) * 0.3
    i, v, st, _ = three(mmf, X, 2, metric="dot", exclude_self=False)
    check_oracle(X, i, v, metric="dot", exclude_self=False)


def test_the_switch_is_read_per_call(mmf):
    X = make(2000, 512, 800)
    with switches(1, 1, 0):
        i0, v0, s0 = mmf.simtopk(X, metric="cosine", k=5, return_stats=True, query_order="off")
    with switches(1, 1, 1):
        i1, v1, s1 = mmf.simtopk(X, metric="cosine", k=5, return_stats=True, query_order="off")
    with switches(1, 1, 0):
        i2, v2, s2 = mmf.simtopk(X, metric="cosine", k=5, return_stats=True, query_order="off")
    assert s0["scan_grid"] == s1["scan_grid"] == s2["scan_grid"] == sym_grid(mmf, 2000, 1)
    assert torch.equal(i0, i1) and torch.equal(v0, v1) and torch.equal(i0, i2) and torch.equal(v0, v2)
    check_oracle(X, i1, v1)


def test_kept_work_tables_follow_rows_and_group(mmf):
    """The work tables stay in the cached workspace from call to call: a repeated call reuses them, a call with another G, another
    row count or another path in between must not leave a later call with stale ones."""
    X, Y = make(2300, 512, 900), make(1800, 512, 901)
    want = {}
    with switches(0):
        for name, Z in (("X", X), ("Y", Y)):
            want[name] = mmf.simtopk(Z, metric="cosine", k=5, query_order="off")
    plan = [("X", X, 1), ("X", X, 1), ("X", X, 2), ("X", X, 1), ("Y", Y, 1), ("X", X, 1), ("X", X, 3), ("Y", Y, 3), ("Y", Y, 3)]
    for step, (name, Z, G) in enumerate(plan):
        with switches(1, G, None):
            i, v, st = mmf.simtopk(Z, metric="cosine", k=5, return_stats=True, query_order="off")
        assert st["scan_grid"] == sym_grid(mmf, Z.shape[0], G), step
        assert torch.equal(i, want[name][0]) and torch.equal(v, want[name][1]), step
        if step == 4:      # another entry takes the same workspace in between
            with switches(0):
                mmf.simtopk(make(3000, 256, 902), metric="cosine", k=5)
