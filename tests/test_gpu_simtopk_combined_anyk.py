"""The combined top-k for any k on the MI355X (mmf_simtopk_combined_anyk / mmf_simtopk_combined_xy_anyk).

Every case checks three things: the indices are those of the numpy reference of tests/test_gpu_simtopk_combined.py (composed from
the oracle, np.lexsort by (-key, id)); the values are BITWISE the entries ops.sim_dense_combined writes at those indices; and the
values are within 1e-5 of the oracle's.  The shapes are the smallest at which each mechanism can go wrong: k on either side of
every pass boundary (a pass emits 44 - self entries), tie groups that straddle a boundary — exact copies, whose self entry lies
behind the first floor, equal keys from grid positions, and every key equal —, operands without 16-byte loads, a ragged batch
whose short segments run out inside the second pass, forced column ranges, outputs pre-filled with a sentinel, and two node sets
whose ids coincide."""
import ctypes
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combined_xy_restate as xr   # noqa: E402
from test_gpu_simtopk_combined import bits, make_data, offsets_of, reference   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5                    # tests/test_gpu_pipeline.py: values that go through expf
LH, LG = 0.5, 2e-7
RAGGED = [33, 0, 1, 257, 5, 130, 2, 46, 90]

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "Any-k top-k entries"
# (tests/test_simtopk_combined_anyk_cpu.py keeps the two equal)
SYNC = {"mmf_simtopk_combined_anyk": ("once (twice when a segment is short of k columns)", "until the call returns"),
        "mmf_simtopk_combined_xy_anyk": ("once", "no host arguments")}

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def ak():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk_anyk")


def ct():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk")


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def verify(mmf, Fd, Pd, p, k, idx, val, ref, lh=LH, lg=LG):
    """(idx, val) on the host against the reference (ridx, rval): indices, sim_dense_combined's bits, the oracle's values."""
    ridx, rval = ref
    assert idx.shape == ridx.shape == (Fd.shape[0], k)
    bad = np.nonzero((idx != ridx).any(axis=1))[0]
    if bad.size:
        col = int(np.nonzero(idx[bad[0]] != ridx[bad[0]])[0][0])
        raise AssertionError(f"{bad.size} rows differ from the reference, first row {bad[0]} at column {col}: got "
                             f"{idx[bad[0], max(col - 2, 0):col + 3]}, want {ridx[bad[0], max(col - 2, 0):col + 3]}")
    there = ridx >= 0
    assert np.all(np.isneginf(val[~there]))
    for a, b in zip(p[:-1], p[1:]):
        if not there[a:b].any():
            continue
        K = mmf.ops.sim_dense_combined(Fd[a:b], Pd[a:b], lh, lg).cpu().numpy()
        rows = np.broadcast_to(np.arange(b - a)[:, None], (b - a, k))[there[a:b]]
        want = K[rows, (ridx[a:b] - a)[there[a:b]]]
        assert np.array_equal(bits(val[a:b][there[a:b]]), bits(want)), f"segment [{a}, {b}): values differ from sim_dense_combined's bits"
    err = float(np.abs(val[there].astype(np.float64) - rval[there].astype(np.float64)).max()) if there.any() else 0.0
    print(f"k = {k}: max |val - oracle| = {err:.3e}")
    assert err <= TOL


def check(mmf, F, P, ptr, k, lh=LH, lg=LG, exclude_self=True, how="ptr", ref=None, **kw):
    """One call of simtopk_combined_any_k against the reference; returns (idx, val) as device tensors."""
    one = ptr is None
    p = offsets_of([F.shape[0]]) if one else np.asarray(ptr, dtype=np.int64)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    seg = {}
    if not one:
        seg = {"ptr": T(p)} if how == "ptr" else {"batch": torch.repeat_interleave(torch.arange(len(p) - 1), T(p[1:] - p[:-1])).cuda()}
    idx, val = ak().simtopk_combined_any_k(Fd, Pd, lh, lg, k, exclude_self=exclude_self, **seg, **kw)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
    verify(mmf, Fd, Pd, p, k, idx.cpu().numpy(), val.cpu().numpy(), ref if ref is not None else reference(F, P, p, k, lh, lg, exclude_self), lh, lg)
    return idx, val


# ---- 1. pass boundaries ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph():
    """n = 300, d = 40, dp = 2, and the reference at the largest k of each self mode: a reference for a smaller k is its first
    columns (one total order)."""
    F, P = make_data(300, 40, 2, seed=3, plant=(7, 200))
    p = offsets_of([300])
    return F, P, {True: reference(F, P, p, 130, exclude_self=True), False: reference(F, P, p, 89, exclude_self=False)}


@pytest.mark.parametrize("k,exclude_self", [(43, True), (44, True), (86, True), (87, True), (130, True),
                                            (44, False), (45, False), (88, False), (89, False)])
def test_pass_boundaries(mmf, graph, k, exclude_self):
    F, P, refs = graph
    ridx, rval = refs[exclude_self]
    check(mmf, F, P, None, k, exclude_self=exclude_self, ref=(ridx[:, :k], rval[:, :k]))
    assert ak().anyk_route(k, exclude_self, False) == ("combined_topk.simtopk_combined" if k + exclude_self <= 44 else "mmf_simtopk_combined_anyk")


def test_single_pass_range_and_prefix_equal_the_existing_entry(mmf, graph):
    """k = 43 through the new ENTRY (not the router) and the first 43 columns of k = 44 and k = 130 are bit for bit
    combined_topk.simtopk_combined's k = 43: the yardstick is existing code."""
    F, P, _ = graph
    Fd, Pd = T(F).cuda(), T(P).cuda()
    old = ct().simtopk_combined(Fd, Pd, LH, LG, 43)
    assert same_bits(ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 43), old)
    for k in (43, 44, 130):
        idx = torch.full((300, k), 7777, dtype=torch.int64, device="cuda")
        val = torch.full((300, k), 123.0, dtype=torch.float32, device="cuda")
        opts = mmf._lib.SimtopkOpts(mmf._lib.PRECISIONS["exact"], 0, 0, mmf._lib.QUERY_ORDERS["off"], None)
        mmf.ops._call("mmf_simtopk_combined_anyk", Fd.device, mmf.ops._p(Fd), mmf.ops._p(Pd), 300, 40, 2, LH, LG, k, 1, None, 0,
                      mmf.ops._p(idx), mmf.ops._p(val), ctypes.byref(opts), None)
        torch.cuda.synchronize()
        assert same_bits((idx[:, :43].contiguous(), val[:, :43].contiguous()), old), k
    old0 = ct().simtopk_combined(Fd, Pd, LH, LG, 44, exclude_self=False)
    new0 = ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 89, exclude_self=False)
    assert same_bits((new0[0][:, :44].contiguous(), new0[1][:, :44].contiguous()), old0)


# ---- 2. ties across a boundary ---------------------------------------------------------------------------------------------------
def test_exact_copies_straddle_the_first_floor(mmf):
    """Row 50 and its 60 exact copies (rows 100 .. 159) tie at every key: for each of them the tie group fills entries 0 .. 59,
    across the boundary at entry 43, ranked by id alone; a copy with a high id has its self entry BEHIND the first floor, where
    only the identity test drops it."""
    F, P = make_data(300, 40, 2, seed=4)
    F[100:160] = F[50]
    P[100:160] = P[50]
    idx, _ = check(mmf, F, P, None, 95)
    idx = idx.cpu().numpy()
    group = np.r_[50, 100:160]
    for r in (50, 100, 130, 159):
        assert np.array_equal(idx[r, :60], group[group != r]), r


def test_equal_keys_from_grid_positions(mmf):
    F, P = make_data(300, 40, 2, seed=5)
    check(mmf, F, P, None, 95, lh=0.0, lg=2e-7)


def test_every_key_equal(mmf):
    """lambda_h = lambda_g = 0: the result is the first k ids without self, every boundary inside one tie."""
    F, P = make_data(300, 40, 2, seed=6)
    idx, val = check(mmf, F, P, None, 95, lh=0.0, lg=0.0)
    want = np.stack([np.delete(np.arange(96), r)[:95] if r < 96 else np.arange(95) for r in range(300)])
    assert np.array_equal(idx.cpu().numpy(), want) and bool((val == 1.0).all())


# ---- 3. operand shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dp", [(37, 3), (100, 8), (40, 1)])
def test_operand_shapes(mmf, d, dp):
    F, P = make_data(300, d, dp, seed=7)
    check(mmf, F, P, None, 95)


# ---- 4. ragged batch -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_case():
    F, P = make_data(sum(RAGGED), 40, 2, seed=8, plant=(299, 300))
    p = offsets_of(RAGGED)
    return F, P, p, reference(F, P, p, 95)


@pytest.mark.parametrize("k", [50, 95])
@pytest.mark.parametrize("how", ["ptr", "batch"])
def test_ragged_batch(mmf, ragged_case, k, how):
    """k = 50: the segment of 46 rows runs out in the second pass and pads; k = 95: the segment of 90 rows does.  An empty segment,
    a one-row segment, segments of 257 and 130 rows across tile edges.  Equal to a loop of the one-graph call per segment."""
    F, P, p, (ridx, rval) = ragged_case
    ridx, rval = ridx[:, :k].copy(), rval[:, :k].copy()
    if how == "batch":                       # a batch vector cannot describe the empty segment: the same rows without it
        idx, val = check(mmf, F, P, offsets_of([s for s in RAGGED if s]), k, how="batch", ref=(ridx, rval))
    else:
        idx, val = check(mmf, F, P, p, k, ref=(ridx, rval))
    assert ak().anyk_route(k, True, True) == "mmf_simtopk_combined_anyk"
    Fd, Pd = T(F).cuda(), T(P).cuda()
    for a, b in zip(p[:-1], p[1:]):
        if b > a:
            gi, gv = ak().simtopk_combined_any_k(Fd[a:b], Pd[a:b], LH, LG, k)
            gi = torch.where(gi >= 0, gi + int(a), gi)
            assert same_bits((gi, gv), (idx[a:b], val[a:b])), (a, b)


# ---- 5. column splits ------------------------------------------------------------------------------------------------------------
def test_forced_column_splits(mmf):
    F, P = make_data(600, 40, 2, seed=9)
    ref = reference(F, P, offsets_of([600]), 95)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    first = None
    for cs in (1, 2, 4):
        idx, val, st = ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 95, col_splits=cs, return_stats=True)
        assert st["col_splits"] == cs and st["precision_used"] == mmf._lib.PRECISIONS["exact"], st
        if first is None:
            verify(mmf, Fd, Pd, offsets_of([600]), 95, idx.cpu().numpy(), val.cpu().numpy(), ref)
            first = (idx, val)
        assert same_bits((idx, val), first), cs
    p = T(offsets_of([300, 300]))
    seg = [ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 95, ptr=p, col_splits=cs, return_stats=True) for cs in (1, 2)]
    assert [s[2]["col_splits"] for s in seg] == [1, 2] and same_bits(seg[0], seg[1])


# ---- 6. every column written -----------------------------------------------------------------------------------------------------
def test_no_sentinel_survives(mmf, ragged_case):
    F, P, p, (ridx, _) = ragged_case
    Fd, Pd = T(F).cuda(), T(P).cuda()
    n, k = F.shape[0], 95
    idx = torch.full((n, k), 7777777, dtype=torch.int64, device="cuda")
    val = torch.full((n, k), 123.0, dtype=torch.float32, device="cuda")
    opts = mmf._lib.SimtopkOpts(mmf._lib.PRECISIONS["auto"], 0, 0, mmf._lib.QUERY_ORDERS["off"], None)
    hp = T(p)
    mmf.ops._call("mmf_simtopk_combined_anyk", Fd.device, mmf.ops._p(Fd), mmf.ops._p(Pd), n, 40, 2, LH, LG, k, 1, mmf.ops._hp(hp), len(p) - 1,
                  mmf.ops._p(idx), mmf.ops._p(val), ctypes.byref(opts), None)
    torch.cuda.synchronize()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert not (idx == 7777777).any() and not (val == 123.0).any()
    assert np.array_equal(idx, ridx)
    sizes = np.repeat(np.diff(p), np.diff(p))
    real = (idx >= 0).sum(axis=1)
    assert np.array_equal(real, np.minimum(k, sizes - 1))
    assert all((idx[r, :real[r]] >= 0).all() and (idx[r, real[r]:] == -1).all() and np.isneginf(val[r, real[r]:]).all() for r in range(n))


# ---- 7. two node sets ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sets(mmf):
    F, P = make_data(400, 40, 2, seed=10, plant=(120, 300))
    import oracle
    Fd, Pd = T(F).cuda(), T(P).cuda()
    return F, P, Fd, Pd, oracle.sim_dense_combined(F, P, LH, LG), mmf.ops.sim_dense_combined(Fd, Pd, LH, LG).cpu().numpy()


@pytest.mark.parametrize("c", [(100, 400), (100, 160), (100, 100)], ids=["300 candidates", "60 < k", "none"])
def test_queries_against_candidates(mmf, two_sets, c):
    """140 queries with ids 60 .. 199 against candidates with ids from 100 on: the queries 100 .. 199 meet their own id."""
    F, P, Fd, Pd, K_oracle, K_dev = two_sets
    q, k = (60, 200), 95
    ridx, rval = xr.reference(F, P, q, c, k, LH, LG, True, K_oracle)
    idx, val, st = ak().simtopk_combined_xy_any_k(Fd[q[0]:q[1]].clone(), Pd[q[0]:q[1]].clone(), Fd[c[0]:c[1]].clone(), Pd[c[0]:c[1]].clone(),
                                                  LH, LG, k, exclude_self=True, row_offset=q[0], col_offset=c[0], return_stats=True)
    torch.cuda.synchronize()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    bad = np.nonzero((idx != ridx).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} queries differ from the reference, first {bad[0]}: got {idx[bad[0]]}, want {ridx[bad[0]]}"
    there = ridx >= 0
    assert np.all(np.isneginf(val[~there])) and np.all(idx[~there] == -1)
    if there.any():
        rows = np.broadcast_to(np.arange(q[0], q[1])[:, None], (q[1] - q[0], k))[there]
        assert np.array_equal(bits(val[there]), bits(K_dev[rows, ridx[there]])), "values differ from sim_dense_combined's bits"
        err = float(np.abs(val[there].astype(np.float64) - rval[there].astype(np.float64)).max())
        print(f"max |val - oracle| = {err:.3e}")
        assert err <= TOL
        assert st["precision_used"] == mmf._lib.PRECISIONS["exact"]


def test_row_panels_and_the_sharded_driver(mmf, two_sets):
    from multimodal_fusion_amd.distributed import sharded_simtopk_combined_any_k
    _, _, Fd, Pd, _, _ = two_sets
    whole = ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 95)
    rows = ak().simtopk_combined_rows_any_k(Fd, Pd, 37, 171, LH, LG, 95)
    assert same_bits(rows, (whole[0][37:171], whole[1][37:171]))
    off = ak().simtopk_combined_rows_any_k(Fd, Pd, 37, 171, LH, LG, 95, col_offset=1000)
    assert torch.equal(off[0], whole[0][37:171] + 1000)
    one = sharded_simtopk_combined_any_k(Fd, Pd, 400, lambda_h=LH, lambda_g=LG, k=95, return_stats=True)
    assert same_bits(one, whole) and one[2]["driver"] == "simple"
    small = ak().simtopk_combined_rows_any_k(Fd, Pd, 37, 171, LH, LG, 20)              # one pass: the existing entry's bits
    assert same_bits(small, import_module("multimodal_fusion_amd.combined_topk_xy").simtopk_combined_rows(Fd, Pd, 37, 171, LH, LG, 20, precision="exact"))


# ---- 8. builders -----------------------------------------------------------------------------------------------------------------
def test_builders(mmf, ragged_case):
    F, P, p, (ridx, _) = ragged_case
    Fd, Pd = T(F).cuda(), T(P).cuda()
    k = 95
    ei, ew, eptr = ak().build_topk_weighted_hypergraph_any_k(Fd, Pd, LH, LG, k, ptr=T(p))
    sizes = np.diff(p)
    want_ptr = np.concatenate([[0], np.cumsum(sizes * np.minimum(k, np.maximum(sizes - 1, 0)))])
    assert np.array_equal(eptr.cpu().numpy(), want_ptr) and ei.shape == (2, want_ptr[-1]) and ew.shape == (want_ptr[-1],)
    ei = ei.cpu().numpy()
    assert (ei >= 0).all()
    keep = ridx >= 0
    assert np.array_equal(ei[0], np.broadcast_to(np.arange(F.shape[0])[:, None], ridx.shape)[keep]) and np.array_equal(ei[1], ridx[keep])
    data = ak().build_topk_hypergraph_data_any_k(Fd, Pd, LH, LG, k, ptr=T(p))
    assert np.array_equal(data["edge_index"].cpu().numpy(), ei) and torch.equal(data["edge_attr"], ew)
    assert data["pooled_feature"].shape == (len(RAGGED), 40) and data["batch"].shape == (F.shape[0],)
    one = ak().build_topk_weighted_hypergraph_any_k(Fd[:130], Pd[:130], LH, LG, 64)
    assert one[0].shape == (2, 130 * 64) and one[2].tolist() == [0, 130 * 64]


# ---- 9. stream contract ----------------------------------------------------------------------------------------------------------
GATED_SIZES = [3, 150, 0, 260]


def _gated_inputs(n, seeds):
    def make_inputs(which):
        g = torch.Generator().manual_seed(seeds[0] if which == "truth" else seeds[1])
        return [torch.randn(n, 40, generator=g) * 0.3, torch.rand(n, 2, generator=g) * 4.0]
    return make_inputs


def _gated_anyk(mmf):
    xp = torch.tensor(offsets_of(GATED_SIZES))

    def entry(F, P):
        return ak().simtopk_combined_any_k(F, P, 0.7, 0.3, 50, ptr=xp)        # two passes, one segment on the launch loop
    return entry, _gated_inputs(int(xp[-1]), (41, 42))


def _gated_xy_anyk(mmf):
    def entry(F, P):
        return ak().simtopk_combined_xy_any_k(F[:150], P[:150], F[100:], P[100:], 0.7, 0.3, 50, exclude_self=True, row_offset=0, col_offset=100)
    return entry, _gated_inputs(413, (43, 44))


GATED = {"mmf_simtopk_combined_anyk": _gated_anyk, "mmf_simtopk_combined_xy_anyk": _gated_xy_anyk}


def test_the_gated_cases_are_exactly_the_entries(mmf):
    assert set(GATED) == set(mmf._lib.EXPORTS_TOPK_ANYK) == set(SYNC)


@pytest.mark.parametrize("name", sorted(GATED))
def test_stream_contract_behind_a_closed_gate(mmf, name):
    import streamgate
    entry, make_inputs = GATED[name](mmf)
    streamgate.run_gated(entry, make_inputs, None, name=name, calls=2)      # the idle call's bits; the cases above have the references
