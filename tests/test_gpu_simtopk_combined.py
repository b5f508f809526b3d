"""Top-k of the combined similarity K_h * K_g on the MI355X (mmf_simtopk_combined).

Every case checks three things: the indices are those of a numpy reference composed from the existing oracle (canonical -sq
of the features and of the positions, one float32 add, np.lexsort by (-key, id)); the values are BITWISE the entries
ops.sim_dense_combined writes at those indices; and the values are within 1e-5 (the project's RBF tolerance) of the oracle's.
The shapes are the smallest at which each mechanism can go wrong: an empty segment, a segment of one row, segments shorter than
k, a segment one row past two candidate tiles, d that is no multiple of the staged chunk, every position-chain length, every
list capacity and the limit k + self = 44, forced column splits, and rows planted so that the position alone — and, for exact
copies, the id alone — decides."""
import ctypes
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5                    # tests/test_gpu_pipeline.py: values that go through expf
LH, LG = 0.5, 2e-7
RAGGED = [33, 0, 1, 257, 5, 130, 2]

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "Top-k entries"
# (tests/test_simtopk_combined_cpu.py keeps the two equal)
SYNC_TOPK = {"mmf_simtopk_combined": ("once", "the call")}

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def ct():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk")


# ---- data and reference ------------------------------------------------------------------------------------------------
def make_data(n, d, dp=2, seed=0, plant=None):
    """12 Gaussian centres, rows = a centre + 0.05 noise; positions = grid cells of [0, 24)^dp x 224 (pixel units).
    plant = (src, first): rows first .. first + 9 copy src's features, the first five of them its position too."""
    rng = np.random.RandomState(1000 + seed)
    centres = rng.randn(12, d).astype(np.float32)
    F = (centres[rng.randint(0, 12, n)] + np.float32(0.05) * rng.randn(n, d).astype(np.float32)).astype(np.float32)
    P = (rng.randint(0, 24, (n, dp)) * 224).astype(np.float32)
    if plant is not None:
        src, first = plant
        F[first:first + 10] = F[src]
        P[first:first + 5] = P[src]
    return np.ascontiguousarray(F), np.ascontiguousarray(P)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def reference(F, P, ptr, k, lh=LH, lg=LG, exclude_self=True):
    """(idx [n, k] int64 padded with -1, oracle values [n, k] padded with -inf, keys per segment)."""
    import oracle
    n = F.shape[0]
    idx = np.full((n, k), -1, dtype=np.int64)
    val = np.full((n, k), -np.inf, dtype=np.float32)
    for a, b in zip(ptr[:-1], ptr[1:]):
        ns = int(b - a)
        if ns == 0:
            continue
        A = oracle.sim_dense(F[a:b], metric="neg_sq_l2")
        B = oracle.sim_dense(P[a:b], metric="neg_sq_l2")
        key = (np.float32(lh) * A + np.float32(lg) * B).astype(np.float32)
        if exclude_self:
            np.fill_diagonal(key, -np.inf)
        K = oracle.sim_dense_combined(F[a:b], P[a:b], lh, lg)
        take = min(k, ns - (1 if exclude_self else 0))
        ids = np.arange(ns)
        for i in range(ns):
            order = np.lexsort((ids, -key[i]))[:take]
            idx[a + i, :take] = order + a
            val[a + i, :take] = K[i, order]
    return idx, val


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(mmf, F, P, ptr, k, lh=LH, lg=LG, exclude_self=True, how="ptr", ref=None, **kw):
    """One call against the reference; returns (idx, val) on the host."""
    one = ptr is None
    p = offsets_of([F.shape[0]]) if one else np.asarray(ptr, dtype=np.int64)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    seg = {}
    if not one:
        seg = {"ptr": T(p)} if how == "ptr" else {"batch": torch.repeat_interleave(torch.arange(len(p) - 1), T(p[1:] - p[:-1])).cuda()}
    idx, val = ct().simtopk_combined(Fd, Pd, lh, lg, k, exclude_self=exclude_self, **seg, **kw)
    torch.cuda.synchronize()
    assert idx.shape == (F.shape[0], k) and idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    ridx, rval = ref if ref is not None else reference(F, P, p, k, lh, lg, exclude_self)
    bad = np.nonzero((idx != ridx).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ from the reference, first {bad[0]}: got {idx[bad[0]]}, want {ridx[bad[0]]}"
    there = ridx >= 0
    assert np.all(np.isneginf(val[~there]))
    # bit for bit the entries of the dense combined similarity of the segment
    for a, b in zip(p[:-1], p[1:]):
        if not there[a:b].any():
            continue
        K = mmf.ops.sim_dense_combined(Fd[a:b], Pd[a:b], lh, lg).cpu().numpy()
        rows = np.broadcast_to(np.arange(b - a)[:, None], (b - a, k))[there[a:b]]
        want = K[rows, (ridx[a:b] - a)[there[a:b]]]
        got = val[a:b][there[a:b]]
        assert np.array_equal(bits(got), bits(want)), f"segment [{a}, {b}): values differ from sim_dense_combined's bits"
    err = float(np.abs(val[there].astype(np.float64) - rval[there].astype(np.float64)).max()) if there.any() else 0.0
    print(f"max |val - oracle| = {err:.3e}")
    assert err <= TOL
    return idx, val


# ---- ragged and single-graph shapes --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_case():
    F, P = make_data(sum(RAGGED), 40, 2, seed=1, plant=(299, 300))       # row 299 and its copies lie in the segment of 130 rows
    p = offsets_of(RAGGED)
    return F, P, p, reference(F, P, p, 5)


@pytest.mark.parametrize("how", ["ptr", "batch"])
def test_ragged_batch(mmf, ragged_case, how):
    F, P, p, ref = ragged_case
    if how == "batch":                       # a batch vector cannot describe the empty segment: the same rows without it
        sizes = [s for s in RAGGED if s]
        p2 = offsets_of(sizes)
        idx, _ = check(mmf, F, P, p2, 5, how="batch", ref=ref)
    else:
        idx, _ = check(mmf, F, P, p, 5, ref=ref)
    assert np.all(idx[33] == -1)                                         # the segment of one row
    assert np.all(idx[291:296, 4] == -1) and np.all(idx[291:296, :4] >= 291)      # five rows: four neighbours
    assert np.all(idx[426:428, 1:] == -1) and list(idx[426:428, 0]) == [427, 426]
    # the copies of row 299: features equal, so the position decides; the exact copies tie, so the id decides
    assert list(idx[299, :5]) == [300, 301, 302, 303, 304] and list(idx[302, :4]) == [299, 300, 301, 303]


def test_the_data_needs_both_terms(ragged_case):
    """In the segment of 257 rows the combined top-5 is neither the features' nor the positions': a kernel that drops a term fails."""
    F, P, p, (ridx, _) = ragged_case
    a, b = int(p[3]), int(p[4])
    fi, _ = reference(F[a:b], P[a:b], offsets_of([b - a]), 5, LH, 0.0)
    pi, _ = reference(F[a:b], P[a:b], offsets_of([b - a]), 5, 0.0, LG)
    mine = ridx[a:b] - a
    assert (mine != fi).any(axis=1).mean() > 0.9 and (mine != pi).any(axis=1).mean() > 0.9


@pytest.mark.parametrize("n,k", [(2, 1), (128, 5), (129, 5), (300, 5)])
def test_one_graph(mmf, n, k):
    F, P = make_data(n, 40, 2, seed=2, plant=(n - 1, 100) if n == 300 else None)
    check(mmf, F, P, None, k)


@pytest.mark.parametrize("d", [33, 40, 512])
def test_feature_dims(mmf, d):
    F, P = make_data(300, d, 2, seed=3, plant=(299, 100))
    check(mmf, F, P, None, 5)


@pytest.mark.parametrize("dp", [1, 2, 3, 8])
def test_position_dims(mmf, dp):
    F, P = make_data(300, 40, dp, seed=4, plant=(299, 100))
    check(mmf, F, P, None, 5)


@pytest.mark.parametrize("k", [5, 12, 28, 43])
def test_list_capacities(mmf, k):
    """k + self = 6, 13, 29, 44: list capacity 16, 32, 48 and the limit."""
    F, P = make_data(300, 40, 2, seed=5, plant=(299, 100))
    _, _, st = ct().simtopk_combined(T(F).cuda(), T(P).cuda(), LH, LG, k, return_stats=True)
    assert st["precision_used"] == 1 and st["scan_grid"] >= 3 and st["col_splits"] >= 1
    check(mmf, F, P, None, k)


def test_column_splits_give_identical_bits(mmf):
    F, P = make_data(300, 40, 2, seed=6, plant=(299, 100))
    ref = reference(F, P, offsets_of([300]), 5)
    outs = [check(mmf, F, P, None, 5, ref=ref, col_splits=c) for c in (1, 3, 0)]
    for idx, val in outs[1:]:
        assert np.array_equal(idx, outs[0][0]) and np.array_equal(bits(val), bits(outs[0][1]))
    sts = [ct().simtopk_combined(T(F).cuda(), T(P).cuda(), LH, LG, 5, col_splits=c, return_stats=True)[2]["col_splits"] for c in (1, 3)]
    assert sts == [1, 3]


def test_include_self(mmf):
    F, P = make_data(300, 40, 2, seed=7, plant=(299, 100))
    idx, _ = check(mmf, F, P, None, 5, exclude_self=False)
    for i in range(300):
        j = idx[i, 0]
        assert j == i or (j < i and np.array_equal(F[j], F[i]) and np.array_equal(P[j], P[i])), (i, j)
    assert list(idx[104, :5]) == [100, 101, 102, 103, 104]               # exact copies of row 299 with lower ids precede it


@pytest.mark.parametrize("term", ["features only", "positions only"])
def test_a_zero_lambda_drops_its_term(mmf, term):
    """Against entries that are already pinned: the exact RBF top-k of the one operand that is left."""
    F, P = make_data(300, 40, 2, seed=8, plant=(299, 100))
    Fd, Pd = T(F).cuda(), T(P).cuda()
    if term == "features only":
        got = ct().simtopk_combined(Fd, Pd, LH, 0.0, 5)
        want = mmf.ops.simtopk(Fd, metric="rbf", lam=LH, k=5, precision="exact")
    else:
        got = ct().simtopk_combined(Fd, Pd, 0.0, LG, 5)
        want = mmf.ops.simtopk(Pd, metric="rbf", lam=LG, k=5, precision="exact")
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and np.array_equal(bits(got[1].cpu().numpy()), bits(want[1].cpu().numpy()))


# ---- scale -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scale_rows():
    return make_data(4096, 512, 2, seed=9, plant=(299, 300))


def test_scale_one_graph(mmf, scale_rows):
    F, P = scale_rows
    check(mmf, F, P, None, 5)


def test_scale_sixteen_segments(mmf, scale_rows):
    F, P = scale_rows
    check(mmf, F, P, offsets_of([256] * 16), 5)


# ---- repetition and streams --------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits(mmf, ragged_case):
    F, P, p, _ = ragged_case
    Fd, Pd = T(F).cuda(), T(P).cuda()
    a = ct().simtopk_combined(Fd, Pd, LH, LG, 5, ptr=T(p))
    b = ct().simtopk_combined(Fd, Pd, LH, LG, 5, ptr=T(p))
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and np.array_equal(bits(a[1].cpu().numpy()), bits(b[1].cpu().numpy()))


GATED_P = offsets_of([70, 0, 1, 150, 79])


def gated_inputs(which):
    F, P = make_data(300, 40, 2, seed=20 if which == "truth" else 21, plant=(299, 100))
    return [T(F), T(P)]


def gated_reference(F, P):
    ridx, rval = reference(F, P, GATED_P, 5)
    return lambda got: sg.diff(got[0], ridx, "idx") + sg.diff(got[1], rval, "val", atol=TOL)


def _c_entry(F, P):
    import multimodal_fusion_amd as m
    o = m.ops
    n, k = F.shape[0], 5
    idx = torch.empty((n, k), dtype=torch.int64, device=F.device)
    val = torch.empty((n, k), dtype=torch.float32, device=F.device)
    ptr = T(GATED_P.copy())
    rc = m._lib.lib().mmf_simtopk_combined(o._p(F), o._p(P), n, F.shape[1], P.shape[1], LH, LG, k, 1, o._hp(ptr), len(GATED_P) - 1,
                                           o._p(idx), o._p(val), None, None, F.device.index or 0, o._stream(F.device))
    m._lib.check(rc, "mmf_simtopk_combined")
    return [idx, val]


def _wrapper(F, P):
    return list(ct().simtopk_combined(F, P, LH, LG, 5, ptr=T(GATED_P.copy())))


@pytest.mark.parametrize("name,entry", [("c_entry_simtopk_combined", _c_entry), ("simtopk_combined", _wrapper)])
def test_entry_behind_a_closed_gate(mmf, name, entry):
    assert list(SYNC_TOPK) == list(mmf._lib.EXPORTS_TOPK)
    sg.run_gated(entry, gated_inputs, gated_reference, name=name, calls=2)


# ---- edge builder ------------------------------------------------------------------------------------------------------
def test_edge_builder(mmf, ragged_case):
    F, P, p, (ridx, _) = ragged_case
    Fd, Pd = T(F).cuda(), T(P).cuda()
    idx, val = ct().simtopk_combined(Fd, Pd, LH, LG, 5, ptr=T(p))
    ei, ew, eptr = ct().build_topk_weighted_hypergraph(Fd, Pd, LH, LG, 5, ptr=T(p))
    assert ei.is_cuda and ew.is_cuda and eptr.is_cuda and ei.dtype == torch.int64 and ew.dtype == torch.float32
    sizes = np.asarray(RAGGED)
    want_ptr = offsets_of(sizes * np.minimum(5, np.maximum(sizes - 1, 0)))
    assert np.array_equal(eptr.cpu().numpy(), want_ptr) and ei.shape == (2, int(want_ptr[-1])) and ew.shape == (int(want_ptr[-1]),)
    there = ridx >= 0
    rows = np.broadcast_to(np.arange(len(F))[:, None], ridx.shape)
    assert np.array_equal(ei.cpu().numpy(), np.stack([rows[there], ridx[there]]))          # rows ascend, r ascends within a row
    assert np.array_equal(bits(ew.cpu().numpy()), bits(val.cpu().numpy()[there])) and int(ei.min()) >= 0
    seg = np.searchsorted(p, ei.cpu().numpy(), side="right") - 1
    assert np.array_equal(seg[0], seg[1])                                                  # no edge leaves its segment
    assert np.array_equal(seg[0], np.repeat(np.arange(len(RAGGED)), np.diff(want_ptr)))

    data = ct().build_topk_hypergraph_data(Fd, Pd, LH, LG, 5, ptr=T(p))
    assert sorted(data) == ["batch", "edge_attr", "edge_index", "pooled_feature", "pos", "ptr", "x"]
    assert all(v.is_cuda for v in data.values()) and torch.equal(data["edge_index"], ei) and torch.equal(data["edge_attr"], ew)
    assert data["pooled_feature"].shape == (len(RAGGED), 40) and torch.equal(data["ptr"].cpu(), T(p))
    assert "pooled_feature" not in ct().build_topk_hypergraph_data(Fd, Pd, LH, LG, 5, use_pooling=False, ptr=T(p))

    # a CPU input gives a CPU output with the same bits
    ci, cw, cp = ct().build_topk_weighted_hypergraph(T(F), T(P), LH, LG, 5, ptr=T(p))
    assert not ci.is_cuda and not cw.is_cuda and not cp.is_cuda
    assert torch.equal(ci, ei.cpu()) and torch.equal(cw, ew.cpu()) and torch.equal(cp, eptr.cpu())
    hi, hv = ct().simtopk_combined(T(F), T(P), LH, LG, 5, ptr=T(p))
    assert not hi.is_cuda and torch.equal(hi, idx.cpu()) and torch.equal(hv, val.cpu())
    assert all(not v.is_cuda for v in ct().build_topk_hypergraph_data(T(F), T(P), LH, LG, 5, ptr=T(p)).values())


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(mmf):
    F, P = make_data(300, 40, 2, seed=10)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    with pytest.raises(RuntimeError, match=r"k \+ self = 45 > 44"):
        ct().simtopk_combined(Fd, Pd, LH, LG, 44)
    ct().simtopk_combined(Fd, Pd, LH, LG, 44, exclude_self=False)          # k + self = 44: the limit itself is served
    with pytest.raises(RuntimeError, match="dp = 9 > 8"):
        ct().simtopk_combined(Fd, torch.zeros(300, 9, device="cuda"), LH, LG, 5)
    with pytest.raises(ValueError, match="k must be >= 1"):
        ct().simtopk_combined(Fd, Pd, LH, LG, 0)
    with pytest.raises(ValueError, match="lambda_g must be finite"):
        ct().simtopk_combined(Fd, Pd, LH, float("nan"), 5)
    idx, val = ct().simtopk_combined(Fd[:0], Pd[:0], LH, LG, 5)
    assert idx.shape == (0, 5) and val.shape == (0, 5)
