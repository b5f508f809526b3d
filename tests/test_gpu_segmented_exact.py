"""The segmented exact scan (segmented_exact.*, include/ext/mmf_hg_seg_exact.h): the exact top-k of every segment
of a ragged batch from one table-driven launch of the exact scan and one re-rank.

The references are the loops the calls replace — one ops.simtopk(..., precision="exact", row_offset, col_offset) per segment
(per_segment of tests/test_gpu_segmented.py), combined_topk.simtopk_combined(ptr=...) and ops.sim_dense_combined per segment — and
the CPU oracle per segment.  Indices equal, values bitwise equal (the oracle's RBF values to the project's 1e-5).  None of the
references is code this feature touches."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_segmented import assert_same, dup_rows, offsets, per_segment  # noqa: E402

pytestmark = pytest.mark.gpu

# empty, one row, fewer than k columns, tile edges, two and three row blocks, four tiles
SIZES = [33, 0, 1, 257, 5, 6, 128, 31, 129, 32, 98, 385]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LAM = 0.5


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def rows(n, d, seed, metric="cosine", dtype="f32"):
    return torch.from_numpy(dup_rows(n, d, seed, scale=0.1 if metric == "rbf" else 1.0)).to(DTYPES[dtype])


def table_of(mmf, xs, ys, k, exclude_self, col_splits=0):
    """(scan_grid, col_splits) the call must report: the host table query's."""
    t, lists = mmf.segmented_exact_table(offsets(xs), None if ys is None else offsets(ys), k=k, exclude_self=exclude_self, col_splits=col_splits)
    return t.shape[0], lists // 2


@functools.lru_cache(maxsize=None)
def self_inputs(d, dtype, metric):
    return rows(sum(SIZES), d, 7 + d, metric, dtype).cuda()


@functools.lru_cache(maxsize=None)
def loop_reference(d, dtype, metric, k):
    """The per-segment exact loop over self_inputs cut into SIZES: computed once per shape, kept on the host, never written."""
    import multimodal_fusion_amd as m
    xp = offsets(SIZES)
    idx, val = per_segment(m, self_inputs(d, dtype, metric), None, xp, xp, k, True, metric=metric, lam=LAM, precision="exact")
    return idx.cpu(), val.cpu()


# ---- 1. self, ragged: every metric, dtype and list capacity ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 12, 28])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
@pytest.mark.parametrize("d", [40, 100])
def test_self_ragged_same_bits_as_the_loop(mmf, d, metric, dtype, k):
    X = self_inputs(d, dtype, metric)
    idx, val, st = mmf.simtopk_segmented_exact(X, ptr=offsets(SIZES), metric=metric, lam=LAM, k=k, return_stats=True)
    grid, ranges = table_of(mmf, SIZES, None, k, True)
    print(f"d {d} {metric} {dtype} k {k}: scan_grid {st['scan_grid']} (table {grid}) col_splits {st['col_splits']} candidates {st['candidates']}")
    assert st["precision_used"] == 1 and st["scan_grid"] == grid and st["col_splits"] == ranges == 4      # the 385-row segment: 4 tiles
    assert st["fallback_rows"] == 0 and st["near_rows"] == -1
    assert_same((idx.cpu(), val.cpu()), loop_reference(d, dtype, metric, k))


@pytest.mark.parametrize("sizes", [[128, 256, 0, 384], [100, 27, 130]], ids=["n multiple of 128", "n = 1 mod 128"])
def test_batch_ends_on_and_just_past_a_block_edge(mmf, sizes):
    xp = offsets(sizes)
    assert xp[-1] % 128 == (0 if sizes[0] == 128 else 1)
    X = rows(xp[-1], 100, 3).cuda()
    for k in (5, 28):
        got = mmf.simtopk_segmented_exact(X, ptr=xp, metric="neg_sq_l2", k=k)
        assert_same(got, per_segment(mmf, X, None, xp, xp, k, True, metric="neg_sq_l2", precision="exact"))


# ---- 2. cross calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("metric", ["cosine", "rbf"])
def test_cross_same_bits_as_the_loop(mmf, metric, exclude_self):
    xs = [40, 0, 129, 5, 257, 1, 300, 32]               # segment 1: no queries; 3: no candidates; 6: 4 columns < k
    ys = [300, 7, 33, 0, 128, 256, 4, 1000]
    xp, yp = offsets(xs), offsets(ys)
    X, Y = rows(xp[-1], 100, 1, metric).cuda(), rows(yp[-1], 100, 2, metric).cuda()
    Y[yp[0] + 3] = X[xp[0] + 3]                         # a copy whose global id differs from the row's: not "self"
    kw = dict(metric=metric, lam=LAM, k=5)
    idx, val, st = mmf.simtopk_segmented_exact(X, Y, ptr=xp, y_ptr=yp, exclude_self=exclude_self, return_stats=True, **kw)
    assert (st["scan_grid"], st["col_splits"]) == table_of(mmf, xs, ys, 5, exclude_self)
    assert_same((idx, val), per_segment(mmf, X, Y, xp, yp, exclude_self=exclude_self, precision="exact", **kw))
    assert (idx[xp[3]:xp[4]] == -1).all() and (idx[xp[6]:xp[7], 4:] == -1).all()


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
def test_against_the_oracle_per_segment(mmf, metric):
    sizes = [257, 6, 0, 129, 3, 40]
    xp = offsets(sizes)
    X = rows(xp[-1], 40, 11, metric)
    idx, val = mmf.simtopk_segmented_exact(X.cuda(), ptr=xp, metric=metric, lam=LAM, k=5)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for a, b in zip(xp[:-1], xp[1:]):
        if b == a:
            continue
        ks = min(5, b - a - 1)
        assert (idx[a:b, ks:] == -1).all() and np.isneginf(val[a:b, ks:]).all()
        ridx, rval = oracle.simtopk(X[a:b].numpy(), X[a:b].numpy(), metric=metric, lam=LAM, k=ks, exclude_self=True, row_offset=a, col_offset=a)
        assert np.array_equal(idx[a:b, :ks], ridx), f"segment at {a}: indices differ"
        if metric == "rbf":
            assert np.allclose(val[a:b, :ks], rval, rtol=0, atol=1e-5)
        else:
            assert np.array_equal(val[a:b, :ks].view(np.int32), rval.view(np.int32))


# ---- 4. column ranges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 28])
def test_forced_column_ranges_give_the_same_bits(mmf, k):
    X = self_inputs(100, "f32", "cosine")
    xp = offsets(SIZES)
    ref = loop_reference(100, "f32", "cosine", k)
    for splits in (1, 2, 4):
        idx, val, st = mmf.simtopk_segmented_exact(X, ptr=xp, metric="cosine", lam=LAM, k=k, col_splits=splits, return_stats=True)
        grid, ranges = table_of(mmf, SIZES, None, k, True, splits)
        assert ranges == splits and st["col_splits"] == splits and st["scan_grid"] == grid
        assert_same((idx.cpu(), val.cpu()), ref)


# ---- 5. no neighbour crosses a segment, ties -------------------------------------------------------------------------------------
def test_no_neighbour_crosses_a_segment(mmf):
    """The rows just after a segment's end are exact copies of rows inside it (and the rows just before the next one's start
    likewise): a tile's over-read that leaked, or an id of the wrong segment, would return them — a copy scores like the row itself."""
    base = rows(600, 100, 5)
    mid = base[200:340]                                  # 140 rows: the tile that starts at row 128 of a segment over-reads 116
    X = torch.cat([base[:10], mid, mid, base[400:410], mid]).cuda()        # segments of 150, 150, 140 rows
    xp = offsets([150, 150, 140])
    for splits in (0, 2):
        idx, val = mmf.simtopk_segmented_exact(X, ptr=xp, metric="cosine", k=5, col_splits=splits)
        for s in range(3):
            own = idx[xp[s]:xp[s + 1]]
            assert ((own >= xp[s]) & (own < xp[s + 1])).all(), f"segment {s}: a neighbour from another segment"
        assert_same((idx, val), per_segment(mmf, X, None, xp, xp, 5, True, metric="cosine", precision="exact"))


def test_ties_rank_by_ascending_global_id(mmf):
    base = rows(400, 40, 6)
    base[150:162] = base[150]                            # twelve identical rows inside the second segment
    xp = offsets([140, 200, 60])
    X = base.cuda()
    idx, val = mmf.simtopk_segmented_exact(X, ptr=xp, metric="neg_sq_l2", k=5)
    others = [[j for j in range(150, 162) if j != i][:5] for i in range(150, 162)]
    assert idx[150:162].tolist() == others
    assert_same((idx, val), per_segment(mmf, X, None, xp, xp, 5, True, metric="neg_sq_l2", precision="exact"))


# ---- 6. k + self > 44: passes with floors in the global id space ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_k_inputs():
    sizes = [129, 5, 257, 60, 0, 385, 31]
    X = rows(sum(sizes), 40, 21, "neg_sq_l2")
    a = offsets(sizes)[3]
    X[a:a + 60] = X[a]                                   # a whole segment of identical rows ...
    b = offsets(sizes)[5]
    X[b + 100:b + 160] = X[b + 100]                      # ... and 60 inside a larger one: ties cross every pass boundary
    return sizes, X.cuda()


@pytest.mark.parametrize("metric", ["neg_sq_l2", "cosine"])
@pytest.mark.parametrize("k", [50, 95])
def test_large_k_runs_passes_and_matches_the_loop(mmf, k, metric):
    sizes, X = large_k_inputs()
    xp = offsets(sizes)
    idx, val, st = mmf.simtopk_segmented_exact(X, ptr=xp, metric=metric, k=k, return_stats=True)
    assert (st["scan_grid"], st["col_splits"]) == table_of(mmf, sizes, None, k, True)
    assert_same((idx, val), per_segment(mmf, X, None, xp, xp, k, True, metric=metric, precision="exact"))
    with pytest.raises(RuntimeError, match="k \\+ self"):                    # the existing entry keeps its refusal
        mmf.ops.simtopk_segmented(X, ptr=xp, metric=metric, k=k, precision="exact")


def test_large_k_with_column_ranges_and_without_self(mmf):
    sizes, X = large_k_inputs()
    xp = offsets(sizes)
    got = mmf.simtopk_segmented_exact(X, ptr=xp, metric="neg_sq_l2", k=50, exclude_self=False, col_splits=2)
    assert_same(got, per_segment(mmf, X, None, xp, xp, 50, False, metric="neg_sq_l2", precision="exact"))


# ---- 7. the combined key -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def combined_inputs(dp):
    g = torch.Generator().manual_seed(40 + dp)
    n = sum(SIZES)
    F = rows(n, 40, 9, "rbf")
    P = torch.rand(n, dp, generator=g) * 4.0
    return F.cuda(), P.cuda()


@pytest.mark.parametrize("k", [5, 28])
@pytest.mark.parametrize("dp", [2, 3])
def test_combined_same_bits_as_the_launch_loop_and_the_dense_entries(mmf, dp, k):
    F, P = combined_inputs(dp)
    xp = offsets(SIZES)
    ref = mmf.combined_topk.simtopk_combined(F, P, 0.7, 0.3, k, ptr=xp)
    idx, val, st = mmf.simtopk_combined_exact(F, P, 0.7, 0.3, k, ptr=xp, return_stats=True)
    assert st["precision_used"] == 1 and (st["scan_grid"], st["col_splits"]) == table_of(mmf, SIZES, None, k, True)
    assert_same((idx, val), ref)
    for a, b in zip(xp[:-1], xp[1:]):
        if b - a < 2:
            continue
        K = mmf.ops.sim_dense_combined(F[a:b], P[a:b], 0.7, 0.3)
        ks = min(k, b - a - 1)
        want = torch.gather(K, 1, idx[a:b, :ks] - a)
        assert torch.equal(val[a:b, :ks].view(torch.int32), want.view(torch.int32)), f"segment at {a}: not the dense entries"
    for splits in (2, 4):
        got = mmf.simtopk_combined_exact(F, P, 0.7, 0.3, k, ptr=xp, col_splits=splits, return_stats=True)
        assert got[2]["col_splits"] == splits and got[2]["scan_grid"] == table_of(mmf, SIZES, None, k, True, splits)[0]
        assert_same(got[:2], ref)


def test_combined_refuses_k_plus_self_45(mmf):
    F, P = combined_inputs(2)
    with pytest.raises(RuntimeError, match="k \\+ self = 45 > 44"):
        mmf.simtopk_combined_exact(F, P, 0.7, 0.3, 44, ptr=offsets(SIZES))
    mmf.simtopk_combined_exact(F, P, 0.7, 0.3, 44, ptr=offsets(SIZES), exclude_self=False)


# ---- 8. the router -------------------------------------------------------------------------------------------------------------------
def test_the_router_takes_a_16_bit_scan_where_one_applies(mmf, monkeypatch):
    se = mmf.segmented_exact
    calls = []
    exact, wide = se.simtopk_segmented_exact, mmf.wide_scan.simtopk_segmented
    monkeypatch.setattr(se, "simtopk_segmented_exact", lambda *a, **kw: (calls.append("exact"), exact(*a, **kw))[1])
    monkeypatch.setattr(mmf.wide_scan, "simtopk_segmented", lambda *a, **kw: (calls.append("16-bit"), wide(*a, **kw))[1])
    xp = offsets(SIZES)
    X = self_inputs(100, "f32", "cosine")
    Xw = rows(xp[-1], 600, 13).cuda()
    # (rows, k, precision) -> who answers: a 16-bit scan serves d = 100 at both k; none serves k + self = 29 above d = 512
    for data, k, precision, who in ((X, 5, "auto", "16-bit"), (X, 5, "exact", "exact"), (Xw, 28, "auto", "exact"), (Xw, 5, "auto", "16-bit")):
        fast = mmf.ops.fast_scan_supported(data.shape[1], k, True) or mmf.wide_scan.wide_scan_supported(data.shape[1], k, True)
        assert fast == (who == "16-bit" or precision == "exact")
        del calls[:]
        idx, val, st = se.simtopk_segmented(data, ptr=xp, metric="cosine", k=k, precision=precision, return_stats=True)
        assert calls == [who], (k, precision, calls)
        assert st["precision_used"] == (2 if who == "16-bit" else 1)
        assert_same((idx, val), per_segment(mmf, data, None, xp, xp, k, True, metric="cosine", precision="exact"))
    with pytest.raises(ValueError, match="needs a 16-bit scan"):
        se.simtopk_segmented(Xw, ptr=xp, k=28, precision="fast")


# ---- 9. stream contract ------------------------------------------------------------------------------------------------------------
GATED_SIZES = [3, 150, 0, 260]


def _gated_plain(mmf):
    xp = offsets(GATED_SIZES)

    def make_inputs(which):
        return [rows(xp[-1], 40, 31 if which == "truth" else 32, "neg_sq_l2")]

    def entry(X):
        return mmf.simtopk_segmented_exact(X, ptr=xp, metric="neg_sq_l2", k=50)      # two passes, one segment on the launch loop

    def reference(X):
        idx = np.full((X.shape[0], 50), -1, np.int64)
        val = np.full((X.shape[0], 50), -np.inf, np.float32)
        for a, b in zip(xp[:-1], xp[1:]):
            ks = min(50, b - a - 1)
            if ks > 0:
                idx[a:b, :ks], val[a:b, :ks] = oracle.simtopk(X[a:b], X[a:b], metric="neg_sq_l2", k=ks, exclude_self=True, row_offset=a, col_offset=a)
        return [idx, val]
    return entry, make_inputs, reference


def _gated_combined(mmf):
    xp = offsets(GATED_SIZES)

    def make_inputs(which):
        g = torch.Generator().manual_seed(5 if which == "truth" else 6)
        return [rows(xp[-1], 40, 33 if which == "truth" else 34, "rbf"), torch.rand(xp[-1], 2, generator=g) * 4.0]

    def entry(F, P):
        return mmf.simtopk_combined_exact(F, P, 0.7, 0.3, 5, ptr=xp, col_splits=2)
    return entry, make_inputs, None                       # the idle call's bits; test 7 has the references


GATED = {"mmf_simtopk_segmented_exact": _gated_plain, "mmf_simtopk_combined_segmented_exact": _gated_combined}


def test_the_gated_cases_are_exactly_the_device_entries(mmf):
    assert set(GATED) == set(mmf._lib.EXPORTS_SEG_EXACT) - {"mmf_segmented_exact_table"}


@pytest.mark.parametrize("name", sorted(GATED))
def test_stream_contract_behind_a_closed_gate(mmf, name):
    import streamgate
    entry, make_inputs, reference = GATED[name](mmf)
    streamgate.run_gated(entry, make_inputs, reference, name=name, calls=2)


# ---- 10. cohort routing ------------------------------------------------------------------------------------------------------------
def test_the_cohort_builder_takes_the_exact_entry_where_no_16_bit_scan_applies(mmf, monkeypatch):
    """build_hypergraph_knn_kmeans_segmented at D = 600, k = 25 (k + self = 26 > 20 above d = 512: AUTO is the exact pass): the
    neighbours come from segmented_exact.simtopk_segmented_exact (a spy sees the call), the edges and weights are the per-slide
    mirror's and those of the unrouted builder; at k = 5 the neighbours still come from ops.simtopk_segmented."""
    from importlib import import_module
    from test_gpu_knn_kmeans_segmented import plain_loop
    kk = import_module("multimodal_fusion_amd.knn_kmeans_hypergraph")
    bh = import_module("multimodal_fusion_amd.build_hypergraph")
    se = mmf.segmented_exact
    calls = []
    exact, narrow = se.simtopk_segmented_exact, mmf.ops.simtopk_segmented
    monkeypatch.setattr(se, "simtopk_segmented_exact", lambda *a, **kw: (calls.append(("exact", kw["k"])), exact(*a, **kw))[1])
    monkeypatch.setattr(mmf.ops, "simtopk_segmented", lambda *a, **kw: (calls.append(("ops", kw["k"])), narrow(*a, **kw))[1])
    wp, tp = offsets([120, 64, 200]), offsets([10, 0, 30])
    node_ptr = offsets([130, 64, 230])
    g = torch.Generator().manual_seed(600)
    W, Tm = torch.randn(wp[-1], 600, generator=g).cuda(), torch.randn(tp[-1], 600, generator=g).cuda()
    for k, who in ((25, "exact"), (5, "ops")):
        del calls[:]
        ei, ew, eptr, stats = kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, k, 6, wsi_ptr=wp, tma_ptr=tp)
        assert calls == [(who, k)], calls
        ref = plain_loop(bh, W, Tm, wp, tp, k, 6)
        assert stats["node_ptr"] == node_ptr and eptr.tolist() == offsets([r[0].shape[1] for r in ref])
        assert torch.equal(ei, torch.cat([r[0] + node_ptr[s] for s, r in enumerate(ref)], dim=1))
        assert torch.equal(ew.view(torch.int32), torch.cat([r[1] for r in ref]).view(torch.int32))
        if who == "exact":                                # the unrouted builder: the same edges
            with monkeypatch.context() as m:
                m.setattr(mmf.ops, "fast_scan_supported", lambda *a: True)
                del calls[:]
                ei0, ew0, eptr0, _ = kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, k, 6, wsi_ptr=wp, tma_ptr=tp)
                assert calls == [("ops", k)]
            assert torch.equal(ei, ei0) and torch.equal(ew.view(torch.int32), ew0.view(torch.int32)) and torch.equal(eptr, eptr0)
