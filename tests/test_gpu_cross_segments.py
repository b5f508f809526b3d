"""The cross-segment top-k (cross_segments.*, include/ext/mmf_hg_cross_seg.h): for every row of a ragged batch
the k best columns among the rows of all OTHER segments, from one table-driven launch of the exact scan and one re-rank.

The reference is code this feature does not touch: per segment s the exact ops.simtopk of X_s against Y[:lo] (col_offset 0) and
against Y[hi:] (col_offset hi), exclude_self=False, merged by ops.topk_merge — or, equivalently, the single exact call against the
concatenation of the two runs with the ids mapped back.  The loop takes the merge where it IS equivalent: both sides hold k columns
(topk_merge takes two [n, k] tables) and the metric is not RBF.  topk_merge ranks by VALUE, and an RBF value is exp(key): near 1
thousands of distinct canonical keys share one float, so a merge by value cannot reproduce the order by key that the contract
(and mmf_simtopk_ex on the concatenation) defines; RBF takes the concatenation.  Indices equal, values bitwise equal.  The CPU
oracle per segment is the second reference (RBF values to the project's 1e-5)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_segmented import assert_same, dup_rows, offsets  # noqa: E402

pytestmark = pytest.mark.gpu

# bounds on a tile edge (128, 256), one off it, inside the first tile and inside the last, partial, tile (m = 1300); the 400- and
# 385-row segments swallow whole tiles; a one-row and an empty segment; the first and the last segment have rows
SIZES = [100, 400, 1, 0, 127, 128, 129, 385, 30]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LAM = 0.5


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def rows(n, d, seed, metric="cosine", dtype="f32"):
    return torch.from_numpy(dup_rows(n, d, seed, scale=0.1 if metric == "rbf" else 1.0)).to(DTYPES[dtype])


def loop_reference(mmf, X, Y, xp, yp, k, **kw):
    """The only way to the answer without the entry: a loop over segments of exact ops.simtopk calls (module docstring)."""
    Yf = X if Y is None else Y
    m = Yf.shape[0]
    idx = torch.empty((X.shape[0], k), dtype=torch.int64, device=X.device)
    val = torch.empty((X.shape[0], k), dtype=torch.float32, device=X.device)
    for s in range(len(xp) - 1):
        a, b, lo, hi = int(xp[s]), int(xp[s + 1]), int(yp[s]), int(yp[s + 1])
        if a == b:
            continue
        assert m - (hi - lo) >= k
        if lo >= k and m - hi >= k and kw.get("metric") != "rbf":
            il, vl = mmf.ops.simtopk(X[a:b], Yf[:lo], k=k, exclude_self=False, col_offset=0, precision="exact", **kw)
            ir, vr = mmf.ops.simtopk(X[a:b], Yf[hi:], k=k, exclude_self=False, col_offset=hi, precision="exact", **kw)
            i, v = mmf.ops.topk_merge(il, vl, ir, vr)
        else:
            i, v = mmf.ops.simtopk(X[a:b], torch.cat([Yf[:lo], Yf[hi:]]), k=k, exclude_self=False, precision="exact", **kw)
            i = torch.where(i >= lo, i + (hi - lo), i)
        idx[a:b], val[a:b] = i, v
    return idx, val


def table_of(mmf, xs, ys, k, col_splits=0):
    """(scan_grid, col_splits) the call must report: the host table query's."""
    t, lists = mmf.cross_segments_table(offsets(xs), None if ys is None else offsets(ys), k=k, col_splits=col_splits)
    return t.shape[0], lists // 2


def outside(idx, xp, yp):
    """Every returned id lies outside the row's own segment of Y."""
    for s in range(len(xp) - 1):
        own = idx[xp[s]:xp[s + 1]]
        if ((own >= yp[s]) & (own < yp[s + 1])).any() or (own < 0).any() or (own >= yp[-1]).any():
            return False
    return True


@functools.lru_cache(maxsize=None)
def self_inputs(d, dtype, metric):
    return rows(sum(SIZES), d, 11 + d, metric, dtype).cuda()


@functools.lru_cache(maxsize=None)
def self_reference(d, dtype, metric, k):
    """The loop over self_inputs cut into SIZES: computed once per shape, kept on the host, never written."""
    import multimodal_fusion_amd as m
    xp = offsets(SIZES)
    idx, val = loop_reference(m, self_inputs(d, dtype, metric), None, xp, xp, k, metric=metric, lam=LAM)
    return idx.cpu(), val.cpu()


# ---- 1. same bits as the loop: every metric, dtype and list capacity ----------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 12, 28])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
@pytest.mark.parametrize("d", [40, 100])
def test_self_ragged_same_bits_as_the_loop(mmf, d, metric, dtype, k):
    X = self_inputs(d, dtype, metric)
    xp = offsets(SIZES)
    idx, val, st = mmf.simtopk_cross_segments(X, ptr=xp, metric=metric, lam=LAM, k=k, return_stats=True)
    grid, ranges = table_of(mmf, SIZES, None, k)
    print(f"d {d} {metric} {dtype} k {k}: scan_grid {st['scan_grid']} (table {grid}) col_splits {st['col_splits']} candidates {st['candidates']}")
    assert st["precision_used"] == 1 and st["scan_grid"] == grid and st["col_splits"] == ranges
    assert st["fallback_rows"] == 0 and st["near_rows"] == -1
    assert outside(idx.cpu(), xp, xp)
    assert_same((idx.cpu(), val.cpu()), self_reference(d, dtype, metric, k))


@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
def test_against_the_oracle_per_segment(mmf, metric):
    sizes = [257, 6, 0, 129, 3, 40]
    xp = offsets(sizes)
    X = rows(xp[-1], 40, 13, metric)
    idx, val = mmf.simtopk_cross_segments(X.cuda(), ptr=xp, metric=metric, lam=LAM, k=5)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    Xn = X.numpy()
    for a, b in zip(xp[:-1], xp[1:]):
        if b == a:
            continue
        ridx, rval = oracle.simtopk(Xn[a:b], np.concatenate([Xn[:a], Xn[b:]]), metric=metric, lam=LAM, k=5, exclude_self=False)
        ridx = np.where(ridx >= a, ridx + (b - a), ridx)
        assert np.array_equal(idx[a:b], ridx), f"segment at {a}: indices differ"
        if metric == "rbf":
            assert np.allclose(val[a:b], rval, rtol=0, atol=1e-5)
        else:
            assert np.array_equal(val[a:b].view(np.int32), rval.view(np.int32))


# ---- 2. nothing leaks -------------------------------------------------------------------------------------------------------------
def test_tight_clusters_per_segment_return_no_row_of_the_own_slide(mmf):
    """Each segment is one tight cluster, so every row's nearest rows are its own slide's: a mask that let a column of the row
    block's segment through would return it."""
    rng = np.random.RandomState(5)
    xp = offsets(SIZES)
    centre = rng.randn(len(SIZES), 100).astype(np.float32)
    seg = np.repeat(np.arange(len(SIZES)), SIZES)
    X = torch.from_numpy(centre[seg] + 0.02 * rng.randn(xp[-1], 100).astype(np.float32)).cuda()
    for metric in ("neg_sq_l2", "cosine"):
        plain, _ = mmf.ops.simtopk(X, metric=metric, k=5, precision="exact")
        assert not outside(plain.cpu(), xp, xp)                                   # the plain call fills the lists with the own slide
        for splits in (0, 2):
            idx, val = mmf.simtopk_cross_segments(X, ptr=xp, metric=metric, k=5, col_splits=splits)
            assert outside(idx.cpu(), xp, xp)
            assert_same((idx, val), loop_reference(mmf, X, None, xp, xp, 5, metric=metric))


def test_a_copy_in_the_own_segment_is_never_returned_and_a_copy_elsewhere_is(mmf):
    """Segment s = its rows, an exact copy of them, and an exact copy of the rows of segment s + 1.  For a row of the first part the
    copy inside its segment is never returned; the copy in segment s - 1 (distance 0) is its first neighbour."""
    parts = [rows(n, 40, 20 + i) for i, n in enumerate([70, 130, 45])]
    S = len(parts)
    segs = [torch.cat([parts[s], parts[s], parts[(s + 1) % S]]) for s in range(S)]
    xp = offsets([t.shape[0] for t in segs])
    X = torch.cat(segs).cuda()
    idx, val = mmf.simtopk_cross_segments(X, ptr=xp, metric="neg_sq_l2", k=5)
    assert outside(idx.cpu(), xp, xp)
    for s in range(S):
        n, prev = parts[s].shape[0], (s - 1) % S
        elsewhere = xp[prev] + 2 * parts[prev].shape[0] + torch.arange(n)           # the third part of segment s - 1
        got = idx[xp[s]:xp[s] + n, 0].cpu()
        assert torch.equal(got, elsewhere), f"segment {s}: the copy in segment {prev} is not the first neighbour"
        assert (val[xp[s]:xp[s] + n, 0] == 0).all()
    assert_same((idx, val), loop_reference(mmf, X, None, xp, xp, 5, metric="neg_sq_l2"))


# ---- 3. column ranges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 28])
def test_forced_column_ranges_give_the_same_bits(mmf, k):
    """SIZES: the holes of the 400- and 385-row segments fall inside a range at every count.  [256, 512, 256] at two ranges: the hole
    of the middle segment (tiles 2 .. 5) sits exactly at a range edge."""
    X = self_inputs(100, "f32", "cosine")
    xp = offsets(SIZES)
    ref = self_reference(100, "f32", "cosine", k)
    for splits in (1, 2, 4, 8):
        idx, val, st = mmf.simtopk_cross_segments(X, ptr=xp, metric="cosine", lam=LAM, k=k, col_splits=splits, return_stats=True)
        grid, ranges = table_of(mmf, SIZES, None, k, splits)
        # 11 tiles, 9 of them admissible for the large segments: 8 ranges are runs of two tiles, five or six of them
        assert st["col_splits"] == ranges and st["scan_grid"] == grid and (ranges in (splits, splits + 1) if splits < 8 else ranges == 6)
        assert_same((idx.cpu(), val.cpu()), ref)
    sizes = [256, 512, 256]
    xp = offsets(sizes)
    t, _ = mmf.cross_segments_table(xp, k=k, col_splits=2)
    assert sorted({tuple(e[4:6]) for e in t.tolist() if e[0] == 1}) == [(0, 2), (6, 8)]
    Xa = rows(xp[-1], 40, 17).cuda()
    ref = loop_reference(mmf, Xa, None, xp, xp, k, metric="cosine")
    for splits in (1, 2, 4):
        assert_same(mmf.simtopk_cross_segments(Xa, ptr=xp, metric="cosine", k=k, col_splits=splits), ref)


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------------
def test_ties_rank_by_ascending_global_id(mmf):
    """Fourteen identical rows spread over four segments: a row of them gets the identical rows of the OTHER segments, by id."""
    base = rows(500, 40, 6)
    xp = offsets([140, 200, 60, 100])
    same = [3, 77, 139, 141, 150, 151, 339, 340, 341, 399, 400, 401, 450, 499]
    base[same] = base[same[0]].clone()
    X = base.cuda()
    idx, val = mmf.simtopk_cross_segments(X, ptr=xp, metric="neg_sq_l2", k=5)
    seg = np.searchsorted(np.asarray(xp), np.arange(500), side="right") - 1
    for i in same:
        assert idx[i].tolist() == [j for j in same if seg[j] != seg[i]][:5]
    assert_same((idx, val), loop_reference(mmf, X, None, xp, xp, 5, metric="neg_sq_l2"))


# ---- 5. k > 44: passes behind per-row floors ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_k_inputs():
    sizes = [129, 60, 257, 100, 0, 31]
    X = rows(sum(sizes), 40, 21, "neg_sq_l2")
    p = offsets(sizes)
    X[p[1]:p[2]] = X[p[1]]                               # a whole segment of identical rows ...
    X[p[2] + 100:p[2] + 170] = X[p[1]]                   # ... 70 more inside a larger one ...
    X[p[3]:p[4]] = X[p[1]]                               # ... and another whole segment: for a row of them, the ties of the other
    return sizes, X.cuda()                               # segments (130 to 170 columns) cross the pass boundaries at 44 and 88


@pytest.mark.parametrize("metric", ["neg_sq_l2", "cosine"])
@pytest.mark.parametrize("k", [50, 95])
def test_large_k_runs_passes_and_matches_the_loop(mmf, k, metric):
    sizes, X = large_k_inputs()
    xp = offsets(sizes)
    idx, val, st = mmf.simtopk_cross_segments(X, ptr=xp, metric=metric, k=k, return_stats=True)
    assert (st["scan_grid"], st["col_splits"]) == table_of(mmf, sizes, None, k)
    assert outside(idx.cpu(), xp, xp)
    assert_same((idx, val), loop_reference(mmf, X, None, xp, xp, k, metric=metric))
    got = mmf.simtopk_cross_segments(X, ptr=xp, metric=metric, k=k, col_splits=2)
    assert_same(got, (idx, val))


# ---- 6. two-sided -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "rbf"])
def test_two_sided_same_bits_as_the_loop(mmf, metric):
    xs = [40, 0, 129, 5, 257, 1, 300, 32]               # segment 1: no queries
    ys = [300, 7, 33, 0, 128, 256, 4, 1000]             # segment 3: no rows of Y, nothing excluded for its 5 queries
    xp, yp = offsets(xs), offsets(ys)
    X, Y = rows(xp[-1], 100, 1, metric).cuda(), rows(yp[-1], 100, 2, metric).cuda()
    Y[yp[0] + 3] = X[xp[0] + 3]                         # copies of a query: one inside its segment of Y, one outside
    Y[yp[5] + 9] = X[xp[0] + 3]
    kw = dict(metric=metric, lam=LAM)
    for k in (5, 28):
        idx, val, st = mmf.simtopk_cross_segments(X, Y, ptr=xp, y_ptr=yp, k=k, return_stats=True, **kw)
        assert (st["scan_grid"], st["col_splits"]) == table_of(mmf, xs, ys, k)
        assert outside(idx.cpu(), xp, yp)
        assert_same((idx, val), loop_reference(mmf, X, Y, xp, yp, k, **kw))
    assert idx[xp[0] + 3, 0] == yp[5] + 9
    # the rows of the segment that excludes nothing: the plain exact call against all of Y
    ref = mmf.ops.simtopk(X[xp[3]:xp[4]], Y, k=5, exclude_self=False, precision="exact", **kw)
    got = mmf.simtopk_cross_segments(X, Y, ptr=xp, y_ptr=yp, k=5, **kw)
    assert_same((got[0][xp[3]:xp[4]], got[1][xp[3]:xp[4]]), ref)
    # batch vectors instead of offsets
    xb = torch.repeat_interleave(torch.arange(len(xs)), torch.tensor(xs))
    yb = torch.repeat_interleave(torch.arange(len(ys)), torch.tensor(ys))
    assert_same(mmf.simtopk_cross_segments(X, Y, batch=xb, y_batch=yb, k=5, **kw), got)


# ---- 7. refusals on the device path ---------------------------------------------------------------------------------------------------
def test_refusals_with_device_tensors(mmf):
    X = self_inputs(40, "f32", "cosine")
    xp = offsets(SIZES)
    n = xp[-1]
    with pytest.raises(ValueError, match=r"segment 1 has 900 admissible columns \(m = 1300 minus its own 400 rows of Y\), k = 901"):
        mmf.simtopk_cross_segments(X, ptr=xp, k=901)
    L = mmf._lib.lib()
    p = torch.tensor(xp, dtype=torch.int64)
    idx = torch.empty((n, 900), dtype=torch.int64, device="cuda")              # rows are k wide: room for the largest k that runs
    val = torch.empty((n, 900), dtype=torch.float32, device="cuda")
    P, st = mmf.ops._p, mmf.ops._stream(X.device)

    def entry(k, precision):
        opts = mmf._lib.SimtopkOpts(precision, 0, 0, 1, None)
        rc = L.mmf_simtopk_cross_segments(P(X), n, None, 0, 40, 0, 1, 1.0, k, P(p), None, len(SIZES), P(idx), P(val), ctypes.byref(opts), None, 0, st)
        return rc, L.mmf_last_error().decode()
    rc, msg = entry(901, 1)
    assert rc == mmf._lib.MMF_E_INVALID and "segment 1 has 900 admissible columns" in msg and "simtopk_cross_segments" in msg
    for precision in (2, 3):
        rc, msg = entry(5, precision)
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and "no 16-bit scan serves the cross-segment entry yet" in msg
    rc, msg = entry(900, 1)                                                       # exactly the admissible columns of the largest segment
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert outside(idx.cpu(), xp, xp)
    a, b = xp[1], xp[2]
    rest = torch.cat([torch.arange(0, a), torch.arange(b, n)])
    assert torch.equal(idx[a:b].cpu().sort(dim=1).values, rest.expand(b - a, -1))      # every admissible column, once


# ---- 8. stream contract ---------------------------------------------------------------------------------------------------------------
GATED_SIZES = [3, 150, 0, 260]


def test_stream_contract_behind_a_closed_gate(mmf):
    import streamgate
    xp = offsets(GATED_SIZES)

    def make_inputs(which):
        return [rows(xp[-1], 40, 31 if which == "truth" else 32, "neg_sq_l2")]

    def entry(X):
        return mmf.simtopk_cross_segments(X, ptr=xp, metric="neg_sq_l2", k=50)       # two passes

    def reference(X):
        idx = np.empty((X.shape[0], 50), np.int64)
        val = np.empty((X.shape[0], 50), np.float32)
        for a, b in zip(xp[:-1], xp[1:]):
            if b > a:
                i, v = oracle.simtopk(X[a:b], np.concatenate([X[:a], X[b:]]), metric="neg_sq_l2", k=50, exclude_self=False)
                idx[a:b], val[a:b] = np.where(i >= a, i + (b - a), i), v
        return [idx, val]
    streamgate.run_gated(entry, make_inputs, reference, name="mmf_simtopk_cross_segments", calls=2)


# ---- 9. edges -------------------------------------------------------------------------------------------------------------------------
def test_cross_segment_knn_edges_against_numpy(mmf):
    sizes = [150, 40, 0, 129, 70]
    xp = offsets(sizes)
    Xh = rows(xp[-1], 40, 41)
    X = Xh.cuda()
    ei, ew = mmf.cross_segment_knn_edges(X, ptr=xp, k=5)
    nbr = loop_reference(mmf, X, None, xp, xp, 5, metric="neg_sq_l2")[0].cpu().numpy()
    pairs = sorted({(min(i, int(j)), max(i, int(j))) for i in range(nbr.shape[0]) for j in nbr[i]})
    want = np.asarray(pairs, dtype=np.int64).T
    assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), want)
    seg = np.searchsorted(np.asarray(xp), np.arange(xp[-1]), side="right") - 1
    assert (seg[want[0]] != seg[want[1]]).all()
    w = ew.cpu().numpy()
    assert w.dtype == np.float32 and np.array_equal(w, oracle.edge_cosine(Xh.numpy(), want)) and (w >= 0).all()
    got = mmf.cross_segment_knn_edges(X, batch=torch.from_numpy(seg), k=5)
    assert torch.equal(got[0], ei) and torch.equal(got[1], ew)


def test_link_slides_joins_different_slides_in_the_cohorts_node_numbering(mmf):
    from test_gpu_kmeans_ragged import _clustered
    sizes, tmas, C, d = [60, 90, 75], [16, 24, 5], 12, 32
    wp, tp = offsets(sizes), offsets(tmas)
    F = torch.from_numpy(np.concatenate([_clustered(n, d, 900 + s) for s, n in enumerate(sizes)])).cuda()
    P = torch.from_numpy(np.concatenate([np.random.RandomState(950 + s).rand(n, 2).astype(np.float32) for s, n in enumerate(sizes)])).cuda()
    tma = torch.from_numpy(np.concatenate([_clustered(m, d, 980 + s) for s, m in enumerate(tmas)])).cuda()
    out = mmf.build_cohort_hypergraphs(F, P, tma, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=3, hypergraph_k=3, num_hyperedges=4)
    ei, ew = mmf.cohort.link_slides(out, k=4)
    node_ptr = out["node_ptr"].tolist()
    assert node_ptr == offsets([C + t for t in tmas]) and ei.device == out["super_features"].device
    e = ei.cpu().numpy()
    slide = np.searchsorted(np.asarray(node_ptr), e, side="right") - 1
    local = e - np.asarray(node_ptr)[slide]
    assert e.shape[0] == 2 and e.shape[1] >= 3 * C * 4 // 2 and (slide[0] != slide[1]).all(), "an edge inside one slide"
    assert (local >= 0).all() and (local < C).all(), "an edge ends at a TMA node"
    assert (e[0] < e[1]).all()
    # the same edges as the rows' own numbering gives, moved into the cohort's
    sf = out["super_features"]
    ri, rw = mmf.cross_segment_knn_edges(sf, ptr=out["group_ptr"], k=4)
    r = ri.cpu().numpy()
    moved = r + (np.asarray(node_ptr)[:-1] - np.arange(3) * C)[r // C]
    assert np.array_equal(e, moved) and torch.equal(ew, rw)
    assert np.array_equal(ew.cpu().numpy(), oracle.edge_cosine(sf.cpu().numpy(), r))
