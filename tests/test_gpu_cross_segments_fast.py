"""The 16-bit cross-segment top-k (cross_segments16.*, include/ext/mmf_hg_cross_seg16.h): every row's k best
columns among the rows of all OTHER segments, candidates from one table-driven launch of the 16-bit scan with a per-row column
mask, exact re-rank.

The reference is always the existing exact ``simtopk_cross_segments`` (code this feature does not touch), compared bit for bit,
ids and values; one case also compares against the CPU oracle per segment.  On the seeded Gaussian rows the test asserts
``fallback_rows == 0`` so that a pass cannot come from the exact rescan: counted on the CPU with f16-rounded rows, the columns within
2e-2 of a row's k-th best outside its segment number at most 161 (d = 600, k = 44) and at most 108 for k <= 20 — about five times
the real margin — and the lists plus the 192-entry overflow list hold that."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_segmented import assert_same, offsets  # noqa: E402

pytestmark = pytest.mark.gpu

# n = 2001: bounds off a tile edge, a block spanning three segments (rows 0 .. 256 hold segments 0, 1 and 3), a segment holding whole
# blocks (the 700 rows at the end, and at 128 rows per block the 456 before them), an empty and a one-row segment
SIZES = [3, 150, 0, 260, 400, 31, 1, 456, 700]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PREC = {"fast": 2, "fast_bf16": 3}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def gauss(n, d, seed, dtype="f32"):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, d).astype(np.float32)).to(DTYPES[dtype])


def lam_for(d):
    return 0.5 / d                       # unit Gaussian rows are sqrt(2 d) apart: RBF values stay inside f32


def outside(idx, xp, yp):
    for s in range(len(xp) - 1):
        own = idx[xp[s]:xp[s + 1]]
        if ((own >= yp[s]) & (own < yp[s + 1])).any() or (own < 0).any() or (own >= yp[-1]).any():
            return False
    return True


def table_of(mmf, xs, ys, d, k, col_splits=0):
    t, lists = mmf.cross_segments_fast_table(offsets(xs), None if ys is None else offsets(ys), d=d, k=k, col_splits=col_splits)
    return t.shape[0], lists // 2


@functools.lru_cache(maxsize=None)
def self_inputs(d, dtype):
    return gauss(sum(SIZES), d, 100 + d, dtype).cuda()


@functools.lru_cache(maxsize=None)
def self_reference(d, dtype, metric, k):
    """The exact entry on self_inputs cut into SIZES: computed once per shape, kept on the host, never written."""
    import multimodal_fusion_amd as m
    idx, val = m.simtopk_cross_segments(self_inputs(d, dtype), ptr=offsets(SIZES), metric=metric, lam=lam_for(d), k=k)
    return idx.cpu(), val.cpu()


# ---- 1. every row of the kernel table, both operand types ---------------------------------------------------------------------------
# (d, k) -> padded dim and list capacity: 128 / 256 / 512 with 15 (k <= 11), 16 (k <= 20) and 32 (k <= 44) entries — four tiles per
# barrier at 128 and 256 with 15 entries, the d = 512 kernel, one tile per barrier for the larger lists — and the split-k kernel at
# 1024 (15 entries for every k <= 20).  Metrics and row dtypes rotate over the rows.
TABLE = [(40, 5, "cosine", "f32"), (40, 20, "dot", "f16"), (40, 44, "neg_sq_l2", "bf16"),
         (200, 5, "rbf", "f32"), (200, 20, "neg_sq_l2", "f16"), (200, 44, "cosine", "f32"),
         (300, 5, "neg_sq_l2", "f32"), (300, 20, "rbf", "bf16"), (300, 44, "dot", "f32"),
         (600, 5, "dot", "bf16"), (600, 20, "cosine", "f16")]


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("d,k,metric,dtype", TABLE)
def test_same_bits_as_the_exact_entry_on_every_kernel(mmf, d, k, metric, dtype, precision):
    X = self_inputs(d, dtype)
    xp = offsets(SIZES)
    idx, val, st = mmf.simtopk_cross_segments_fast(X, ptr=xp, metric=metric, lam=lam_for(d), k=k, precision=precision, return_stats=True)
    grid, entries = table_of(mmf, SIZES, None, d, k)
    print(f"d {d} k {k} {metric} {dtype} {precision}: scan_grid {st['scan_grid']} (table {grid}) col_splits {st['col_splits']} "
          f"candidates {st['candidates']} fallback_rows {st['fallback_rows']}")
    assert st["precision_used"] == PREC[precision] and st["scan_grid"] == grid and st["col_splits"] == entries
    assert st["fallback_rows"] == 0 and st["near_rows"] == -1
    assert outside(idx.cpu(), xp, xp)
    assert_same((idx.cpu(), val.cpu()), self_reference(d, dtype, metric, k))


@pytest.mark.parametrize("metric", ["cosine", "neg_sq_l2"])
def test_against_the_oracle_per_segment(mmf, metric):
    sizes = [257, 6, 0, 129, 3, 40]
    xp = offsets(sizes)
    X = gauss(xp[-1], 40, 13)
    idx, val, st = mmf.simtopk_cross_segments_fast(X.cuda(), ptr=xp, metric=metric, k=5, return_stats=True)
    assert st["precision_used"] == 2 and st["fallback_rows"] == 0
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    Xn = X.numpy()
    for a, b in zip(xp[:-1], xp[1:]):
        if b == a:
            continue
        ridx, rval = oracle.simtopk(Xn[a:b], np.concatenate([Xn[:a], Xn[b:]]), metric=metric, k=5, exclude_self=False)
        ridx = np.where(ridx >= a, ridx + (b - a), ridx)
        assert np.array_equal(idx[a:b], ridx), f"segment at {a}: indices differ"
        assert np.array_equal(val[a:b].view(np.int32), rval.view(np.int32))


# ---- 2. forced column runs: threshold sharing and list slots ---------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(300, 5), (300, 44), (600, 20)])
def test_forced_column_runs_give_the_same_bits(mmf, d, k):
    X = self_inputs(d, "f32")
    xp = offsets(SIZES)
    ref = self_reference(d, "f32", "cosine", k)
    for splits in (1, 2, 4, 8):
        idx, val, st = mmf.simtopk_cross_segments_fast(X, ptr=xp, metric="cosine", lam=lam_for(d), k=k, col_splits=splits, return_stats=True)
        grid, entries = table_of(mmf, SIZES, None, d, k, splits)
        assert st["scan_grid"] == grid and st["col_splits"] == entries and entries in (splits, splits + 1) and st["fallback_rows"] == 0
        assert_same((idx.cpu(), val.cpu()), ref)


def test_the_hole_inside_a_run_and_at_a_run_edge(mmf):
    """d = 300: 256 rows per block.  [512, 512, 1024] at two runs: the middle segment's hole (tiles 16 .. 32) lies inside the first run
    of 24 admissible tiles, which becomes two entries.  [512, 1024, 512] at two runs: the hole (tiles 16 .. 48) sits exactly between
    the two runs of 16."""
    for sizes, want in (([512, 512, 1024], [(0, 16), (32, 40), (40, 64)]), ([512, 1024, 512], [(0, 16), (48, 64)])):
        xp = offsets(sizes)
        t, _ = mmf.cross_segments_fast_table(xp, d=300, k=5, col_splits=2)
        assert sorted({tuple(e[3:5]) for e in t.tolist() if e[1] == 512}) == want
        X = gauss(xp[-1], 300, 17).cuda()
        ref = mmf.simtopk_cross_segments(X, ptr=xp, metric="cosine", k=5)
        for splits in (1, 2, 4):
            idx, val, st = mmf.simtopk_cross_segments_fast(X, ptr=xp, metric="cosine", k=5, col_splits=splits, return_stats=True)
            assert st["fallback_rows"] == 0 and (st["scan_grid"], st["col_splits"]) == table_of(mmf, sizes, None, 300, 5, splits)
            assert_same((idx, val), ref)


# ---- 3. two-sided ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,precision", [("cosine", "fast"), ("rbf", "fast_bf16")])
def test_two_sided_same_bits_as_the_exact_entry(mmf, metric, precision):
    xs = [40, 0, 129, 5, 257, 1, 300, 32]               # segment 1: no queries
    ys = [300, 7, 33, 0, 128, 256, 4, 1000]             # segment 3: no rows of Y, nothing excluded for its 5 queries
    xp, yp = offsets(xs), offsets(ys)
    X, Y = gauss(xp[-1], 100, 1).cuda(), gauss(yp[-1], 100, 2).cuda()
    Y[yp[0] + 3] = X[xp[0] + 3]                         # copies of a query: one inside its segment of Y, one outside
    Y[yp[5] + 9] = X[xp[0] + 3]
    kw = dict(metric=metric, lam=lam_for(100))
    for k in (5, 28):
        idx, val, st = mmf.simtopk_cross_segments_fast(X, Y, ptr=xp, y_ptr=yp, k=k, precision=precision, return_stats=True, **kw)
        assert (st["scan_grid"], st["col_splits"]) == table_of(mmf, xs, ys, 100, k) and st["precision_used"] == PREC[precision]
        assert st["fallback_rows"] == 0
        assert outside(idx.cpu(), xp, yp)
        assert_same((idx, val), mmf.simtopk_cross_segments(X, Y, ptr=xp, y_ptr=yp, k=k, **kw))
    assert idx[xp[0] + 3, 0] == yp[5] + 9
    got = mmf.simtopk_cross_segments_fast(X, Y, ptr=xp, y_ptr=yp, k=5, precision=precision, **kw)
    xb = torch.repeat_interleave(torch.arange(len(xs)), torch.tensor(xs))
    yb = torch.repeat_interleave(torch.arange(len(ys)), torch.tensor(ys))
    assert_same(mmf.simtopk_cross_segments_fast(X, Y, batch=xb, y_batch=yb, k=5, precision=precision, **kw), got)
    # the router takes this call under "auto"
    assert_same(mmf.cross_segments16.simtopk_cross_segments(X, Y, ptr=xp, y_ptr=yp, k=5, **kw), got)


# ---- 4. the mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 600])
def test_tight_clusters_per_segment_return_no_row_of_the_own_slide(mmf, d):
    """Each segment is one tight cluster, so every row's nearest rows are its own slide's: the plain 16-bit call returns them, and a
    mask that let one column of a row's own segment through would return it here."""
    rng = np.random.RandomState(5)
    xp = offsets(SIZES)
    centre = rng.randn(len(SIZES), d).astype(np.float32)
    seg = np.repeat(np.arange(len(SIZES)), SIZES)
    X = torch.from_numpy(centre[seg] + 0.02 * rng.randn(xp[-1], d).astype(np.float32)).cuda()
    for metric in ("neg_sq_l2", "cosine"):
        plain, _ = mmf.ops.simtopk(X, metric=metric, k=5, precision="fast")
        assert not outside(plain.cpu(), xp, xp)
        ref = mmf.simtopk_cross_segments(X, ptr=xp, metric=metric, k=5)
        for splits in (0, 2):
            idx, val = mmf.simtopk_cross_segments_fast(X, ptr=xp, metric=metric, k=5, col_splits=splits)
            assert outside(idx.cpu(), xp, xp)
            assert_same((idx, val), ref)


def test_a_copy_in_the_own_segment_is_never_returned_and_a_copy_elsewhere_comes_first(mmf):
    """Segment s = its rows, an exact copy of them, and an exact copy of the rows of segment s + 1."""
    parts = [gauss(n, 40, 20 + i) for i, n in enumerate([70, 130, 45])]
    S = len(parts)
    segs = [torch.cat([parts[s], parts[s], parts[(s + 1) % S]]) for s in range(S)]
    xp = offsets([t.shape[0] for t in segs])
    X = torch.cat(segs).cuda()
    idx, val = mmf.simtopk_cross_segments_fast(X, ptr=xp, metric="neg_sq_l2", k=5)
    assert outside(idx.cpu(), xp, xp)
    for s in range(S):
        n, prev = parts[s].shape[0], (s - 1) % S
        elsewhere = xp[prev] + 2 * parts[prev].shape[0] + torch.arange(n)           # the third part of segment s - 1
        assert torch.equal(idx[xp[s]:xp[s] + n, 0].cpu(), elsewhere), f"segment {s}: the copy in segment {prev} is not the first neighbour"
        assert (val[xp[s]:xp[s] + n, 0] == 0).all()
    assert_same((idx, val), mmf.simtopk_cross_segments(X, ptr=xp, metric="neg_sq_l2", k=5))


def test_ties_rank_by_ascending_global_id(mmf):
    """Fourteen identical rows spread over four segments: a row of them gets the identical rows of the OTHER segments, by id."""
    base = gauss(500, 40, 6)
    xp = offsets([140, 200, 60, 100])
    same = [3, 77, 139, 141, 150, 151, 339, 340, 341, 399, 400, 401, 450, 499]
    base[same] = base[same[0]].clone()
    X = base.cuda()
    idx, val = mmf.simtopk_cross_segments_fast(X, ptr=xp, metric="neg_sq_l2", k=5)
    seg = np.searchsorted(np.asarray(xp), np.arange(500), side="right") - 1
    for i in same:
        assert idx[i].tolist() == [j for j in same if seg[j] != seg[i]][:5]
    assert_same((idx, val), mmf.simtopk_cross_segments(X, ptr=xp, metric="neg_sq_l2", k=5))


# ---- 5. flagged rows: the exact cross-segment rescan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,precision", [(40, "fast"), (600, "fast_bf16")])
def test_flagged_rows_take_the_exact_cross_scan_and_give_the_same_bits(mmf, d, precision):
    """400 exact copies of one vector, 100 in each of four segments.  With one column run a row has at most two entries: 2 x 2 x 15
    list entries and 192 overflow slots.  A copy has 300 copies outside its segment, all tied at the best key and all inside any
    margin, which the lists cannot hold: every copy is flagged — rows of four segments — and the first five ids of the tie must
    come from the exact rescan."""
    xp = offsets(SIZES)
    Xh = gauss(xp[-1], d, 300 + d)
    copies = np.concatenate([xp[s] + 7 + np.arange(100) for s in (3, 4, 7, 8)])
    Xh[copies] = Xh[copies[0]].clone()
    X = Xh.cuda()
    for metric in ("neg_sq_l2", "cosine"):
        idx, val, st = mmf.simtopk_cross_segments_fast(X, ptr=xp, metric=metric, k=5, col_splits=1, precision=precision, return_stats=True)
        print(f"d {d} {metric}: fallback_rows {st['fallback_rows']} overflow_rows {st['overflow_rows']} short_rows {st['short_rows']}")
        assert st["precision_used"] == PREC[precision] and st["fallback_rows"] >= 400
        assert outside(idx.cpu(), xp, xp)
        assert_same((idx, val), mmf.simtopk_cross_segments(X, ptr=xp, metric=metric, k=5))
        seg = np.searchsorted(np.asarray(xp), copies, side="right") - 1
        first = idx[torch.from_numpy(copies).cuda()].cpu().numpy()
        for i, s in zip(range(0, 400, 57), seg[::57]):
            assert first[i].tolist() == [int(j) for j in copies[seg != s][:5]]


# ---- 6. refusals and the router with device tensors -------------------------------------------------------------------------------------
def test_unserved_shapes_are_refused_under_fast_and_exact_under_auto(mmf):
    cs16 = mmf.cross_segments16
    sizes = [100, 60, 140]
    xp = offsets(sizes)
    L = mmf._lib.lib()
    P, stream = mmf.ops._p, mmf.ops._stream(torch.device("cuda", 0))
    p = torch.tensor(xp, dtype=torch.int64)
    for d, k in ((1100, 5), (600, 21)):
        X = gauss(xp[-1], d, 50 + k).cuda()
        for precision in ("fast", "fast_bf16"):
            with pytest.raises(ValueError, match=f"does not serve d = {d}, k = {k}"):
                mmf.simtopk_cross_segments_fast(X, ptr=xp, k=k, precision=precision)
            idx = torch.empty((xp[-1], k), dtype=torch.int64, device="cuda")
            val = torch.empty((xp[-1], k), dtype=torch.float32, device="cuda")
            opts = mmf._lib.SimtopkOpts(PREC[precision], 0, 0, 1, None)
            rc = L.mmf_simtopk_cross_segments_fast(P(X), xp[-1], None, 0, d, 0, 1, 1.0, k, P(p), None, len(sizes), P(idx), P(val),
                                                   ctypes.byref(opts), None, 0, stream)
            msg = L.mmf_last_error().decode()
            assert rc == mmf._lib.MMF_E_UNSUPPORTED and f"d = {d}, k = {k}" in msg and "simtopk_cross_segments_fast" in msg
        ref = mmf.simtopk_cross_segments(X, ptr=xp, k=k)
        idx, val, st = cs16.simtopk_cross_segments(X, ptr=xp, k=k, return_stats=True)                  # auto: the exact entry
        assert st["precision_used"] == 1
        assert_same((idx, val), ref)
        stats = mmf._lib.SimtopkStats()
        idx.zero_()
        rc = L.mmf_simtopk_cross_segments_fast(P(X), xp[-1], None, 0, d, 0, 1, 1.0, k, P(p), None, len(sizes), P(idx), P(val), None,
                                               ctypes.byref(stats), 0, stream)                            # the C entry's AUTO: the exact driver
        torch.cuda.synchronize()
        assert rc == 0 and stats.precision_used == 1
        assert_same((idx, val), ref)
    X = gauss(xp[-1], 64, 3).cuda()
    for precision, used in (("auto", 2), ("exact", 1), ("fast_bf16", 3)):
        idx, val, st = cs16.simtopk_cross_segments(X, ptr=xp, k=5, precision=precision, return_stats=True)
        assert st["precision_used"] == used
        assert_same((idx, val), mmf.simtopk_cross_segments(X, ptr=xp, k=5))


# ---- 7. stream contract ---------------------------------------------------------------------------------------------------------------
GATED_SIZES = [3, 150, 0, 260]


def test_stream_contract_behind_a_closed_gate(mmf):
    import streamgate
    xp = offsets(GATED_SIZES)

    def make_inputs(which):
        return [gauss(xp[-1], 40, 31 if which == "truth" else 32)]

    def entry(X):
        return mmf.simtopk_cross_segments_fast(X, ptr=xp, metric="neg_sq_l2", k=5, col_splits=2)

    def reference(X):
        idx = np.empty((X.shape[0], 5), np.int64)
        val = np.empty((X.shape[0], 5), np.float32)
        for a, b in zip(xp[:-1], xp[1:]):
            if b > a:
                i, v = oracle.simtopk(X[a:b], np.concatenate([X[:a], X[b:]]), metric="neg_sq_l2", k=5, exclude_self=False)
                idx[a:b], val[a:b] = np.where(i >= a, i + (b - a), i), v
        return [idx, val]
    streamgate.run_gated(entry, make_inputs, reference, name="mmf_simtopk_cross_segments_fast", calls=2)


# ---- 8. edge builders -----------------------------------------------------------------------------------------------------------------
def test_edge_builders_under_auto_equal_their_default_precision(mmf):
    cs16 = mmf.cross_segments16
    sizes = [150, 40, 0, 129, 70]
    xp = offsets(sizes)
    X = gauss(xp[-1], 40, 41).cuda()
    ei, ew = mmf.cross_segment_knn_edges(X, ptr=xp, k=5)
    for got in (cs16.cross_segment_knn_edges(X, ptr=xp, k=5, precision="auto"), cs16.cross_segment_knn_edges(X, ptr=xp, k=5)):
        assert torch.equal(got[0], ei) and torch.equal(got[1].view(torch.int32), ew.view(torch.int32))
    from test_gpu_kmeans_ragged import _clustered
    sizes, tmas, C, d = [60, 90, 75], [16, 24, 5], 12, 32
    wp, tp = offsets(sizes), offsets(tmas)
    F = torch.from_numpy(np.concatenate([_clustered(n, d, 900 + s) for s, n in enumerate(sizes)])).cuda()
    P = torch.from_numpy(np.concatenate([np.random.RandomState(950 + s).rand(n, 2).astype(np.float32) for s, n in enumerate(sizes)])).cuda()
    tma = torch.from_numpy(np.concatenate([_clustered(m, d, 980 + s) for s, m in enumerate(tmas)])).cuda()
    out = mmf.build_cohort_hypergraphs(F, P, tma, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=3, hypergraph_k=3, num_hyperedges=4)
    ei, ew = mmf.cohort.link_slides(out, k=4)
    for got in (cs16.link_slides(out, k=4, precision="auto"), cs16.link_slides(out, 4)):
        assert torch.equal(got[0], ei) and torch.equal(got[1].view(torch.int32), ew.view(torch.int32))
