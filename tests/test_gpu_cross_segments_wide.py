"""The wide 16-bit cross-segment top-k (cross_segments_wide.*, include/ext/mmf_hg_cross_segw.h): every row's k best
columns among the rows of all OTHER segments at feature dims above 1024, candidates from one table-driven launch of the wide 16-bit
scan with a per-row column mask, exact re-rank.

The reference is always the existing exact ``simtopk_cross_segments`` (code this feature does not touch), compared bit for bit,
ids and values; one case also compares against the CPU oracle per segment.  How many rows the scan may hand to the exact rescan is
bounded from the reference alone: ``band_sizes_outside`` (tests/test_cross_segments_wide_cpu.py) restates the margin band over a
row's admissible columns, a row whose band fits its list capacity is never flagged (header of mmf_scan_b16w.hip), and the CPU test
shows that with f16 operands no row of the kernel table's data has a larger band — so ``fallback_rows == 0`` there."""
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
from test_cross_segments_wide_cpu import OFFSETS, TABLE, WHOLE, band_sizes_outside, gauss, table_rows  # noqa: E402

pytestmark = pytest.mark.gpu

PREC = {"fast": 2, "fast_bf16": 3}
OPERAND = {"fast": "f16", "fast_bf16": "bf16"}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def lam_for(d):
    return 0.5 / d                       # unit Gaussian rows are sqrt(2 d) apart: RBF values stay inside f32


def outside(idx, xp, yp):
    for s in range(len(xp) - 1):
        own = idx[xp[s]:xp[s + 1]]
        if ((own >= yp[s]) & (own < yp[s + 1])).any() or (own < 0).any() or (own >= yp[-1]).any():
            return False
    return True


def table_of(mmf, xp, yp, d, k, col_splits=0):
    t, lists = mmf.cross_segments_wide_table(xp, yp, d=d, k=k, col_splits=col_splits)
    return t.shape[0], lists // 2


def crowded_rows(X, xp, metric, precision, k):
    """Rows whose margin band over their admissible columns exceeds the list capacity: the only rows the scan may flag."""
    cap = 16 if k <= 11 else 32
    return int((band_sizes_outside(X.cpu(), xp, metric, OPERAND[precision], k) > cap).sum())


@functools.lru_cache(maxsize=None)
def table_reference(d, dtype, metric, k):
    """The exact entry on the kernel table's rows: computed once per shape, kept on the host, never written."""
    import multimodal_fusion_amd as m
    idx, val = m.simtopk_cross_segments(table_rows(d, dtype).cuda(), ptr=OFFSETS, metric=metric, lam=lam_for(d), k=k)
    return idx.cpu(), val.cpu()


# ---- 1. the kernel table: both padded dims, both list capacities, both operand types ---------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("d,k,metric,dtype", TABLE)
def test_same_bits_as_the_exact_entry_on_every_kernel(mmf, d, k, metric, dtype, precision):
    X = table_rows(d, dtype).cuda()
    idx, val, st = mmf.simtopk_cross_segments_wide(X, ptr=OFFSETS, metric=metric, lam=lam_for(d), k=k, precision=precision, return_stats=True)
    grid, entries = table_of(mmf, OFFSETS, None, d, k)
    crowded = 0 if precision == "fast" else crowded_rows(table_rows(d, dtype), OFFSETS, metric, precision, k)
    print(f"d {d} k {k} {metric} {dtype} {precision}: scan_grid {st['scan_grid']} (table {grid}) col_splits {st['col_splits']} "
          f"candidates {st['candidates']} fallback_rows {st['fallback_rows']} (rows with a band beyond the lists: {crowded})")
    assert st["precision_used"] == PREC[precision] and st["scan_grid"] == grid and st["col_splits"] == entries
    assert st["near_rows"] == -1
    # f16: tests/test_cross_segments_wide_cpu.py shows that no row's band exceeds its lists; bf16: the restated count bounds it
    assert st["fallback_rows"] <= crowded
    assert outside(idx.cpu(), OFFSETS, OFFSETS)
    assert_same((idx.cpu(), val.cpu()), table_reference(d, dtype, metric, k))


# ---- 2. the CPU oracle per segment ---------------------------------------------------------------------------------------------------
def per_segment_oracle(X, xp, metric, k):
    idx = np.empty((X.shape[0], k), np.int64)
    val = np.empty((X.shape[0], k), np.float32)
    for a, b in zip(xp[:-1], xp[1:]):
        if b > a:
            i, v = oracle.simtopk(X[a:b], np.concatenate([X[:a], X[b:]]), metric=metric, k=k, exclude_self=False)
            idx[a:b], val[a:b] = np.where(i >= a, i + (b - a), i), v
    return idx, val


@pytest.mark.parametrize("metric", ["cosine", "neg_sq_l2"])
def test_against_the_oracle_per_segment(mmf, metric):
    xp = offsets([257, 6, 0, 129, 3, 40])
    X = gauss(xp[-1], 1100, 13)
    idx, val, st = mmf.simtopk_cross_segments_wide(X.cuda(), ptr=xp, metric=metric, k=5, return_stats=True)
    assert st["precision_used"] == 2 and st["fallback_rows"] <= crowded_rows(X, xp, metric, "fast", 5)
    ridx, rval = per_segment_oracle(X.numpy(), xp, metric, 5)
    assert np.array_equal(idx.cpu().numpy(), ridx)
    assert np.array_equal(val.cpu().numpy().view(np.int32), rval.view(np.int32))


# ---- 3. forced column runs: the hole inside a run and at a run's edge, list slots, the threshold union -----------------------------
@pytest.mark.parametrize("k,precision", [(5, "fast"), (20, "fast_bf16")])
def test_forced_column_runs_give_the_same_bits(mmf, k, precision):
    """n = 1100, one 400-row segment from row 128: the blocks inside it leave out tiles 1 .. 4 of 10, which lie inside a run (one and
    two runs) or end one (four runs of two tiles); segment 0 is tile 0, a hole at a run's front edge, and the last segment's hole runs
    to the end of Y.  More than one entry per block goes through the threshold union."""
    xp = offsets(WHOLE)
    X = gauss(xp[-1], 1100, 17)
    crowded = crowded_rows(X, xp, "cosine", precision, k)
    X = X.cuda()
    ref = mmf.simtopk_cross_segments(X, ptr=xp, metric="cosine", k=k)
    for splits in (1, 2, 4, 8):
        idx, val, st = mmf.simtopk_cross_segments_wide(X, ptr=xp, metric="cosine", k=k, col_splits=splits, precision=precision, return_stats=True)
        grid, entries = table_of(mmf, xp, None, 1100, k, splits)
        print(f"k {k} {precision} col_splits {splits}: scan_grid {st['scan_grid']} entries per block {st['col_splits']} "
              f"fallback_rows {st['fallback_rows']} (rows with a band beyond the lists: {crowded})")
        assert st["scan_grid"] == grid and st["col_splits"] == entries
        assert st["fallback_rows"] <= crowded and outside(idx.cpu(), xp, xp)
        assert_same((idx, val), ref)


# ---- 4. two-sided ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,precision", [("cosine", "fast"), ("rbf", "fast_bf16")])
def test_two_sided_same_bits_as_the_exact_entry(mmf, metric, precision):
    xs = [40, 0, 129, 5, 257, 1, 300, 32]               # segment 1: no queries
    ys = [300, 7, 33, 0, 128, 256, 4, 1000]             # segment 3: no rows of Y, nothing excluded for its 5 queries
    xp, yp = offsets(xs), offsets(ys)
    d = 1300
    X, Y = gauss(xp[-1], d, 1).cuda(), gauss(yp[-1], d, 2).cuda()
    Y[yp[0] + 3] = X[xp[0] + 3]                         # copies of a query: one inside its segment of Y, one outside
    Y[yp[5] + 9] = X[xp[0] + 3]
    kw = dict(metric=metric, lam=lam_for(d))
    for k in (5, 20):
        idx, val, st = mmf.simtopk_cross_segments_wide(X, Y, ptr=xp, y_ptr=yp, k=k, precision=precision, return_stats=True, **kw)
        assert (st["scan_grid"], st["col_splits"]) == table_of(mmf, xp, yp, d, k) and st["precision_used"] == PREC[precision]
        assert outside(idx.cpu(), xp, yp)
        assert_same((idx, val), mmf.simtopk_cross_segments(X, Y, ptr=xp, y_ptr=yp, k=k, **kw))
        assert idx[xp[0] + 3, 0] == yp[5] + 9
    got = mmf.simtopk_cross_segments_wide(X, Y, ptr=xp, y_ptr=yp, k=5, precision=precision, **kw)
    xb = torch.repeat_interleave(torch.arange(len(xs)), torch.tensor(xs))
    yb = torch.repeat_interleave(torch.arange(len(ys)), torch.tensor(ys))
    assert_same(mmf.simtopk_cross_segments_wide(X, Y, batch=xb, y_batch=yb, k=5, precision=precision, **kw), got)
    assert_same(mmf.cross_segments_wide.simtopk_cross_segments(X, Y, ptr=xp, y_ptr=yp, k=5, precision=precision, **kw), got)


# ---- 5. the mask under pressure ----------------------------------------------------------------------------------------------------------
def test_tight_clusters_per_segment_return_no_row_of_the_own_slide(mmf):
    """Each segment is one cluster (cosine about 0.9 inside, about 0 across), so every row's nearest rows are its own slide's: the
    plain wide call returns them, and a mask that let one column of a row's own segment through would return it here.  The noise is
    large enough that the rows stay on the 16-bit path (the band count bounds the flagged rows), so the mask is what is tested."""
    d = 1100
    rng = np.random.RandomState(5)
    sizes = [b - a for a, b in zip(OFFSETS[:-1], OFFSETS[1:])]
    centre = rng.randn(len(sizes), d).astype(np.float32)
    seg = np.repeat(np.arange(len(sizes)), sizes)
    Xh = torch.from_numpy(centre[seg] + 0.3 * rng.randn(OFFSETS[-1], d).astype(np.float32))
    X = Xh.cuda()
    for metric in ("neg_sq_l2", "cosine"):
        plain, _ = mmf.ops.simtopk(X, metric=metric, k=5, precision="fast")
        assert not outside(plain.cpu(), OFFSETS, OFFSETS)
        ref = mmf.simtopk_cross_segments(X, ptr=OFFSETS, metric=metric, k=5)
        crowded = crowded_rows(Xh, OFFSETS, metric, "fast", 5)
        for splits in (0, 2):
            idx, val, st = mmf.simtopk_cross_segments_wide(X, ptr=OFFSETS, metric=metric, k=5, col_splits=splits, return_stats=True)
            print(f"{metric} col_splits {splits}: fallback_rows {st['fallback_rows']} (rows with a band beyond the lists: {crowded})")
            assert st["fallback_rows"] <= crowded and crowded < OFFSETS[-1] // 4
            assert outside(idx.cpu(), OFFSETS, OFFSETS)
            assert_same((idx, val), ref)


def test_a_copy_in_the_own_segment_is_never_returned_and_a_copy_elsewhere_comes_first(mmf):
    """Segment s = its rows, an exact copy of them, and an exact copy of the rows of segment s + 1."""
    parts = [gauss(n, 1100, 20 + i) for i, n in enumerate([70, 130, 45])]
    S = len(parts)
    segs = [torch.cat([parts[s], parts[s], parts[(s + 1) % S]]) for s in range(S)]
    xp = offsets([t.shape[0] for t in segs])
    X = torch.cat(segs).cuda()
    idx, val = mmf.simtopk_cross_segments_wide(X, ptr=xp, metric="neg_sq_l2", k=5)
    assert outside(idx.cpu(), xp, xp)
    for s in range(S):
        n, prev = parts[s].shape[0], (s - 1) % S
        elsewhere = xp[prev] + 2 * parts[prev].shape[0] + torch.arange(n)           # the third part of segment s - 1
        assert torch.equal(idx[xp[s]:xp[s] + n, 0].cpu(), elsewhere), f"segment {s}: the copy in segment {prev} is not the first neighbour"
        assert (val[xp[s]:xp[s] + n, 0] == 0).all()
    assert_same((idx, val), mmf.simtopk_cross_segments(X, ptr=xp, metric="neg_sq_l2", k=5))


def test_ties_rank_by_ascending_global_id(mmf):
    """Fourteen identical rows spread over four segments: a row of them gets the identical rows of the OTHER segments, by id."""
    base = gauss(500, 1100, 6)
    xp = offsets([140, 200, 60, 100])
    same = [3, 77, 139, 141, 150, 151, 339, 340, 341, 399, 400, 401, 450, 499]
    base[same] = base[same[0]].clone()
    X = base.cuda()
    idx, val = mmf.simtopk_cross_segments_wide(X, ptr=xp, metric="neg_sq_l2", k=5)
    seg = np.searchsorted(np.asarray(xp), np.arange(500), side="right") - 1
    for i in same:
        assert idx[i].tolist() == [j for j in same if seg[j] != seg[i]][:5]
    assert_same((idx, val), mmf.simtopk_cross_segments(X, ptr=xp, metric="neg_sq_l2", k=5))


# ---- 6. flagged rows: the exact cross-segment rescan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_flagged_rows_take_the_exact_cross_scan_and_give_the_same_bits(mmf, precision):
    """400 exact copies of one vector, 100 in each of four segments.  A copy has 300 copies outside its segment, all tied at the best
    key and all inside any margin; its lists hold 2 x 16 per entry and there is no overflow list on this path, so every copy is flagged
    — rows of four segments — and the first five ids of the tie must come from the exact rescan."""
    xp = offsets([120, 100, 137, 300, 128, 135])
    Xh = gauss(xp[-1], 1100, 300)
    copies = np.concatenate([xp[s] + 7 + np.arange(100) for s in (0, 2, 3, 5)])
    Xh[copies] = Xh[copies[0]].clone()
    X = Xh.cuda()
    for metric in ("neg_sq_l2", "cosine"):
        idx, val, st = mmf.simtopk_cross_segments_wide(X, ptr=xp, metric=metric, k=5, col_splits=1, precision=precision, return_stats=True)
        print(f"{metric} {precision}: fallback_rows {st['fallback_rows']} overflow_rows {st['overflow_rows']} short_rows {st['short_rows']}")
        assert st["precision_used"] == PREC[precision] and st["fallback_rows"] >= 400
        assert outside(idx.cpu(), xp, xp)
        assert_same((idx, val), mmf.simtopk_cross_segments(X, ptr=xp, metric=metric, k=5))
        seg = np.searchsorted(np.asarray(xp), copies, side="right") - 1
        first = idx[torch.from_numpy(copies).cuda()].cpu().numpy()
        for i, s in zip(range(0, 400, 57), seg[::57]):
            assert first[i].tolist() == [int(j) for j in copies[seg != s][:5]]


# ---- 7. refusals and the router with device tensors -------------------------------------------------------------------------------------
def test_unserved_shapes_are_refused_under_fast_and_exact_under_auto(mmf):
    csw = mmf.cross_segments_wide
    sizes = [100, 60, 140]
    xp = offsets(sizes)
    L = mmf._lib.lib()
    P, stream = mmf.ops._p, mmf.ops._stream(torch.device("cuda", 0))
    p = torch.tensor(xp, dtype=torch.int64)

    def c_entry(X, d, k, opts, stats):
        idx = torch.zeros((xp[-1], k), dtype=torch.int64, device="cuda")
        val = torch.zeros((xp[-1], k), dtype=torch.float32, device="cuda")
        rc = L.mmf_simtopk_cross_segments_wide(P(X), xp[-1], None, 0, d, 0, 1, 1.0, k, P(p), None, len(sizes), P(idx), P(val),
                                               None if opts is None else ctypes.byref(opts), None if stats is None else ctypes.byref(stats), 0, stream)
        torch.cuda.synchronize()
        return rc, L.mmf_last_error().decode(), (idx, val)

    X600 = gauss(xp[-1], 600, 3).cuda()
    with pytest.raises(ValueError, match="does not serve d = 600, k = 5"):
        mmf.simtopk_cross_segments_wide(X600, ptr=xp, k=5)
    for d, k in ((4200, 5), (1100, 21)):
        X = gauss(xp[-1], d, 50 + k).cuda()
        for precision in ("fast", "fast_bf16"):
            with pytest.raises(ValueError, match=f"does not serve d = {d}, k = {k}"):
                mmf.simtopk_cross_segments_wide(X, ptr=xp, k=k, precision=precision)
            with pytest.raises(ValueError, match=f"does not serve d = {d}, k = {k}"):
                csw.simtopk_cross_segments(X, ptr=xp, k=k, precision=precision)
            rc, msg, _ = c_entry(X, d, k, mmf._lib.SimtopkOpts(PREC[precision], 0, 0, 1, None), None)
            assert rc == mmf._lib.MMF_E_UNSUPPORTED and f"d = {d}, k = {k}" in msg and "simtopk_cross_segments_wide" in msg
        ref = mmf.simtopk_cross_segments(X, ptr=xp, k=k)
        idx, val, st = csw.simtopk_cross_segments(X, ptr=xp, k=k, return_stats=True)                   # auto: the exact entry
        assert st["precision_used"] == 1
        assert_same((idx, val), ref)
        stats = mmf._lib.SimtopkStats()
        rc, _, got = c_entry(X, d, k, None, stats)                                                      # the C entry's AUTO: the exact driver
        assert rc == 0 and stats.precision_used == 1
        assert_same(got, ref)
    # the C entry's AUTO does not forward to the narrow scan (d = 600: the exact driver) and takes the wide scan where it serves
    stats = mmf._lib.SimtopkStats()
    rc, _, got = c_entry(X600, 600, 5, None, stats)
    assert rc == 0 and stats.precision_used == 1
    assert_same(got, mmf.simtopk_cross_segments(X600, ptr=xp, k=5))
    X = gauss(xp[-1], 1100, 4).cuda()
    ref = mmf.simtopk_cross_segments(X, ptr=xp, k=5)
    stats = mmf._lib.SimtopkStats()
    rc, _, got = c_entry(X, 1100, 5, None, stats)
    assert rc == 0 and stats.precision_used == 2
    assert_same(got, ref)
    # the router: narrow at d = 600, the measured decision at d = 1100 under "auto", the wide call under "fast", exact on request
    for precision, used in (("auto", 2), ("exact", 1), ("fast_bf16", 3)):
        idx, val, st = csw.simtopk_cross_segments(X600, ptr=xp, k=5, precision=precision, return_stats=True)
        assert st["precision_used"] == used
        assert_same((idx, val), mmf.simtopk_cross_segments(X600, ptr=xp, k=5))
    for precision, used in (("auto", 2 if csw.AUTO_TAKES_WIDE else 1), ("exact", 1), ("fast", 2), ("fast_bf16", 3)):
        idx, val, st = csw.simtopk_cross_segments(X, ptr=xp, k=5, precision=precision, return_stats=True)
        assert st["precision_used"] == used, precision
        assert_same((idx, val), ref)
    with pytest.raises(ValueError, match="does not serve d = 1100, k = 5"):
        mmf.cross_segments16.simtopk_cross_segments(X, ptr=xp, k=5, precision="fast")                  # the narrow module's router is unchanged


# ---- 8. stream contract ---------------------------------------------------------------------------------------------------------------
def test_stream_contract_behind_a_closed_gate(mmf):
    import streamgate
    xp = offsets([3, 150, 0, 260])

    def make_inputs(which):
        return [gauss(xp[-1], 1100, 31 if which == "truth" else 32)]

    def entry(X):
        return mmf.simtopk_cross_segments_wide(X, ptr=xp, metric="neg_sq_l2", k=5, col_splits=2)      # two runs: the threshold union too

    def reference(X):
        return list(per_segment_oracle(X, xp, "neg_sq_l2", 5))
    streamgate.run_gated(entry, make_inputs, reference, name="mmf_simtopk_cross_segments_wide", calls=2)


# ---- 9. edge builders -----------------------------------------------------------------------------------------------------------------
def test_edge_builders_under_auto_equal_their_default_precision(mmf):
    csw = mmf.cross_segments_wide
    xp = offsets([150, 40, 0, 129, 70])
    X = gauss(xp[-1], 1100, 41).cuda()
    ei, ew = mmf.cross_segment_knn_edges(X, ptr=xp, k=5)
    for got in (csw.cross_segment_knn_edges(X, ptr=xp, k=5, precision="auto"), csw.cross_segment_knn_edges(X, ptr=xp, k=5)):
        assert torch.equal(got[0], ei) and torch.equal(got[1].view(torch.int32), ew.view(torch.int32))
    gp, node_ptr = offsets([60, 45, 80]), offsets([100, 45, 90])
    out = dict(super_features=gauss(gp[-1], 1100, 42).cuda(), group_ptr=torch.tensor(gp), node_ptr=torch.tensor(node_ptr))
    ei, ew = mmf.cohort.link_slides(out, k=4)
    for got in (csw.link_slides(out, k=4, precision="auto"), csw.link_slides(out, 4)):
        assert torch.equal(got[0], ei) and torch.equal(got[1].view(torch.int32), ew.view(torch.int32))
