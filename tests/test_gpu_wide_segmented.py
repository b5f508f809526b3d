"""The segmented wide 16-bit scan (wide_scan.simtopk_segmented, mmf_simtopk_segmented_wide): the k-NN of every
segment of a ragged batch at feature dims 1025 .. 4096 in one call.

The reference everywhere is the loop the call replaces — one ops.simtopk(..., precision="exact", row_offset, col_offset) per
segment, short segments padded with -1 / -inf: indices equal, values bitwise equal.  Rows are the planted clusters of
tests/test_gpu_wide_scan.py.  The band of a row — the columns OF ITS OWN SEGMENT whose 16-bit value G lies within the row's margin
of the segment's (k + self)-th best G — is restated here from oracle/scan16_restate and the margin formula in the header of
mmf_scan_b16w.hip; scale and maxima are those of the call (all rows for the scale, the rows in the operand image for the maxima).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import scan16_restate as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_segmented import assert_same, offsets, per_segment  # noqa: E402
from test_gpu_wide_scan import LAM, PRECISION_USED, planted, planted_rows  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [33, 0, 1, 257, 5, 6, 128, 31, 129, 32, 98]     # 720 rows: empty, one row, fewer than k columns, tile edges, two row blocks
USED = dict(PRECISION_USED, auto=2)                      # auto takes the f16 wide scan
AUTO_SPLITS = False                                      # the automatic column-splits rule is off ("Decisions")


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


# ---- restatements: which segments the scan serves, its work table's size, the bands ------------------------------------------
def served(xs, ys, k, exclude_self):
    """Segments the 16-bit scan serves (rows present, at least k admissible columns); self calls: ys is xs."""
    return [s for s, (n, m) in enumerate(zip(xs, ys)) if n > 0 and m - (1 if exclude_self else 0) >= k]


def schedule(xs, ys, k, exclude_self, forced=0):
    """(scan_grid, col_splits) of the call: the splits rule of DESIGN.md §4.16 restated."""
    kk = k + (1 if exclude_self else 0)
    cap = 16 if kk <= 11 else 32
    seg = served(xs, ys, k, exclude_self)
    R_blocks = sum((xs[s] + 127) // 128 for s in seg)
    fits = lambda sp: 2 * sp * cap <= 1024 - 192        # noqa: E731  select's capacity per row minus the overflow slots
    call = 1
    if forced > 0:
        while call < forced and fits(2 * call):
            call *= 2
    elif AUTO_SPLITS:
        while R_blocks > 0 and R_blocks * call < 256 and fits(2 * call):
            call *= 2
    grid, smax = 0, 1
    for s in seg:
        tiles, sp = (ys[s] + 127) // 128, 1
        while 2 * sp <= call and 2 * sp <= tiles:
            sp *= 2
        grid += (xs[s] + 127) // 128 * sp
        smax = max(smax, sp)
    return grid, smax


def segment_bands(X, xp, metric, operand, k):
    """Per row of a self call: the number of columns j of the row's segment with G_ij >= (kk-th best G_i. of the segment) - margin_i
    (self included), 0 for rows of segments the scan does not serve."""
    f = np.float32
    kk = k + 1
    X = np.ascontiguousarray(X.float().numpy(), f)
    d = X.shape[1]
    dp = (d + 127) // 128 * 128
    scal = R.row_scalars(X, metric)
    scale = R.common_scale(float(R.sq_norms(X).max()), metric)
    u = ((X / scal[:, None]).astype(f) if metric == R.COSINE else X) * scale
    u = u.astype(f)
    z = u.astype(np.float16).astype(f) if operand == "f16" else R.bf16_to_f32(R.round_bf16(u))
    z64, u64 = z.astype(np.float64), u.astype(np.float64)
    norm = lambda v: np.sqrt((v * v).sum(axis=1).astype(f)) * R.UP   # noqa: E731
    zn, rn, un = norm(z64), norm((z - u).astype(np.float64)), norm(u64)
    cb = (f(-0.5) * scal * scale * scale).astype(f) if metric in (R.NEG_SQ_L2, R.RBF) else np.zeros(X.shape[0], f)
    sizes = [b - a for a, b in zip(xp[:-1], xp[1:])]
    seg = served(sizes, sizes, k, True)
    img = np.concatenate([np.arange(xp[s], xp[s + 1]) for s in seg])          # the rows in the operand image
    ZB, RB, UB, CB = zn[img].max(), rn[img].max(), un[img].max(), np.abs(cb[img]).max()
    g_acc, g_chain = f(dp + 8) * R.EPS24, f(d + 2) * R.EPS24
    e1 = rn * ZB + un * RB + g_acc * (zn * ZB + CB)
    if metric == R.DOT:
        e2 = g_chain * un * UB
    elif metric == R.COSINE:
        e2 = (g_chain + f(4.7683716e-7)) * un * UB * f(1.01)
    else:
        e2 = g_chain * un * UB + f(2.3841858e-7) * (un * un + UB * UB)
    margin = (f(2.0) * (e1 + e2) * f(1.001) + f(1e-30)).astype(np.float64)
    band = np.zeros(X.shape[0], np.int64)
    for s in seg:
        a, b = xp[s], xp[s + 1]
        G = cb[a:b].astype(np.float64)[None, :] + z64[a:b] @ z64[a:b].T
        t = -np.partition(-G, kk - 1, axis=1)[:, kk - 1]
        band[a:b] = (G >= (t - margin[a:b])[:, None]).sum(axis=1)
    return band


@functools.lru_cache(maxsize=None)
def loop_reference(d, dtype, metric, k):
    """The per-segment exact loop over planted(d) cut into SIZES, computed once per shape and left on the host."""
    import multimodal_fusion_amd as m
    X = planted(d, dtype).cuda()
    xp = offsets(SIZES)
    idx, val = per_segment(m, X, None, xp, xp, k, True, metric=metric, lam=LAM, precision="exact")
    return idx.cpu(), val.cpu()


@functools.lru_cache(maxsize=None)
def self_call(d, dtype, metric, k, precision, col_splits=0):
    import multimodal_fusion_amd as m
    X = planted(d, dtype).cuda()
    idx, val, st = m.wide_scan.simtopk_segmented(X, ptr=offsets(SIZES), metric=metric, lam=LAM, k=k, precision=precision,
                                                 col_splits=col_splits, return_stats=True)
    torch.cuda.synchronize()
    return idx.cpu(), val.cpu(), st


def check_self(d, dtype, metric, k, precision):
    idx, val, st = self_call(d, dtype, metric, k, precision)
    grid, smax = schedule(SIZES, SIZES, k, True)
    print(f"d {d} {dtype} {metric} k {k} {precision}: fallback_rows {st['fallback_rows']} col_splits {st['col_splits']} "
          f"scan_grid {st['scan_grid']} (expected {grid}, {smax}) candidates {st['candidates']}")
    assert st["precision_used"] == USED[precision]
    assert st["scan_grid"] == grid and st["col_splits"] == smax
    assert st["near_rows"] == -1
    assert_same((idx, val), loop_reference(d, dtype, metric, k))


# ---- 1. self, ragged -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16", "auto"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
@pytest.mark.parametrize("d", [1100, 1536])
def test_self_ragged_same_bits_as_the_loop(mmf, d, metric, k, precision):
    check_self(d, "f32", metric, k, precision)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16", "auto"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_self_ragged_16_bit_rows(mmf, dtype, k, precision):
    check_self(1100, dtype, "cosine", k, precision)


# ---- 2. capacity condition ---------------------------------------------------------------------------------------------------
def check_capacity(mmf, d, dtype, metric, k, precision, col_splits=0, sizes=SIZES, call=None):
    st = (call or self_call(d, dtype, metric, k, precision, col_splits))[2]
    band = segment_bands(planted(d, dtype), offsets(sizes), metric, "f16" if precision == "fast" else "bf16", k)
    cap = mmf.wide_scan.list_capacity(k, True)
    crowded = int((band > cap).sum())
    print(f"d {d} {dtype} {metric} k {k} {precision} col_splits {col_splits}: largest band {int(band.max())} of capacity {cap}, rows beyond it "
          f"{crowded}, fallback_rows {st['fallback_rows']}")
    assert st["fallback_rows"] <= crowded
    if precision == "fast":
        assert st["fallback_rows"] == 0


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
@pytest.mark.parametrize("d", [1100, 1536])
def test_capacity_condition_inside_the_segments(mmf, d, metric, k, precision):
    check_capacity(mmf, d, "f32", metric, k, precision)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_capacity_condition_16_bit_rows(mmf, dtype, precision):
    for k in (5, 15):
        check_capacity(mmf, 1100, dtype, "cosine", k, precision)


# ---- 3. cross ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16", "auto"])
@pytest.mark.parametrize("metric", ["neg_sq_l2", "cosine"])
def test_cross_same_bits_as_the_loop(mmf, metric, precision):
    xs = [40, 0, 129, 5, 257, 1, 130]                   # segment 1: no queries; segment 3: no candidates; segment 6: 4 columns < k
    ys = [300, 7, 33, 0, 128, 256, 4]
    xp, yp = offsets(xs), offsets(ys)
    pool = planted_rows(60, 24, 1100, seed=77)          # X and Y draw from the same clusters
    perm = np.random.default_rng(3).permutation(pool.shape[0])
    X = torch.from_numpy(pool[perm[:xp[-1]]]).cuda()
    Y = torch.from_numpy(pool[perm[xp[-1]:xp[-1] + yp[-1]]]).cuda()
    kw = dict(metric=metric, lam=LAM, k=5)
    idx, val, st = mmf.wide_scan.simtopk_segmented(X, Y, ptr=xp, y_ptr=yp, precision=precision, return_stats=True, **kw)
    grid, smax = schedule(xs, ys, 5, False)
    print(f"cross {metric} {precision}: fallback_rows {st['fallback_rows']} col_splits {st['col_splits']} scan_grid {st['scan_grid']}")
    assert st["precision_used"] == USED[precision] and st["scan_grid"] == grid and st["col_splits"] == smax
    assert_same((idx, val), per_segment(mmf, X, Y, xp, yp, exclude_self=False, precision="exact", **kw))
    assert (idx[xp[3]:xp[4]] == -1).all() and (idx[xp[6]:, 4:] == -1).all() and (idx[xp[6]:, :4] >= yp[6]).all()


# ---- 4. against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["rbf", "neg_sq_l2"])
def test_against_the_oracle_per_segment(mmf, metric):
    sizes = [257, 6, 0, 129, 3]
    xp = offsets(sizes)
    X = planted(1100)[:xp[-1]].clone()
    idx, val = mmf.wide_scan.simtopk_segmented(X.cuda(), ptr=xp, metric=metric, lam=LAM, k=5, precision="fast")
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for a, b in zip(xp[:-1], xp[1:]):
        ks = min(5, b - a - 1)
        if b == a:
            continue
        assert (idx[a:b, ks:] == -1).all() and np.isneginf(val[a:b, ks:]).all()
        if ks == 0:
            continue
        ridx, rval = oracle.simtopk(X[a:b].numpy(), X[a:b].numpy(), metric=metric, lam=LAM, k=ks, exclude_self=True, row_offset=a, col_offset=a)
        assert np.array_equal(idx[a:b, :ks], ridx), f"segment at {a}: indices differ"
        if metric == "rbf":
            assert np.allclose(val[a:b, :ks], rval, rtol=0, atol=1e-5)
        else:
            assert np.array_equal(val[a:b, :ks].view(np.int32), rval.view(np.int32))


# ---- 5. no neighbour crosses a segment -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "exact"])
def test_no_neighbour_crosses_a_segment(mmf, precision):
    """Exact copies of the middle segment's rows sit in the segment before it and in the segment after it: a scan that looked
    one tile too far, or an id offset of the wrong segment, would return them (a copy scores like the row itself)."""
    base = planted(1100)
    mid = base[200:340]
    X = torch.cat([base[:10], mid, mid, base[400:410], mid]).cuda()        # segments of 150, 150, 140 rows
    xp = offsets([150, 150, 140])
    idx, val, st = mmf.wide_scan.simtopk_segmented(X, ptr=xp, metric="cosine", k=5, precision=precision, return_stats=True)
    assert st["precision_used"] == (2 if precision == "fast" else 1)
    idx = idx.cpu()
    for s in range(3):
        own = idx[xp[s]:xp[s + 1]]
        assert ((own >= xp[s]) & (own < xp[s + 1])).all(), f"segment {s}: a neighbour from another segment"
    assert_same((idx, val.cpu()), [t.cpu() for t in per_segment(mmf, X, None, xp, xp, 5, True, metric="cosine", precision="exact")])


# ---- 6. padding cannot win -------------------------------------------------------------------------------------------------------
def test_padding_cannot_win(mmf):
    """Metric dot, a segment of 129 rows e_i - 0.001 * 1: every off-diagonal dot is -2 c + c^2 d = -0.0009 < 0, and a zero
    padding column (the segment's second tile holds 127 of them) would score 0."""
    d, c = 1100, 0.001
    E = torch.full((129, d), -c)
    E[torch.arange(129), torch.arange(129)] += 1.0
    base = planted(d)
    X = torch.cat([base[:100], E, base[300:400]]).cuda()
    xp = offsets([100, 129, 100])
    got = mmf.wide_scan.simtopk_segmented(X, ptr=xp, metric="dot", k=5, precision="fast", return_stats=True)
    print(f"padding: fallback_rows {got[2]['fallback_rows']}")
    assert got[2]["precision_used"] == 2
    assert (got[1][100:229] < 0).all() and (got[0][100:229] >= 100).all() and (got[0][100:229] < 229).all()
    assert_same(got[:2], per_segment(mmf, X, None, xp, xp, 5, True, metric="dot", precision="exact"))


# ---- 7. flagged rows inside one segment --------------------------------------------------------------------------------------------
def test_flagged_rows_stay_inside_their_segment(mmf):
    base = planted(1100)
    rng = np.random.default_rng(9)
    # 40 near-identical rows at the head of their segment: one column tile, 20 per list of capacity 16, all inside each other's band
    cluster = base[500] + 1e-4 * torch.from_numpy(rng.standard_normal((40, 1100)).astype(np.float32))
    segs = [base[:192], torch.cat([cluster, base[240:360]]), base[528:720]]
    kw = dict(metric="cosine", k=5, precision="fast", return_stats=True)
    X = torch.cat(segs).cuda()
    xp = offsets([192, 160, 192])
    got = mmf.wide_scan.simtopk_segmented(X, ptr=xp, **kw)
    print(f"flagged: fallback_rows {got[2]['fallback_rows']}")
    assert 0 < got[2]["fallback_rows"] <= 160
    assert_same(got[:2], per_segment(mmf, X, None, xp, xp, 5, True, metric="cosine", precision="exact"))
    # the same call without that segment flags nothing: every flagged row above belongs to it
    rest = mmf.wide_scan.simtopk_segmented(torch.cat([segs[0], segs[2]]).cuda(), ptr=offsets([192, 192]), **kw)
    assert rest[2]["fallback_rows"] == 0
    assert torch.equal(rest[0][:192], got[0][:192]) and torch.equal(rest[0][192:], got[0][352:] - 160)


# ---- 8. column splits ------------------------------------------------------------------------------------------------------------
SPLIT_SIZES = [100, 400, 220]                            # one tile (fewer tiles than splits), four tiles, two tiles


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 15])
def test_column_splits_give_the_same_bits(mmf, k, precision):
    X = planted(1536).cuda()
    xp = offsets(SPLIT_SIZES)
    ref = per_segment(mmf, X, None, xp, xp, k, True, metric="cosine", precision="exact")
    for splits in (1, 2, 4):
        got = mmf.wide_scan.simtopk_segmented(X, ptr=xp, metric="cosine", k=k, precision=precision, col_splits=splits, return_stats=True)
        torch.cuda.synchronize()
        grid, smax = schedule(SPLIT_SIZES, SPLIT_SIZES, k, True, forced=splits)
        assert smax == splits and got[2]["col_splits"] == splits and got[2]["scan_grid"] == grid
        assert_same(got[:2], ref)
        check_capacity(mmf, 1536, "f32", "cosine", k, precision, splits, SPLIT_SIZES, call=got)
    auto = mmf.wide_scan.simtopk_segmented(X, ptr=xp, metric="cosine", k=k, precision=precision, return_stats=True)
    assert (auto[2]["scan_grid"], auto[2]["col_splits"]) == schedule(SPLIT_SIZES, SPLIT_SIZES, k, True)
    assert_same(auto[:2], ref)


# ---- 9. outside the wide range the call is the existing one ------------------------------------------------------------------------
def test_outside_the_wide_range_the_call_is_the_existing_one(mmf):
    xp = offsets([300, 0, 5, 129, 40])
    X = torch.from_numpy(planted_rows(20, 24, 512, seed=4)[:xp[-1]]).cuda()
    a = mmf.wide_scan.simtopk_segmented(X, ptr=xp, metric="cosine", k=5, precision="auto", return_stats=True)
    b = mmf.ops.simtopk_segmented(X, ptr=xp, metric="cosine", k=5, precision="auto", return_stats=True)
    assert_same(a[:2], b[:2])
    assert sorted(a[2]) == sorted(b[2])
    for key in ("precision_used", "col_splits", "scan_grid", "fallback_rows", "overflow_rows", "short_rows", "candidates", "near_rows"):
        assert a[2][key] == b[2][key], key
    assert a[2]["precision_used"] == 2
    with pytest.raises(RuntimeError, match="not supported"):
        mmf.wide_scan.simtopk_segmented(X, ptr=xp, k=5, col_splits=2)
    # k + self = 21 at d = 1536: auto is the exact pass
    xq = offsets([360, 360])
    Xw = planted(1536).cuda()
    got = mmf.wide_scan.simtopk_segmented(Xw, ptr=xq, metric="cosine", k=20, precision="auto", return_stats=True)
    assert got[2]["precision_used"] == 1
    assert_same(got[:2], per_segment(mmf, Xw, None, xq, xq, 20, True, metric="cosine", precision="exact"))
    with pytest.raises(RuntimeError, match="does not support"):
        mmf.wide_scan.simtopk_segmented(Xw, ptr=xq, metric="cosine", k=20, precision="fast")
    with pytest.raises(RuntimeError, match="does not support"):               # the existing entry keeps its refusal
        mmf.ops.simtopk_segmented(Xw, ptr=xq, metric="cosine", k=5, precision="fast")
    auto = mmf.ops.simtopk_segmented(Xw, ptr=xq, metric="cosine", k=5, precision="auto", return_stats=True)
    assert auto[2]["precision_used"] == 1                                      # ... and its AUTO -> exact above d = 1024


# ---- 10. stream contract -----------------------------------------------------------------------------------------------------------
def test_stream_contract_behind_a_closed_gate(mmf):
    """tests/streamgate.py: the call on a busy non-default stream, its inputs produced behind a closed gate; three segments, one
    short of columns, one with a flagged cluster."""
    import streamgate
    sizes = [3, 150, 120]
    xp = offsets(sizes)

    def make_inputs(which):
        seed = 31 if which == "truth" else 32
        X = planted_rows(12, 24, 1100, seed=seed)[:xp[-1]].copy()
        rng = np.random.default_rng(seed)
        X[60:100] = X[60] + 1e-4 * rng.standard_normal((40, 1100)).astype(np.float32)
        return [torch.from_numpy(X)]

    def entry(X):
        idx, val, st = mmf.wide_scan.simtopk_segmented(X, ptr=xp, metric="neg_sq_l2", k=5, precision="fast", return_stats=True)
        assert st["precision_used"] == 2 and st["fallback_rows"] > 0, st
        return idx, val

    def reference(X):
        idx = np.full((X.shape[0], 5), -1, np.int64)
        val = np.full((X.shape[0], 5), -np.inf, np.float32)
        for a, b in zip(xp[:-1], xp[1:]):
            ks = min(5, b - a - 1)
            i, v = oracle.simtopk(X[a:b], X[a:b], metric="neg_sq_l2", k=ks, exclude_self=True, row_offset=a, col_offset=a)
            idx[a:b, :ks], val[a:b, :ks] = i, v
        return [idx, val]

    streamgate.run_gated(entry, make_inputs, reference, name="wide_scan.simtopk_segmented")


# ---- 11. cohort routing ------------------------------------------------------------------------------------------------------------
def test_the_cohort_builder_takes_the_wide_entry_above_1024(mmf, monkeypatch):
    """build_hypergraph_knn_kmeans_segmented at D = 1100: the per-slide mirror's edges and weights, with the neighbours from
    wide_scan.simtopk_segmented (a spy sees the call); at D = 512 the neighbours still come from ops.simtopk_segmented."""
    from importlib import import_module
    from test_gpu_knn_kmeans_segmented import plain_loop
    kk = import_module("multimodal_fusion_amd.knn_kmeans_hypergraph")
    bh = import_module("multimodal_fusion_amd.build_hypergraph")
    calls = []
    wide, narrow = mmf.wide_scan.simtopk_segmented, mmf.ops.simtopk_segmented

    def spy_wide(*a, **kw):
        calls.append(("wide", a[0].shape[1]))
        return wide(*a, **kw)

    def spy_narrow(*a, **kw):
        calls.append(("ops", a[0].shape[1]))
        return narrow(*a, **kw)
    monkeypatch.setattr(mmf.wide_scan, "simtopk_segmented", spy_wide)
    monkeypatch.setattr(mmf.ops, "simtopk_segmented", spy_narrow)
    wp, tp = offsets([120, 64, 200]), offsets([10, 0, 30])
    node_ptr = offsets([130, 64, 230])
    for d, who in ((1100, "wide"), (512, "ops")):
        g = torch.Generator().manual_seed(d)
        W, Tm = torch.randn(wp[-1], d, generator=g).cuda(), torch.randn(tp[-1], d, generator=g).cuda()
        del calls[:]
        ei, ew, eptr, stats = kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, 5, 6, wsi_ptr=wp, tma_ptr=tp)
        assert calls == [(who, d)], calls
        ref = plain_loop(bh, W, Tm, wp, tp, 5, 6)
        assert stats["node_ptr"] == node_ptr and eptr.tolist() == offsets([r[0].shape[1] for r in ref])
        assert torch.equal(ei, torch.cat([r[0] + node_ptr[s] for s, r in enumerate(ref)], dim=1))
        assert torch.equal(ew.view(torch.int32), torch.cat([r[1] for r in ref]).view(torch.int32))
