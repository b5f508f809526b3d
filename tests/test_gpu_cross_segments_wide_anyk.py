"""The wide 16-bit cross-segment top-k for any k (cross_segments_wide_anyk.*, include/ext/mmf_hg_cross_segw_anyk.h):
several passes of the masked table-driven wide 16-bit scan (1024 < d <= 4096), the later ones under per-row ceilings, each re-ranked
exactly.

The reference is always the exact ``cross_segments.simtopk_cross_segments`` on the same inputs (code this feature does not touch),
compared bit for bit, ids and values; one case compares against a Python loop of exact ``ops.simtopk`` calls and one against the
CPU oracle, segment by segment.  With f16 operands the test caps the rows that took the exact rescan at ceil(N / 64) per pass, so
that a pass cannot come from the rescan: tests/test_cross_segments_wide_anyk_cpu.py counts, on these same inputs and from the
reference alone, the already-emitted columns that slip under a row's ceiling and the rows whose margin band outgrows a list."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg  # noqa: E402
from test_gpu_segmented import assert_same  # noqa: E402
from test_fast_anyk_cpu import N, case_inputs, lam_for  # noqa: E402
from test_segmented_anyk_cpu import X_SIZES, Y_SIZES, offsets  # noqa: E402
from test_wide_anyk_cpu import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

# test_gpu_cross_segments_fast.py's cohort: bounds off a tile edge, a block spanning three segments, an empty and a one-row segment
SIZES = [3, 150, 0, 260, 400, 31, 1, 456, 700]
D, K = 1100, 21                # the smallest shape of several passes: padded dim 1152, one entry beyond a pass


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def exact(mmf, X, Y=None, **kw):
    return mmf.cross_segments.simtopk_cross_segments(X, Y, **kw)


def check_info(info, k, passes_at_least=2):
    assert info["passes"] >= passes_at_least, info
    assert sum(info["yield"]) == k, info
    assert all(y >= 1 for y in info["yield"]), info


def rows(seed, n, d):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, d).astype(np.float32)).cuda()


def outside(idx, xp, yp):
    """No id of a row lies in the row's own segment (or outside Y)."""
    idx = idx.cpu()
    xp, yp = [int(v) for v in xp], [int(v) for v in yp]
    for s in range(len(xp) - 1):
        own = idx[xp[s]:xp[s + 1]]
        if bool(((own >= yp[s]) & (own < yp[s + 1])).any()) or bool((own < 0).any()) or bool((own >= yp[-1]).any()):
            return False
    return True


_REF = {}


def deep_case(mmf, d, k, metric, dtype, two_sided):
    """The deep cohort of a case on the device, with the exact call's answer: computed once per case, never written."""
    key = (d, k, metric, dtype, two_sided)
    if key not in _REF:
        X, Y = case_inputs(d, dtype, two_sided)
        X = X.cuda()
        Y = None if Y is None else Y.cuda()
        kw = dict(ptr=offsets(X_SIZES), metric=metric, lam=lam_for(d), k=k)
        if two_sided:
            kw["y_ptr"] = offsets(Y_SIZES)
        _REF[key] = (X, Y, kw, exact(mmf, X, Y, **kw))
    return _REF[key]


# ---- 1. both kernels, X against itself and against Y ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("d,k,metric,dtype", CASES)
def test_same_bits_as_the_exact_call_on_every_kernel(mmf, d, k, metric, dtype, two_sided, precision):
    X, Y, kw, ref = deep_case(mmf, d, k, metric, dtype, two_sided)
    idx, val, st, info = mmf.simtopk_cross_segments_wide_any_k(X, Y, precision=precision, return_stats=True, return_info=True, **kw)
    print(f"d={d} k={k} {metric} {dtype} two_sided={two_sided} {precision}: {info}")
    assert_same((idx, val), ref)
    assert outside(idx, kw["ptr"], kw.get("y_ptr", kw["ptr"]))
    assert st["precision_used"] == {"fast": 2, "fast_bf16": 3}[precision]
    check_info(info, k)
    if precision == "fast":      # the 16-bit passes, not the rescan, produced the answer
        assert sum(info["exact_rows"]) <= info["passes"] * -(-N // 64), info


# ---- 2. forced column runs: several list pairs per row, the threshold union under ceilings ---------------------------------------------------
@pytest.mark.parametrize("d,k,metric", [(1100, 32, "cosine"), (1536, 64, "rbf")])
def test_forced_column_runs_give_the_same_bits(mmf, d, k, metric):
    X, _, kw, ref = deep_case(mmf, d, k, metric, "f32", False)
    for splits in (2, 8):
        idx, val, st, info = mmf.simtopk_cross_segments_wide_any_k(X, col_splits=splits, return_stats=True, return_info=True, **kw)
        table, lists = mmf.cross_segments_wide_table(kw["ptr"], d=d, k=20, col_splits=splits)      # the table of a pass: depth 20
        print(f"d={d} k={k} col_splits={splits}: entries per block {st['col_splits']}, grid {st['scan_grid']}, {info}")
        assert st["col_splits"] == lists // 2 >= splits and st["scan_grid"] == table.shape[0]
        assert_same((idx, val), ref)
        check_info(info, k)


# ---- 3. edge cohorts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[0, 1, 30, 22, 23, 129, 256, 257, 600, 0, 635], [300, 22, 1], [300, 21]])
def test_edge_cohorts(mmf, sizes):
    """The last two: outside the 300-row segment lie 23 and exactly k = 21 columns, so its rows have three or one unemitted columns
    left after the first pass: their lists come up short in the second and they take the rescan from their floors."""
    X = rows(23 + D + len(sizes), sum(sizes), D)
    ptr = offsets(sizes)
    kw = dict(ptr=ptr, metric="neg_sq_l2", k=K)
    idx, val, info = mmf.simtopk_cross_segments_wide_any_k(X, return_info=True, **kw)
    print(f"edge cohort {sizes} d={D} k={K}: {info}")
    assert_same((idx, val), exact(mmf, X, **kw))
    check_info(info, K)
    assert outside(idx, ptr, ptr)
    if sizes[0] == 300:
        assert sum(info["exact_rows"][1:]) >= 300, info


# ---- 4. near-duplicate rows ------------------------------------------------------------------------------------------------------------------
def test_tight_clusters_per_segment_return_no_row_of_the_own_slide(mmf):
    """Each segment is one tight cluster, so every row's nearest rows are its own slide's, and the next ones are whole foreign
    clusters of near-ties."""
    rng = np.random.RandomState(5)
    xp = offsets(SIZES)
    centre = rng.randn(len(SIZES), D).astype(np.float32)
    seg = np.repeat(np.arange(len(SIZES)), SIZES)
    X = torch.from_numpy(centre[seg] + 0.02 * rng.randn(int(xp[-1]), D).astype(np.float32)).cuda()
    for metric in ("neg_sq_l2", "cosine"):
        idx, val, info = mmf.simtopk_cross_segments_wide_any_k(X, ptr=xp, metric=metric, k=K, return_info=True)
        print(f"tight clusters d={D} k={K} {metric}: {info}")
        assert outside(idx, xp, xp)
        assert_same((idx, val), exact(mmf, X, ptr=xp, metric=metric, k=K))
        check_info(info, K)


def test_a_copy_in_the_own_segment_is_never_returned_and_a_copy_elsewhere_comes_first(mmf):
    """Segment s = its rows, an exact copy of them, and an exact copy of the rows of segment s + 1."""
    parts = [torch.from_numpy(np.random.RandomState(20 + i).randn(n, D).astype(np.float32)) for i, n in enumerate([70, 130, 45])]
    S = len(parts)
    segs = [torch.cat([parts[s], parts[s], parts[(s + 1) % S]]) for s in range(S)]
    xp = offsets([t.shape[0] for t in segs]).tolist()
    X = torch.cat(segs).cuda()
    idx, val, info = mmf.simtopk_cross_segments_wide_any_k(X, ptr=xp, metric="neg_sq_l2", k=K, return_info=True)
    assert outside(idx, xp, xp)
    for s in range(S):
        n, prev = parts[s].shape[0], (s - 1) % S
        elsewhere = xp[prev] + 2 * parts[prev].shape[0] + torch.arange(n)           # the third part of segment s - 1
        assert torch.equal(idx[xp[s]:xp[s] + n, 0].cpu(), elsewhere), f"segment {s}: the copy in segment {prev} is not the first neighbour"
        assert bool((val[xp[s]:xp[s] + n, 0] == 0).all())
    assert_same((idx, val), exact(mmf, X, ptr=xp, metric="neg_sq_l2", k=K))
    check_info(info, K)


def test_ties_rank_by_ascending_global_id_across_a_pass_boundary(mmf):
    """One foreign row duplicated 30 times over two other segments: the tie run leads every row of segment 0 and continues ascending
    across the boundary between the first pass (20 entries) and the second."""
    rs = np.random.RandomState(11)
    row = rs.randn(1, D).astype(np.float32)
    X = rs.randn(600, D).astype(np.float32)
    X[:200] = 3.0 * row + 0.05 * rs.randn(200, D).astype(np.float32)          # segment 0: near the repeated row
    copies = np.sort(rs.choice(np.arange(200, 600), 30, replace=False))
    assert copies[0] < 400 <= copies[-1]                                       # spread over both foreign segments
    X[copies] = row
    Xc = torch.from_numpy(X).cuda()
    kw = dict(ptr=[0, 200, 400, 600], metric="dot", k=32)
    idx, val, info = mmf.simtopk_cross_segments_wide_any_k(Xc, return_info=True, **kw)
    print(f"tie run: {info}")
    assert_same((idx, val), exact(mmf, Xc, **kw))
    check_info(info, 32)
    assert torch.equal(idx[:200, :30].cpu(), torch.from_numpy(copies).expand(200, 30)), "the tie run is not in ascending id order"


# ---- independent references: a loop of exact calls, a slide's rows against the rest; the CPU oracle per segment ---------------------------------
def test_against_a_loop_of_exact_calls(mmf):
    X, _, kw, _ = deep_case(mmf, 1100, 32, "cosine", "f32", False)
    idx, val, info = mmf.simtopk_cross_segments_wide_any_k(X, return_info=True, **kw)
    check_info(info, 32)
    xo = offsets(X_SIZES).tolist()
    for a, b in zip(xo[:-1], xo[1:]):
        ri, rv = mmf.ops.simtopk(X[a:b], torch.cat([X[:a], X[b:]]), metric="cosine", k=32, exclude_self=False, precision="exact")
        ri = torch.where(ri >= a, ri + (b - a), ri)
        assert_same((idx[a:b], val[a:b]), (ri, rv))


def per_segment_oracle(X, o, metric, k):
    idx = np.empty((X.shape[0], k), np.int64)
    val = np.empty((X.shape[0], k), np.float32)
    for a, b in zip(o[:-1], o[1:]):
        if b > a:
            i, v = oracle.simtopk(X[a:b], np.concatenate([X[:a], X[b:]]), metric=metric, k=k, exclude_self=False)
            idx[a:b], val[a:b] = np.where(i >= a, i + (b - a), i), v
    return idx, val


@pytest.mark.parametrize("metric", ["cosine", "neg_sq_l2"])
def test_against_the_oracle(mmf, metric):
    sizes = [120, 70, 110]
    X = np.random.RandomState(7).randn(sum(sizes), D).astype(np.float32)
    idx, val, info = mmf.simtopk_cross_segments_wide_any_k(torch.from_numpy(X).cuda(), ptr=offsets(sizes), metric=metric, k=30, return_info=True)
    check_info(info, 30)
    ridx, rval = per_segment_oracle(X, offsets(sizes).tolist(), metric, 30)
    assert np.array_equal(idx.cpu().numpy(), ridx), "indices differ"
    assert np.array_equal(val.cpu().numpy().view(np.int32), rval.view(np.int32))


# ---- 5. special paths ------------------------------------------------------------------------------------------------------------------------------
def test_the_exact_precision_is_the_exact_call(mmf):
    X, Y, kw, ref = deep_case(mmf, 1536, 32, "neg_sq_l2", "f16", True)
    idx, val, st, info = mmf.simtopk_cross_segments_wide_any_k(X, Y, precision="exact", return_stats=True, return_info=True, **kw)
    assert_same((idx, val), ref)
    assert st["precision_used"] == 1 and info["passes"] == 1 and info["yield"] == [32]


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_one_pass_is_the_wide_call(mmf, precision):
    X, _ = case_inputs(1100, "f32", False)
    X = X.cuda()
    kw = dict(ptr=offsets(X_SIZES), metric="cosine", k=20)
    idx, val, st, info = mmf.simtopk_cross_segments_wide_any_k(X, precision=precision, return_stats=True, return_info=True, **kw)
    ridx, rval, rst = mmf.simtopk_cross_segments_wide(X, precision=precision, return_stats=True, **kw)
    assert_same((idx, val), (ridx, rval))
    assert info["passes"] == 1 and info["yield"] == [20]
    assert (st["precision_used"], st["scan_grid"], st["col_splits"]) == (rst["precision_used"], rst["scan_grid"], rst["col_splits"])


def test_refusals_and_the_router(mmf):
    cw = mmf.cross_segments_wide_anyk
    xp = offsets([100, 60, 140])
    for precision in ("fast", "fast_bf16", "exact"):
        with pytest.raises(ValueError, match="d = 600 is not above 1024.*mmf_simtopk_cross_segments_fast_anyk"):
            mmf.simtopk_cross_segments_wide_any_k(rows(52, 300, 600), ptr=xp, k=K, precision=precision)
    for precision in ("fast", "fast_bf16"):
        with pytest.raises(ValueError, match="d = 5000 is beyond the wide 16-bit scan"):
            mmf.simtopk_cross_segments_wide_any_k(rows(53, 300, 5000), ptr=xp, k=K, precision=precision)
    X = rows(51, 300, D)
    L = mmf._lib.lib()
    idx = torch.empty((300, K), dtype=torch.int64, device="cuda")
    val = torch.empty((300, K), dtype=torch.float32, device="cuda")
    opts = mmf._lib.SimtopkOpts(2, 0, 0, 0, None)
    args = (300, None, 0, 600, 0, 1, 1.0, K, xp.data_ptr(), None, 3, idx.data_ptr(), val.data_ptr(), ctypes.byref(opts), None, 0, None, None)
    rc = L.mmf_simtopk_cross_segments_wide_anyk(X.data_ptr(), *args)                      # the entry itself at d = 600 ...
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and b"mmf_simtopk_cross_segments_fast_anyk" in L.mmf_last_error()
    args = args[:3] + (5000,) + args[4:]
    rc = L.mmf_simtopk_cross_segments_wide_anyk(X.data_ptr(), *args)                      # ... and at d = 5000 under FAST
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and b"d = 5000 is beyond the wide 16-bit scan" in L.mmf_last_error()
    # the old entry still refuses what this one serves
    with pytest.raises(ValueError, match="d = 1100, k = 21"):
        mmf.simtopk_cross_segments_fast_any_k(X, ptr=xp, k=K)
    args = args[:3] + (D,) + args[4:]
    rc = L.mmf_simtopk_cross_segments_fast_anyk(X.data_ptr(), *args)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and b"d = 1100, k = 21" in L.mmf_last_error()
    # the router above 1024 beyond one pass, under each precision and for whatever table was committed (may be empty)
    ref = exact(mmf, X, ptr=xp, k=K)
    for precision, used in (("fast", 2), ("fast_bf16", 3), ("exact", 1), ("auto", 2 if cw._auto_takes(300, D, K) else 1)):
        idx, val, st = cw.simtopk_cross_segments(X, ptr=xp, k=K, precision=precision, return_stats=True)
        assert_same((idx, val), ref)
        assert st["precision_used"] == used, precision
    for dl, dh, kl, kh, nl in cw._AUTO_SHAPES:
        assert cw._auto_takes(nl, dl, kl) and not cw._auto_takes(nl - 1, dl, kl) and not cw._auto_takes(nl, dl, 20)
    # ... where one pass serves, and at d <= 1024: the narrow module's router
    for Xr, k in ((X, 20), (rows(54, 300, 600), K)):
        idx, val, st = cw.simtopk_cross_segments(Xr, ptr=xp, k=k, precision="fast", return_stats=True)
        assert st["precision_used"] == 2
        assert_same((idx, val), mmf.cross_segments_anyk.simtopk_cross_segments(Xr, ptr=xp, k=k, precision="fast"))
        assert_same((idx, val), exact(mmf, Xr, ptr=xp, k=k))


# ---- 6. a busy non-default stream -------------------------------------------------------------------------------------------------------------------
GATED_SIZES = [3, 150, 0, 260]


def test_stream_contract_behind_a_closed_gate(mmf):
    xp = offsets(GATED_SIZES).tolist()

    def make_inputs(which):
        return [torch.from_numpy(np.random.RandomState(31 if which == "truth" else 32).randn(xp[-1], D).astype(np.float32))]

    def entry(X):
        return list(mmf.simtopk_cross_segments_wide_any_k(X, ptr=xp, metric="neg_sq_l2", k=K, col_splits=2))

    def reference(X):
        return list(per_segment_oracle(X, xp, "neg_sq_l2", K))
    sg.run_gated(entry, make_inputs, reference, name="mmf_simtopk_cross_segments_wide_anyk", calls=2)


# ---- 7. edge builders ---------------------------------------------------------------------------------------------------------------------------------
def test_edge_builders_under_auto_equal_their_default_precision(mmf):
    cw = mmf.cross_segments_wide_anyk
    xp = offsets([150, 40, 0, 129, 70])
    X = rows(41, int(xp[-1]), D)
    ei, ew = mmf.cross_segment_knn_edges(X, ptr=xp, k=K)
    for got in (cw.cross_segment_knn_edges(X, ptr=xp, k=K, precision="auto"), cw.cross_segment_knn_edges(X, ptr=xp, k=K)):
        assert torch.equal(got[0], ei) and torch.equal(got[1].view(torch.int32), ew.view(torch.int32))
    from test_gpu_kmeans_ragged import _clustered
    sizes, tmas, C, d = [60, 90, 75], [16, 24, 5], 24, 32
    wp, tp = offsets(sizes), offsets(tmas)
    F = torch.from_numpy(np.concatenate([_clustered(n, d, 900 + s) for s, n in enumerate(sizes)])).cuda()
    P = torch.from_numpy(np.concatenate([np.random.RandomState(950 + s).rand(n, 2).astype(np.float32) for s, n in enumerate(sizes)])).cuda()
    tma = torch.from_numpy(np.concatenate([_clustered(m, d, 980 + s) for s, m in enumerate(tmas)])).cuda()
    out = mmf.build_cohort_hypergraphs(F, P, tma, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=3, hypergraph_k=3, num_hyperedges=4)
    ei, ew = mmf.cohort.link_slides(out, k=45)                    # 2 x 24 super patches outside every slide
    for got in (cw.link_slides(out, k=45, precision="auto"), cw.link_slides(out, 45)):
        assert torch.equal(got[0], ei) and torch.equal(got[1].view(torch.int32), ew.view(torch.int32))
