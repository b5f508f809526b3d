"""Segmented WSI x TMA similarity, grouping and median edge filter on the GPU.

  * bit identity: every block of S_flat and every row of the [S, 5] statistics against the UNCHANGED plain entry
    (mmf_sim_dense_stats through ops.sim_dense_stats, and called directly for the five raw doubles) on the slide's rows;
  * the flat ragged median against ops.lower_median and torch.median, slice by slice;
  * the reference's own outputs (tests/golden/g8_pipeline.npz) with the tolerances tests/test_gpu_pipeline.py applies to the
    plain mirror on the same arrays;
  * the grouping and the whole cohort chain against the per-slide chain of the plain mirrors;
  * the stream contract of both C entries and of every public function of the module, behind a closed gate
    (tests/streamgate.py).

Every comparison covers every slide of its cohort.
"""
import ctypes
import inspect
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5                   # tests/test_gpu_pipeline.py: matrices that go through expf

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md §7 "Cohort entries"
# (tests/test_wsi_tma_segmented_cpu.py keeps the two equal, and checks that these are the entries of _lib.EXPORTS_COHORT)
CALL = "until the call returns"
SYNC_COHORT = {
    "mmf_sim_dense_stats_segmented": ("none", CALL),
    "mmf_lower_median_segmented": ("none", CALL),
}

T = torch.from_numpy
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def wt():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.wsi_tma_similarity")


def pp():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.build_hypergraph.preprocess_hypergraph")


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def rows(n, d, seed):
    """randn rows scaled so that squared distances are about 1: the similarities spread over (0, 1) for any d."""
    return (np.random.RandomState(seed).randn(n, d) * (0.7 / np.sqrt(d))).astype(np.float32)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def plain_entry(mmf, Xs, Ys, lam):
    """mmf_sim_dense_stats(MMF_RBF_DIRECT) called directly: (S [n_s, m_s] f32, the five raw doubles)."""
    ops, L = mmf.ops, mmf._lib.lib()
    out = torch.empty((Xs.shape[0], Ys.shape[0]), dtype=torch.float32, device=Xs.device)
    st = torch.empty((5,), dtype=torch.float64, device=Xs.device)
    rc = L.mmf_sim_dense_stats(ops._p(Xs), Xs.shape[0], ops._p(Ys), Ys.shape[0], Xs.shape[1], ops._DT[Xs.dtype], mmf._lib.RBF_DIRECT,
                               float(lam), ops._p(out), ops._p(st), 0, Xs.device.index or 0, ops._stream(Xs.device))
    mmf._lib.check(rc, "mmf_sim_dense_stats")
    return out, st


# ---------------------------------------------------------------------------------------------------
# bit identity against the unchanged plain entries
# ---------------------------------------------------------------------------------------------------
def _tiny(count, seed):
    rng = np.random.RandomState(seed)
    return list(zip(rng.randint(1, 41, count).tolist(), rng.randint(1, 25, count).tolist()))


COHORTS = {
    # a 1 x 1 block first (every later optr is odd: unaligned), m_s % 4 != 0, several tiles in both directions, a last block
    # that ends at the last row of X and Y
    "mixed_d64": ([(1, 1), (5, 3), (129, 128), (7, 10), (300, 200), (100, 37), (64, 64), (33, 130), (128, 129)], 64, "f32", (1.0, 0.37)),
    "pooled_d512": ([(100, 64), (40, 16), (257, 129), (3, 5), (100, 40)], 512, "f32", (1.0, 2.5)),
    "d30_not_a_multiple_of_4": ([(17, 9), (130, 131), (1, 7), (64, 12)], 30, "f32", (1.0,)),
    "d1": ([(9, 4), (200, 3), (1, 1), (130, 260)], 1, "f32", (1.0, 0.5)),
    "bf16_d64": ([(100, 48), (1, 1), (131, 70), (12, 129)], 64, "bf16", (1.0,)),
    "f16_d30": ([(100, 48), (5, 5), (131, 70), (12, 129)], 30, "f16", (0.8,)),
    "f16_d512": ([(100, 64), (64, 64), (3, 2)], 512, "f16", (1.0,)),
    # one block of 40 x 24 = 960 tiles (more than the 256 threads of the finish) and 229 histogram workgroups on 16 copies
    "one_large_block": ([(10, 10), (5000, 3000), (3, 7)], 64, "f32", (1.0,)),
    "2000_tiny_slides": (_tiny(2000, 7), 64, "f32", (1.0,)),
}


@pytest.mark.parametrize("name", list(COHORTS))
def test_blocks_and_statistics_are_the_plain_calls_bits(mmf, name):
    sizes, d, dtype, lams = COHORTS[name]
    xp, yp = offsets([n for n, _ in sizes]), offsets([m for _, m in sizes])
    X = T(rows(xp[-1], d, 11)).to(DT[dtype]).cuda()
    Y = T(rows(yp[-1], d, 12)).to(DT[dtype]).cuda()
    for lam in lams:
        S_flat, s_ptr, stats = wt().sim_dense_stats_segmented(X, Y, x_ptr=xp, y_ptr=yp, lam=lam)
        again = wt().sim_dense_stats_segmented(X, Y, x_batch=torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor([n for n, _ in sizes])),
                                               y_ptr=torch.tensor(yp), lam=lam)
        assert s_ptr.tolist() == offsets([n * m for n, m in sizes]) and s_ptr.device.type == "cpu" and again[1].tolist() == s_ptr.tolist()
        assert S_flat.dtype == torch.float32 and S_flat.shape == (s_ptr[-1],) and stats.shape == (len(sizes), 5) and stats.dtype == torch.float64
        assert torch.equal(bits(S_flat), bits(again[0])) and torch.equal(bits(stats), bits(again[2])), "two calls, different bits"
        S_bits, st_bits, st32 = bits(S_flat), bits(stats), stats.to(torch.float32).cpu().tolist()
        bad = []
        for s, (n_s, m_s) in enumerate(sizes):
            Xs, Ys = X[xp[s]:xp[s + 1]], Y[yp[s]:yp[s + 1]]
            want_S, want_st = plain_entry(mmf, Xs, Ys, lam)
            mirror_S, mirror_st = mmf.ops.sim_dense_stats(Xs, Ys, metric="rbf_direct", lam=lam)
            blk = S_bits[s_ptr[s]:s_ptr[s + 1]]
            if not torch.equal(blk, bits(want_S).reshape(-1)) or not torch.equal(blk, bits(mirror_S).reshape(-1)):
                bad.append(f"slide {s} ({n_s} x {m_s}): block differs")
            if not torch.equal(st_bits[s], bits(want_st)):
                bad.append(f"slide {s} ({n_s} x {m_s}): statistics {stats[s].tolist()} != {want_st.tolist()}")
            if repr(dict(zip(("mean", "std", "min", "max", "median"), st32[s]))) != repr(mirror_st):
                bad.append(f"slide {s}: f32-rounded statistics differ from ops.sim_dense_stats")
            if n_s * m_s == 1 and not np.isnan(st32[s][1]):
                bad.append(f"slide {s}: a 1 x 1 block must have NaN std")
        assert not bad, f"{name} lam={lam}: " + "; ".join(bad[:6])


# ---------------------------------------------------------------------------------------------------
# the flat ragged median
# ---------------------------------------------------------------------------------------------------
def _median_blocks():
    rng = np.random.RandomState(3)
    blocks = [rng.randn(c).astype(np.float32) for c in (1, 2, 3, 4, 100, 255, 256, 257, 65536, 65537, 1000, 131073)]
    blocks += [np.full(c, v, np.float32) for c, v in ((1, 2.5), (7, -3.0), (1000, 0.125), (70000, 1e-30))]
    blocks += [np.zeros(6, np.float32), -np.zeros(5, np.float32),
               np.where(rng.rand(1001) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32),
               np.array([-0.0, 0.0], np.float32), np.array([0.0, -0.0, -1.0, 1.0], np.float32)]
    blocks += [np.array([v], np.float32) for v in (0.0, -0.0, np.float32(np.inf), -1.5)]
    blocks += [rng.randn((1 << 22) + 5).astype(np.float32)]                  # above 2^22: the plain entry takes its one-sweep path
    blocks += [rng.rand(300000).astype(np.float32) ** 8, rng.randn(17).astype(np.float32)]      # 5 histogram workgroups; the last block ends the array
    return blocks


def test_flat_median_is_the_plain_median_of_every_block(mmf):
    blocks = _median_blocks()
    ptr = offsets([b.size for b in blocks])
    v = T(np.concatenate(blocks)).cuda()
    got = wt().lower_median_segmented(v, ptr=ptr)
    again = wt().lower_median_segmented(v, batch=torch.repeat_interleave(torch.arange(len(blocks)), torch.tensor([b.size for b in blocks])).cuda())
    assert got.shape == (len(blocks),) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(bits(got), bits(again))
    bad = []
    for s in range(len(blocks)):
        sl = v[ptr[s]:ptr[s + 1]]
        plain, tm = mmf.ops.lower_median(sl), torch.median(sl)
        if not torch.equal(bits(got[s]), bits(plain)):
            bad.append(f"block {s} ({blocks[s].size} values): {got[s].item()!r} != ops.lower_median {plain.item()!r}")
        if not (got[s].item() == tm.item()):                                 # -0.0 == 0.0: torch.median's sort does not order the zeros
            bad.append(f"block {s} ({blocks[s].size} values): {got[s].item()!r} != torch.median {tm.item()!r}")
        # rank (c - 1) / 2 in the f2ord total order, which puts -0.0 before 0.0
        key = np.sort(np.where(blocks[s].view(np.int32) < 0, ~blocks[s].view(np.uint32), blocks[s].view(np.uint32) | np.uint32(0x80000000)))
        k = key[(blocks[s].size - 1) // 2]
        want = np.array([~k if k < 0x80000000 else k & np.uint32(0x7fffffff)], np.uint32).view(np.float32)[0]
        if got[s].cpu().numpy().view(np.uint32) != want.view(np.uint32):
            bad.append(f"block {s}: {got[s].item()!r} is not the element of rank (c - 1) / 2 ({want!r})")
    assert not bad, "; ".join(bad[:6])


# ---------------------------------------------------------------------------------------------------
# the reference's own outputs (golden G8)
# ---------------------------------------------------------------------------------------------------
def _g8_cohort(g):
    wsi = T(np.concatenate([g["super_features"], g["rb_super_features"]]))
    tma = T(np.concatenate([g["tma_features"], g["tma_features"]]))
    n0, n1, m = g["super_features"].shape[0], g["rb_super_features"].shape[0], g["tma_features"].shape[0]
    return wsi, tma, [0, n0, n0 + n1], [0, m, 2 * m], [(n0, m), (n1, m)]


def test_similarity_against_the_references_outputs(mmf):
    """G8 holds two slides of one width: process_single_file's (super_features x tma_features -> sim, lambda_h of the golden's
    `lambdas`) and the rebuild's (rb_super_features x tma_features -> rb_sim, which rebuild_hypergraph_from_similarity forms
    with lambda_h = 1.0).  A cohort call has one lambda, so the cohort of two runs once per lambda: the slide the reference formed
    with that lambda is compared with its golden arrays, and BOTH slides with the plain mirror, bit for bit."""
    g = load_golden("g8_pipeline.npz")
    wsi, tma, wp, tp, sizes = _g8_cohort(g)
    pos = torch.zeros(wsi.shape[0], 2)
    for lam, slide, key in ((float(g["lambdas"][0]), 0, ""), (1.0, 1, "rb_")):
        S_flat, s_ptr, stats = wt().compute_wsi_tma_similarity_segmented(wsi, pos, tma, lambda_h=lam, lambda_g=float(g["lambdas"][1]),
                                                                         wsi_ptr=wp, tma_ptr=tp)
        assert S_flat.device.type == "cpu" and len(stats) == 2            # CPU inputs, device None: results on the CPU, as the mirror
        blk = wt().similarity_block(S_flat, s_ptr, sizes, slide)
        np.testing.assert_allclose(blk.numpy(), g[key + "sim"], rtol=0, atol=TOL)
        np.testing.assert_allclose([stats[slide][q] for q in ("mean", "std", "min", "max", "median")], g[key + "sim_stats"], rtol=2e-5, atol=1e-6)
        for s in range(2):
            Sm, stm = pp().compute_wsi_tma_similarity(wsi[wp[s]:wp[s + 1]], None, tma[tp[s]:tp[s + 1]], lambda_h=lam)
            assert torch.equal(bits(wt().similarity_block(S_flat, s_ptr, sizes, s)), bits(Sm)), (lam, s)
            assert repr(stats[s]) == repr(stm) and all(isinstance(v, float) for v in stats[s].values()), (lam, s)


def test_grouping_and_filter_against_the_references_outputs(mmf, kmeans_backend):
    """The two slides' num_groups differ (6 and 4): each is grouped as a one-slide cohort against its golden labels, and both
    as one two-slide cohort with a common G against the plain mirror.  rb_median / rb_threshold / rb_num_edges pin the median
    filter on the rebuilt slide."""
    g = load_golden("g8_pipeline.npz")
    wsi, tma, wp, tp, sizes = _g8_cohort(g)
    G, k, H = int(g["params"][1]), int(g["params"][2]), int(g["params"][3])
    G2, ratio = int(g["rb_params"][1]), float(g["rb_ratio"])
    dev = torch.device("cuda")
    # slide 0 with process_single_file's lambda, slide 1 with the rebuild's
    S0, _, _ = wt().compute_wsi_tma_similarity_segmented(wsi[:wp[1]], None, tma[:tp[1]], lambda_h=float(g["lambdas"][0]), device=dev,
                                                         wsi_ptr=[0, wp[1]], tma_ptr=[0, tp[1]])
    S1, _, _ = wt().compute_wsi_tma_similarity_segmented(wsi[wp[1]:], None, tma[tp[1]:], lambda_h=1.0, device=dev,
                                                         wsi_ptr=[0, wp[2] - wp[1]], tma_ptr=[0, tp[2] - tp[1]])
    assert S0.is_cuda and S1.is_cuda
    lab0, st0, _ = wt().group_by_similarity_segmented(S0, G, wsi_ptr=[0, sizes[0][0]], tma_ptr=[0, sizes[0][1]])
    assert lab0.dtype == np.int32 and np.array_equal(lab0, g["group_labels"])
    assert st0 == [{"method": "kmeans", "num_groups": G, "group_sizes": g["group_sizes"].tolist()}]
    lab1, st1, _ = wt().group_by_similarity_segmented(S1, G2, wsi_batch=torch.zeros(sizes[1][0], dtype=torch.long), tma_ptr=[0, sizes[1][1]])
    assert np.array_equal(lab1, g["rb_group_labels"])
    assert st1[0]["group_sizes"] == np.bincount(g["rb_group_labels"], minlength=G2).tolist()
    # both slides, a common G, against the plain mirror
    both = torch.cat([S0, S1])
    for Gc in (G2, 3):
        lab, st, info = wt().group_by_similarity_segmented(both, Gc, wsi_ptr=wp, tma_ptr=tp)
        assert info["kmeans_backend"] == kmeans_backend and (info["ambiguous_draws"] is None) == (kmeans_backend == "sklearn")
        for s, Ss in enumerate((S0, S1)):
            want_lab, want_st = pp().group_by_similarity(Ss.view(*sizes[s]), Gc)
            assert np.array_equal(lab[wp[s]:wp[s + 1]], want_lab) and st[s] == want_st, (Gc, s)
    # the rebuilt slide's hypergraph and its median filter
    n1 = sizes[1][0]
    ei, ew, eptr, hg = mmf.build_hypergraph_knn_kmeans_segmented(wsi[wp[1]:], tma[tp[1]:], lab1, k, H, device=dev, wsi_ptr=[0, n1],
                                                                 tma_ptr=[0, sizes[1][1]])
    assert hg["num_edges"] == int(g["rb_num_edges"]) == ei.shape[1]
    ei2, ew2, eptr2, flt = wt().filter_edges_by_median_segmented(ei, ew, [0, hg["num_edges"]], ratio)
    assert len(flt) == 1 and flt[0]["threshold_ratio"] == ratio
    assert abs(flt[0]["threshold"] - float(g["rb_threshold"])) < 1e-6 and abs(flt[0]["threshold"] / ratio - float(g["rb_median"])) < 1e-6
    assert flt[0]["num_edges_after_threshold"] == g["rb_ei_sorted"].shape[1] == ei2.shape[1] and eptr2.tolist() == [0, ei2.shape[1]]
    e = ei2.cpu().numpy()
    order = np.lexsort((e[1], e[0]))
    assert np.array_equal(e[:, order], g["rb_ei_sorted"])
    np.testing.assert_allclose(ew2.cpu().numpy()[order], g["rb_ew_sorted"], rtol=0, atol=TOL)


# ---------------------------------------------------------------------------------------------------
# grouping and the cohort chain against the per-slide chain of the plain mirrors
# ---------------------------------------------------------------------------------------------------
def _clustered(n, d, seed, centres=5):
    rng = np.random.RandomState(seed)
    c = rng.randn(centres, d) * (0.9 / np.sqrt(d))
    return (c[rng.randint(0, centres, n)] + rng.randn(n, d) * (0.25 / np.sqrt(d))).astype(np.float32)


# three distinct TMA widths in shuffled slide order (16, 24, 16, 33, 24, 16)
CHAIN_SIZES = [(30, 16), (25, 24), (40, 16), (35, 33), (28, 24), (32, 16)]


def _chain_cohort(d=32):
    wp, tp = offsets([n for n, _ in CHAIN_SIZES]), offsets([m for _, m in CHAIN_SIZES])
    wsi = T(np.concatenate([_clustered(n, d, 100 + s) for s, (n, _) in enumerate(CHAIN_SIZES)]))
    tma = T(np.concatenate([_clustered(m, d, 200 + s) for s, (_, m) in enumerate(CHAIN_SIZES)]))
    return wsi, tma, wp, tp


def test_grouping_equals_the_plain_mirror_per_slide(mmf, kmeans_backend):
    wsi, tma, wp, tp = _chain_cohort()
    assert len({m for _, m in CHAIN_SIZES}) == 3
    S_flat, s_ptr, _ = wt().compute_wsi_tma_similarity_segmented(wsi.cuda(), None, tma.cuda(), lambda_h=0.9, wsi_ptr=wp, tma_ptr=tp)
    for G in (4, 1):
        lab, st, info = wt().group_by_similarity_segmented(S_flat, G, wsi_ptr=wp, tma_batch=torch.repeat_interleave(
            torch.arange(len(CHAIN_SIZES)), torch.tensor([m for _, m in CHAIN_SIZES])))
        assert lab.shape == (wp[-1],) and lab.dtype == np.int32 and len(st) == len(CHAIN_SIZES)
        if kmeans_backend == "device":
            assert len(info["ambiguous_draws"]) == len(info["ambiguous_trials"]) == len(CHAIN_SIZES)
        for s in range(len(CHAIN_SIZES)):
            want_lab, want_st = pp().group_by_similarity(wt().similarity_block(S_flat, s_ptr, CHAIN_SIZES, s), G)
            assert np.array_equal(lab[wp[s]:wp[s + 1]], want_lab), (G, s)
            assert st[s] == want_st and sum(st[s]["group_sizes"]) == CHAIN_SIZES[s][0], (G, s)


def test_cohort_chain_equals_the_per_slide_chain(mmf, kmeans_backend):
    """similarity -> grouping -> k-NN + KMeans hypergraph -> median filter, cohort call by cohort call, against the plain mirrors
    slide by slide: blocks, statistics, labels, edge ids (shifted by node_ptr[s]) and weight bits."""
    wsi, tma, wp, tp = _chain_cohort()
    wsi_d, tma_d = wsi.cuda(), tma.cuda()
    lam, G, k, H, ratio = 0.9, 4, 3, 5, 0.9
    S_flat, s_ptr, sim_stats = wt().compute_wsi_tma_similarity_segmented(wsi_d, None, tma_d, lambda_h=lam, wsi_ptr=wp, tma_ptr=tp)
    labels, group_stats, _ = wt().group_by_similarity_segmented(S_flat, G, wsi_ptr=wp, tma_ptr=tp)
    ei, ew, eptr, hg = mmf.build_hypergraph_knn_kmeans_segmented(wsi_d, tma_d, labels, k, H, wsi_ptr=wp, tma_ptr=tp)
    counts = [seg["num_edges"] for seg in hg["segments"]]
    ei2, ew2, eptr2, flt = wt().filter_edges_by_median_segmented(ei, ew, offsets(counts), ratio)
    assert eptr.tolist() == offsets(counts) and ei2.is_cuda and ew2.is_cuda and eptr2.dtype == torch.int64
    via_device_ptr = wt().filter_edges_by_median_segmented(ei, ew, eptr, ratio)          # the builder's own edge_ptr (a device tensor)
    assert torch.equal(via_device_ptr[0], ei2) and torch.equal(bits(via_device_ptr[1]), bits(ew2)) and via_device_ptr[3] == flt
    e2 = eptr2.tolist()
    assert e2[0] == 0 and e2[-1] == ei2.shape[1] == ew2.shape[0]
    for s, (n_s, m_s) in enumerate(CHAIN_SIZES):
        w_s, t_s = wsi_d[wp[s]:wp[s + 1]], tma_d[tp[s]:tp[s + 1]]
        S_s, st_s = pp().compute_wsi_tma_similarity(w_s, None, t_s, lambda_h=lam)
        assert torch.equal(bits(S_flat[s_ptr[s]:s_ptr[s + 1]]), bits(S_s).reshape(-1)) and repr(sim_stats[s]) == repr(st_s), s
        lab_s, gst_s = pp().group_by_similarity(S_s, G)
        assert np.array_equal(labels[wp[s]:wp[s + 1]], lab_s) and group_stats[s] == gst_s, s
        ei_s, ew_s, hg_s = pp().build_hypergraph_knn_kmeans(w_s, t_s, lab_s, k, H)
        assert hg["segments"][s] == hg_s, s
        # the rebuild's filter, as rebuild_hypergraph_from_similarity writes it (:885-897)
        median = mmf.ops.lower_median(ew_s).item()
        thr = median * ratio
        mask = ew_s >= thr
        assert flt[s] == {"threshold": thr, "num_edges_after_threshold": int(mask.sum()), "threshold_ratio": ratio}, s
        assert e2[s + 1] - e2[s] == int(mask.sum()), s
        assert torch.equal(ei2[:, e2[s]:e2[s + 1]] - hg["node_ptr"][s], ei_s[:, mask]), s
        assert torch.equal(bits(ew2[e2[s]:e2[s + 1]]), bits(ew_s[mask])), s


# ---------------------------------------------------------------------------------------------------
# the stream contract: both C entries and every public function of the module behind a closed gate
# ---------------------------------------------------------------------------------------------------
def seeded(fn):
    return lambda which: [t if isinstance(t, torch.Tensor) else T(np.ascontiguousarray(t)) for t in fn(1 if which == "truth" else 2)]


def hp(a):
    return ctypes.c_void_p(a.data_ptr())


def _stats_reference(sizes, lam):
    xp, yp = offsets([n for n, _ in sizes]), offsets([m for _, m in sizes])

    def want(X, Y):
        S, st = [], []
        for s in range(len(sizes)):
            a, b = X[xp[s]:xp[s + 1]].astype(np.float64), Y[yp[s]:yp[s + 1]].astype(np.float64)
            blk = np.exp(-lam * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)).astype(np.float32).reshape(-1)
            S.append(blk)
            v = blk.astype(np.float64)
            st.append([v.mean(), v.std(ddof=1) if v.size > 1 else np.nan, v.min(), v.max(), np.sort(blk)[(blk.size - 1) // 2]])
        return np.concatenate(S), np.array(st, np.float64)

    def check(got, X, Y):
        S, st = want(X, Y)
        return sg.diff(got[0], S, "S_flat", atol=TOL) + sg.diff(got[-1], st, "stats", atol=2e-5)
    return xp, yp, check


CASES = {}


def case(name, covers, nonsync=False):
    def reg(fn):
        CASES[name] = dict(build=fn, covers=tuple(covers), nonsync=nonsync, calls=2 if nonsync else 1)
        return fn
    return reg


GATED_SIZES = [(100, 64), (1, 1), (129, 130), (40, 37), (64, 64)]


@case("c_entry_sim_dense_stats_segmented", ["mmf_sim_dense_stats_segmented"], nonsync=True)
def _():
    import multimodal_fusion_amd as m
    lam, d = 0.8, 48
    xp, yp, check = _stats_reference(GATED_SIZES, lam)
    hx, hy = torch.tensor(xp), torch.tensor(yp)

    def entry(X, Y):
        out = torch.empty((sum(n * mm for n, mm in GATED_SIZES),), dtype=torch.float32, device=X.device)
        st = torch.empty((len(GATED_SIZES), 5), dtype=torch.float64, device=X.device)
        px, py = hx.clone(), hy.clone()                 # host tables that die with the call
        rc = m._lib.lib().mmf_sim_dense_stats_segmented(m.ops._p(X), X.shape[0], m.ops._p(Y), Y.shape[0], d, m._lib.F32, m._lib.RBF_DIRECT,
                                                        lam, hp(px), hp(py), len(GATED_SIZES), m.ops._p(out), m.ops._p(st),
                                                        X.device.index or 0, m.ops._stream(X.device))
        m._lib.check(rc, "mmf_sim_dense_stats_segmented")
        return out, st
    return dict(entry=entry, make_inputs=seeded(lambda s: [rows(xp[-1], d, 300 + s), rows(yp[-1], d, 310 + s)]),
                reference=lambda X, Y: (lambda got: check(got, X, Y)))


def _median_reference(sizes):
    ptr = offsets(sizes)
    return ptr, lambda v: np.array([np.sort(v[ptr[s]:ptr[s + 1]])[(c - 1) // 2] for s, c in enumerate(sizes)], np.float32)


@case("c_entry_lower_median_segmented", ["mmf_lower_median_segmented"], nonsync=True)
def _():
    import multimodal_fusion_amd as m
    sizes = [5, 1, 70000, 2, 64, 257, 200000]
    ptr, ref = _median_reference(sizes)
    hptr = torch.tensor(ptr)

    def entry(v):
        out = torch.empty((len(sizes),), dtype=torch.float32, device=v.device)
        p = hptr.clone()
        rc = m._lib.lib().mmf_lower_median_segmented(m.ops._p(v), hp(p), len(sizes), m.ops._p(out), v.device.index or 0, m.ops._stream(v.device))
        m._lib.check(rc, "mmf_lower_median_segmented")
        return out
    return dict(entry=entry, make_inputs=seeded(lambda s: [np.random.RandomState(320 + s).rand(ptr[-1]).astype(np.float32)]), reference=ref)


@case("sim_dense_stats_segmented", ["sim_dense_stats_segmented"], nonsync=True)
def _():
    lam, d = 1.3, 30
    xp, yp, check = _stats_reference(GATED_SIZES, lam)
    return dict(entry=lambda X, Y: wt().sim_dense_stats_segmented(X, Y, x_ptr=xp, y_ptr=yp, lam=lam),
                make_inputs=seeded(lambda s: [rows(xp[-1], d, 330 + s), rows(yp[-1], d, 340 + s)]),
                reference=lambda X, Y: (lambda got: check(got, X, Y) + sg.diff(got[1], np.array(offsets([n * mm for n, mm in GATED_SIZES])), "s_ptr")))


@case("sim_dense_stats_segmented_50000_slides", ["sim_dense_stats_segmented"], nonsync=True)
def _():
    # host tables of more than 1 MiB (the work table: 3 x 8 bytes per tile, the select states: 32 bytes per slide)
    rng = np.random.RandomState(5)
    sizes = list(zip(rng.randint(1, 4, 50000).tolist(), rng.randint(1, 4, 50000).tolist()))
    lam, d = 1.0, 8
    xp, yp = offsets([n for n, _ in sizes]), offsets([m for _, m in sizes])
    seg_x, seg_y = np.repeat(np.arange(len(sizes)), [n for n, _ in sizes]), np.repeat(np.arange(len(sizes)), [m for _, m in sizes])

    def check(got, X, Y):
        # slide s's first pair, exactly: S_flat[s_ptr[s]] = exp(-lam |x_first - y_first|^2) to TOL; every statistic's minimum and
        # maximum bracket the median
        first = np.exp(-lam * ((X[np.array(xp[:-1])].astype(np.float64) - Y[np.array(yp[:-1])]) ** 2).sum(-1)).astype(np.float32)
        S_flat, s_ptr, st = got
        out = sg.diff(S_flat[s_ptr[:-1]], first, "first entries", atol=TOL)
        if not (np.all(st[:, 2] <= st[:, 4]) and np.all(st[:, 4] <= st[:, 3]) and np.all(st[:, 2] <= st[:, 0] + 1e-12)):
            out.append("statistics out of order")
        return out
    assert seg_x.size == xp[-1] and seg_y.size == yp[-1]
    return dict(entry=lambda X, Y: wt().sim_dense_stats_segmented(X, Y, x_ptr=xp, y_ptr=yp, lam=lam),
                make_inputs=seeded(lambda s: [rows(xp[-1], d, 350 + s), rows(yp[-1], d, 360 + s)]),
                reference=lambda X, Y: (lambda got: check(got, X, Y)))


@case("lower_median_segmented", ["lower_median_segmented"], nonsync=True)
def _():
    sizes = np.random.RandomState(13).randint(1, 400, 3000).tolist()
    ptr, ref = _median_reference(sizes)
    return dict(entry=lambda v: wt().lower_median_segmented(v, ptr=ptr),
                make_inputs=seeded(lambda s: [np.random.RandomState(370 + s).randn(ptr[-1]).astype(np.float32)]), reference=ref)


@case("compute_wsi_tma_similarity_segmented", ["compute_wsi_tma_similarity_segmented"])
def _():
    lam, d = 0.8, 64
    xp, yp, check = _stats_reference(GATED_SIZES, lam)

    def ref(X, Y):
        def chk(got):
            S_flat, s_ptr, dicts = got
            st = np.array([[dd[q] for q in ("mean", "std", "min", "max", "median")] for dd in dicts], np.float64)
            return check((S_flat, st), X, Y)
        return chk
    return dict(entry=lambda X, Y: wt().compute_wsi_tma_similarity_segmented(X, None, Y, lambda_h=lam, wsi_ptr=xp, tma_ptr=yp),
                make_inputs=seeded(lambda s: [rows(xp[-1], d, 380 + s), rows(yp[-1], d, 390 + s)]), reference=ref)


@case("similarity_block", ["similarity_block"], nonsync=True)
def _():
    sizes = [(3, 4), (1, 1), (5, 2)]
    sp = offsets([n * m for n, m in sizes])
    return dict(entry=lambda S: [wt().similarity_block(S, sp, sizes, s) for s in range(3)],
                make_inputs=seeded(lambda s: [np.random.RandomState(400 + s).rand(sp[-1]).astype(np.float32)]),
                reference=lambda S: [S[sp[s]:sp[s + 1]].reshape(sizes[s]) for s in range(3)])


@case("median_thresholds", ["median_thresholds"], nonsync=True)
def _():
    return dict(entry=lambda med: list(wt().median_thresholds(med, 0.8)),
                make_inputs=seeded(lambda s: [np.random.RandomState(410 + s).rand(100).astype(np.float32)]),
                reference=lambda med: [med.astype(np.float64) * 0.8, (med.astype(np.float64) * 0.8).astype(np.float32)])


@case("group_by_similarity_segmented", ["group_by_similarity_segmented"])
def _():
    sizes = [(30, 16), (25, 24), (40, 16)]
    wp, tp = offsets([n for n, _ in sizes]), offsets([m for _, m in sizes])
    sp = offsets([n * m for n, m in sizes])

    def reference(S):
        def chk(got):
            lab, st, info = got
            out = []
            for s, (n_s, m_s) in enumerate(sizes):
                want_lab, want_st = pp().group_by_similarity(T(S[sp[s]:sp[s + 1]].reshape(n_s, m_s)), 3)
                if not np.array_equal(lab[wp[s]:wp[s + 1]], want_lab) or st[s] != want_st:
                    out.append(f"slide {s}: labels or group sizes differ from group_by_similarity")
            return out
        return chk
    return dict(entry=lambda S: wt().group_by_similarity_segmented(S, 3, wsi_ptr=wp, tma_ptr=tp),
                make_inputs=seeded(lambda s: [np.exp(-np.random.RandomState(420 + s).rand(sp[-1]) * 3).astype(np.float32)]), reference=reference)


@case("filter_edges_by_median_segmented", ["filter_edges_by_median_segmented"])
def _():
    counts = [40, 1, 300, 7, 65]
    ep = offsets(counts)

    def reference(ei, ew):
        def chk(got):
            ei2, ew2, ep2, flt = got
            out, at = [], 0
            for s in range(len(counts)):
                w = ew[ep[s]:ep[s + 1]]
                thr = float(np.sort(w)[(w.size - 1) // 2]) * 0.9
                keep = T(w) >= thr                                          # torch's own scalar comparison, on the host
                n = int(keep.sum())
                if flt[s] != {"threshold": thr, "num_edges_after_threshold": n, "threshold_ratio": 0.9}:
                    out.append(f"slide {s}: stats {flt[s]}")
                out += sg.diff(ew2[at:at + n], w[keep.numpy()], f"weights of slide {s}") + sg.diff(ei2[:, at:at + n], ei[:, ep[s]:ep[s + 1]][:, keep.numpy()], f"edges of slide {s}")
                at += n
                if int(ep2[s + 1]) != at:
                    out.append(f"slide {s}: edge_ptr")
            return out
        return chk
    return dict(entry=lambda ei, ew: wt().filter_edges_by_median_segmented(ei, ew, ep, 0.9),
                make_inputs=seeded(lambda s: [np.random.RandomState(430 + s).randint(0, 1000, (2, ep[-1])).astype(np.int64),
                                              np.round(np.random.RandomState(440 + s).rand(ep[-1]) * 50).astype(np.float32) / 50]),
                reference=reference)


@pytest.mark.parametrize("name", list(CASES))
def test_entry_behind_a_closed_gate(mmf, name):
    c = CASES[name]
    kw = c["build"]()
    try:
        res = sg.run_gated(kw["entry"], kw["make_inputs"], kw["reference"], name=name, nonsync=c["nonsync"], calls=c["calls"])
    except RuntimeError as e:
        if "HIP error" in str(e) or "(code -3)" in str(e):          # a fault of the device: nothing more is started on it
            pytest.exit(f"{name}: the HIP runtime reported a failure, stopping the run: {e}", returncode=3)
        raise
    assert res.gate_ms >= 0.9 * sg.GATE_MIN_MS, f"{name}: the gate lasted {res.gate_ms:.1f} ms"
    if c["nonsync"]:
        assert res.returned_closed, name


def test_every_public_function_and_both_entries_have_a_case(mmf):
    """The stream-contract test of the parent pins ops.py and _lib.EXPORTS; this one carries the same contract for the new module
    and the second list."""
    mod = wt()
    public = {n for n, f in inspect.getmembers(mod, inspect.isfunction) if f.__module__ == mod.__name__ and not n.startswith("_")}
    public -= {"width_plan"}                                        # a pure function of Python lists: no tensor, no stream
    covered = {f for c in CASES.values() for f in c["covers"]}
    assert public <= covered, sorted(public - covered)
    assert set(mmf._lib.EXPORTS_COHORT) == set(SYNC_COHORT) <= covered
    # every entry and function documented as not synchronising is gated as such
    none = {e for e, (sync, _) in SYNC_COHORT.items() if sync == "none"} | {"sim_dense_stats_segmented", "lower_median_segmented"}
    gated_none = {f for c in CASES.values() if c["nonsync"] for f in c["covers"]}
    assert none <= gated_none, sorted(none - gated_none)
