"""Streamed super-patch statistics on the MI355X (include/mmf_hg_stream.h): the cluster means and the five
statistics of K = K_h * K_g from row panels that are recomputed and never stored.

  1. bits against the materialised path (ops.sim_dense_combined -> ops.segment_offdiag_mean, mmf_array_stats) at the smallest sizes
     at which each mechanism can go wrong, for four panel heights; order=None leaves intra_mean alone
  2. the same under MMF_MEDIAN_RADIX (stats_partial_kernel's assignment: the path of every slide that cannot be stored at all)
  3. heavy ties: the bracket's buffer overflows, the partials still come from the first sweep
  4. a small block (materialised inside the call), 5. run to run
  6. against the reference's arithmetic on the CPU (oracle/ref_restate.py)
  7. the cohort: a slide over the budget is streamed, everything else equal; the empty-cluster error keeps its words
  8. the stream contract of the entry and of the wrapper behind a closed gate (tests/streamgate.py)
"""
import ctypes
import json
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5                   # tests/test_gpu_pipeline.py: matrices that go through expf
LAM = (0.9, 0.4)
C = 8
PANELS = (0, 128, 333, "n")

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "Streaming entries"
# (tests/test_super_patch_stats_streamed_cpu.py keeps the two equal)
SYNC_STREAM = {"mmf_super_patch_stats_streamed": ("data-dependent", "—")}

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def sps():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.super_patch_stats")


def sp():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.super_patches")


def co():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.cohort")


def _clustered(n, d, seed, centres=5):
    """tests/test_gpu_super_patches_segmented.py's generator: squared distances of about 1."""
    rng = np.random.RandomState(seed)
    c = rng.randn(centres, d) * (0.9 / np.sqrt(d))
    return (c[rng.randint(0, centres, n)] + rng.randn(n, d) * (0.25 / np.sqrt(d))).astype(np.float32)


def shaped_labels(n, seed):
    """Labels in [0, C): cluster 0 is one row (NaN), cluster 1 two rows at the two ends of the slide, cluster 2 every 25th row
    (every 4th of a small slide) — more than 64 members (the lane-strided loop wraps) and some in every panel of 128 rows or
    more —, the rest random."""
    rng = np.random.RandomState(seed)
    lab = rng.randint(3, C, n).astype(np.int64)
    lab[5::25 if n >= 2048 else 4] = 2
    lab[7] = 0
    lab[11] = lab[n - 3] = 1
    assert (lab == 0).sum() == 1 and (lab == 1).sum() == 2 and (lab == 2).sum() > 64
    return lab


def raw_array_stats(mmf, K):
    """mmf_array_stats on the (aligned) allocation of K: the five raw doubles."""
    v = K.reshape(-1)
    assert v.data_ptr() % 16 == 0
    out = torch.empty((5,), dtype=torch.float64, device=v.device)
    rc = mmf._lib.lib().mmf_array_stats(mmf.ops._p(v), v.numel(), mmf.ops._p(out), v.device.index or 0, mmf.ops._stream(v.device))
    mmf._lib.check(rc, "mmf_array_stats")
    return out


SIZES = {2048: (16, 2), 2051: (40, 3), 6151: (16, 2), 300: (16, 2)}         # n -> (d, dp)
_CASES = {}


def inputs(n):
    d, dp = SIZES[n]
    F = T(_clustered(n, d, 1000 + n)).cuda()
    P = T(np.random.RandomState(2000 + n).rand(n, dp).astype(np.float32)).cuda()
    return F, P, T(shaped_labels(n, 3000 + n)).cuda()


def materialised(mmf, n, radix):
    """(F, P, seg, wanted intra, wanted stats) of size n; the wanted values come from the stored K, once per (n, environment)."""
    key = (n, bool(radix))
    assert bool(os.environ.get("MMF_MEDIAN_RADIX")) == bool(radix)
    if key not in _CASES:
        F, P, lab = inputs(n)
        seg = mmf.ops.segment_sort(lab, C)
        K = mmf.ops.sim_dense_combined(F, P, *LAM)
        want_i = mmf.ops.segment_offdiag_mean(K, seg).cpu().numpy()
        want_s = raw_array_stats(mmf, K).cpu().numpy()
        del K
        assert np.isnan(want_i[0]) and not np.isnan(want_i[1:]).any()
        _CASES[key] = (F, P, seg, want_i, want_s)
    return _CASES[key]


def check_bits(mmf, n, panel, radix=False):
    F, P, seg, want_i, want_s = materialised(mmf, n, radix)
    rows = n if panel == "n" else panel
    intra, k_stats = sps().super_patch_stats_streamed(F, P, seg.order, seg.offsets, C, *LAM, panel_rows=rows)
    assert intra.dtype == torch.float64 and intra.shape == (C,) and k_stats.dtype == torch.float64 and k_stats.shape == (5,)
    got_i, got_s = intra.cpu().numpy(), k_stats.cpu().numpy()
    print(f"n={n} panel_rows={rows} radix={radix}: stats {got_s.tolist()} wanted {want_s.tolist()}")
    print(f"n={n} panel_rows={rows} radix={radix}: intra {got_i.tolist()} wanted {want_i.tolist()}")
    assert np.array_equal(got_s, want_s, equal_nan=True), (got_s.tolist(), want_s.tolist())
    assert np.array_equal(got_i, want_i, equal_nan=True), (got_i.tolist(), want_i.tolist())


# ---------------------------------------------------------------------------------------------------
# 1. bits against the materialised path
# ---------------------------------------------------------------------------------------------------
# 2048: n^2 = 2^22, the first size on the one-sweep path, one flat row per wave.  2051: odd, flat rows straddle matrix rows, a
# ragged last flat row, d = 40 is no multiple of the f32 image's padding.  6151: 9236 flat rows > 4 x 2040, so the workgroup cap
# binds and some waves own two flat rows, in different panels.
@pytest.mark.parametrize("panel", PANELS)
@pytest.mark.parametrize("n", [2048, 2051, 6151])
def test_bits_equal_the_materialised_path(mmf, n, panel):
    assert n * n >= 1 << 22 and (n != 6151 or n * n // 4096 > 4 * 2040) and (n != 2051 or (n * n) % 4096)
    check_bits(mmf, n, panel)


def test_without_order_intra_mean_is_left_untouched(mmf):
    n = 2051
    F, P, seg, _, want_s = materialised(mmf, n, False)
    o = mmf.ops
    intra = torch.full((C,), -7.25, dtype=torch.float64, device=F.device)
    k_stats = torch.empty((5,), dtype=torch.float64, device=F.device)
    rc = mmf._lib.lib().mmf_super_patch_stats_streamed(o._p(F), o._p(P), n, F.shape[1], P.shape[1], LAM[0], LAM[1], None, None, 0, 333,
                                                       o._p(intra), o._p(k_stats), F.device.index or 0, o._stream(F.device))
    mmf._lib.check(rc, "mmf_super_patch_stats_streamed")
    assert bool((intra == -7.25).all())
    assert np.array_equal(k_stats.cpu().numpy(), want_s)
    got = sps().super_patch_stats_streamed(F, P, None, None, 0, *LAM, panel_rows=333)
    assert got[0] is None and np.array_equal(got[1].cpu().numpy(), want_s)


# ---------------------------------------------------------------------------------------------------
# 2. the assignment of stats_partial_kernel: what every slide that cannot be stored takes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel", PANELS)
@pytest.mark.parametrize("n", [2051, 6151])
def test_bits_equal_under_the_radix_select(mmf, monkeypatch, n, panel):
    monkeypatch.setenv("MMF_MEDIAN_RADIX", "1")
    check_bits(mmf, n, panel, radix=True)


# ---------------------------------------------------------------------------------------------------
# 3. heavy ties: the bracket fails, the partials are the first sweep's
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel", [0, 333])
def test_bits_equal_when_the_bracket_overflows(mmf, panel):
    n, d = 2304, 16
    rng = np.random.RandomState(77)
    src = rng.randint(0, 4, n)
    Fh = (rng.randn(4, d) * (0.7 / np.sqrt(d))).astype(np.float32)[src]
    Ph = np.zeros((n, 2), np.float32)
    # on the CPU: K takes at most 16 values, and the median's value fills more than the in-bracket buffer holds (5 % of the
    # values + 65536, mmf_edges.hip), so the one sweep cannot give a verdict
    d2 = ((Fh[:, None, :].astype(np.float64) - Fh[None, :, :]) ** 2).sum(-1)
    Kc = np.exp(-LAM[0] * d2).astype(np.float32).reshape(-1)
    med = np.sort(Kc)[(Kc.size - 1) // 2]
    assert np.unique(Kc).size <= 16
    assert (Kc == med).mean() > 0.05 and (Kc == med).sum() > Kc.size // 20 + 65536 + 8192
    F, P = T(Fh).cuda(), T(Ph).cuda()
    seg = mmf.ops.segment_sort(T(shaped_labels(n, 78)).cuda(), C)
    K = mmf.ops.sim_dense_combined(F, P, *LAM)
    dev_med = K.reshape(-1).median()
    assert int((K == dev_med).sum()) > K.numel() // 20 + 65536 + 8192          # the same on the matrix the device computes
    want_i, want_s = mmf.ops.segment_offdiag_mean(K, seg).cpu().numpy(), raw_array_stats(mmf, K).cpu().numpy()
    del K
    intra, k_stats = sps().super_patch_stats_streamed(F, P, seg.order, seg.offsets, C, *LAM, panel_rows=panel)
    print(f"ties panel_rows={panel}: stats {k_stats.tolist()} wanted {want_s.tolist()}")
    assert np.array_equal(k_stats.cpu().numpy(), want_s, equal_nan=True), (k_stats.tolist(), want_s.tolist())
    assert np.array_equal(intra.cpu().numpy(), want_i, equal_nan=True), (intra.tolist(), want_i.tolist())
    assert float(k_stats[4]) == float(dev_med)


# ---------------------------------------------------------------------------------------------------
# 4. a small block, 5. run to run
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel", [0, 128])
def test_a_small_block_has_the_plain_bits(mmf, panel):
    assert 300 * 300 < 1 << 22
    check_bits(mmf, 300, panel)


def test_two_calls_give_the_same_bits(mmf):
    F, P, seg, _, _ = materialised(mmf, 6151, False)
    a = sps().super_patch_stats_streamed(F, P, seg.order, seg.offsets, C, *LAM, panel_rows=333)
    b = sps().super_patch_stats_streamed(F, P, seg.order, seg.offsets, C, *LAM, panel_rows=333)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy(), equal_nan=True) and np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy())


# ---------------------------------------------------------------------------------------------------
# 6. the reference's arithmetic
# ---------------------------------------------------------------------------------------------------
def test_against_the_references_arithmetic(mmf):
    from oracle import ref_restate
    n, d = 2048, 32
    Fh, Ph = T(_clustered(n, d, 41)), T(np.random.RandomState(42).rand(n, 2).astype(np.float32))
    lab = shaped_labels(n, 43)
    K = ref_restate.compute_combined_similarity(Fh, Ph, *LAM)
    want_s = np.array([float(K.mean()), float(K.std()), float(K.min()), float(K.max()), float(K.median())])
    want_i = np.full(C, np.nan)
    Kd = K.double().numpy()
    for c in range(C):
        idx = np.nonzero(lab == c)[0]
        if idx.size > 1:
            blk = Kd[np.ix_(idx, idx)]
            want_i[c] = (blk.sum() - np.trace(blk)) / (idx.size * (idx.size - 1))
    seg = mmf.ops.segment_sort(T(lab).cuda(), C)
    intra, k_stats = sps().super_patch_stats_streamed(Fh.cuda(), Ph.cuda(), seg.order, seg.offsets, C, *LAM, panel_rows=128)
    got_s, got_i = k_stats.cpu().numpy(), intra.cpu().numpy()
    err = np.abs(got_s - want_s)
    print(f"reference: stats error {err.tolist()}, intra error {np.nanmax(np.abs(got_i - want_i))}")
    # every entry of K is within TOL, so are mean, min, max, median and the cluster means; the std is 1-Lipschitz in the RMS of the
    # element-wise difference up to sqrt(n / (n - 1)): 2 TOL
    assert err[0] <= TOL and err[2] <= TOL and err[3] <= TOL and err[4] <= TOL and err[1] <= 2 * TOL, err.tolist()
    assert np.isnan(got_i[0]) and np.isnan(want_i[0]) and np.nanmax(np.abs(got_i - want_i)) <= TOL


# ---------------------------------------------------------------------------------------------------
# 7. the cohort
# ---------------------------------------------------------------------------------------------------
COHORT_SIZES = [2100, 300, 2500]
COHORT_TMA = [16, 24, 16]
COHORT_D = 16
SMALL_BUDGET = 4 * 2200 * 2200


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def covering_labels(rng, n, n_clusters):
    lab = np.concatenate([np.arange(n_clusters), rng.randint(0, n_clusters, n - n_clusters)])
    return lab[rng.permutation(n)].astype(np.int64)


def cohort():
    ptr = offsets(COHORT_SIZES)
    F = T(np.concatenate([_clustered(n, COHORT_D, 500 + s) for s, n in enumerate(COHORT_SIZES)])).cuda()
    P = T(np.concatenate([np.random.RandomState(600 + s).rand(n, 2).astype(np.float32) for s, n in enumerate(COHORT_SIZES)])).cuda()
    tma = T(np.concatenate([_clustered(m, COHORT_D, 700 + s) for s, m in enumerate(COHORT_TMA)])).cuda()
    rng = np.random.RandomState(8)
    labels = np.concatenate([covering_labels(rng, n, C) for n in COHORT_SIZES])
    return F, P, tma, ptr, offsets(COHORT_TMA), labels


def same_stats(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)          # nan -> "NaN": equal as text


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def test_a_slide_over_the_budget_is_streamed_and_nothing_else_changes(mmf, monkeypatch):
    F, P, _, ptr, _, labels = cohort()
    monkeypatch.setattr(sp(), "_cohort_labels", lambda F, p, n_clusters: (T(labels).to(F.device), None, None))
    assert 2500 ** 2 >= 1 << 22 and 4 * 2500 ** 2 > SMALL_BUDGET >= 4 * (2100 ** 2 + 300 ** 2)
    whole = sp().aggregate_wsi_super_patches_segmented(F, P, C, *LAM, ptr=ptr, keep_similarity=False, return_info=True)
    lean = sp().aggregate_wsi_super_patches_segmented(F, P, C, *LAM, ptr=ptr, keep_similarity=False, budget_bytes=SMALL_BUDGET,
                                                      return_info=True)
    assert whole[5]["groups"] == [[0, 3]] and whole[5]["streamed"] == [False]
    assert lean[5]["groups"] == [[0, 2], [2, 3]] and lean[5]["streamed"] == [False, True]
    assert whole[3] is None and lean[3] is None and torch.equal(whole[4], lean[4])
    assert torch.equal(bits(whole[0]), bits(lean[0])) and torch.equal(bits(whole[1]), bits(lean[1]))
    for s in range(len(COHORT_SIZES)):
        assert same_stats(whole[2][s], lean[2][s]), (s, whole[2][s], lean[2][s])
    # every slide alone over the budget: the one of 300 rows (fewer than 2^22 values) is still stored
    tiny = sp().aggregate_wsi_super_patches_segmented(F, P, C, *LAM, ptr=ptr, keep_similarity=False, budget_bytes=4 * 100 * 100,
                                                      return_info=True)
    assert tiny[5]["groups"] == [[0, 1], [1, 2], [2, 3]] and tiny[5]["streamed"] == [True, False, True]
    assert all(same_stats(whole[2][s], tiny[2][s]) for s in range(3))
    # with K kept (or given) nothing is streamed
    kept = sp().aggregate_wsi_super_patches_segmented(F[:ptr[2]], P[:ptr[2]], C, *LAM, ptr=ptr[:3], budget_bytes=1, return_info=True)
    assert kept[5]["streamed"] == [False] and kept[3] is not None


def test_an_empty_cluster_of_a_streamed_slide_raises_the_mirrors_error(mmf, monkeypatch):
    F, P, _, ptr, _, labels = cohort()
    labels = labels.copy()
    tail = labels[ptr[2]:]
    tail[tail == 5] = 1                               # cluster 5 of slide 2 has no member
    monkeypatch.setattr(sp(), "_cohort_labels", lambda F, p, n_clusters: (T(labels).to(F.device), None, None))
    with pytest.raises(ValueError, match=r"^slide 2: Cluster 5 is empty$"):
        sp().aggregate_wsi_super_patches_segmented(F, P, C, *LAM, ptr=ptr, keep_similarity=False, budget_bytes=SMALL_BUDGET)


def test_the_cohort_chain_is_the_same_under_both_budgets(mmf, monkeypatch):
    F, P, tma, wp, tp, labels = cohort()
    monkeypatch.setattr(sp(), "_cohort_labels", lambda F, p, n_clusters: (T(labels).to(F.device), None, None))
    kw = dict(wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=3, hypergraph_k=3, num_hyperedges=4, lambda_h=LAM[0],
              lambda_g=LAM[1])
    a = co().build_cohort_hypergraphs(F, P, tma, **kw)
    b = co().build_cohort_hypergraphs(F, P, tma, budget_bytes=SMALL_BUDGET, **kw)
    assert sorted(a) == sorted(b) and a["K_flat"] is None and b["K_flat"] is None
    for key, va in a.items():
        if isinstance(va, torch.Tensor):
            assert torch.equal(bits(va), bits(b[key])), key
        elif isinstance(va, np.ndarray):
            assert np.array_equal(va, b[key]), key
    assert same_stats(a["stats"], b["stats"])


# ---------------------------------------------------------------------------------------------------
# 8. the stream contract: "data-dependent" — the call may wait for its stream, and enqueues on that stream only
# ---------------------------------------------------------------------------------------------------
GATED_N, GATED_D = 2051, 24


def gated_inputs(which):
    seed = 1 if which == "truth" else 2
    lab = shaped_labels(GATED_N, 900 + seed)
    order = np.argsort(lab, kind="stable").astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=C))]).astype(np.int64)
    return [T(_clustered(GATED_N, GATED_D, 910 + seed)), T(np.random.RandomState(920 + seed).rand(GATED_N, 2).astype(np.float32)),
            T(order), T(offs)]


def gated_reference(F, P, order, offs):
    d2 = lambda X: np.maximum((X * X).sum(1)[:, None] + (X * X).sum(1)[None, :] - 2.0 * X @ X.T, 0.0)   # noqa: E731
    K = np.exp(-LAM[0] * d2(F.astype(np.float64))) * np.exp(-LAM[1] * d2(P.astype(np.float64)))
    intra = np.full(C, np.nan)
    for c in range(C):
        idx = order[offs[c]:offs[c + 1]]
        if idx.size > 1:
            blk = K[np.ix_(idx, idx)]
            intra[c] = (blk.sum() - np.trace(blk)) / (idx.size * (idx.size - 1))
    v = K.reshape(-1)
    st = np.array([v.mean(), v.std(ddof=1), v.min(), v.max(), np.sort(v)[(v.size - 1) // 2]])
    return lambda got: sg.diff(got[0], intra, "intra", atol=TOL) + sg.diff(got[1], st, "k_stats", atol=2 * TOL)


def _c_entry(F, P, order, offs):
    import multimodal_fusion_amd as m
    o = m.ops
    intra = torch.empty((C,), dtype=torch.float64, device=F.device)
    k_stats = torch.empty((5,), dtype=torch.float64, device=F.device)
    rc = m._lib.lib().mmf_super_patch_stats_streamed(o._p(F), o._p(P), F.shape[0], F.shape[1], P.shape[1], LAM[0], LAM[1], o._p(order),
                                                     o._p(offs), C, 333, o._p(intra), o._p(k_stats), F.device.index or 0, o._stream(F.device))
    m._lib.check(rc, "mmf_super_patch_stats_streamed")
    return [intra, k_stats]


def _wrapper(F, P, order, offs):
    return list(sps().super_patch_stats_streamed(F, P, order, offs, C, *LAM, panel_rows=128))


@pytest.mark.parametrize("name,entry", [("c_entry_super_patch_stats_streamed", _c_entry), ("super_patch_stats_streamed", _wrapper)])
def test_entry_behind_a_closed_gate(mmf, name, entry):
    assert list(SYNC_STREAM) == [e for e in mmf._lib.EXPORTS_STREAM if not e.endswith("_bytes")]
    sg.run_gated(entry, gated_inputs, gated_reference, name=name, calls=2)
