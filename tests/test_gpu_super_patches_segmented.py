"""Segmented super-patch aggregation and the one-call cohort pipeline on the GPU.

  * the segmented sort against the UNCHANGED ops.segment_sort on every slice, and its two status flags;
  * bit identity of the pooled features / positions, the intra-cluster means and the five raw doubles of the statistics against
    the plain entries (mmf_segment_mean, mmf_segment_offdiag_mean, mmf_array_stats) on every slide, blocks that start off a
    16-byte boundary and one block above 2^22 values included;
  * aggregate_wsi_super_patches_segmented against the plain mirror slide by slide (both KMeans backends, groups under a memory
    budget, a given similarity), and against the reference's own outputs (tests/golden/g8_pipeline.npz);
  * build_cohort_hypergraphs against the per-slide chain of the four plain mirrors, and against g8's edges and group labels;
  * the stream contract of both C entries and of every public function of the two new modules behind a closed gate
    (tests/streamgate.py).

Every comparison covers every slide of its cohort.
"""
import ctypes
import inspect
import json
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

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "Pooling entries"
# (tests/test_super_patches_segmented_cpu.py keeps the two equal, and checks that these are the entries of _lib.EXPORTS_POOL)
CALL = "until the call returns"
SYNC_POOL = {
    "mmf_segment_sort_segmented": ("none", CALL),
    "mmf_super_patches_segmented": ("none", CALL),
}

T = torch.from_numpy
STAT_KEYS = ("mean", "std", "min", "max", "median")


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def sp():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.super_patches")


def co():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.cohort")


def pp():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.build_hypergraph.preprocess_hypergraph")


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def covering_labels(rng, n, C):
    """n >= C random labels in [0, C) with no empty cluster: every label once, the rest random, shuffled."""
    lab = np.concatenate([np.arange(C), rng.randint(0, C, n - C)])
    return lab[rng.permutation(n)].astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# 1. the sort is the plain sort per slide
# ---------------------------------------------------------------------------------------------------
def check_sort(mmf, per_slide, C, want_status=(-1, -1)):
    ptr = offsets([len(v) for v in per_slide])
    labels = T(np.concatenate(per_slide).astype(np.int64)).cuda()
    counts, offs, order, status = sp().segment_sort_segmented(labels, C, ptr=ptr)
    S = len(per_slide)
    assert counts.shape == (S * C,) and offs.shape == (S * C + 1,) and order.shape == (ptr[-1],) and status.shape == (2,)
    assert all(t.is_cuda and t.dtype == torch.int64 for t in (counts, offs, order, status))
    assert status.tolist() == list(want_status)
    assert int(offs[0]) == 0 and torch.equal(offs[1:], torch.cumsum(counts, 0))
    bad = []
    for s in range(S):
        seg = mmf.ops.segment_sort(labels[ptr[s]:ptr[s + 1]], C)
        lo, hi = int(offs[s * C]), int(offs[(s + 1) * C])
        if not torch.equal(counts[s * C:(s + 1) * C], seg.counts):
            bad.append(f"slide {s}: counts")
        if not torch.equal(offs[s * C:(s + 1) * C + 1] - lo, seg.offsets):
            bad.append(f"slide {s}: offsets")
        if hi - lo != ptr[s + 1] - ptr[s] or not torch.equal(order[lo:hi] - ptr[s], seg.order):
            bad.append(f"slide {s}: order")
    assert not bad, "; ".join(bad[:6])
    return counts, offs, order


def test_sort_chunk_boundaries_at_and_past_a_slides_end(mmf):
    rng = np.random.RandomState(1)
    # chunks of 1024 labels: slide 1 ends at its chunk's end, slide 2 one label and slide 3 one label past two chunks
    check_sort(mmf, [covering_labels(rng, n, 5) for n in (5, 1024, 1025, 2049, 7)], 5)


def test_sort_more_clusters_than_the_plain_entry_holds(mmf):
    rng = np.random.RandomState(2)
    S, C = 600, 30
    assert S * C > 16384
    check_sort(mmf, [rng.permutation(C).astype(np.int64) for _ in range(S)], C)           # every cluster a singleton
    patched = []
    for _ in range(S):                           # random labels, then every missing label written over a duplicate
        lab = rng.randint(0, C, C).astype(np.int64)
        missing = [c for c in range(C) if c not in set(lab.tolist())]
        seen = set()
        for i, v in enumerate(lab.tolist()):
            if v in seen and missing:
                lab[i] = missing.pop()
            seen.add(int(lab[i]))
        patched.append(lab)
    check_sort(mmf, patched, C)


def test_sort_one_cluster_and_the_largest_cluster_count(mmf):
    rng = np.random.RandomState(3)
    check_sort(mmf, [np.zeros(n, np.int64) for n in (3, 1500, 1, 64)], 1)
    check_sort(mmf, [covering_labels(rng, 16400, 16384)], 16384)


def test_sort_status_flags(mmf):
    rng = np.random.RandomState(4)
    C, sizes = 5, [40, 50, 1100, 70, 45]
    ptr = offsets(sizes)
    base = [covering_labels(rng, n, C) for n in sizes]
    # one label out of range in slide 3: status[0] is that row, and the other rows are sorted as if it were absent
    shared = lambda v: next(i for i in range(5, len(v)) if (v == v[i]).sum() >= 2)   # noqa: E731  (its cluster keeps a member)
    row, row1 = shared(base[3]), shared(base[1])
    lab = [v.copy() for v in base]
    lab[3][row] = C
    counts, offs, order, status = sp().segment_sort_segmented(T(np.concatenate(lab)).cuda(), C, ptr=ptr)
    assert status.tolist() == [ptr[3] + row, -1]
    for s in range(len(sizes)):
        keep = np.array([i for i in range(sizes[s]) if not (s == 3 and i == row)])
        seg = mmf.ops.segment_sort(T(lab[s][keep]).cuda(), C)
        lo, hi = int(offs[s * C]), int(offs[(s + 1) * C])
        assert torch.equal(counts[s * C:(s + 1) * C], seg.counts), s
        assert torch.equal(order[lo:hi] - ptr[s], T(keep).cuda()[seg.order]), s
    assert int(offs[-1]) == ptr[-1] - 1
    # a negative label is out of range too, and the LOWEST bad row is reported
    lab[1][row1] = -1
    assert sp().segment_sort_segmented(T(np.concatenate(lab)).cuda(), C, ptr=ptr)[3].tolist() == [ptr[1] + row1, -1]
    # one cluster emptied in slide 2
    c = 3
    lab = [v.copy() for v in base]
    lab[2][lab[2] == c] = 0
    assert sp().segment_sort_segmented(T(np.concatenate(lab)).cuda(), C, ptr=ptr)[3].tolist() == [-1, 2 * C + c]


# ---------------------------------------------------------------------------------------------------
# 3. pooling bits against the plain entries
# ---------------------------------------------------------------------------------------------------
POOL_SIZES = [33, 35, 64, 12, 130, 2049]          # odd sizes: the following blocks are unaligned; 12 = C: singletons; 2049^2 >= 2^22
POOL_C, POOL_D = 12, 70


def raw_array_stats(mmf, v):
    """mmf_array_stats called directly on an aligned copy: the five raw doubles."""
    v = v.clone().reshape(-1)
    out = torch.empty((5,), dtype=torch.float64, device=v.device)
    rc = mmf._lib.lib().mmf_array_stats(mmf.ops._p(v), v.numel(), mmf.ops._p(out), v.device.index or 0, mmf.ops._stream(v.device))
    mmf._lib.check(rc, "mmf_array_stats")
    return out


@pytest.fixture(scope="module")
def pool_cohort(mmf):
    """Features, labels, the sort and K_flat of the pooling cohort, and the plain entries' results per slide (computed once)."""
    assert POOL_SIZES[-1] ** 2 >= 1 << 22 and POOL_C in POOL_SIZES and POOL_D % 64
    rng = np.random.RandomState(5)
    ptr = offsets(POOL_SIZES)
    F = T((rng.randn(ptr[-1], POOL_D) * (0.7 / np.sqrt(POOL_D))).astype(np.float32)).cuda()
    P = {dp: T(rng.rand(ptr[-1], dp).astype(np.float32)).cuda() for dp in (2, 3)}
    labels = T(np.concatenate([covering_labels(rng, n, POOL_C) for n in POOL_SIZES])).cuda()
    K_flat, kptr = mmf.ops.sim_dense_combined_segmented(F, P[2], 1.0, 0.5, ptr=ptr)
    assert any(int(k) % 4 for k in kptr[:-1]), "no unaligned block in the cohort"
    _, offs, order, status = sp().segment_sort_segmented(labels, POOL_C, ptr=ptr)
    assert status.tolist() == [-1, -1]
    plain = []
    for s, n_s in enumerate(POOL_SIZES):
        seg = mmf.ops.segment_sort(labels[ptr[s]:ptr[s + 1]], POOL_C)
        K_s = K_flat[int(kptr[s]):int(kptr[s + 1])].clone().view(n_s, n_s)       # the per-slide call sees an aligned allocation
        plain.append(dict(f=mmf.ops.segment_mean(F[ptr[s]:ptr[s + 1]], seg),
                          p={dp: mmf.ops.segment_mean(P[dp][ptr[s]:ptr[s + 1]], seg) for dp in (2, 3)},
                          intra=mmf.ops.segment_offdiag_mean(K_s, seg), stats=raw_array_stats(mmf, K_s)))
    return dict(ptr=ptr, F=F, P=P, K_flat=K_flat, order=order, offs=offs, plain=plain)


@pytest.mark.parametrize("dp", [2, 3])
def test_pooling_carries_the_plain_entries_bits(mmf, pool_cohort, dp):
    c = pool_cohort
    C = POOL_C
    sf, spos, intra, k_stats = sp().pool_super_patches_segmented(c["F"], c["P"][dp], c["order"], c["offs"], C, ptr=c["ptr"], K_flat=c["K_flat"])
    assert sf.shape == (len(POOL_SIZES) * C, POOL_D) and spos.shape == (len(POOL_SIZES) * C, dp)
    assert intra.shape == (len(POOL_SIZES) * C,) and intra.dtype == torch.float64 and k_stats.shape == (len(POOL_SIZES), 5)
    bad = []
    for s, n_s in enumerate(POOL_SIZES):
        w = c["plain"][s]
        if not torch.equal(bits(sf[s * C:(s + 1) * C]), bits(w["f"])):
            bad.append(f"slide {s} ({n_s} rows): pooled features differ")
        if not torch.equal(bits(spos[s * C:(s + 1) * C]), bits(w["p"][dp])):
            bad.append(f"slide {s} ({n_s} rows): pooled positions differ")
        got_i, want_i = intra[s * C:(s + 1) * C].cpu().numpy(), w["intra"].cpu().numpy()
        if not np.array_equal(got_i, want_i, equal_nan=True):
            bad.append(f"slide {s} ({n_s} rows): intra means {got_i.tolist()} != {want_i.tolist()}")
        if n_s == C and not np.isnan(got_i).all():
            bad.append(f"slide {s}: singleton clusters must have NaN intra means")
        if n_s > C and np.isnan(got_i).all():
            bad.append(f"slide {s}: no cluster with two members")
        if not np.array_equal(k_stats[s].cpu().numpy(), w["stats"].cpu().numpy(), equal_nan=True):
            bad.append(f"slide {s} ({n_s} rows): statistics {k_stats[s].tolist()} != {w['stats'].tolist()}")
    assert not bad, "; ".join(bad[:6])


def test_pooling_without_k_leaves_the_two_k_outputs_untouched(mmf, pool_cohort):
    c = pool_cohort
    C, S, n = POOL_C, len(POOL_SIZES), c["ptr"][-1]
    dev = c["F"].device
    sf = torch.empty((S * C, POOL_D), dtype=torch.float32, device=dev)
    spos = torch.empty((S * C, 2), dtype=torch.float32, device=dev)
    intra = torch.full((S * C,), -7.25, dtype=torch.float64, device=dev)
    k_stats = torch.full((S, 5), -7.25, dtype=torch.float64, device=dev)
    hptr = torch.tensor(c["ptr"])
    o = mmf.ops
    rc = mmf._lib.lib().mmf_super_patches_segmented(o._p(c["F"]), o._p(c["P"][2]), n, POOL_D, 2, ctypes.c_void_p(hptr.data_ptr()), S, C,
                                                    o._p(c["order"]), o._p(c["offs"]), None, o._p(sf), o._p(spos), o._p(intra),
                                                    o._p(k_stats), dev.index or 0, o._stream(dev))
    mmf._lib.check(rc, "mmf_super_patches_segmented")
    assert bool((intra == -7.25).all()) and bool((k_stats == -7.25).all())
    for s in range(S):
        assert torch.equal(bits(sf[s * C:(s + 1) * C]), bits(c["plain"][s]["f"])), s
        assert torch.equal(bits(spos[s * C:(s + 1) * C]), bits(c["plain"][s]["p"][2])), s
    got = sp().pool_super_patches_segmented(c["F"], c["P"][2], c["order"], c["offs"], C, ptr=c["ptr"])
    assert got[2] is None and got[3] is None and torch.equal(bits(got[0]), bits(sf))


# ---------------------------------------------------------------------------------------------------
# 4. the mirror per slide
# ---------------------------------------------------------------------------------------------------
def _clustered(n, d, seed, centres=5):
    rng = np.random.RandomState(seed)
    c = rng.randn(centres, d) * (0.9 / np.sqrt(d))
    return (c[rng.randint(0, centres, n)] + rng.randn(n, d) * (0.25 / np.sqrt(d))).astype(np.float32)


MIRROR_SIZES = [60, 300, 120, 250, 90, 150]
MIRROR_TMA = [16, 24, 16, 33, 24, 16]
MIRROR_C, MIRROR_D, MIRROR_LAM = 8, 32, (0.9, 0.4)
MIRROR_BUDGET = 375000                             # bytes: blocks of 14400, 360000 | 57600, 250000, 32400 | 90000


def _mirror_cohort():
    ptr = offsets(MIRROR_SIZES)
    F = T(np.concatenate([_clustered(n, MIRROR_D, 500 + s) for s, n in enumerate(MIRROR_SIZES)]))
    P = T(np.concatenate([np.random.RandomState(600 + s).rand(n, 2).astype(np.float32) for s, n in enumerate(MIRROR_SIZES)]))
    tma = T(np.concatenate([_clustered(m, MIRROR_D, 700 + s) for s, m in enumerate(MIRROR_TMA)]))
    return F, P, tma, ptr, offsets(MIRROR_TMA)


_PLAIN = {}


def plain_mirror(backend):
    """aggregate_wsi_super_patches on every slide of the mirror cohort with the current backend, computed once per backend."""
    if backend not in _PLAIN:
        F, P, _, ptr, _ = _mirror_cohort()
        Fd, Pd = F.cuda(), P.cuda()
        _PLAIN[backend] = [pp().aggregate_wsi_super_patches(Fd[ptr[s]:ptr[s + 1]], Pd[ptr[s]:ptr[s + 1]], MIRROR_C, *MIRROR_LAM)
                           for s in range(len(MIRROR_SIZES))]
    return _PLAIN[backend]


def same_stats(a, b):
    """== on the stats dicts, with NaN == NaN for the statistics (std of a 1 x 1 block)."""
    def norm(d):
        return json.dumps(d, sort_keys=True)          # nan -> "NaN": equal as text; floats print with repr
    return norm(a) == norm(b)


def check_against_plain(got, plain, ptr, with_k=True):
    sf, spos, stats, K_flat, k_ptr = got[:5]
    C = MIRROR_C
    assert k_ptr.tolist() == offsets([n * n for n in MIRROR_SIZES]) and k_ptr.device.type == "cpu" and len(stats) == len(MIRROR_SIZES)
    assert (K_flat is not None) == with_k
    for s, n_s in enumerate(MIRROR_SIZES):
        f_s, p_s, st_s, K_s = plain[s]
        assert torch.equal(bits(sf[s * C:(s + 1) * C]), bits(f_s)), s
        assert torch.equal(bits(spos[s * C:(s + 1) * C]), bits(p_s)), s
        if with_k:
            assert torch.equal(bits(K_flat[int(k_ptr[s]):int(k_ptr[s + 1])]), bits(K_s).reshape(-1)), s
        assert same_stats(stats[s], st_s), (s, stats[s], st_s)
        assert stats[s]["num_original_patches"] == n_s and isinstance(stats[s]["avg_intra_cluster_similarity"], float)
        assert all(type(v) is float for v in stats[s]["wsi_similarity_matrix_stats"].values()), s


def test_aggregate_equals_the_plain_mirror_per_slide(mmf, kmeans_backend):
    F, P, _, ptr, _ = _mirror_cohort()
    Fd, Pd = F.cuda(), P.cuda()
    plain = plain_mirror(kmeans_backend)
    got = sp().aggregate_wsi_super_patches_segmented(Fd, Pd, MIRROR_C, *MIRROR_LAM, ptr=ptr, return_info=True)
    assert got[0].is_cuda and got[3].is_cuda
    check_against_plain(got, plain, ptr)
    info = got[5]
    assert info["kmeans_backend"] == kmeans_backend and info["groups"] == [[0, len(MIRROR_SIZES)]]
    assert (info["ambiguous_draws"] is None) == (kmeans_backend == "sklearn")
    if kmeans_backend == "device":
        assert len(info["ambiguous_draws"]) == len(info["ambiguous_trials"]) == len(MIRROR_SIZES)
    # slides by batch vector instead of offsets: the same bits
    batch = torch.repeat_interleave(torch.arange(len(MIRROR_SIZES)), torch.tensor(MIRROR_SIZES))
    again = sp().aggregate_wsi_super_patches_segmented(Fd, Pd, MIRROR_C, *MIRROR_LAM, batch=batch)
    assert torch.equal(bits(again[0]), bits(got[0])) and torch.equal(bits(again[3]), bits(got[3])) and same_stats(again[2], got[2])
    # groups under a memory budget: nothing of K is returned, everything else is identical
    lean = sp().aggregate_wsi_super_patches_segmented(Fd, Pd, MIRROR_C, *MIRROR_LAM, ptr=ptr, keep_similarity=False,
                                                      budget_bytes=MIRROR_BUDGET, return_info=True)
    assert lean[5]["groups"] == [[0, 2], [2, 5], [5, 6]]
    check_against_plain(lean, plain, ptr, with_k=False)
    # the similarity given: used as K and returned
    given = sp().aggregate_wsi_super_patches_segmented(Fd, Pd, MIRROR_C, *MIRROR_LAM, wsi_similarity_flat=got[3], ptr=ptr)
    check_against_plain(given, plain, ptr)
    # CPU inputs, device None: the results live on the CPU, as the mirror's
    cpu = sp().aggregate_wsi_super_patches_segmented(F, P, MIRROR_C, *MIRROR_LAM, ptr=ptr, keep_similarity=False)
    assert cpu[0].device.type == "cpu" and cpu[1].device.type == "cpu" and cpu[3] is None
    assert torch.equal(bits(cpu[0]), bits(got[0])) and torch.equal(bits(cpu[1]), bits(got[1]))


# ---------------------------------------------------------------------------------------------------
# 5. the reference's own outputs (golden G8)
# ---------------------------------------------------------------------------------------------------
def _g8_cohort(g):
    d = g["wsi_features"].shape[1]
    sizes, tma_sizes = [100, g["wsi_features"].shape[0], 80], [20, g["tma_features"].shape[0], 20]
    F = T(np.concatenate([_clustered(sizes[0], d, 801), g["wsi_features"], _clustered(sizes[2], d, 802)]))
    P = T(np.concatenate([np.random.RandomState(803).rand(sizes[0], 2).astype(np.float32), g["wsi_positions"],
                          np.random.RandomState(804).rand(sizes[2], 2).astype(np.float32)]))
    tma = T(np.concatenate([_clustered(tma_sizes[0], d, 805), g["tma_features"], _clustered(tma_sizes[2], d, 806)]))
    return F, P, tma, offsets(sizes), offsets(tma_sizes)


def test_aggregate_against_the_references_outputs(mmf):
    g = load_golden("g8_pipeline.npz")
    C = int(g["params"][0])
    lam_h, lam_g = (float(v) for v in g["lambdas"])
    F, P, _, ptr, _ = _g8_cohort(g)
    sf, spos, stats, K_flat, k_ptr = sp().aggregate_wsi_super_patches_segmented(F, P, C, lam_h, lam_g, ptr=ptr)
    assert sf.device.type == "cpu" and K_flat.device.type == "cpu"
    n = g["wsi_features"].shape[0]
    np.testing.assert_allclose(sf[C:2 * C].numpy(), g["super_features"], rtol=0, atol=TOL)
    np.testing.assert_allclose(spos[C:2 * C].numpy(), g["super_positions"], rtol=0, atol=TOL)
    np.testing.assert_allclose(K_flat[int(k_ptr[1]):int(k_ptr[2])].view(n, n).numpy(), g["K_wsi"], rtol=0, atol=TOL)
    ws = stats[1]
    got = [ws["avg_intra_cluster_similarity"]] + [ws["wsi_similarity_matrix_stats"][q] for q in STAT_KEYS]
    np.testing.assert_allclose(got, g["wsi_stats"], rtol=2e-5, atol=1e-6)
    assert ws["num_original_patches"] == n and ws["num_super_patches"] == C


# ---------------------------------------------------------------------------------------------------
# 6. an empty cluster
# ---------------------------------------------------------------------------------------------------
def test_an_empty_cluster_raises_the_mirrors_error_with_the_slide(mmf, monkeypatch):
    rng = np.random.RandomState(9)
    sizes, C = [20, 30, 25], 4
    ptr = offsets(sizes)
    lab = [covering_labels(rng, n, C) for n in sizes]
    lab[1][lab[1] == 2] = 0                         # cluster 2 of slide 1 has no member
    lab[2][lab[2] == 1] = 3                         # a later one too: the FIRST is named
    labels = np.concatenate(lab)
    monkeypatch.setattr(sp(), "_cohort_labels", lambda F, p, n_clusters: (T(labels).to(F.device), None, None))
    F, P = torch.randn(ptr[-1], 16).cuda(), torch.rand(ptr[-1], 2).cuda()
    with pytest.raises(ValueError, match=r"^slide 1: Cluster 2 is empty$"):
        sp().aggregate_wsi_super_patches_segmented(F, P, C, ptr=ptr)
    with pytest.raises(ValueError, match=r"^slide 1: Cluster 2 is empty$"):
        sp().aggregate_wsi_super_patches_segmented(F, P, C, ptr=ptr, keep_similarity=False, budget_bytes=20 * 20 * 4)


# ---------------------------------------------------------------------------------------------------
# 7. the chain
# ---------------------------------------------------------------------------------------------------
def test_cohort_chain_equals_the_per_slide_chain(mmf, kmeans_backend):
    F, P, tma, wp, tp = _mirror_cohort()
    Fd, Pd, Td = F.cuda(), P.cuda(), tma.cuda()
    C, G, k, H = MIRROR_C, 3, 3, 4
    lam_h, lam_g = MIRROR_LAM
    out = co().build_cohort_hypergraphs(Fd, Pd, Td, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=G, hypergraph_k=k,
                                        num_hyperedges=H, lambda_h=lam_h, lambda_g=lam_g, keep_similarity=True)
    json.dumps(out["stats"])                                                         # JSON-serialisable as it is
    S = len(MIRROR_SIZES)
    assert out["group_ptr"].tolist() == [s * C for s in range(S + 1)] and out["group_labels"].dtype == np.int32
    ep, node_ptr, s_ptr, k_ptr = out["edge_ptr"].tolist(), out["node_ptr"].tolist(), out["s_ptr"], out["k_ptr"]
    assert node_ptr == offsets([C + m for m in MIRROR_TMA]) and ep[-1] == out["edge_index"].shape[1] == out["edge_weights"].shape[0]
    for s in range(S):
        w_s, p_s, t_s = Fd[wp[s]:wp[s + 1]], Pd[wp[s]:wp[s + 1]], Td[tp[s]:tp[s + 1]]
        sf, spos, agg, K = pp().aggregate_wsi_super_patches(w_s, p_s, C, lam_h, lam_g)
        S_s, sim = pp().compute_wsi_tma_similarity(sf, spos, t_s, lam_h, lam_g)
        lab, grp = pp().group_by_similarity(S_s, G)
        ei, ew, hg = pp().build_hypergraph_knn_kmeans(sf, t_s, lab, k, H)
        assert torch.equal(bits(out["super_features"][s * C:(s + 1) * C]), bits(sf)), s
        assert torch.equal(bits(out["super_positions"][s * C:(s + 1) * C]), bits(spos)), s
        assert torch.equal(bits(out["K_flat"][int(k_ptr[s]):int(k_ptr[s + 1])]), bits(K).reshape(-1)), s
        assert torch.equal(bits(out["S_flat"][int(s_ptr[s]):int(s_ptr[s + 1])]), bits(S_s).reshape(-1)), s
        assert np.array_equal(out["group_labels"][s * C:(s + 1) * C], lab), s
        assert torch.equal(out["edge_index"][:, ep[s]:ep[s + 1]] - node_ptr[s], ei), s
        assert torch.equal(bits(out["edge_weights"][ep[s]:ep[s + 1]]), bits(ew)), s
        want = {"wsi_aggregation": agg, "similarity": sim, "grouping": grp, "hypergraph": hg}
        assert same_stats(out["stats"][s], want), (s, out["stats"][s], want)
    # nothing of K unless asked for
    lean = co().build_cohort_hypergraphs(Fd, Pd, Td, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=G, hypergraph_k=k,
                                         num_hyperedges=H, lambda_h=lam_h, lambda_g=lam_g)
    assert lean["K_flat"] is None and torch.equal(lean["edge_index"], out["edge_index"]) and same_stats(lean["stats"], out["stats"])


def test_cohort_chain_against_the_references_outputs(mmf):
    g = load_golden("g8_pipeline.npz")
    C, G, k, H = (int(v) for v in g["params"])
    lam_h, lam_g = (float(v) for v in g["lambdas"])
    F, P, tma, wp, tp = _g8_cohort(g)
    out = co().build_cohort_hypergraphs(F, P, tma, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=G, hypergraph_k=k,
                                        num_hyperedges=H, lambda_h=lam_h, lambda_g=lam_g)
    assert out["edge_index"].device.type == "cpu" and out["K_flat"] is None
    ep, node_ptr = out["edge_ptr"].tolist(), out["node_ptr"].tolist()
    e = (out["edge_index"][:, ep[1]:ep[2]] - node_ptr[1]).numpy()
    order = np.lexsort((e[1], e[0]))
    assert np.array_equal(e[:, order], g["ei_sorted"])
    np.testing.assert_allclose(out["edge_weights"][ep[1]:ep[2]].numpy()[order], g["ew_sorted"], rtol=0, atol=TOL)
    assert np.array_equal(out["group_labels"][C:2 * C], g["group_labels"])
    assert out["stats"][1]["grouping"]["group_sizes"] == g["group_sizes"].tolist()
    assert out["stats"][1]["hypergraph"]["num_edges"] == int(g["num_edges"])


# ---------------------------------------------------------------------------------------------------
# 8. the stream contract: both C entries and every public function of the two modules behind a closed gate
# ---------------------------------------------------------------------------------------------------
def seeded(fn):
    return lambda which: [t if isinstance(t, torch.Tensor) else T(np.ascontiguousarray(t)) for t in fn(1 if which == "truth" else 2)]


def hp(a):
    return ctypes.c_void_p(a.data_ptr())


GATED_SIZES = [70, 33, 1025, 12, 129]
GATED_C = 6


def gated_labels(seed):
    rng = np.random.RandomState(900 + seed)
    return np.concatenate([covering_labels(rng, n, GATED_C) for n in GATED_SIZES])


def sort_reference(labels):
    """(counts, offsets, order, status) of valid labels with numpy's stable sort."""
    ptr, C = offsets(GATED_SIZES), GATED_C
    g = labels + np.repeat(np.arange(len(GATED_SIZES)), GATED_SIZES) * C
    counts = np.bincount(g, minlength=len(GATED_SIZES) * C).astype(np.int64)
    return [counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.argsort(g, kind="stable").astype(np.int64),
            np.array([-1, -1], np.int64)]


def pool_inputs(seed, d=20, dp=2):
    rng = np.random.RandomState(920 + seed)
    n = sum(GATED_SIZES)
    lab = gated_labels(seed)
    _, offs, order, _ = sort_reference(lab)
    K = np.exp(-rng.rand(sum(v * v for v in GATED_SIZES)) * 3).astype(np.float32)
    return [rng.randn(n, d).astype(np.float32), rng.rand(n, dp).astype(np.float32), order, offs, K]


def pool_reference(F, P, order, offs, K):
    ptr, C = offsets(GATED_SIZES), GATED_C
    kptr = offsets([v * v for v in GATED_SIZES])
    G = len(GATED_SIZES) * C
    sf = np.stack([F[order[offs[g]:offs[g + 1]]].astype(np.float64).mean(0) for g in range(G)]).astype(np.float32)
    spos = np.stack([P[order[offs[g]:offs[g + 1]]].astype(np.float64).mean(0) for g in range(G)]).astype(np.float32)
    intra, st = np.full(G, np.nan), []
    for s, n_s in enumerate(GATED_SIZES):
        K_s = K[kptr[s]:kptr[s + 1]].reshape(n_s, n_s).astype(np.float64)
        for c in range(C):
            idx = order[offs[s * C + c]:offs[s * C + c + 1]] - ptr[s]
            if idx.size > 1:
                blk = K_s[np.ix_(idx, idx)]
                intra[s * C + c] = (blk.sum() - np.trace(blk)) / (idx.size * (idx.size - 1))
        v = K_s.reshape(-1)
        st.append([v.mean(), v.std(ddof=1), v.min(), v.max(), np.sort(v)[(v.size - 1) // 2]])
    st = np.array(st, np.float64)

    def check(got):
        return (sg.diff(got[0], sf, "super_f", atol=TOL) + sg.diff(got[1], spos, "super_p", atol=TOL) +
                sg.diff(got[2], intra, "intra", atol=1e-6) + sg.diff(got[3], st, "k_stats", atol=2e-5))
    return check


CASES = {}


def case(name, covers, nonsync=False):
    def reg(fn):
        CASES[name] = dict(build=fn, covers=tuple(covers), nonsync=nonsync, calls=2 if nonsync else 1)
        return fn
    return reg


@case("c_entry_segment_sort_segmented", ["mmf_segment_sort_segmented"], nonsync=True)
def _():
    import multimodal_fusion_amd as m
    ptr, C, S = offsets(GATED_SIZES), GATED_C, len(GATED_SIZES)
    hptr = torch.tensor(ptr)

    def entry(labels):
        dev = labels.device
        counts = torch.empty((S * C,), dtype=torch.int64, device=dev)
        offs = torch.empty((S * C + 1,), dtype=torch.int64, device=dev)
        order = torch.empty((ptr[-1],), dtype=torch.int64, device=dev)
        status = torch.empty((2,), dtype=torch.int64, device=dev)
        p = hptr.clone()                                # a host table that dies with the call
        rc = m._lib.lib().mmf_segment_sort_segmented(m.ops._p(labels), ptr[-1], hp(p), S, C, m.ops._p(counts), m.ops._p(offs),
                                                     m.ops._p(order), m.ops._p(status), dev.index or 0, m.ops._stream(dev))
        m._lib.check(rc, "mmf_segment_sort_segmented")
        return counts, offs, order, status
    return dict(entry=entry, make_inputs=seeded(lambda s: [gated_labels(s)]), reference=sort_reference)


@case("c_entry_super_patches_segmented", ["mmf_super_patches_segmented"], nonsync=True)
def _():
    import multimodal_fusion_amd as m
    ptr, C, S = offsets(GATED_SIZES), GATED_C, len(GATED_SIZES)
    hptr = torch.tensor(ptr)

    def entry(F, P, order, offs, K):
        dev = F.device
        sf = torch.empty((S * C, F.shape[1]), dtype=torch.float32, device=dev)
        spos = torch.empty((S * C, P.shape[1]), dtype=torch.float32, device=dev)
        intra = torch.empty((S * C,), dtype=torch.float64, device=dev)
        st = torch.empty((S, 5), dtype=torch.float64, device=dev)
        p = hptr.clone()
        o = m.ops
        rc = m._lib.lib().mmf_super_patches_segmented(o._p(F), o._p(P), ptr[-1], F.shape[1], P.shape[1], hp(p), S, C, o._p(order), o._p(offs),
                                                      o._p(K), o._p(sf), o._p(spos), o._p(intra), o._p(st), dev.index or 0, o._stream(dev))
        m._lib.check(rc, "mmf_super_patches_segmented")
        return sf, spos, intra, st
    return dict(entry=entry, make_inputs=seeded(pool_inputs), reference=pool_reference)


@case("segment_sort_segmented", ["segment_sort_segmented"], nonsync=True)
def _():
    ptr = offsets(GATED_SIZES)
    return dict(entry=lambda labels: sp().segment_sort_segmented(labels, GATED_C, ptr=ptr), make_inputs=seeded(lambda s: [gated_labels(s)]),
                reference=sort_reference)


@case("segment_sort_segmented_60000_slides", ["segment_sort_segmented"], nonsync=True)
def _():
    # host tables of more than 1 MiB would wait for the stream if they were copied out of pageable memory (3 x 8 bytes per chunk)
    S, C = 60000, 3
    sizes = np.random.RandomState(11).randint(3, 7, S)
    ptr = offsets(sizes)

    def labels(seed):
        rng = np.random.RandomState(940 + seed)
        return np.concatenate([covering_labels(rng, int(n), C) for n in sizes])

    def reference(lab):
        g = lab + np.repeat(np.arange(S), sizes) * C
        counts = np.bincount(g, minlength=S * C).astype(np.int64)
        return [counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.argsort(g, kind="stable").astype(np.int64),
                np.array([-1, -1], np.int64)]
    assert S * 3 * 8 > 1 << 20
    return dict(entry=lambda lab: sp().segment_sort_segmented(lab, C, ptr=ptr), make_inputs=seeded(lambda s: [labels(s)]), reference=reference)


@case("pool_super_patches_segmented", ["pool_super_patches_segmented"], nonsync=True)
def _():
    ptr = offsets(GATED_SIZES)
    return dict(entry=lambda F, P, order, offs, K: sp().pool_super_patches_segmented(F, P, order, offs, GATED_C, ptr=ptr, K_flat=K),
                make_inputs=seeded(lambda s: pool_inputs(s, d=70, dp=3)), reference=pool_reference)


def _aggregate_check(F, P, ptr, sizes, C, lam):
    """The plain mirror on every slide of the truth (made on the idle default stream, before the gate)."""
    Fd, Pd = T(F).cuda(), T(P).cuda()
    plain = [pp().aggregate_wsi_super_patches(Fd[ptr[s]:ptr[s + 1]], Pd[ptr[s]:ptr[s + 1]], C, *lam) for s in range(len(sizes))]
    want_f = torch.cat([q[0] for q in plain]).cpu().numpy()
    want_p = torch.cat([q[1] for q in plain]).cpu().numpy()
    want_k = torch.cat([q[3].reshape(-1) for q in plain]).cpu().numpy()

    def check(sf, spos, stats, K_flat):
        out = sg.diff(sf, want_f, "super_features") + sg.diff(spos, want_p, "super_positions")
        if K_flat is not None:
            out += sg.diff(K_flat, want_k, "K_flat")
        out += [f"slide {s}: stats differ" for s in range(len(sizes)) if not same_stats(stats[s], plain[s][2])]
        return out
    return check


@case("aggregate_wsi_super_patches_segmented", ["aggregate_wsi_super_patches_segmented"])
def _():
    sizes, C, d, lam = [60, 45, 130], 5, 32, (0.9, 0.4)
    ptr = offsets(sizes)

    def inputs(seed):
        return [np.concatenate([_clustered(n, d, 950 + 10 * seed + s) for s, n in enumerate(sizes)]),
                np.random.RandomState(970 + seed).rand(ptr[-1], 2).astype(np.float32)]

    def reference(F, P):
        check = _aggregate_check(F, P, ptr, sizes, C, lam)
        return lambda got: check(got[0], got[1], got[2], got[3])
    return dict(entry=lambda F, P: sp().aggregate_wsi_super_patches_segmented(F, P, C, *lam, ptr=ptr), make_inputs=seeded(inputs),
                reference=reference)


@case("build_cohort_hypergraphs", ["build_cohort_hypergraphs"])
def _():
    sizes, tmas, C, d, lam = [60, 45, 130], [16, 24, 16], 5, 32, (0.9, 0.4)
    wp, tp = offsets(sizes), offsets(tmas)

    def inputs(seed):
        return [np.concatenate([_clustered(n, d, 980 + 10 * seed + s) for s, n in enumerate(sizes)]),
                np.random.RandomState(990 + seed).rand(wp[-1], 2).astype(np.float32),
                np.concatenate([_clustered(m, d, 1000 + 10 * seed + s) for s, m in enumerate(tmas)])]

    def reference(F, P, tma):
        check = _aggregate_check(F, P, wp, sizes, C, lam)
        Td = T(tma).cuda()

        def chk(got):
            out = check(got["super_features"], got["super_positions"], [st["wsi_aggregation"] for st in got["stats"]], None)
            ep, node_ptr = got["edge_ptr"], got["node_ptr"]
            for s in range(len(sizes)):
                sf = T(got["super_features"][s * C:(s + 1) * C]).cuda()
                S_s, _ = pp().compute_wsi_tma_similarity(sf, None, Td[tp[s]:tp[s + 1]], lam[0])
                lab, _ = pp().group_by_similarity(S_s, 3)
                ei, ew, _ = pp().build_hypergraph_knn_kmeans(sf, Td[tp[s]:tp[s + 1]], lab, 3, 4)
                out += sg.diff(got["group_labels"][s * C:(s + 1) * C], lab, f"labels of slide {s}")
                out += sg.diff(got["edge_index"][:, ep[s]:ep[s + 1]] - node_ptr[s], ei.cpu().numpy(), f"edges of slide {s}")
                out += sg.diff(got["edge_weights"][ep[s]:ep[s + 1]], ew.cpu().numpy(), f"weights of slide {s}")
            return out
        return chk
    return dict(entry=lambda F, P, tma: co().build_cohort_hypergraphs(F, P, tma, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=3,
                                                                      hypergraph_k=3, num_hyperedges=4, lambda_h=lam[0], lambda_g=lam[1]),
                make_inputs=seeded(inputs), reference=reference)


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
    public = set()
    for mod in (sp(), co()):
        public |= {n for n, f in inspect.getmembers(mod, inspect.isfunction) if f.__module__ == mod.__name__ and not n.startswith("_")}
    public -= {"group_plan"}                                        # a pure function of Python lists: no tensor, no stream
    covered = {f for c in CASES.values() for f in c["covers"]}
    assert public <= covered, sorted(public - covered)
    assert set(mmf._lib.EXPORTS_POOL) == set(SYNC_POOL) <= covered
    # every entry and function documented as not synchronising is gated as such
    none = {e for e, (sync, _) in SYNC_POOL.items() if sync == "none"} | {"segment_sort_segmented", "pool_super_patches_segmented"}
    gated_none = {f for c in CASES.values() if c["nonsync"] for f in c["covers"]}
    assert none <= gated_none, sorted(none - gated_none)
