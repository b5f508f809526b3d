"""Ragged-width segmented KMeans on the GPU (kmeans_ragged.*, include/ext/mmf_hg_kmeans_ragged.h): one fit for
blocks that each have a feature width of their own.

Every comparison is exact: torch.equal on labels and seeds, the raw bits of the centres, == on every info field except
'lockstep_iterations' (which is the group's).  The yardstick is the UNCHANGED plain fit (ops.kmeans_fit / kmeans.kmeans_fit_predict)
on each block, which tests/test_gpu_kmeans.py pins to scikit-learn and to oracle/kmeans_restate.py.

  1. seven blocks, rows {12 .. 300} x widths {1 .. 130}, stored out of order with gaps, k = 3 and 10: every block is the plain fit;
  2. one width: the segmented entry's results;
  3. a block that relocates empty clusters among blocks of other widths;
  4. several lockstep groups: by the segment limit and by the padding rule, both as ragged_groups says;
  5. the labels of the CPU restatement on case 1's data;
  6. group_by_similarity_segmented makes ONE ragged call for five widths and equals the plain mirror per slide; so does the cohort
     pipeline;
  7. the stream contract of the entry and of both Python functions behind a closed gate (tests/streamgate.py).
"""
import ctypes
import functools
import inspect
import json
import os
import re
import sys
import warnings
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "Ragged KMeans entries"
CALL = "until the call returns"
SYNC_KMEANS_RAGGED = {
    "mmf_kmeans_fit_ragged": ("per iteration", CALL),
    "mmf_kmeans_ragged_groups": ("host only: no device, no stream", CALL),
}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def kr():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.kmeans_ragged")


def km():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.kmeans")


def pp():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.build_hypergraph.preprocess_hypergraph")


def wt():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.wsi_tma_similarity")


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def blobs(n, d, seed):
    """Blob-structured rows in (0, 1), as the rows of a WSI x TMA similarity block are."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.15, 0.85, (max(2, min(6, n // 5)), d))
    x = c[rng.integers(0, len(c), n)] + rng.normal(0, 0.04, (n, d))
    return np.clip(x, 0.01, 0.99).astype(np.float32)


def flat(blocks, place, gap=3):
    """The blocks in one flat buffer, stored in the order `place` with `gap` NaN values before each: (V, xoff per block).  A stray
    read of a gap poisons the result; it cannot fault."""
    xoff, parts, at = [0] * len(blocks), [], 0
    for s in place:
        parts.append(np.full(gap, np.nan, np.float32))
        at += gap
        xoff[s] = at
        parts.append(blocks[s].reshape(-1))
        at += blocks[s].size
    parts.append(np.full(gap, np.nan, np.float32))
    return np.concatenate(parts), xoff


def strip(info):
    d = dict(info)
    d.pop("lockstep_iterations")
    return d


def plain_fit(mmf, block, k):
    """ops.kmeans_fit on one block with scikit-learn's stream: (labels, centres, info, seeds) on the device."""
    f1, u1 = km().sklearn_stream(42, 10, k, block.shape[0])
    return mmf.ops.kmeans_fit(block, k, f1, u1, return_seeds=True)


def check_blocks(mmf, blocks, k, labels, centres, info, seeds=None, plain=None, what=""):
    """Results in block order against the plain fit of every block; returns nothing, raises with every mismatch."""
    ptr, bad = offsets([b.shape[0] for b in blocks]), []
    assert labels.shape == (ptr[-1],) and labels.dtype == torch.int64 and len(centres) == len(info) == len(blocks)
    for s, b in enumerate(blocks):
        l1, c1, i1, s1 = plain[s] if plain is not None else plain_fit(mmf, T(b).cuda(), k)
        tag = f"{what}block {s} ({b.shape[0]} x {b.shape[1]}, k = {k})"
        if not torch.equal(labels[ptr[s]:ptr[s + 1]], l1):
            bad.append(f"{tag}: labels differ")
        if tuple(centres[s].shape) != (k, b.shape[1]) or not torch.equal(bits(centres[s]), bits(c1)):
            bad.append(f"{tag}: centres differ")
        if seeds is not None and not torch.equal(seeds[s], s1):
            bad.append(f"{tag}: seeds differ")
        if strip(info[s]) != strip(i1):
            bad.append(f"{tag}: info {strip(info[s])} != {strip(i1)}")
    assert not bad, "; ".join(bad[:6])


def centre_views(cen_flat, widths, k):
    off = offsets([k * w for w in widths])
    return [cen_flat[off[s]:off[s + 1]].view(k, widths[s]) for s in range(len(widths))]


# ---------------------------------------------------------------------------------------------------
# 1. ragged widths against the plain fit (and 5: against the CPU restatement)
# ---------------------------------------------------------------------------------------------------
# the widths cover the 32-chunk and 64-strip edges (31 / 32 / 33, 65, 130 = three strips, 1); 257 rows are two column-sum blocks;
# 12 rows with k = 10 are nearly one point per cluster.  SEEDS: per block, the first data seed from 1000 on for which
# oracle/kmeans_restate.py reports no ambiguous draw and no ambiguous trial choice for k = 3 and k = 10 (checked on the CPU; test 5
# asserts it again).
ROWS = [12, 33, 40, 64, 100, 257, 300]
WIDTHS = [33, 130, 1, 65, 7, 31, 32]
SEEDS = [1001, 1002, 1002, 1000, 1000, 1002, 1000]
PLACE = [4, 1, 6, 0, 3, 5, 2]                       # storage order in the flat buffer: not the call order, not sorted by anything


@functools.lru_cache(maxsize=None)
def case1_blocks():
    return tuple(blobs(n, d, s) for n, d, s in zip(ROWS, WIDTHS, SEEDS))


_PLAIN1 = {}


def case1_plain(mmf, k):
    """The plain fit of every block of case 1, computed once per k and shared by the tests below."""
    if k not in _PLAIN1:
        _PLAIN1[k] = [plain_fit(mmf, T(b).cuda(), k) for b in case1_blocks()]
    return _PLAIN1[k]


@pytest.mark.parametrize("k", [3, 10])
def test_ragged_widths_equal_the_plain_fit_of_every_block(mmf, k):
    blocks = list(case1_blocks())
    V, xoff = flat(blocks, PLACE)
    assert np.isnan(V).sum() == 3 * (len(blocks) + 1) and sorted(xoff) != xoff
    Vd = T(V).cuda()
    plain = case1_plain(mmf, k)
    # the thin binding, segments in the caller's order: groups as they fall (internal widths 160 and 32 for k = 10)
    first, u = km().segment_streams(42, 10, k, ROWS)
    labels, cen, info, seeds = kr().kmeans_fit_ragged(Vd, xoff, ROWS, WIDTHS, k, first, u, return_seeds=True)
    assert cen.shape == (k * sum(WIDTHS),) and seeds.shape == (len(ROWS), 10, k)
    check_blocks(mmf, blocks, k, labels, centre_views(cen, WIDTHS, k), info, seeds, plain, "kmeans_fit_ragged: ")
    bounds, _ = kr().ragged_groups(ROWS, WIDTHS, k)
    for a, b in zip(bounds[:-1], bounds[1:]):
        assert len({i["lockstep_iterations"] for i in info[a:b]}) == 1, (a, b)
    # the driver: sorted by internal width, labels and centres back in the caller's order
    labels2, centres2, inertia2, info2 = kr().kmeans_fit_predict_ragged(Vd, k, rows=ROWS, widths=WIDTHS, xoff=xoff, return_info=True)
    check_blocks(mmf, blocks, k, labels2, centres2, info2, None, plain, "kmeans_fit_predict_ragged: ")
    assert inertia2.dtype == np.float64 and inertia2.tolist() == [i["inertia"] for i in info2]
    for s, b in enumerate(blocks):                   # and the public plain function
        l1, c1, in1 = km().kmeans_fit_predict(T(b).cuda(), k)
        a = offsets(ROWS)[s]
        assert torch.equal(labels2[a:a + ROWS[s]], l1) and torch.equal(bits(centres2[s]), bits(c1)) and inertia2[s] == in1, s


@pytest.mark.parametrize("k", [3, 10])
def test_labels_equal_the_cpu_restatement(mmf, k):
    """Against the CPU contract (oracle/kmeans_restate.py), every block of case 1; none is skipped."""
    import oracle.kmeans_restate as restate
    blocks = list(case1_blocks())
    V, xoff = flat(blocks, PLACE)
    labels, _, _, info = kr().kmeans_fit_predict_ragged(T(V).cuda(), k, rows=ROWS, widths=WIDTHS, xoff=xoff, return_info=True)
    lab, ptr = labels.cpu().numpy(), offsets(ROWS)
    for s, b in enumerate(blocks):
        rinfo = {}
        want = restate.kmeans_fit_predict(b, k, info=rinfo)
        assert not rinfo["ambiguous"], f"block {s}: the restatement's seeding has ambiguous decisions with data seed {SEEDS[s]}: {rinfo['ambiguous']}"
        assert info[s]["ambiguous_draws"] == 0 and info[s]["ambiguous_trials"] == 0, (s, info[s])
        assert np.array_equal(lab[ptr[s]:ptr[s + 1]], want), f"block {s} ({ROWS[s]} x {WIDTHS[s]}, k = {k}): labels differ from the restatement"


# ---------------------------------------------------------------------------------------------------
# 2. one width: the segmented entry's results
# ---------------------------------------------------------------------------------------------------
def test_one_width_equals_the_segmented_fit(mmf):
    rows = [40, 100, 64, 33, 257, 90]
    blocks = [blobs(n, 64, 2000 + s) for s, n in enumerate(rows)]
    X = T(np.concatenate(blocks)).cuda()
    ptr = offsets(rows)
    for k in (4, 10):
        want_l, want_c, want_in, want_info = km().kmeans_fit_predict_segmented(X, k, ptr=ptr, return_info=True)
        labels, centres, inertia, info = kr().kmeans_fit_predict_ragged(X.reshape(-1), k, rows=rows, widths=[64] * 6, return_info=True)
        assert torch.equal(labels, want_l) and np.array_equal(inertia.view(np.uint64), want_in.view(np.uint64))
        for s in range(6):
            assert torch.equal(bits(centres[s]), bits(want_c[s])) and strip(info[s]) == strip(want_info[s]), (k, s)
        assert kr().ragged_groups(rows, [64] * 6, k) == ([0, 6], [64] * 6)


# ---------------------------------------------------------------------------------------------------
# 3. relocation of empty clusters inside a ragged call
# ---------------------------------------------------------------------------------------------------
def lattice():
    """20 x 2 with duplicate rows: empty clusters, KM_RELOC (tests/test_gpu_kmeans_segmented.py::_data('lattice'), seed 27)."""
    r = np.random.default_rng(27)
    r.choice([20, 30, 50]); r.choice([6, 8, 12])
    return r.integers(0, 4, (20, 2)).astype(np.float32) + r.standard_normal((20, 2)).astype(np.float32) * float(r.choice([0, 0.01, 0.3]))


def test_a_relocating_block_among_blocks_of_other_widths(mmf):
    import oracle.kmeans_restate as restate
    k = 12
    blocks = [blobs(100, 40, 3000), lattice(), blobs(37, 70, 3001), lattice(), blobs(64, 5, 3002)]
    rows, widths = [b.shape[0] for b in blocks], [b.shape[1] for b in blocks]
    V, xoff = flat(blocks, [2, 0, 4, 1, 3])
    Vd = T(V).cuda()
    first, u = km().segment_streams(42, 10, k, rows)
    labels, cen, info, seeds = kr().kmeans_fit_ragged(Vd, xoff, rows, widths, k, first, u, return_seeds=True)
    check_blocks(mmf, blocks, k, labels, centre_views(cen, widths, k), info, seeds)
    labels2, centres2, _, info2 = kr().kmeans_fit_predict_ragged(Vd, k, rows=rows, widths=widths, xoff=xoff, return_info=True)
    check_blocks(mmf, blocks, k, labels2, centres2, info2)
    lat = labels2[100:120].cpu().numpy()
    assert len(np.unique(blocks[1], axis=0)) < 20                       # duplicate rows: restarts seed the same point twice
    assert np.array_equal(lat, restate.kmeans_fit_predict(blocks[1], k))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from sklearn.cluster import KMeans
        assert np.array_equal(lat, KMeans(n_clusters=k, random_state=42, n_init=10).fit_predict(blocks[1]))


# ---------------------------------------------------------------------------------------------------
# 4. several lockstep groups
# ---------------------------------------------------------------------------------------------------
def test_groups_by_the_segment_limit(mmf):
    """170 blocks with k = 10: n_seg * n_init * k = 17000 > 16384, so 163 + 7 segments."""
    k = 10
    rng = np.random.default_rng(4)
    rows = [int(v) for v in rng.integers(12, 21, 170)]
    widths = [(5, 40, 70)[s % 3] for s in range(170)]
    blocks = [blobs(n, d, 4000 + s) for s, (n, d) in enumerate(zip(rows, widths))]
    V, xoff = flat(blocks, list(range(170)), gap=0)
    Vd = T(V).cuda()
    plain = [plain_fit(mmf, T(b).cuda(), k) for b in blocks]
    bounds, ds = kr().ragged_groups(rows, widths, k)
    assert bounds == [0, 163, 170] and set(ds) == {96}
    first, u = km().segment_streams(42, 10, k, rows)
    labels, cen, info, seeds = kr().kmeans_fit_ragged(Vd, xoff, rows, widths, k, first, u, return_seeds=True)
    check_blocks(mmf, blocks, k, labels, centre_views(cen, widths, k), info, seeds, plain)
    for a, b in zip(bounds[:-1], bounds[1:]):
        assert len({i["lockstep_iterations"] for i in info[a:b]}) == 1, (a, b)
    # the driver sorts by internal width: 57 blocks of 32, 57 of 64, 56 of 96, cut after 163
    order = np.argsort((np.array(widths) + 31) // 32, kind="stable")
    b2, ds2 = kr().ragged_groups(np.array(rows)[order], np.array(widths)[order], k)
    assert b2 == [0, 163, 170] and ds2[:163].count(96) == 163 and set(ds2[163:]) == {96}
    labels2, centres2, _, info2 = kr().kmeans_fit_predict_ragged(Vd, k, rows=rows, widths=widths, return_info=True)
    check_blocks(mmf, blocks, k, labels2, centres2, info2, None, plain)


def test_groups_by_the_padding_rule(mmf):
    """Widths 8, 8, 2000, 8 with 40 rows each: 120 rows x 2016 is more than twice 2 x 40 x 32 + 40 x 2016, so the wide block
    starts a group; the last block joins it (80 x 2016 <= 2 x (40 x 2016 + 40 x 32))."""
    k = 5
    rows, widths = [40] * 4, [8, 8, 2000, 8]
    blocks = [blobs(n, d, 5000 + s) for s, (n, d) in enumerate(zip(rows, widths))]
    V, xoff = flat(blocks, [3, 2, 1, 0])
    Vd = T(V).cuda()
    assert kr().ragged_groups(rows, widths, k) == ([0, 2, 4], [32, 32, 2016, 2016])
    first, u = km().segment_streams(42, 10, k, rows)
    labels, cen, info, seeds = kr().kmeans_fit_ragged(Vd, xoff, rows, widths, k, first, u, return_seeds=True)
    check_blocks(mmf, blocks, k, labels, centre_views(cen, widths, k), info, seeds)
    assert info[0]["lockstep_iterations"] == info[1]["lockstep_iterations"] and info[2]["lockstep_iterations"] == info[3]["lockstep_iterations"]
    # sorted: 8, 8, 8 | 2000
    assert kr().ragged_groups([40] * 4, [8, 8, 8, 2000], k) == ([0, 3, 4], [32, 32, 32, 2016])
    labels2, centres2, _, info2 = kr().kmeans_fit_predict_ragged(Vd, k, rows=rows, widths=widths, xoff=xoff, return_info=True)
    check_blocks(mmf, blocks, k, labels2, centres2, info2)


# ---------------------------------------------------------------------------------------------------
# 6. the grouping step and the cohort pipeline
# ---------------------------------------------------------------------------------------------------
def _clustered(n, d, seed, centres=5):
    rng = np.random.RandomState(seed)
    c = rng.randn(centres, d) * (0.9 / np.sqrt(d))
    return (c[rng.randint(0, centres, n)] + rng.randn(n, d) * (0.25 / np.sqrt(d))).astype(np.float32)


GROUP_SIZES = [(30, 16), (25, 24), (40, 70), (35, 33), (28, 5)]          # five slides, five TMA widths


class Spy:
    """Counts the calls of the bound library functions and forwards them."""

    def __init__(self, monkeypatch, L, names):
        self.calls = {n: 0 for n in names}
        for n in names:
            monkeypatch.setattr(L, n, self._wrap(n, getattr(L, n)), raising=True)

    def _wrap(self, name, fn):
        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call


def test_grouping_is_one_ragged_call_and_equals_the_plain_mirror(mmf, monkeypatch):
    assert pp().KMEANS_BACKEND == "device"
    d, G = 32, 4
    wp, tp = offsets([n for n, _ in GROUP_SIZES]), offsets([m for _, m in GROUP_SIZES])
    wsi = T(np.concatenate([_clustered(n, d, 100 + s) for s, (n, _) in enumerate(GROUP_SIZES)])).cuda()
    tma = T(np.concatenate([_clustered(m, d, 200 + s) for s, (_, m) in enumerate(GROUP_SIZES)])).cuda()
    S_flat, s_ptr, _ = wt().compute_wsi_tma_similarity_segmented(wsi, None, tma, lambda_h=0.9, wsi_ptr=wp, tma_ptr=tp)
    spy = Spy(monkeypatch, mmf._lib.lib(), ["mmf_kmeans_fit_ragged", "mmf_kmeans_fit_segmented", "mmf_kmeans_fit"])
    lab, st, info = wt().group_by_similarity_segmented(S_flat, G, wsi_ptr=wp, tma_ptr=tp)
    assert spy.calls == {"mmf_kmeans_fit_ragged": 1, "mmf_kmeans_fit_segmented": 0, "mmf_kmeans_fit": 0}
    assert lab.shape == (wp[-1],) and lab.dtype == np.int32 and info["kmeans_backend"] == "device"
    for s, (n_s, m_s) in enumerate(GROUP_SIZES):
        blk = wt().similarity_block(S_flat, s_ptr, GROUP_SIZES, s)
        want_lab, want_st = pp().group_by_similarity(blk, G)
        assert np.array_equal(lab[wp[s]:wp[s + 1]], want_lab) and st[s] == want_st, s
        assert sum(st[s]["group_sizes"]) == n_s
        _, _, _, i1 = km().kmeans_fit_predict(blk, G, return_info=True)
        assert (info["ambiguous_draws"][s], info["ambiguous_trials"][s]) == (i1["ambiguous_draws"], i1["ambiguous_trials"]), s
    # one distinct width keeps the segmented call
    before = dict(spy.calls)
    one = [(30, 16), (25, 16)]
    S1 = S_flat[:30 * 16 + 25 * 16].clone()
    wt().group_by_similarity_segmented(S1, G, wsi_ptr=offsets([n for n, _ in one]), tma_ptr=offsets([m for _, m in one]))
    assert spy.calls["mmf_kmeans_fit_segmented"] == before["mmf_kmeans_fit_segmented"] + 1
    assert spy.calls["mmf_kmeans_fit_ragged"] == before["mmf_kmeans_fit_ragged"]


def _same_stats(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def test_cohort_pipeline_equals_the_chain_of_plain_mirrors(mmf, monkeypatch):
    sizes, tmas = [60, 150, 90, 120, 75], [16, 24, 70, 33, 5]
    C, G, k, H, d, lam_h, lam_g = 8, 3, 3, 4, 32, 0.9, 0.4
    wp, tp = offsets(sizes), offsets(tmas)
    F = T(np.concatenate([_clustered(n, d, 500 + s) for s, n in enumerate(sizes)])).cuda()
    P = T(np.concatenate([np.random.RandomState(600 + s).rand(n, 2).astype(np.float32) for s, n in enumerate(sizes)])).cuda()
    tma = T(np.concatenate([_clustered(m, d, 700 + s) for s, m in enumerate(tmas)])).cuda()
    spy = Spy(monkeypatch, mmf._lib.lib(), ["mmf_kmeans_fit_ragged"])
    out = mmf.build_cohort_hypergraphs(F, P, tma, wsi_ptr=wp, tma_ptr=tp, num_wsi_super_patches=C, num_groups=G, hypergraph_k=k,
                                       num_hyperedges=H, lambda_h=lam_h, lambda_g=lam_g)
    assert spy.calls["mmf_kmeans_fit_ragged"] == 1                     # the grouping step; the other KMeans steps have one width each
    ep, node_ptr, s_ptr = out["edge_ptr"].tolist(), out["node_ptr"].tolist(), out["s_ptr"]
    for s in range(len(sizes)):
        w_s, p_s, t_s = F[wp[s]:wp[s + 1]], P[wp[s]:wp[s + 1]], tma[tp[s]:tp[s + 1]]
        sf, spos, agg, _ = pp().aggregate_wsi_super_patches(w_s, p_s, C, lam_h, lam_g)
        S_s, sim = pp().compute_wsi_tma_similarity(sf, spos, t_s, lam_h, lam_g)
        lab, grp = pp().group_by_similarity(S_s, G)
        ei, ew, hg = pp().build_hypergraph_knn_kmeans(sf, t_s, lab, k, H)
        assert torch.equal(bits(out["S_flat"][int(s_ptr[s]):int(s_ptr[s + 1])]), bits(S_s).reshape(-1)), s
        assert np.array_equal(out["group_labels"][s * C:(s + 1) * C], lab), s
        assert torch.equal(out["edge_index"][:, ep[s]:ep[s + 1]] - node_ptr[s], ei), s
        assert torch.equal(bits(out["edge_weights"][ep[s]:ep[s + 1]]), bits(ew)), s
        want = {"wsi_aggregation": agg, "similarity": sim, "grouping": grp, "hypergraph": hg}
        assert _same_stats(out["stats"][s], want), (s, out["stats"][s], want)


# ---------------------------------------------------------------------------------------------------
# 7. the stream contract, and the lists that name the entries
# ---------------------------------------------------------------------------------------------------
GATED_ROWS, GATED_WIDTHS, GATED_K = [40, 33, 64, 20], [16, 70, 5, 33], 4


def seeded(fn):
    return lambda which: [t if isinstance(t, torch.Tensor) else T(np.ascontiguousarray(t)) for t in fn(1 if which == "truth" else 2)]


def _gated_values(seed):
    return np.concatenate([blobs(n, d, 6000 + 10 * seed + s).reshape(-1) for s, (n, d) in enumerate(zip(GATED_ROWS, GATED_WIDTHS))])


def _gated_reference(V):
    """The CPU restatement's labels per block (the gated data's seeding may hold ambiguous decisions: then only the partition
    sizes are pinned, and the comparison with the idle call's bits carries the contract)."""
    import oracle.kmeans_restate as restate
    xoff = offsets([n * d for n, d in zip(GATED_ROWS, GATED_WIDTHS)])
    want = []
    for s, (n, d) in enumerate(zip(GATED_ROWS, GATED_WIDTHS)):
        rinfo = {}
        lab = restate.kmeans_fit_predict(V[xoff[s]:xoff[s + 1]].reshape(n, d), GATED_K, info=rinfo)
        want.append(None if rinfo["ambiguous"] else lab)
    ptr = offsets(GATED_ROWS)

    def chk(got):
        labels = np.asarray(got[0])
        out = []
        for s, w in enumerate(want):
            part = labels[ptr[s]:ptr[s + 1]]
            if part.min() < 0 or part.max() >= GATED_K:
                out.append(f"block {s}: labels outside [0, k)")
            elif w is not None and not np.array_equal(part, w):
                out.append(f"block {s}: labels differ from the restatement")
        return out
    return chk


CASES = {}


def case(name, covers):
    def reg(fn):
        CASES[name] = dict(build=fn, covers=tuple(covers))
        return fn
    return reg


@case("c_entry_kmeans_fit_ragged", ["mmf_kmeans_fit_ragged"])
def _():
    import multimodal_fusion_amd as m
    n_seg, k = len(GATED_ROWS), GATED_K
    first, u = km().segment_streams(42, 10, k, GATED_ROWS)
    xoff = offsets([n * d for n, d in zip(GATED_ROWS, GATED_WIDTHS)])[:-1]

    def hp(a):
        return ctypes.c_void_p(a.ctypes.data)

    def entry(V):
        labels = torch.empty(sum(GATED_ROWS), dtype=torch.int64, device=V.device)
        cen = torch.empty(k * sum(GATED_WIDTHS), dtype=torch.float32, device=V.device)
        seeds = torch.empty((n_seg, 10, k), dtype=torch.int64, device=V.device)
        info = np.zeros((n_seg, 27), np.float64)
        tabs = [np.array(t, dtype=np.int64) for t in (xoff, GATED_ROWS, GATED_WIDTHS)]      # host tables that die with the call
        f, uu = first.copy(), u.copy()
        rc = m._lib.lib().mmf_kmeans_fit_ragged(m.ops._p(V), V.numel(), hp(tabs[0]), hp(tabs[1]), hp(tabs[2]), n_seg, k, 10, u.shape[2], hp(f),
                                                hp(uu), 300, 1e-4, m.ops._p(labels), m.ops._p(cen), m.ops._p(seeds), hp(info),
                                                V.device.index or 0, m.ops._stream(V.device))
        m._lib.check(rc, "mmf_kmeans_fit_ragged")
        return labels, cen, seeds, T(info[:, :6].copy())
    return dict(entry=entry, make_inputs=seeded(lambda s: [_gated_values(s)]), reference=_gated_reference)


@case("kmeans_fit_ragged", ["kmeans_fit_ragged"])
def _():
    first, u = km().segment_streams(42, 10, GATED_K, GATED_ROWS)
    xoff = offsets([n * d for n, d in zip(GATED_ROWS, GATED_WIDTHS)])[:-1]

    def entry(V):
        labels, cen, info, seeds = kr().kmeans_fit_ragged(V, xoff, GATED_ROWS, GATED_WIDTHS, GATED_K, first, u, return_seeds=True)
        return labels, cen, seeds, [strip(i) for i in info]
    return dict(entry=entry, make_inputs=seeded(lambda s: [_gated_values(s)]), reference=_gated_reference)


@case("kmeans_fit_predict_ragged", ["kmeans_fit_predict_ragged"])
def _():
    def entry(V):
        labels, centres, inertia, info = kr().kmeans_fit_predict_ragged(V, GATED_K, rows=GATED_ROWS, widths=GATED_WIDTHS, return_info=True)
        return labels, centres, T(inertia), [strip(i) for i in info]
    return dict(entry=entry, make_inputs=seeded(lambda s: [_gated_values(s)]), reference=_gated_reference)


@pytest.mark.parametrize("name", list(CASES))
def test_entry_behind_a_closed_gate(mmf, name):
    c = CASES[name]
    kw = c["build"]()
    try:
        res = sg.run_gated(kw["entry"], kw["make_inputs"], kw["reference"], name=name)
    except RuntimeError as e:
        if "HIP error" in str(e) or "(code -3)" in str(e):          # a fault of the device: nothing more is started on it
            pytest.exit(f"{name}: the HIP runtime reported a failure, stopping the run: {e}", returncode=3)
        raise
    assert res.gate_ms >= 0.9 * sg.GATE_MIN_MS, f"{name}: the gate lasted {res.gate_ms:.1f} ms"


def _declared(path):
    with open(os.path.join(ROOT, "include", path)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


def _integration_rows():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        section = re.split(r"^## [0-9. ]*Ragged KMeans entries$", f.read(), 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_every_public_function_and_the_entry_have_a_case(mmf):
    mod = kr()
    public = {n for n, f in inspect.getmembers(mod, inspect.isfunction) if f.__module__ == mod.__name__ and not n.startswith("_")}
    public -= {"ragged_groups"}                                     # host only: no tensor, no stream
    covered = {f for c in CASES.values() for f in c["covers"]}
    assert public <= covered, sorted(public - covered)
    exports = list(mmf._lib.EXPORTS_KMEANS_RAGGED)
    assert set(exports) == _declared(os.path.join("ext", "mmf_hg_kmeans_ragged.h")) == set(SYNC_KMEANS_RAGGED)
    assert _integration_rows() == SYNC_KMEANS_RAGGED
    assert set(exports) - {"mmf_kmeans_ragged_groups"} <= covered
