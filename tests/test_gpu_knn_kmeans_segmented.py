"""Segmented k-NN + KMeans hypergraph: the ordered edge entry against the existing pair ops and against the
CPU restatement of the reference, past the old 16384-cluster limit, and the batched builder against the loop of the plain
mirror (bitwise) and the golden fixture G5.  Inputs are seeded Gaussian rows: no exact distance ties, so no row and no edge is
left out of any comparison."""
import json

import numpy as np
import pytest
import torch
from importlib import import_module

from conftest import load_golden
from oracle import ref_restate

pytestmark = pytest.mark.gpu
TOL = 1e-5            # the weight tolerance of test_gpu_mirrors.py


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


@pytest.fixture(scope="module")
def kk(mmf):
    return import_module("multimodal_fusion_amd.knn_kmeans_hypergraph")


@pytest.fixture(scope="module")
def bh(mmf):
    return import_module("multimodal_fusion_amd.build_hypergraph")


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def random_table(sizes, k, seed):
    """[n, k] neighbour table with global ids: k distinct rows of the own segment, never the row itself."""
    g = torch.Generator().manual_seed(seed)
    out, base = [], 0
    for n_s in sizes:
        assert n_s > k
        r = torch.rand(n_s, n_s, generator=g)
        r.fill_diagonal_(-1.0)
        out.append(torch.topk(r, k, dim=1).indices + base)
        base += n_s
    return torch.cat(out).to(torch.int64)


def random_labels(sizes, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randint(0, H, (n_s,), generator=g) for n_s in sizes]).to(torch.int64)


def global_labels(labels, sizes, H):
    seg = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return seg * H + labels


def by_pieces(ops, nbr, labels_global, n_ids):
    """The existing ops: segment_sort + clique_pairs + knn_pairs over (global) labels, then the sort of the plain mirror."""
    n = nbr.shape[0]
    if labels_global is None:
        lo, hi = ops.knn_pairs(nbr, None)
    else:
        seg = ops.segment_sort(labels_global, n_ids)
        c_lo, c_hi = ops.clique_pairs(seg)
        k_lo, k_hi = ops.knn_pairs(nbr, labels_global)
        lo, hi = torch.cat([c_lo, k_lo]), torch.cat([c_hi, k_hi])
    code = torch.sort(lo * n + hi).values
    return torch.stack([code // n, code % n])


def check_entry(ops, nbr, labels, H, sizes):
    p = offsets(sizes)
    nbr_d = nbr.cuda()
    lab_d = None if labels is None else labels.cuda()
    ei, eptr = ops.knn_clique_edges(nbr_d, lab_d, H, ptr=p)
    gl = None if labels is None else global_labels(labels, sizes, H).cuda()
    ref = by_pieces(ops, nbr_d, gl, len(sizes) * H)
    assert ei.dtype == torch.int64 and ei.is_contiguous() and tuple(ei.shape) == tuple(ref.shape), (ei.shape, ref.shape)
    assert torch.equal(ei, ref)
    want = torch.searchsorted(ref[0].contiguous(), torch.tensor(p, device="cuda"))
    assert torch.equal(eptr, want)
    ei2, eptr2 = ops.knn_clique_edges(nbr_d, lab_d, H, ptr=p)
    assert torch.equal(ei, ei2) and torch.equal(eptr, eptr2)
    return ei, eptr


RAGGED = [37, 64, 65, 22, 129, 300, 1000, 23, 128]


@pytest.mark.parametrize("k", [1, 5, 20])
@pytest.mark.parametrize("H", [1, 2, 10, 300])
def test_entry_equals_the_existing_pieces_on_ragged_segments(mmf, k, H):
    nbr = random_table(RAGGED, k, 11 + k)
    labels = random_labels(RAGGED, H, 5 + H)          # H = 1: all cliques; H = 300: mostly clusters of one member
    check_entry(mmf.ops, nbr, labels, H, RAGGED)


@pytest.mark.parametrize("k", [1, 5, 20])
def test_entry_without_labels(mmf, k):
    check_entry(mmf.ops, random_table(RAGGED, k, 3), None, 1, RAGGED)


def test_entry_one_segment_and_default_ptr(mmf):
    nbr, labels = random_table([777], 5, 8), random_labels([777], 10, 9)
    a, pa = check_entry(mmf.ops, nbr, labels, 10, [777])
    b, pb = mmf.ops.knn_clique_edges(nbr.cuda(), labels.cuda(), 10)            # neither ptr nor batch: one segment
    assert torch.equal(a, b) and torch.equal(pa, pb) and pb.tolist() == [0, a.shape[1]]


def test_entry_one_large_segment(mmf):
    """The plain case at a size where one wave walks 1100 steps of the member scatter and the row scan spans 69 workgroups."""
    n, k, H, stride = 70000, 5, 200, 7919
    g = torch.Generator().manual_seed(61)
    r = torch.randint(1, n - k * stride, (n, 1), generator=g)
    nbr = (torch.arange(n)[:, None] + r + torch.arange(k)[None, :] * stride) % n          # k distinct rows, never the row itself
    ei, eptr = check_entry(mmf.ops, nbr, random_labels([n], H, 62), H, [n])
    assert eptr.tolist() == [0, ei.shape[1]] and ei.shape[1] > 12_000_000


def test_entry_batch_vector_and_an_empty_segment(mmf):
    sizes = [40, 0, 33, 90]
    nbr, labels = random_table([40, 33, 90], 5, 1), random_labels([40, 33, 90], 4, 2)
    a, pa = check_entry(mmf.ops, nbr, labels, 4, sizes)
    batch = torch.repeat_interleave(torch.tensor([0, 2, 3]), torch.tensor([40, 33, 90]))
    b, pb = mmf.ops.knn_clique_edges(nbr.cuda(), labels.cuda(), 4, batch=batch)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    assert int(pa[1]) == int(pa[2])


@pytest.mark.parametrize("n_hub", [100, 2000])
def test_entry_hub(mmf, n_hub):
    """Every row of one segment lists the segment's first row, whose cluster holds nobody else: that row's k-NN tail is n_hub - 1
    entries long (the in-place sort and merge-path of kc_merge_kernel), next to segments of the common kind."""
    sizes, k, H = [150, n_hub, 64], 5, 7
    nbr = random_table(sizes, k, 21)
    labels = random_labels(sizes, H - 1, 22)
    h0 = sizes[0]
    g = torch.Generator().manual_seed(23)
    for i in range(1, n_hub):                         # rows 1 .. : k - 1 distinct rows from 1 .., then the hub
        c = torch.randperm(n_hub - 1, generator=g)[:k] + 1
        c = c[c != i][:k - 1]
        nbr[h0 + i, :k - 1] = c + h0
        nbr[h0 + i, k - 1] = h0
    nbr[h0] = torch.arange(1, k + 1) + h0
    labels[h0] = H - 1
    ei, eptr = check_entry(mmf.ops, nbr, labels, H, sizes)
    assert int(((ei[0] == h0).sum())) == n_hub - 1


def test_entry_mutual_pairs_and_ignored_entries(mmf):
    sizes, k, H = [64, 200, 31], 4, 3
    nbr = random_table(sizes, k, 31)
    n = sum(sizes)
    for a in range(0, n - 1, 2):                      # rows 2m and 2m + 1 of one segment list each other
        if any(a < p <= a + 1 for p in offsets(sizes)[1:-1]):
            continue
        for r, v in ((a, a + 1), (a + 1, a)):
            nbr[r, 1:][nbr[r, 1:] == v] = -1           # no id twice in a row
            nbr[r, 0] = v
    g = torch.Generator().manual_seed(32)
    drop = torch.rand(n, k, generator=g) < 0.2
    drop[:, 0] = False
    nbr[drop] = -1                                     # ignored, as in knn_pairs
    nbr[5, 3] = n + 7                                  # out of range: ignored
    nbr[6, 3] = 6                                      # the row itself: ignored
    labels = random_labels(sizes, H, 33)
    labels[0::2] = 0
    labels[1::2] = torch.where(labels[1::2] == 0, torch.ones_like(labels[1::2]), labels[1::2])     # the mutual pairs cross clusters
    check_entry(mmf.ops, nbr, labels, H, sizes)


def test_entry_rejects_a_label_out_of_range(mmf):
    nbr, labels = random_table([50, 60], 3, 1).cuda(), random_labels([50, 60], 4, 2).cuda()
    labels[77] = 4
    with pytest.raises(ValueError, match="label"):
        mmf.ops.knn_clique_edges(nbr, labels, 4, ptr=[0, 50, 110])
    labels[77] = -1
    with pytest.raises(ValueError, match="label"):
        mmf.ops.knn_clique_edges(nbr, labels, 4, ptr=[0, 50, 110])


@pytest.mark.parametrize("k,H", [(1, 1), (5, 10), (20, 2)])
def test_entry_against_the_restated_reference(mmf, k, H):
    """Per segment: the reference's clique pairs and directed k-NN pairs through its dedup (oracle/ref_restate.py)."""
    sizes = [k + 2, 64, 150, 33, 260]
    p = offsets(sizes)
    nbr, labels = random_table(sizes, k, 41), random_labels(sizes, H, 42)
    ei, eptr = mmf.ops.knn_clique_edges(nbr.cuda(), labels.cuda(), H, ptr=p)
    ei, eptr = ei.cpu(), eptr.tolist()
    feats = torch.randn(sum(sizes), 4, generator=torch.Generator().manual_seed(43))
    for s, n_s in enumerate(sizes):
        local = (nbr[p[s]:p[s + 1]] - p[s]).numpy()
        directed = np.stack([np.repeat(np.arange(n_s), k), local.reshape(-1)], axis=1)
        pairs = np.concatenate([directed, ref_restate.clique_pairs(labels[p[s]:p[s + 1]].numpy(), H)], axis=0)
        ref, _ = ref_restate.dedup_and_weight(feats[p[s]:p[s + 1]], pairs)
        assert torch.equal(ei[:, eptr[s]:eptr[s + 1]] - p[s], ref), s
    assert eptr[-1] == ei.shape[1]


def test_entry_past_the_old_cluster_limit(mmf):
    """4096 segments x 8 clusters = 32768 cluster ids (mmf_segment_sort holds 16384): against a loop of the existing pieces."""
    S, n_s, k, H = 4096, 24, 5, 8
    sizes = [n_s] * S
    assert S * H > 16384
    nbr, labels = random_table(sizes, k, 51).cuda(), random_labels(sizes, H, 52).cuda()
    ei, eptr = mmf.ops.knn_clique_edges(nbr, labels, H, ptr=offsets(sizes))
    parts, counts = [], []
    for s in range(S):
        a = s * n_s
        e = by_pieces(mmf.ops, nbr[a:a + n_s] - a, labels[a:a + n_s], H)
        parts.append(e + a)
        counts.append(e.shape[1])
    assert torch.equal(ei, torch.cat(parts, dim=1))
    assert eptr.tolist() == offsets(counts)


# ---- the builder ---------------------------------------------------------------------------------------------------------
def cohort(sizes, d, seed, no_tma=()):
    """wsi / tma rows of every slide (about 60 % wsi; the slides in `no_tma` have no tma rows) and the two offset lists."""
    g = torch.Generator().manual_seed(seed)
    nw = [n_s if s in no_tma else max(1, (3 * n_s) // 5) for s, n_s in enumerate(sizes)]
    nt = [n_s - w for n_s, w in zip(sizes, nw)]
    W = torch.randn(sum(nw), d, generator=g)
    Tm = torch.randn(sum(nt), d, generator=g)
    return W, Tm, offsets(nw), offsets(nt)


def plain_loop(bh, W, Tm, wp, tp, k, H, device=None):
    out = []
    for s in range(len(wp) - 1):
        out.append(bh.build_hypergraph_knn_kmeans(W[wp[s]:wp[s + 1]], Tm[tp[s]:tp[s + 1]], None, k, H, device))
    return out


def check_builder(kk, bh, sizes, d, k, H, seed, no_tma=()):
    W, Tm, wp, tp = cohort(sizes, d, seed, no_tma)
    W, Tm = W.cuda(), Tm.cuda()
    ei, ew, eptr, stats = kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, k, H, wsi_ptr=wp, tma_ptr=tp)
    ref = plain_loop(bh, W, Tm, wp, tp, k, H)
    node_ptr = offsets(sizes)
    assert stats["node_ptr"] == node_ptr
    assert eptr.tolist() == offsets([r[0].shape[1] for r in ref])
    assert torch.equal(ei, torch.cat([r[0] + node_ptr[s] for s, r in enumerate(ref)], dim=1))
    assert torch.equal(ew.view(torch.int32), torch.cat([r[1] for r in ref]).view(torch.int32))       # weight bits
    assert stats["segments"] == [r[2] for r in ref]
    json.dumps(stats)
    return ei, ew, eptr, stats


def ragged_sizes(k, H):
    lo = max(k + 2, H)                    # the smallest slide both steps accept: k + 1 neighbours' worth of rows and H clusters
    return [lo, 700, lo + 1, 64, 17 + lo, 129, 300, 65, lo]


@pytest.mark.parametrize("k,H", [(1, 1), (5, 10), (20, 2)])
@pytest.mark.parametrize("d", [32, 512, 1000])
@pytest.mark.parametrize("shape", ["equal", "ragged", "large_small"])
def test_builder_equals_the_loop_of_the_plain_mirror(kk, bh, shape, d, k, H):
    sizes = {"equal": [64] * 40, "ragged": ragged_sizes(k, H), "large_small": [2048, 12, 12]}[shape]
    if min(sizes) < k + 1:
        # the 12-row slides cannot have 20 neighbours: both sides refuse, the batched builder naming the slide
        W, Tm, wp, tp = cohort(sizes, d, 7)
        with pytest.raises(ValueError, match=r"segment 1: Expected n_neighbors <= n_samples_fit, but n_neighbors = 21"):
            kk.build_hypergraph_knn_kmeans_segmented(W.cuda(), Tm.cuda(), None, k, H, wsi_ptr=wp, tma_ptr=tp)
        with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit, but n_neighbors = 21"):
            bh.build_hypergraph_knn_kmeans(W[wp[1]:wp[2]].cuda(), Tm[tp[1]:tp[2]].cuda(), None, k, H)
        return
    check_builder(kk, bh, sizes, d, k, H, seed=100 + d + k, no_tma=(1,))


def test_builder_per_kmeans_backend(kk, bh, kmeans_backend):
    _, _, _, stats = check_builder(kk, bh, [64] * 40, 32, 5, 10, seed=9)
    assert stats["kmeans_backend"] == kmeans_backend
    if kmeans_backend == "device":
        assert len(stats["ambiguous_draws"]) == 40 and len(stats["ambiguous_trials"]) == 40
        assert all(isinstance(v, int) and v >= 0 for v in stats["ambiguous_draws"] + stats["ambiguous_trials"])
    else:
        assert stats["ambiguous_draws"] is None and stats["ambiguous_trials"] is None


@pytest.mark.parametrize("tag,copies", [("mid", 3), ("small", 4)])
def test_builder_reproduces_golden_g5_in_every_copy(kk, tag, copies):
    g = load_golden("g5_knn_kmeans.npz")
    W1, T1 = torch.from_numpy(g[f"{tag}_W"]), torch.from_numpy(g[f"{tag}_T"])
    k, H, d = int(g[f"{tag}_k"]), int(g[f"{tag}_H"]), W1.shape[1]
    ei_ref, ew_ref = torch.from_numpy(g[f"{tag}_ei_sorted"]), g[f"{tag}_ew_sorted"]
    gen = torch.Generator().manual_seed(5)

    def run(with_random):
        ws, ts = [W1] * copies, [T1] * copies
        if with_random:                                # a random slide before and one after the copies
            ws = [torch.randn(50, d, generator=gen)] + ws + [torch.randn(70, d, generator=gen)]
            ts = [torch.randn(30, d, generator=gen)] + ts + [torch.randn(20, d, generator=gen)]
        wp, tp = offsets([w.shape[0] for w in ws]), offsets([t.shape[0] for t in ts])
        ei, ew, eptr, st = kk.build_hypergraph_knn_kmeans_segmented(torch.cat(ws), torch.cat(ts), None, k, H, "cuda",
                                                                    wsi_ptr=wp, tma_ptr=tp)
        first = 1 if with_random else 0
        out = []
        for s in range(first, first + copies):
            a, b = int(eptr[s]), int(eptr[s + 1])
            out.append((ei[:, a:b].cpu() - st["node_ptr"][s], ew[a:b].cpu()))
        return out

    alone = run(False)
    batches = [alone] + ([run(True)] if tag == "mid" else [])      # 'mid' also between two random slides of the same d
    for got in batches:
        for e, w in got:
            assert torch.equal(e, ei_ref)
            np.testing.assert_allclose(w.numpy(), ew_ref, rtol=0, atol=TOL)
            assert torch.equal(e, alone[0][0]) and torch.equal(w.view(torch.int32), alone[0][1].view(torch.int32))   # no leak


def test_builder_ptr_batch_devices_repeat_and_stats(kk, bh):
    sizes, d, k, H = [30, 45, 12, 80], 64, 5, 10
    W, Tm, wp, tp = cohort(sizes, d, 77, no_tma=(2,))
    wb = torch.repeat_interleave(torch.arange(4), torch.tensor(np.diff(wp)))
    tb = torch.repeat_interleave(torch.arange(4), torch.tensor(np.diff(tp)))
    assert int(tp[2]) == int(tp[3]) and tb.max() == 3               # slide 2 has no tma rows, the batch vector skips its id
    a = kk.build_hypergraph_knn_kmeans_segmented(W.cuda(), Tm.cuda(), None, k, H, wsi_ptr=wp, tma_ptr=tp)
    b = kk.build_hypergraph_knn_kmeans_segmented(W.cuda(), Tm.cuda(), np.zeros(3), k, H, wsi_batch=wb.cuda(), tma_batch=tb)
    c = kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, k, H, wsi_ptr=torch.tensor(wp), tma_batch=tb)      # CPU in, CPU out
    e = kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, k, H, torch.device("cuda"), wsi_ptr=wp, tma_ptr=tp)
    for t in a[:3] + e[:3]:
        assert t.is_cuda
    for t in c[:3]:
        assert not t.is_cuda
    for other in (b, c, e):
        assert torch.equal(a[0].cpu(), other[0].cpu()) and torch.equal(a[2].cpu(), other[2].cpu())
        assert torch.equal(a[1].cpu().view(torch.int32), other[1].cpu().view(torch.int32))
        assert other[3] == a[3]
    stats = a[3]
    json.dumps(stats)
    ref = plain_loop(bh, W.cuda(), Tm.cuda(), wp, tp, k, H)
    assert stats["segments"] == [r[2] for r in ref]
    assert stats["num_segments"] == 4 and stats["num_nodes"] == sum(sizes) and stats["num_edges"] == a[0].shape[1]
    assert stats["num_edges"] == sum(r[2]["num_edges"] for r in ref)
    # the lower-level call on already concatenated nodes
    X = torch.cat([torch.cat([W[wp[s]:wp[s + 1]], Tm[tp[s]:tp[s + 1]]]) for s in range(4)]).cuda()
    ei, ew, eptr, info = kk.knn_kmeans_edges_segmented(X, k, H, batch=torch.repeat_interleave(torch.arange(4), torch.tensor(sizes)),
                                                       return_info=True)
    assert torch.equal(ei, a[0]) and torch.equal(ew.view(torch.int32), a[1].view(torch.int32)) and torch.equal(eptr, a[2])
    assert info["ambiguous_draws"] == stats["ambiguous_draws"] and len(info["ambiguous_trials"]) == 4
