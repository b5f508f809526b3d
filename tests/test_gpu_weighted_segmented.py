"""Segmented weighted hypergraph: the combined similarity, the off-diagonal median and the threshold edges of
every graph of a ragged batch in one call.  Every segment is checked against the plain call on its slice (bitwise), a batch
against the CPU oracle, and the golden fixtures against the reference's own edges."""
import numpy as np
import pytest
import torch
from importlib import import_module

import oracle
from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-5
RATIOS = (0.0, 0.5, 1.0, 2.0, float("inf"))


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


@pytest.fixture(scope="module")
def wh(mmf):
    return import_module("multimodal_fusion_amd.weighted_hypergraph")


@pytest.fixture(scope="module")
def bh(mmf):
    return import_module("multimodal_fusion_amd.build_hypergraph")


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def inputs(n, d, dp, seed):
    """Features scaled so that |f_i - f_j|^2 is of order one (similarities spread over (0, 1)), positions in the unit box."""
    rng = np.random.RandomState(seed)
    F = (rng.randn(n, d) * (0.6 / np.sqrt(d))).astype(np.float32)
    P = rng.rand(n, dp).astype(np.float32)
    return torch.from_numpy(F).cuda(), torch.from_numpy(P).cuda()


def blocks(K, kptr, ptr):
    for s in range(len(ptr) - 1):
        n_s = ptr[s + 1] - ptr[s]
        yield s, K[int(kptr[s]):int(kptr[s + 1])].view(n_s, n_s)


def bits(t):
    return t.contiguous().view(torch.int32)


RAGGED = [2, 3, 31, 127, 128, 129, 500, 3000]


@pytest.mark.parametrize("d", [3, 64, 512, 1000])
@pytest.mark.parametrize("dp", [2, 3])
def test_blocks_equal_the_plain_call(mmf, d, dp):
    sizes = RAGGED if d != 1000 else RAGGED[::-1]
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], d, dp, d + dp)
    K, kptr = mmf.ops.sim_dense_combined_segmented(F, P, 0.7, 1.3, ptr=ptr)
    assert K.shape == (sum(v * v for v in sizes),) and kptr.tolist() == offsets([v * v for v in sizes])
    for s, Ks in blocks(K, kptr, ptr):
        ref = mmf.ops.sim_dense_combined(F[ptr[s]:ptr[s + 1]], P[ptr[s]:ptr[s + 1]], 0.7, 1.3)
        assert torch.equal(bits(Ks), bits(ref)), f"segment {s} (n_s = {sizes[s]})"
    med = mmf.ops.offdiag_lower_median_segmented(K, ptr=ptr)
    for s, Ks in blocks(K, kptr, ptr):
        assert torch.equal(bits(med[s]), bits(mmf.ops.offdiag_lower_median(Ks))), f"median of segment {s}"


def test_many_small_segments(mmf):
    rng = np.random.RandomState(11)
    sizes = rng.randint(16, 65, 2048).tolist()
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], 64, 2, 11)
    K, kptr = mmf.ops.sim_dense_combined_segmented(F, P, ptr=ptr)
    med = mmf.ops.offdiag_lower_median_segmented(K, ptr=ptr)
    for s, Ks in blocks(K, kptr, ptr):
        ref = mmf.ops.sim_dense_combined(F[ptr[s]:ptr[s + 1]], P[ptr[s]:ptr[s + 1]])
        assert torch.equal(bits(Ks), bits(ref)), f"segment {s}"
        assert torch.equal(bits(med[s]), bits(mmf.ops.offdiag_lower_median(ref))), f"median of segment {s}"


def test_last_tile_starts_unaligned_and_ends_at_the_last_row(mmf):
    """The last segment starts at row 377 and ends at the last row of F: its tiles read past the image's real rows into the
    never-written block (prep_f32_bytes); only masked outputs may see them.  Every block is also the full matrix's block."""
    sizes = [77, 300, 129]
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], 96, 2, 5)
    K, kptr = mmf.ops.sim_dense_combined_segmented(F, P, ptr=ptr)
    full = mmf.ops.sim_dense_combined(F, P)
    for s, Ks in blocks(K, kptr, ptr):
        a, b = ptr[s], ptr[s + 1]
        assert torch.equal(bits(Ks), bits(full[a:b, a:b])), f"segment {s}"
        assert torch.equal(bits(Ks), bits(mmf.ops.sim_dense_combined(F[a:b], P[a:b])))


def test_batch_vector_and_empty_segments(mmf):
    """batch= gives the same blocks as ptr=; a segment with no rows is a zero-size block."""
    sizes = [40, 0, 130, 7]
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], 32, 2, 9)
    K1, k1 = mmf.ops.sim_dense_combined_segmented(F, P, ptr=ptr)
    batch = torch.repeat_interleave(torch.arange(4), torch.tensor(sizes)).cuda()
    K2, k2 = mmf.ops.sim_dense_combined_segmented(F, P, batch=batch)
    assert torch.equal(bits(K1), bits(K2)) and torch.equal(k1, k2)


def hand_blocks():
    rng = np.random.RandomState(3)
    out = [np.full((5, 5), 0.25, np.float32),                                    # constant
           np.array([[1.0, 0.5], [0.25, 1.0]], np.float32),                      # two rows: median of {0.5, 0.25}
           np.array([[7.0, -3.0], [-3.0, 7.0]], np.float32)]
    r = rng.rand(6, 6).astype(np.float32)
    out.append(np.concatenate([r[:3], r[:3]]))                                   # duplicate rows
    z = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), (9, 9)).astype(np.float32)
    out.append(z)                                                                # +-0.0
    w = rng.randn(11, 11).astype(np.float32)
    w[rng.rand(11, 11) < 0.3] = np.inf
    w[rng.rand(11, 11) < 0.3] = -np.inf
    out.append(w)                                                                # +-inf
    out.append(np.where(rng.rand(64, 64) < 0.5, -0.0, 0.0).astype(np.float32))
    out.append(rng.rand(2100, 2100).astype(np.float32))                          # >= 2049 rows: the plain call's one-sweep path
    out.append(rng.rand(3, 3).astype(np.float32))
    return out


def test_medians_of_hand_made_blocks(mmf):
    Bs = hand_blocks()
    ptr = offsets([b.shape[0] for b in Bs])
    K = torch.from_numpy(np.concatenate([b.reshape(-1) for b in Bs])).cuda()
    med = mmf.ops.offdiag_lower_median_segmented(K, ptr=ptr)
    for s, b in enumerate(Bs):
        ref = mmf.ops.offdiag_lower_median(torch.from_numpy(b).cuda())
        assert torch.equal(bits(med[s]), bits(ref)), f"block {s}"
        assert float(med[s]) == oracle.offdiag_lower_median(b) or (np.isnan(float(med[s])) and np.isnan(oracle.offdiag_lower_median(b)))
    # K_s < thr per block, ids global
    thr = [0.25, 0.3, 7.0, 0.5, 0.0, 0.0, 0.0, 0.5, 0.5]
    ei, ew, eptr = mmf.ops.threshold_edges_segmented(K, thr, ptr=ptr)
    for s, b in enumerate(Bs):
        rei, rew = mmf.ops.threshold_edges(torch.from_numpy(b).cuda(), thr[s])
        e0, e1 = int(eptr[s]), int(eptr[s + 1])
        assert torch.equal(ei[:, e0:e1], rei + ptr[s]) and torch.equal(bits(ew[e0:e1]), bits(rew)), f"block {s}"
    assert int(eptr[-1]) == ei.shape[1]


@pytest.mark.parametrize("sizes", [[2, 3, 31, 127, 128, 129, 500], [64] * 40, [700, 2, 2]])
def test_edges_equal_the_plain_builder(bh, wh, sizes):
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], 48, 2, len(sizes))
    for ratio in RATIOS:
        ei, ew, eptr = wh.build_weighted_hypergraph_segmented(F, P, 1.0, 1.0, ratio, ptr=ptr)
        assert ei.is_cuda and ei.dtype == torch.int64 and ei.is_contiguous() and ew.dtype == torch.float32
        assert eptr.tolist()[0] == 0 and int(eptr[-1]) == ei.shape[1] == ew.shape[0]
        for s in range(len(sizes)):
            a, b = ptr[s], ptr[s + 1]
            rei, rew = bh.build_weighted_hypergraph(F[a:b], P[a:b], 1.0, 1.0, ratio)
            e0, e1 = int(eptr[s]), int(eptr[s + 1])
            assert torch.equal(ei[:, e0:e1], rei + a), f"ratio {ratio}, segment {s}"
            assert torch.equal(bits(ew[e0:e1]), bits(rew)), f"ratio {ratio}, segment {s}"


def test_against_the_oracle(mmf, wh):
    sizes = [300, 17, 2, 129, 6, 513]
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], 40, 2, 21)
    K, kptr = mmf.ops.sim_dense_combined_segmented(F, P, 0.5, 2.0, ptr=ptr)
    med = mmf.ops.offdiag_lower_median_segmented(K, ptr=ptr).cpu().numpy()
    thr = wh.f32_ceil_array(med.astype(np.float64) * 0.9)
    ei, ew, eptr = mmf.ops.threshold_edges_segmented(K, thr, ptr=ptr)
    ei, ew = ei.cpu().numpy(), ew.cpu().numpy()
    Fh, Ph = F.cpu().numpy(), P.cpu().numpy()
    for s, Ks in blocks(K, kptr, ptr):
        a, b = ptr[s], ptr[s + 1]
        Kh = Ks.cpu().numpy()
        np.testing.assert_allclose(Kh, oracle.sim_dense_combined(Fh[a:b], Ph[a:b], 0.5, 2.0), rtol=0, atol=TOL)
        assert float(med[s]) == oracle.offdiag_lower_median(Kh)
        rei, rew = oracle.threshold_edges(Kh, float(thr[s]))
        e0, e1 = int(eptr[s]), int(eptr[s + 1])
        assert np.array_equal(ei[:, e0:e1], rei + a) and np.array_equal(ew[e0:e1], rew), f"segment {s}"


def test_golden_batch_reproduces_the_reference(wh):
    g = load_golden("g2_threshold.npz")
    Ns = (2, 8, 64)
    ptr = offsets(Ns)
    F = torch.from_numpy(np.concatenate([g[f"N{N}_X"] for N in Ns]))
    P = torch.from_numpy(np.concatenate([g[f"N{N}_P"] for N in Ns]))
    for ratio in (0.0, 0.5, 1.0, 2.0):
        ei, ew, eptr = wh.build_weighted_hypergraph_segmented(F, P, 1.0, 1.0, ratio, ptr=ptr)
        assert ei.device.type == "cpu" and ew.device.type == "cpu"           # CPU inputs: results on the CPU, as the mirror
        for s, N in enumerate(Ns):
            e0, e1 = int(eptr[s]), int(eptr[s + 1])
            assert np.array_equal(ei[:, e0:e1].numpy() - ptr[s], g[f"N{N}_r{ratio}_ei"]), f"ratio {ratio}, N = {N}"
            np.testing.assert_allclose(ew[e0:e1].numpy(), g[f"N{N}_r{ratio}_ew"], rtol=0, atol=TOL)
    data = wh.build_hypergraph_data_segmented(F, P, 1.0, 1.0, 0.5, True, ptr=ptr)
    ei, ew = data["edge_index"].numpy(), data["edge_attr"].numpy()
    bounds = np.searchsorted(ei[0], ptr)                                      # edges are segment-major
    for s, N in enumerate(Ns):
        assert np.array_equal(ei[:, bounds[s]:bounds[s + 1]] - ptr[s], g[f"N{N}_data_ei"])
        np.testing.assert_allclose(ew[bounds[s]:bounds[s + 1]], g[f"N{N}_data_ew"], rtol=0, atol=TOL)
        np.testing.assert_allclose(data["pooled_feature"][s:s + 1].numpy(), g[f"N{N}_data_pool"], rtol=0, atol=1e-6)


def test_groups_and_streamed_segments_give_the_same_edges(wh, monkeypatch):
    sk = import_module("multimodal_fusion_amd.build_hypergraph.similarity_kernel")
    sizes = [40, 50, 300, 60, 70, 2, 45]
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], 24, 2, 31)
    ref = wh.build_weighted_hypergraph_segmented(F, P, 1.0, 1.0, 0.8, ptr=ptr)
    assert wh._groups(sizes, sk.STREAM_BYTES) == [(0, len(sizes), False)]
    monkeypatch.setattr(sk, "STREAM_BYTES", 4 * 100 * 100)                # 300 rows stream; the rest form three groups
    monkeypatch.setattr(sk, "PANEL_ROWS", 128)
    assert wh._groups(sizes, sk.STREAM_BYTES) == [(0, 2, False), (2, 3, True), (3, 6, False), (6, 7, False)]
    got = wh.build_weighted_hypergraph_segmented(F, P, 1.0, 1.0, 0.8, ptr=ptr)
    for r, g_ in zip(ref, got):
        assert torch.equal(r, g_) if r.dtype != torch.float32 else torch.equal(bits(r), bits(g_))


def test_data_dict(wh):
    sizes = [5, 130, 2, 64, 257]
    ptr = offsets(sizes)
    F, P = inputs(ptr[-1], 20, 3, 41)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    for dev_in in ("cpu", "cuda"):
        Fi, Pi = F.to(dev_in), P.to(dev_in)
        d = wh.build_hypergraph_data_segmented(Fi, Pi, 1.0, 1.0, 0.5, True, batch=batch)
        assert sorted(d) == ["batch", "edge_attr", "edge_index", "pooled_feature", "pos", "ptr", "x"]
        for k, v in d.items():
            assert v.device.type == dev_in, k
        assert torch.equal(d["batch"].cpu(), batch) and d["ptr"].cpu().tolist() == ptr
        assert torch.equal(d["x"], Fi) and torch.equal(d["pos"], Pi)
        ref = torch.stack([Fi[ptr[s]:ptr[s + 1]].mean(dim=0) for s in range(len(sizes))])
        assert d["pooled_feature"].shape == (len(sizes), 20)
        torch.testing.assert_close(d["pooled_feature"], ref, rtol=0, atol=1e-6)
        ei, ew, _ = wh.build_weighted_hypergraph_segmented(Fi, Pi, 1.0, 1.0, 0.5, batch=batch)
        assert torch.equal(d["edge_index"], ei) and torch.equal(bits(d["edge_attr"]), bits(ew))
        assert "pooled_feature" not in wh.build_hypergraph_data_segmented(Fi, Pi, 1.0, 1.0, 0.5, False, batch=batch)
