"""Hypergraph propagation on the GPU (mmf.hgconv, include/ext/mmf_hg_hgconv.h): out and the hyperedge features Y
have the BITS of the numpy restatement (tests/hgconv_restate.py) on every path of the gather-sum kernel (float4 / scalar, one wave
per row / several rows per wave, column chunks, id blocks of 64, batches of 8), do not depend on the order of the columns of
edge_index, and are the same from call to call; the backward is the restatement's transposed form; HypergraphConv is
propagate(lin(x)) + bias; out-of-range ids are flagged by column and left out of the plan; plan build and propagation keep the stream
contract (tests/streamgate.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hgconv_restate as hr      # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got: torch.Tensor, want: np.ndarray, what: str):
    g = got.detach().cpu().numpy()
    assert g.shape == want.shape and g.dtype == np.float32, (what, g.shape, want.shape, g.dtype)
    bad = int(np.count_nonzero(hr.bits(g) != hr.bits(want)))
    assert bad == 0, f"{what}: {bad} of {g.size} values differ from the restatement (max |diff| {np.nanmax(np.abs(g - want)):.3e})"


def check(mmf, ei, N, M, x, w=None, what="", x_dev=None):
    """propagate on the device against the restatement, out and Y; returns the device results."""
    plan = mmf.incidence_plan(dev(ei), N, M, None if w is None else dev(w))
    out, Y = mmf.hypergraph_propagate(dev(x) if x_dev is None else x_dev, plan=plan, return_edge_features=True)
    want, want_y = hr.propagate(x, ei, M, w)
    same_bits(Y, want_y, what + " Y")
    same_bits(out, want, what + " out")
    return out, Y, plan


BASE = dict(N=300, M=200, E=1500)


@pytest.fixture(scope="module")
def base():
    ei = hr.random_incidence(BASE["N"], BASE["M"], BASE["E"], 1)
    return ei, hr.weights(BASE["M"], 2)


# ---- bits on every path of the kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 16, 64, 65, 256, 300])
@pytest.mark.parametrize("weighted", [False, True])
def test_bits_over_channel_counts(mmf, base, C, weighted):
    ei, w = base
    check(mmf, ei, BASE["N"], BASE["M"], hr.features(BASE["N"], C, 3 + C), w if weighted else None, f"C={C}")


@pytest.mark.parametrize("weighted", [False, True])
def test_empty_rows_give_zeros(mmf, weighted):
    """Node 9 isolated, hyperedge 17 unused in the middle of the range, num_edges = 40 with the largest id 30."""
    N, M = 50, 40
    ei = hr.random_incidence(N, 31, 260, 4)
    ei = ei[:, (ei[0] != 9) & (ei[1] != 17)]
    ei = np.concatenate([ei, np.array([[3], [30]])], axis=1)
    x, w = hr.features(N, 20, 5), hr.weights(M, 6)
    out, Y, plan = check(mmf, ei, N, M, x, w if weighted else None, "empty rows")
    assert not out[9].any() and not Y[17].any() and not Y[31:].any() and Y.shape == (M, 20)
    assert float(plan.edge_scale[17]) == 0.0 and float(plan.node_scale[9]) == 0.0
    # num_edges=None reads max + 1 = 31
    out31, Y31 = mmf.hypergraph_propagate(dev(x), dev(ei), hyperedge_weight=dev(w[:31]) if weighted else None, return_edge_features=True)
    assert Y31.shape == (31, 20) and torch.equal(out31, out) and torch.equal(Y31, Y[:31])


def test_the_same_pair_three_times_counts_three_times(mmf):
    N, M = 30, 12
    ei = hr.random_incidence(N, M, 90, 7)
    ei = np.concatenate([ei[:, :40], np.array([[4, 4, 4], [2, 2, 2]]), ei[:, 40:]], axis=1)
    x = hr.features(N, 8, 8)
    out, Y, plan = check(mmf, ei, N, M, x, None, "triple pair")
    check(mmf, ei, N, M, x, hr.weights(M, 9), "triple pair, weighted")
    B2 = int(np.count_nonzero(ei[1] == 2))
    assert int(plan.eptr[3] - plan.eptr[2]) == B2 and float(plan.edge_scale[2]) == float(np.float32(1.0) / np.float32(B2))
    members = plan.emem[int(plan.eptr[2]):int(plan.eptr[3])].tolist()
    assert members == sorted(members) and members.count(4) >= 3


@pytest.mark.parametrize("C", [64, 256, 6])
def test_hub_rows_next_to_rows_of_degree_one(mmf, C):
    """One hyperedge of degree 1000 and one node of degree 1002 beside rows of degree 1 and 2: 15 full id blocks of 64 and a block
    of 40 (resp. 42), whose last batch of 8 is whole (resp. holds 2)."""
    ei = hr.hub_incidence()
    N, M = 1200, 1100
    x = hr.features(N, C, 11)
    check(mmf, ei, N, M, x, None, "hubs")
    check(mmf, ei, N, M, x, hr.weights(M, 12), "hubs, weighted")


@pytest.mark.parametrize("C", [4, 32, 256, 7])
def test_degrees_around_the_batch_and_the_id_block(mmf, C):
    """Rows of degree 7, 8, 9 (the batch of 8) and 63, 64, 65 (the id block of 64) on both sides."""
    ei = hr.degree_incidence()
    N, M = 110, 10 + 70 * 6
    pl = hr.plan(ei, N, M)
    assert sorted(set(np.diff(pl["eptr"])) & {7, 8, 9, 63, 64, 65}) == [7, 8, 9, 63, 64, 65]
    assert sorted(set(np.diff(pl["nptr"])) & {7, 8, 9, 63, 64, 65}) == [7, 8, 9, 63, 64, 65]
    x = hr.features(N, C, 13)
    check(mmf, ei, N, M, x, None, "degrees")
    check(mmf, ei, N, M, x, hr.weights(M, 14), "degrees, weighted")


def test_x_as_a_slice_of_a_larger_tensor(mmf, base):
    ei, w = base
    N, M = BASE["N"], BASE["M"]
    big = torch.from_numpy(hr.features(N + 20, 100, 15)).cuda()
    for what, view in (("rows 10.. of [N + 20, 100]", big[10:10 + N]), ("columns 4..68: pitch 100, aligned", big[:N, 4:68]),
                       ("columns 1..65: pitch 100, unaligned", big[:N, 1:65]), ("columns 0..3", big[5:5 + N, 0:3]),
                       ("every second column: copied", big[:N, ::2][:, :32])):
        x = view.cpu().numpy()
        check(mmf, ei, N, M, x, w, what, x_dev=view)


def test_shuffled_columns_and_repeated_calls_give_the_same_bits(mmf, base):
    ei, w = base
    N, M = BASE["N"], BASE["M"]
    x = dev(hr.features(N, 96, 16))
    order = np.lexsort((ei[0], ei[1]))
    results = []
    for cols in (ei, ei[:, order], ei[:, np.random.RandomState(17).permutation(ei.shape[1])], ei):
        results.append(mmf.hypergraph_propagate(x, dev(cols), num_edges=M, hyperedge_weight=dev(w), return_edge_features=True))
    for out, Y in results[1:]:
        assert torch.equal(out, results[0][0]) and torch.equal(Y, results[0][1])
    plan = mmf.incidence_plan(dev(ei), N, M, dev(w))
    a = mmf.hypergraph_propagate(x, plan=plan)
    b = mmf.hypergraph_propagate(x, plan=plan)
    assert torch.equal(a, b) and torch.equal(a, results[0][0])


# ---- incidences from the library's own products ---------------------------------------------------------------------------------------
def test_knn_incidence_of_simtopk(mmf):
    N = 300
    x = hr.features(N, 32, 18)
    idx, _ = mmf.simtopk(dev(x), k=5)
    ei = mmf.knn_incidence(idx)
    assert ei.shape == (2, 6 * N) and ei.is_cuda
    check(mmf, ei.cpu().numpy(), N, N, x, None, "knn incidence")
    out = mmf.hypergraph_propagate(dev(x), ei, num_edges=N)
    assert out.shape == (N, 32)


def test_knn_incidence_of_simtopk_segmented(mmf):
    ptr = [0, 100, 104, 300]                       # the middle segment has 4 rows: 3 neighbours and two -1 per row
    x = hr.features(300, 32, 19)
    idx, _ = mmf.simtopk_segmented(dev(x), ptr=ptr, k=5)
    assert int((idx < 0).sum()) == 8
    ei = mmf.knn_incidence(idx).cpu().numpy()
    assert ei.shape[1] == 6 * 300 - 8
    seg = np.searchsorted(np.array(ptr), ei, side="right")
    assert (seg[0] == seg[1]).all()                # block-diagonal because the ids are global
    check(mmf, ei, 300, 300, x, None, "segmented knn incidence")


def test_golden_edge_index_as_the_reference_model_reads_it(mmf):
    """g5's ordered k-NN + KMeans edge list, row 1 read as the hyperedge id (cust_omics.py:58: HypergraphConv(x, edge_index))."""
    g = load_golden("g5_knn_kmeans.npz")
    for tag in ("small", "zero", "mid"):
        ei = g[f"{tag}_ei_sorted"].astype(np.int64)
        N = g[f"{tag}_W"].shape[0] + g[f"{tag}_T"].shape[0]
        M = int(ei[1].max()) + 1
        x = hr.features(N, 48, 20)
        out, Y, _ = check(mmf, ei, N, M, x, None, f"golden {tag}")
        got = mmf.hypergraph_propagate(dev(x), dev(ei))
        assert torch.equal(got, out)


def test_mid_size(mmf):
    N, M, E, C = 20000, 15000, 200000, 128
    ei = hr.random_incidence(N, M, E, 21)
    check(mmf, ei, N, M, hr.features(N, C, 22), hr.weights(M, 23), "mid size")


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_backward_is_the_transposed_form(mmf, base, weighted):
    ei, w = base
    w = w if weighted else None
    N, M, C = BASE["N"], BASE["M"], 40
    x = dev(hr.features(N, C, 24)).requires_grad_()
    g = hr.features(N, C, 25)
    plan = mmf.incidence_plan(dev(ei), N, M, None if w is None else dev(w))
    out = mmf.hypergraph_propagate(x, plan=plan)
    out.backward(dev(g))
    want, _ = hr.propagate(g, ei, M, w, transpose=True)
    same_bits(x.grad, want, "x.grad")
    P, max_b, max_deg = hr.dense_operator(ei, N, M, w)
    err = np.abs(x.grad.cpu().numpy().astype(np.float64) - P.T @ g.astype(np.float64))
    tol = hr.bound(P.T, g, max_b, max_deg)
    print(f"backward weighted={weighted}: max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()
    # and the forward against the dense operator, within the same bound
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - P @ x.detach().cpu().numpy().astype(np.float64))
    assert (err <= hr.bound(P, x.detach().cpu().numpy(), max_b, max_deg)).all()


def test_a_plan_reused_for_three_layers(mmf, base):
    ei, w = base
    N, M, C = BASE["N"], BASE["M"], 24
    x0, g = hr.features(N, C, 26), dev(hr.features(N, C, 27))
    plan = mmf.incidence_plan(dev(ei), N, M, dev(w))
    xa = dev(x0).requires_grad_()
    h = xa
    for _ in range(3):
        h = torch.tanh(mmf.hypergraph_propagate(h, plan=plan))
    h.backward(g)
    xb = dev(x0).requires_grad_()
    hb = xb
    for _ in range(3):
        hb = torch.tanh(mmf.hypergraph_propagate(hb, dev(ei), num_edges=M, hyperedge_weight=dev(w)))     # a plan of its own per call
    hb.backward(g)
    assert torch.equal(h, hb) and torch.equal(xa.grad, xb.grad) and bool(xa.grad.abs().sum() > 0)
    with pytest.raises(ValueError, match="requires grad"):
        mmf.hypergraph_propagate(xa, dev(ei), num_edges=M, hyperedge_weight=dev(w).requires_grad_())


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_hypergraph_conv_module(mmf, base):
    ei, w = base
    N, M = BASE["N"], BASE["M"]
    torch.manual_seed(0)
    conv = mmf.HypergraphConv(48, 20).cuda()
    assert sorted(conv.state_dict()) == ["bias", "lin.weight"] and conv.state_dict()["lin.weight"].shape == (20, 48)
    with torch.no_grad():
        conv.bias.copy_(torch.linspace(-1, 1, 20))
    x = dev(hr.features(N, 48, 28))
    y = conv(x, dev(ei), dev(w), num_edges=M)
    h = torch.nn.functional.linear(x, conv.lin.weight)
    want = mmf.hypergraph_propagate(h, dev(ei), num_edges=M, hyperedge_weight=dev(w)) + conv.bias
    assert torch.equal(y, want)
    plan = mmf.incidence_plan(dev(ei), N, M, dev(w))
    assert torch.equal(conv(x, plan=plan), y)
    y.sum().backward()
    assert conv.lin.weight.grad is not None and conv.bias.grad is not None and bool(conv.lin.weight.grad.abs().sum() > 0)
    # a torch_geometric checkpoint's keys load
    conv.load_state_dict({"lin.weight": torch.zeros(20, 48), "bias": torch.ones(20)})
    with pytest.raises(NotImplementedError):
        mmf.HypergraphConv(48, 20, use_attention=True)
    with pytest.raises(NotImplementedError):
        mmf.HypergraphConv(48, 20, heads=4)
    with pytest.raises(NotImplementedError):
        conv(x, dev(ei), hyperedge_attr=torch.zeros(M, 48, device="cuda"))


# ---- out-of-range ids -----------------------------------------------------------------------------------------------------------------
def test_out_of_range_ids_are_flagged_by_column_and_left_out(mmf):
    """The C-level plan leaves such pairs out of both CSRs (they are checked before they are counted or turned into a key:
    hg_keys_kernel gives them the key N * M, which sorts behind every valid pair and lies past the last offset), so propagating over
    it is the restatement on the valid pairs; the Python layer reads the status word and raises."""
    N, M = 60, 45
    good = hr.random_incidence(N, M, 400, 29)
    bad = np.array([[N, 5, -1, 2 ** 40, 7, -(2 ** 62)], [3, M, 4, 6, -9, M + 100]], dtype=np.int64)
    ei = np.concatenate([good[:, :100], bad[:, :3], good[:, 100:250], bad[:, 3:], good[:, 250:]], axis=1)
    x, w = hr.features(N, 33, 30), hr.weights(M, 31)
    plan = mmf.incidence_plan(dev(ei), N, M, dev(w), check=False)
    assert plan.status.tolist() == [100, 101]                    # lowest column with a bad node id, with a bad hyperedge id
    assert int(plan.eptr[-1]) == int(plan.nptr[-1]) == 400
    assert int(plan.emem.min()) >= 0 and int(plan.emem.max()) < N and int(plan.nmem.min()) >= 0 and int(plan.nmem.max()) < M
    assert not plan.emem[400:].any() and not plan.nmem[400:].any()
    out, Y = mmf.hypergraph_propagate(dev(x), plan=plan, return_edge_features=True)
    want, want_y = hr.propagate(x, good, M, w)
    same_bits(Y, want_y, "valid pairs only, Y")
    same_bits(out, want, "valid pairs only, out")
    with pytest.raises(ValueError, match=r"edge_index\[0, 100\] is no node id in \[0, 60\)"):
        plan.check()
    with pytest.raises(ValueError, match=r"edge_index\[0, 100\]"):
        mmf.incidence_plan(dev(ei), N, M)
    only_edge = np.concatenate([good[:, :7], np.array([[1], [-3]]), good[:, 7:]], axis=1)
    with pytest.raises(ValueError, match=r"edge_index\[1, 7\] is no hyperedge id in \[0, 45\)"):
        mmf.hypergraph_propagate(dev(x), dev(only_edge), num_edges=M)
    # every pair bad, and no pair at all: an empty plan, zeros
    for cols in (bad, np.zeros((2, 0), dtype=np.int64)):
        p = mmf.incidence_plan(dev(cols), N, M, check=False)
        assert not p.eptr.any() and not p.nptr.any()
        o, y = mmf.hypergraph_propagate(dev(x), plan=p, return_edge_features=True)
        assert not o.any() and not y.any()


# ---- the stream contract --------------------------------------------------------------------------------------------------------------
def test_plan_build_and_propagate_on_a_busy_side_stream(mmf):
    """Both entries enqueue on the caller's stream only and return while the gate in front of their inputs is still closed; the bits
    are those of the idle default stream and of the restatement."""
    import streamgate as sg
    N, M, E, C = 2000, 1500, 30000, 64

    def make_inputs(kind):
        s = 0 if kind == "truth" else 50
        return [torch.from_numpy(hr.random_incidence(N, M, E, 32 + s)), torch.from_numpy(hr.features(N, C, 33 + s)),
                torch.from_numpy(hr.weights(M, 34 + s))]

    def entry(ei, x, w):
        plan = mmf.incidence_plan(ei, N, M, w, check=False)
        out, Y = mmf.hypergraph_propagate(x, plan=plan, return_edge_features=True)
        return [out, Y, plan.status, plan.eptr, plan.nmem]

    def reference(ei, x, w):
        def verdict(got):
            want, want_y = hr.propagate(x, ei, M, w)
            pl = hr.plan(ei, N, M, w)
            return (sg.diff(got[0], want, "out") + sg.diff(got[1], want_y, "Y") + sg.diff(got[2], np.array([-1, -1]), "status") +
                    sg.diff(got[3], pl["eptr"], "eptr") + sg.diff(got[4], pl["nmem"].astype(np.int32), "nmem"))
        return verdict

    sg.run_gated(entry, make_inputs, reference, name="hgconv plan + propagate", nonsync=True, calls=2)
