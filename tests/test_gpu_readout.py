"""The attention readout on the GPU (mmf.readout, include/ext/mmf_hg_readout.h): out, alpha, seg_max and seg_sum have
the BITS of the numpy restatement (tests/readout_restate.py) on every path of the kernels (float4 / scalar, one wave per chunk /
several chunks per wave, column trips, batches of 8, empty segments, one chunk and many), for x as a slice of a larger tensor and for
extreme gates; the backward has the restatement's bits with and without the gate's gradient; calls repeat bit for bit; GlobalAttention
and HypergraphNetwork are the composition of their parts and match float64 restatements within derived bounds; plan build, forward
and backward keep the stream contract (tests/streamgate.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hgconv_restate as hr      # noqa: E402
import readout_restate as rr     # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got: torch.Tensor, want: np.ndarray, what: str):
    g = got.detach().cpu().numpy()
    assert g.shape == want.shape and g.dtype == np.float32, (what, g.shape, want.shape, g.dtype)
    bad = int(np.count_nonzero(rr.bits(g) != rr.bits(want)))
    with np.errstate(invalid="ignore"):
        assert bad == 0, f"{what}: {bad} of {g.size} values differ from the restatement (max |diff| {np.nanmax(np.abs(g - want)):.3e})"


def run(mmf, x, gate, ptr, x_dev=None):
    """The four results of one call over a fresh plan."""
    plan = mmf.readout_plan(ptr=torch.from_numpy(np.asarray(ptr)))
    from multimodal_fusion_amd.readout import _Readout
    return _Readout.apply(dev(x) if x_dev is None else x_dev, dev(gate), plan)


def check(mmf, x, gate, ptr, what, x_dev=None):
    out, alpha, seg_max, seg_sum = run(mmf, x, gate, ptr, x_dev)
    w_out, w_alpha, w_max, w_sum = rr.forward(x, gate, ptr)
    same_bits(seg_max, w_max, what + " seg_max")
    same_bits(seg_sum, w_sum, what + " seg_sum")
    same_bits(alpha, w_alpha, what + " alpha")
    same_bits(out, w_out, what + " out")
    return out, alpha


@pytest.fixture(scope="module")
def edge():
    ptr = rr.offsets(rr.EDGE_SIZES)
    return ptr, rr.gates(int(ptr[-1]), 1)


# ---- bits on every path of the kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4, 16, 64, 65, 256, 300])
def test_bits_over_channel_counts(mmf, edge, C):
    """Segments of 0, 1, 63, 64, 65, 127, 128, 129, 0, 1000, 7 rows: the chunk edges, the batch-of-8 edges, an empty segment first and
    in the middle, and one of 16 chunks."""
    ptr, gate = edge
    x = rr.features(int(ptr[-1]), C, 2 + C)
    out, alpha = check(mmf, x, gate, ptr, f"C={C}")
    assert not out[0].any() and not out[8].any()
    o64, a64 = rr.reference64(x, gate, ptr)
    err = np.abs(out.cpu().numpy().astype(np.float64) - o64)
    tol = rr.bound(x, gate, ptr)
    print(f"C={C}: max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()


def test_x_as_a_slice_of_a_larger_tensor(mmf, edge):
    ptr, gate = edge
    N = int(ptr[-1])
    big = torch.from_numpy(rr.features(N + 20, 100, 3)).cuda()
    for what, view in (("rows 10.. of [N + 20, 100]", big[10:10 + N]), ("columns 4..68: pitch 100, aligned", big[:N, 4:68]),
                       ("columns 1..65: pitch 100, unaligned", big[:N, 1:65]), ("columns 0..3", big[5:5 + N, 0:3]),
                       ("every second column: copied", big[:N, ::2][:, :32])):
        check(mmf, view.cpu().numpy(), gate, ptr, what, x_dev=view)


def test_gate_shapes(mmf):
    sizes = (200, 64, 130, 5)
    ptr = rr.offsets(sizes)
    N = int(ptr[-1])
    x = rr.features(N, 40, 4)
    # all equal: every e is 1, alpha = 1 / n_s up to the rounding of the chain
    out, alpha = check(mmf, x, np.full(N, 0.75, dtype=np.float32), ptr, "equal gates")
    assert float(alpha[:200].max()) == float(alpha[:200].min()) == float(np.float32(1.0) / np.float32(200.0))
    # one row ahead of the rest by more than 87: its alpha is exactly 1, the others exactly 0, out is that row
    g = rr.gates(N, 5, scale=1.0)
    for s, lead in enumerate((17, 200 + 63, 264 + 129, 394 + 2)):
        g[lead] = 100.0 + s
    out, alpha = check(mmf, x, g, ptr, "a leading row")
    a = alpha.cpu().numpy()
    assert a.sum() == 4.0 and all(a[i] == 1.0 for i in (17, 263, 393, 396))
    assert np.array_equal(out.cpu().numpy(), x[[17, 263, 393, 396]])
    # magnitudes around +-1e4
    g = (1e4 * np.random.RandomState(6).choice([-1.0, 1.0], size=N) + 10.0 * np.random.RandomState(7).randn(N)).astype(np.float32)
    check(mmf, x, g, ptr, "gates around +-1e4")
    # the maximum in the last row of the last chunk of every segment
    g = rr.gates(N, 8)
    g[ptr[1:] - 1] = 20.0
    out, _ = check(mmf, x, g, ptr, "maximum in the last row")
    assert np.isfinite(out.cpu().numpy()).all()


# ---- backward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [40, 256, 16])
@pytest.mark.parametrize("gate_grad", [True, False])
def test_backward_bits(mmf, edge, C, gate_grad):
    ptr, gate = edge
    N, S = int(ptr[-1]), ptr.size - 1
    x0, G = rr.features(N, C, 9 + C), rr.features(S, C, 10 + C)
    x = dev(x0).requires_grad_()
    g = dev(gate).requires_grad_(gate_grad)
    plan = mmf.readout_plan(ptr=torch.from_numpy(ptr))
    out, alpha = mmf.attention_readout(x, g, plan=plan, return_attention=True)
    assert not alpha.requires_grad
    out.backward(dev(G))
    w_out, w_alpha, _, _ = rr.forward(x0, gate, ptr)
    gx, gg = rr.backward(x0, ptr, w_alpha, w_out, G)
    same_bits(x.grad, gx, f"C={C} x.grad")
    if gate_grad:
        same_bits(g.grad, gg, f"C={C} gate.grad")
        gx64, gg64 = rr.backward64(x0, gate, ptr, G)
        tol_x, tol_g = rr.bound_backward(x0, gate, ptr, G)
        ex, eg = np.abs(x.grad.cpu().numpy() - gx64), np.abs(g.grad.cpu().numpy() - gg64)
        print(f"C={C}: grad_x max err / bound = {np.max(ex / np.maximum(tol_x, 1e-300)):.3f}, grad_gate {np.max(eg / np.maximum(tol_g, 1e-300)):.3f}")
        assert (ex <= tol_x).all() and (eg <= tol_g).all()
    else:
        assert g.grad is None
    # gate [N, 1], as a gate network gives it
    x2, g2 = dev(x0).requires_grad_(), dev(gate).reshape(N, 1).requires_grad_(gate_grad)
    mmf.attention_readout(x2, g2, plan=plan).backward(dev(G))
    assert torch.equal(x2.grad, x.grad) and (not gate_grad or (g2.grad.shape == (N, 1) and torch.equal(g2.grad.reshape(N), g.grad)))


# ---- repeatability --------------------------------------------------------------------------------------------------------------------
def test_repeated_calls_and_both_descriptions_give_the_same_bits(mmf, edge):
    ptr, gate = edge
    N = int(ptr[-1])
    x, g = dev(rr.features(N, 96, 11)), dev(gate)
    plan = mmf.readout_plan(ptr=torch.from_numpy(ptr))
    a = mmf.attention_readout(x, g, plan=plan, return_attention=True)
    b = mmf.attention_readout(x, g, plan=plan, return_attention=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    batch = torch.from_numpy(np.repeat(np.arange(ptr.size - 1), np.diff(ptr)))
    for desc in (dict(batch=batch, size=ptr.size - 1), dict(batch=batch.cuda(), size=ptr.size - 1), dict(ptr=ptr.tolist()),
                 dict(plan=mmf.readout_plan(batch=batch, size=ptr.size - 1))):
        c = mmf.attention_readout(x, g, return_attention=True, **desc)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # a batch vector ends at its last id: without size the trailing segments are absent, the rest is the same
    short = mmf.attention_readout(x, g, batch=batch)
    assert short.shape[0] == int(batch.max()) + 1 and torch.equal(short, a[0][:short.shape[0]])
    # one slide: batch=None is ptr = [0, 200] is the reference's batch = zeros
    x1, g1 = x[:200], g[:200]
    one = mmf.attention_readout(x1, g1)
    assert one.shape == (1, 96) and torch.equal(one, mmf.attention_readout(x1, g1, ptr=[0, 200]))
    assert torch.equal(one, mmf.attention_readout(x1, g1, batch=torch.zeros(200, dtype=torch.int64, device="cuda")))
    # no rows at all
    none = mmf.attention_readout(x[:0], g[:0], ptr=[0, 0, 0], return_attention=True)
    assert none[0].shape == (2, 96) and not none[0].any() and none[1].shape == (0,)


def test_mid_size(mmf):
    sizes = rr.ragged_sizes(37, 20000, 12)
    assert (sizes == 0).any() and sizes.max() > 1000
    ptr = rr.offsets(sizes)
    check(mmf, rr.features(20000, 128, 13), rr.gates(20000, 14), ptr, "mid size")


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def test_global_attention_module(mmf, edge):
    ptr, _ = edge
    N = int(ptr[-1])
    torch.manual_seed(0)
    gate_nn = torch.nn.Sequential(torch.nn.Linear(24, 12), torch.nn.Tanh(), torch.nn.Linear(12, 1))
    pool = mmf.GlobalAttention(gate_nn, torch.nn.Linear(24, 10)).cuda()
    assert sorted(pool.state_dict()) == ["gate_nn.0.bias", "gate_nn.0.weight", "gate_nn.2.bias", "gate_nn.2.weight", "nn.bias", "nn.weight"]
    x = dev(rr.features(N, 24, 15))
    plan = mmf.readout_plan(ptr=torch.from_numpy(ptr))
    y, alpha = pool(x, plan=plan, return_attention=True)
    want, want_a = mmf.attention_readout(pool.nn(x), pool.gate_nn(x), plan=plan, return_attention=True)
    assert y.shape == (ptr.size - 1, 10) and torch.equal(y, want) and torch.equal(alpha, want_a)
    assert torch.equal(pool(x, ptr=torch.from_numpy(ptr)), y)
    y.sum().backward()
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in pool.parameters())
    plain = mmf.GlobalAttention(gate_nn)
    assert plain.nn is None and torch.equal(plain(x, plan=plan), mmf.attention_readout(x, gate_nn(x), plan=plan))


def golden_batch():
    """The three g5 slides as one batch: node and hyperedge ids offset per slide (a block-diagonal incidence), batch = the slide."""
    g = load_golden("g5_knn_kmeans.npz")
    eis, batch, n0, m0 = [], [], 0, 0
    for s, tag in enumerate(("small", "zero", "mid")):
        ei = g[f"{tag}_ei_sorted"].astype(np.int64)
        n = g[f"{tag}_W"].shape[0] + g[f"{tag}_T"].shape[0]
        eis.append(ei + np.array([[n0], [m0]]))
        batch += [s] * n
        n0, m0 = n0 + n, m0 + int(ei[1].max()) + 1
    return np.concatenate(eis, axis=1), np.array(batch, dtype=np.int64), n0, m0


def test_hypergraph_network_against_its_parts_and_float64(mmf):
    """eval(): the module is first_h -> conv -> output_layer -> attention_pool of its own parts, bit for bit.  Against float64 a
    running error bound E is carried beside the float64 values, layer by layer (eps = 2^-24):
      Linear [K inputs]   E' = |W| E + (K + 2) eps (|W| |h| + |b|)       (any summation order of K products, the bias add)
      BatchNorm (eval)    y = (h - mean) * rsqrt(var + 1e-5) * w + b:  E' = s E + 6 eps (s (|h| + |mean|) + |b|), s = |w| / sqrt(var + 1e-5)
      ReLU                E' = E;   Tanh  E' = E + 4 eps (|tanh'| <= 1, a few ulps of the device's tanh on a value below 1)
      propagate           E' = P E + hgconv's bound (tests/hgconv_restate.py), P >= 0
      readout             a gate error of at most Eg moves every alpha_i by a relative 2 Eg (1 + 2 Eg) (numerator and denominator, each
                          within exp(+-Eg)):  E' = 2 Eg (1 + 2 Eg) (alpha64 |h|) + alpha64 E + rr.bound (1 + 2 Eg)
    each with a factor (1 + 2^-10) for the second order."""
    ei, batch, N, M = golden_batch()
    torch.manual_seed(1)
    net = mmf.HypergraphNetwork(32, [48, 40, 24], 24, dropout=0.2).cuda().eval()
    with torch.no_grad():
        net.first_h[1].running_mean.copy_(torch.linspace(-0.2, 0.2, 48))
        net.first_h[1].running_var.copy_(torch.linspace(0.5, 1.5, 48))
        for conv in net.convs:
            conv.bias.copy_(torch.linspace(-0.1, 0.1, conv.out_channels))
    x = dev(rr.features(N, 32, 16))
    b = dev(batch)
    y, alpha = net(x, dev(ei), b, return_attention=True)
    assert y.shape == (3, 24) and alpha.shape == (N,)
    # the composition of its parts
    with torch.no_grad():
        plan = mmf.incidence_plan(dev(ei), N)
        h = net.first_h(x)
        for conv in net.convs:
            h = conv(h, plan=plan)
        h = net.output_layer(h)
        want = net.attention_pool(h, b)
    assert torch.equal(y.detach(), want)
    rplan = mmf.readout_plan(batch=b)
    assert torch.equal(net(x, None, None, incidence=plan, readout=rplan), y)
    # float64 with the running bound
    second = 1 + 2.0 ** -10
    P, max_b, max_deg = hr.dense_operator(ei, N, M)
    sd = {k: v.detach().cpu().double().numpy() for k, v in net.state_dict().items()}

    def linear(h, E, W, bias):
        K = W.shape[1]
        return h @ W.T + bias, E @ np.abs(W).T + (K + 2) * EPS * second * (np.abs(h) @ np.abs(W).T + np.abs(bias))

    h, E = x.cpu().double().numpy(), np.zeros((N, 32))
    h, E = linear(h, E, sd["first_h.0.weight"], sd["first_h.0.bias"])
    s = np.abs(sd["first_h.1.weight"]) / np.sqrt(sd["first_h.1.running_var"] + 1e-5)
    E = s * E + 6 * EPS * second * (s * (np.abs(h) + np.abs(sd["first_h.1.running_mean"])) + np.abs(sd["first_h.1.bias"]))
    h = (h - sd["first_h.1.running_mean"]) / np.sqrt(sd["first_h.1.running_var"] + 1e-5) * sd["first_h.1.weight"] + sd["first_h.1.bias"]
    h = np.maximum(h, 0.0)
    for i in range(2):
        h, E = linear(h, E, sd[f"convs.{i}.lin.weight"], np.zeros(sd[f"convs.{i}.bias"].shape))
        E = P @ E + hr.bound(P, h, max_b, max_deg) * second + EPS * (np.abs(P @ h) + np.abs(sd[f"convs.{i}.bias"]))
        h = P @ h + sd[f"convs.{i}.bias"]
    h, E = linear(h, E, sd["output_layer.weight"], sd["output_layer.bias"])
    t, Et = linear(h, E, sd["attention_pool.gate_nn.0.weight"], sd["attention_pool.gate_nn.0.bias"])
    t, Et = np.tanh(t), Et + 4 * EPS
    gate, Eg = linear(t, Et, sd["attention_pool.gate_nn.2.weight"], sd["attention_pool.gate_nn.2.bias"])
    ptr = rr.offsets(np.bincount(batch))
    o64, a64 = rr.reference64(h, gate[:, 0], ptr)
    eg = float(Eg.max())
    seg = np.repeat(np.arange(3), np.diff(ptr))
    ah, aE = np.zeros((3, 24)), np.zeros((3, 24))
    np.add.at(ah, seg, a64[:, None] * np.abs(h))
    np.add.at(aE, seg, a64[:, None] * E)
    tol = (2 * eg * (1 + 2 * eg) * ah + aE + rr.bound(h, gate[:, 0], ptr) * (1 + 2 * eg)) * second
    err = np.abs(y.detach().cpu().double().numpy() - o64)
    print(f"HypergraphNetwork against float64: max err {err.max():.3e}, max err / bound = {np.max(err / tol):.3f}, gate error bound {eg:.3e}")
    assert eg < 1e-2 and (err <= tol).all()
    assert np.abs(alpha.cpu().double().numpy() - a64).max() <= 2 * eg * (1 + 2 * eg) + float(rr.alpha_rel(gate[:, 0], ptr).max()) + rr.FLUSH
    # training: every parameter receives a gradient
    net.train()
    net(x, dev(ei), b).square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0) for p in net.parameters())
    with pytest.raises(NotImplementedError):
        mmf.HypergraphNetwork(32, [48, 40], 20, use_attention=True)


# ---- the stream contract --------------------------------------------------------------------------------------------------------------
def test_plan_forward_and_backward_on_a_busy_side_stream(mmf):
    """Plan build, forward and backward enqueue on the caller's stream only and return while the gate in front of their inputs is still
    closed; the bits are those of the idle default stream and of the restatement."""
    import streamgate as sg
    N, C = 2000, 64
    sizes = rr.ragged_sizes(9, N, 17)
    ptr = rr.offsets(sizes)

    def make_inputs(kind):
        s = 0 if kind == "truth" else 50
        return [torch.from_numpy(rr.features(N, C, 18 + s)), torch.from_numpy(rr.gates(N, 19 + s)), torch.from_numpy(rr.features(9, C, 20 + s))]

    def entry(x, gate, G):
        plan = mmf.readout_plan(ptr=ptr.tolist(), device=x.device)
        xx, gg = x.detach().clone().requires_grad_(), gate.detach().clone().requires_grad_()
        out, alpha = mmf.attention_readout(xx, gg, plan=plan, return_attention=True)
        out.backward(G)
        return [out.detach(), alpha, xx.grad, gg.grad, plan.ptr, plan.table]

    def reference(x, gate, G):
        def verdict(got):
            w_out, w_alpha, _, _ = rr.forward(x, gate, ptr)
            gx, gg = rr.backward(x, ptr, w_alpha, w_out, G)
            return (sg.diff(got[0], w_out, "out") + sg.diff(got[1], w_alpha, "alpha") + sg.diff(got[2], gx, "x.grad") +
                    sg.diff(got[3], gg, "gate.grad") + sg.diff(got[4], ptr, "ptr") + sg.diff(got[5], rr.chunk_table(ptr), "table"))
        return verdict

    sg.run_gated(entry, make_inputs, reference, name="readout plan + forward + backward", nonsync=True, calls=2)
