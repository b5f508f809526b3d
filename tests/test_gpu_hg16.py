"""The 16-bit hypergraph branch on the GPU (include/ext/mmf_hg_hg16.h, multimodal-fusion_amd/hg16.py), bit for bit,
for float16 and bfloat16, against two things: the numpy restatement tests/hg16_restate.py, and the float32 GPU functions composed with
torch casts — Y16 == propagate32(x16.float()).Y.to(T), out16 == (gather32(Y16.float()) [+ bias]).to(T), and the same composition for
the pairs, the transposed forms, grad_a and the readout.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hg16_restate as h16      # noqa: E402
import hgconv_restate as hr     # noqa: E402
import hgpair_restate as hp     # noqa: E402
import readout_restate as rr    # noqa: E402

pytestmark = pytest.mark.gpu
T = {"bf16": torch.bfloat16, "f16": torch.float16}
KINDS = h16.KINDS


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev16(a, kind):
    """A float32 array of 16-bit values on the device in the 16-bit type (the cast is exact)."""
    t = dev(np.asarray(a, dtype=np.float32)).to(T[kind])
    assert torch.equal(t.float().cpu(), torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return t


def same16(got: torch.Tensor, want: np.ndarray, kind, what: str):
    assert got.dtype == T[kind] and tuple(got.shape) == want.shape, (what, got.dtype, tuple(got.shape), want.shape)
    g = got.detach().float().cpu().numpy()
    bad = int(np.count_nonzero(h16.bits(g) != h16.bits(want)))
    assert bad == 0, f"{what} ({kind}): {bad} of {g.size} values differ from the restatement"


def same32(got: torch.Tensor, want: np.ndarray, what: str):
    g = got.detach().cpu().numpy()
    assert g.dtype == np.float32 and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    bad = int(np.count_nonzero(h16.bits(g) != h16.bits(want)))
    assert bad == 0, f"{what}: {bad} of {g.size} values differ from the restatement"


def equal(a: torch.Tensor, b: torch.Tensor, what: str):
    """Same dtype, same shape, same bits (a 16-bit tensor is compared through its integer view: -0 is not +0)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}[a.dtype]
    bad = int((a.contiguous().view(view) != b.contiguous().view(view)).sum())
    assert bad == 0, f"{what}: {bad} of {a.numel()} values differ from the float32 composition"


# ---- the float32 GPU steps the compositions are made of -------------------------------------------------------------------------------
def gather32(mmf, ptr, col, src, scale=None, scale2=None):
    """mmf_csr_gather_sum on a dense float32 src: [rows, C]."""
    rows, C = ptr.numel() - 1, src.shape[1]
    out = torch.empty((rows, C), dtype=torch.float32, device=src.device)
    o = mmf.ops
    o._call("mmf_csr_gather_sum", src.device, o._p(ptr), o._p(col), rows, o._p(src), C, C, o._p(scale), o._p(scale2), o._p(out), C)
    return out


def pair_gather32(mmf, plan, a, src, side, scale=None, scale2=None):
    """One weighted gather step in float32: the first step of mmf_hypergraph_propagate_pairs, which on the plan with the roles of
    nodes and hyperedges exchanged is the node step.  side "edge": rows are hyperedges; "node": rows are nodes."""
    o = mmf.ops
    N, M, C = plan.num_nodes, plan.num_edges, src.shape[1]
    if side == "edge":
        first, second, R1, R2 = (plan.eptr, plan.emem, plan.epos), (plan.nptr, plan.nmem, plan.npos), M, N
    else:
        first, second, R1, R2 = (plan.nptr, plan.nmem, plan.npos), (plan.eptr, plan.emem, plan.epos), N, M
    ones = torch.ones(max(R1, 1), dtype=torch.float32, device=src.device)
    Y = torch.empty((R1, C), dtype=torch.float32, device=src.device)
    rest = torch.empty((R2, C), dtype=torch.float32, device=src.device)
    src = src.contiguous()
    o._call("mmf_hypergraph_propagate_pairs", src.device, o._p(first[0]), o._p(first[1]), o._p(first[2]), o._p(second[0]), o._p(second[1]),
            o._p(second[2]), o._p(ones if scale is None else scale), None, o._p(scale2), o._p(a), plan.num_pairs, o._p(src), C, R2, R1, C, o._p(Y),
            o._p(rest), 1)
    return Y


def comp_plain(mmf, x16, plan, bias=None, transpose=False):
    """(out, Y) of the plain propagation as the float32 GPU functions and torch casts compose it."""
    dt = x16.dtype
    src = x16.float() * plan.node_scale.unsqueeze(1) if transpose else x16.float()
    Y = gather32(mmf, plan.eptr, plan.emem, src.contiguous(), plan.edge_scale, plan.hyperedge_weight).to(dt)
    out = gather32(mmf, plan.nptr, plan.nmem, Y.float(), None if transpose else plan.node_scale)
    if bias is not None and not transpose:
        out = out + bias
    return out.to(dt), Y


def comp_pairs(mmf, x16, a, plan, es, ns, bias=None, transpose=False):
    dt = x16.dtype
    src = x16.float() * ns.unsqueeze(1) if transpose else x16.float()
    Y = pair_gather32(mmf, plan, a, src, "edge", es, plan.hyperedge_weight).to(dt)
    out = pair_gather32(mmf, plan, a, Y.float(), "node", None if transpose else ns)
    if bias is not None and not transpose:
        out = out + bias
    return out.to(dt), Y


def check_plain(mmf, ei, N, M, x, kind, w=None, bias=None, what="", x_dev=None):
    """Forward (with and without bias) and backward of hypergraph_propagate_16 against the restatement and the composition."""
    plan = mmf.incidence_plan(dev(ei), N, M, None if w is None else dev(w))
    xd = (dev16(x, kind) if x_dev is None else x_dev).requires_grad_()
    bd = None if bias is None else dev(bias).requires_grad_()
    out, Y = mmf.hypergraph_propagate_16(xd, plan=plan, bias=bd, return_edge_features=True)
    want, want_y = h16.propagate16(x, ei, M, kind, w, bias)
    same16(Y, want_y, kind, f"{what} Y")
    same16(out, want, kind, f"{what} out")
    c_out, c_y = comp_plain(mmf, xd.detach(), plan, None if bd is None else bd.detach())
    equal(Y, c_y, f"{what} Y")
    equal(out.detach(), c_out, f"{what} out")
    # the plain float32 entry on the widened x gives the same Y in one call
    equal(Y, mmf.hypergraph_propagate(xd.detach().float(), plan=plan, return_edge_features=True)[1].to(T[kind]), f"{what} Y (propagate32)")
    G = h16.features16(N, x.shape[1], 977, kind)
    Gd = dev16(G, kind)
    out.backward(Gd)
    want_gx, _ = h16.propagate16(G, ei, M, kind, w, transpose=True)
    same16(xd.grad, want_gx, kind, f"{what} grad_x")
    equal(xd.grad, comp_plain(mmf, Gd, plan, transpose=True)[0], f"{what} grad_x")
    if bd is not None:
        equal(bd.grad, Gd.sum(0, dtype=torch.float32), f"{what} grad_bias")
    return out.detach(), Y


@pytest.fixture(scope="module")
def base():
    N, M, E = 300, 200, 1500
    return dict(N=N, M=M, E=E, ei=hr.random_incidence(N, M, E, 5), w=hr.weights(M, 6))


# ---- channel counts: both lane forms, L from 1 to 64, two rows per wave, one wave per row, a second column trip ----------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [1, 7, 8, 24, 64, 66, 256, 264, 512, 520])
@pytest.mark.parametrize("kind", KINDS)
def test_bits_over_channel_counts(mmf, base, kind, C, weighted):
    N, M, ei = base["N"], base["M"], base["ei"]
    x = h16.features16(N, C, 7 + C, kind)
    check_plain(mmf, ei, N, M, x, kind, base["w"] if weighted else None, bias=hr.features(1, C, 8 + C)[0] if weighted else None, what=f"C={C}")


@pytest.mark.parametrize("C", [6, 8, 256, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_degrees_around_the_batch_and_the_id_block_and_hubs(mmf, kind, C):
    ei = hr.degree_incidence()
    N, M = int(ei[0].max()) + 1, int(ei[1].max()) + 1
    check_plain(mmf, ei, N, M, h16.features16(N, C, 11, kind), kind, hr.weights(M, 12), what=f"degrees C={C}")
    ei = hr.hub_incidence()
    N, M = 1200, 1100
    check_plain(mmf, ei, N, M, h16.features16(N, C, 13, kind), kind, None, bias=hr.features(1, C, 14)[0], what=f"hubs C={C}")


@pytest.mark.parametrize("kind", KINDS)
def test_empty_rows_a_triple_pair_column_order_and_repeated_calls(mmf, kind):
    # nodes 3 and 7 in no hyperedge, hyperedges 2 and 5 empty, the pair (1, 0) three times
    ei = np.array([[0, 1, 1, 1, 2, 4, 5, 6, 8, 9, 0], [0, 0, 0, 0, 1, 1, 3, 3, 4, 6, 6]], dtype=np.int64)
    N, M, C = 10, 7, 8
    x = h16.features16(N, C, 15, kind)
    bias = hr.features(1, C, 16)[0]
    out, Y = check_plain(mmf, ei, N, M, x, kind, None, bias=bias, what="empty rows")
    assert not Y[2].any() and not Y[5].any()
    same16(out[3:4], h16.r16(bias[None, :], kind), kind, "a node without hyperedges gets the bias")
    out0, _ = check_plain(mmf, ei, N, M, x, kind, None, what="empty rows, no bias")
    assert not out0[3].any() and not out0[7].any() and not out0.view(torch.int16)[3].any()          # +0, not -0
    # the order of the columns does not matter, and two calls give equal bits
    N, M, E, C = 300, 200, 1500, 24
    ei = hr.random_incidence(N, M, E, 17)
    xd = dev16(h16.features16(N, C, 18, kind), kind)
    perm = np.random.RandomState(19).permutation(E)
    a = mmf.hypergraph_propagate_16(xd, dev(ei), num_edges=M, return_edge_features=True)
    b = mmf.hypergraph_propagate_16(xd, dev(ei[:, perm]), num_edges=M, return_edge_features=True)
    c = mmf.hypergraph_propagate_16(xd, dev(ei), num_edges=M, return_edge_features=True)
    for u, v in zip(a + a, b + c):
        equal(u, v, "column order / repeated call")


# ---- views ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("kind", KINDS)
def test_x_as_a_view_of_a_larger_tensor(mmf, base, kind, C):
    N, M, ei = base["N"], base["M"], base["ei"]
    plan = mmf.incidence_plan(dev(ei), N, M, dev(base["w"]))
    big = h16.features16(N + 10, C + 16, 21, kind)
    bd = dev16(big, kind)
    views = {"row slice": (bd[5:5 + N, :C], big[5:5 + N, :C]),                                    # pitch C + 16, base 16-byte aligned: wide form
             "column slice at 8": (bd[:N, 8:8 + C], big[:N, 8:8 + C]),                             # wide form, pitch > C
             "column slice at 3": (bd[:N, 3:3 + C], big[:N, 3:3 + C])}                             # misaligned base: narrow form
    odd = dev16(h16.features16(N, C + 4, 22, kind), kind)                                          # pitch C + 4 with C % 8 == 0: narrow form
    views["pitch C + 4"] = (odd[:, :C], odd[:, :C].float().cpu().numpy())
    for name, (view, host) in views.items():
        assert view.stride(1) == 1 and view.stride(0) > C and view.data_ptr() >= (odd if name == "pitch C + 4" else bd).data_ptr()
        got = mmf.hypergraph_propagate_16(view, plan=plan, return_edge_features=True)
        want = mmf.hypergraph_propagate_16(view.contiguous(), plan=plan, return_edge_features=True)
        for g, w_ in zip(got, want):
            equal(g, w_, name)
        same16(got[0], h16.propagate16(host, ei, M, kind, base["w"])[0], kind, name)
    assert views["column slice at 3"][0].data_ptr() % 16 != 0 and views["column slice at 8"][0].data_ptr() % 16 == 0
    # and the readout reads the same views
    rp = mmf.readout_plan(ptr=[0, 100, 100, N])
    gate = dev(rr.gates(N, 23))
    for name, (view, host) in views.items():
        got = mmf.attention_readout_16(view, gate, plan=rp, return_attention=True)
        want = mmf.attention_readout_16(view.contiguous(), gate, plan=rp, return_attention=True)
        for g, w_ in zip(got, want):
            equal(g, w_, f"readout, {name}")
    # the backward from views: x a column slice of a leaf, the output gradient a column slice of a larger tensor too
    pplan = mmf.incidence_pair_plan(dev(ei), N, M, dev(base["w"]))
    a = dev(hp.pair_weights(ei.shape[1], 24, signed=True))
    g16 = dev16(h16.features16(N, C + 16, 25, kind), kind)
    g32 = dev(rr.features(3, C + 16, 26))

    def grads(op, sl, dense):
        leaf = bd.detach().clone().requires_grad_()
        other = (a if op == "pairs" else gate).clone().requires_grad_()
        xv, g = leaf[:N, sl:sl + C], (g32 if op == "readout" else g16)[:, sl:sl + C]
        if dense:
            xv, g = xv.contiguous(), g.contiguous()
        else:
            assert not xv.is_contiguous() and not g.is_contiguous()
        out = (mmf.hypergraph_propagate_16(xv, plan=plan) if op == "plain" else
               mmf.hypergraph_propagate_pairs_16(xv, other, plan=pplan) if op == "pairs" else mmf.attention_readout_16(xv, other, plan=rp))
        out.backward(g)
        return [leaf.grad] + ([] if op == "plain" else [other.grad])

    for op in ("plain", "pairs", "readout"):
        for sl in (8, 3):                                                      # wide and narrow form of x; grad_a and grad_gate read x by its pitch
            for g, w_ in zip(grads(op, sl, False), grads(op, sl, True)):
                assert bool(g.any())
                equal(g, w_, f"backward from views, {op}, column slice at {sl}")


# ---- rounding -------------------------------------------------------------------------------------------------------------------------
def test_rounding_ties_subnormals_and_overflow(mmf):
    def edge_features(values, kind, C, w=None):
        n = len(values)
        ei = np.array([list(range(n)), [0] * n], dtype=np.int64)
        x = np.repeat(np.asarray(values, dtype=np.float32)[:, None], C, axis=1)
        assert np.array_equal(h16.r16(x, kind), x)
        wv = None if w is None else np.array([w], dtype=np.float32)
        out, Y = mmf.hypergraph_propagate_16(dev16(x, kind), dev(ei), num_edges=1, hyperedge_weight=None if wv is None else dev(wv),
                                             return_edge_features=True)
        want, want_y = h16.propagate16(x, ei, 1, kind, wv)
        same16(Y, want_y, kind, f"Y of {values[:4]}")
        same16(out, want, kind, f"out of {values[:4]}")
        return Y.float().cpu().numpy()

    for C in (1, 8):                                                           # both lane forms
        assert (edge_features([1.0, 1.0078125], "bf16", C) == 1.0).all()                          # mean 1.00390625: a tie, to the even 1.0
        assert (edge_features([1.0078125, 1.015625], "bf16", C) == 1.015625).all()                # mean 1.01171875: a tie, to the even 1.015625
        sub = [(16 + (i % 3)) * 2.0 ** -24 for i in range(64)]                                    # f16 subnormals near 2^-20, B_e = 64
        Y = edge_features(sub, "f16", C)
        assert (Y > 0).all() and (Y < 2.0 ** -14).all()                                           # the subnormal, not zero
        assert (edge_features([60000.0] * 4, "f16", C) == 60000.0).all()                          # the chain runs in float32: 240000 / 4
        assert np.isposinf(edge_features([40000.0], "f16", C, w=2.0)).all()                       # 80000 overflows to +inf


# ---- pairs ----------------------------------------------------------------------------------------------------------------------------
def check_pairs(mmf, ei, N, M, x, a, kind, w=None, normalization="count", bias=None, what="", scales=False):
    plan = mmf.incidence_pair_plan(dev(ei), N, M, None if w is None else dev(w))
    xd, ad = dev16(x, kind).requires_grad_(), dev(a)
    if normalization == "count":
        ad.requires_grad_()
    bd = None if bias is None else dev(bias).requires_grad_()
    sc = mmf.pair_scales(ad.detach(), plan=plan) if scales else None
    out, Y = mmf.hypergraph_propagate_pairs_16(xd, ad, plan=plan, normalization=normalization, scales=sc, bias=bd, return_edge_features=True)
    want, want_y = h16.propagate_pairs16(x, a, ei, M, kind, w, normalization, bias)
    same16(Y, want_y, kind, f"{what} Y")
    same16(out, want, kind, f"{what} out")
    es, ns = (plan.edge_scale, plan.node_scale) if normalization == "count" else mmf.pair_scales(ad.detach(), plan=plan)
    c_out, c_y = comp_pairs(mmf, xd.detach(), ad.detach(), plan, es, ns, None if bd is None else bd.detach())
    equal(Y, c_y, f"{what} Y")
    equal(out.detach(), c_out, f"{what} out")
    equal(Y, mmf.hypergraph_propagate_pairs(xd.detach().float(), ad.detach(), plan=plan, normalization=normalization,
                                            return_edge_features=True)[1].to(T[kind]), f"{what} Y (pairs32)")
    G = h16.features16(N, x.shape[1], 978, kind)
    Gd = dev16(G, kind)
    out.backward(Gd)
    want_gx, want_t = h16.propagate_pairs16(G, a, ei, M, kind, w, normalization, transpose=True)
    same16(xd.grad, want_gx, kind, f"{what} grad_x")
    c_gx, c_t = comp_pairs(mmf, Gd, ad.detach(), plan, es, ns, transpose=True)
    equal(xd.grad, c_gx, f"{what} grad_x")
    same16(c_t, want_t, kind, f"{what} T")
    if bd is not None:
        equal(bd.grad, Gd.sum(0, dtype=torch.float32), f"{what} grad_bias")
    if normalization == "count":
        same32(ad.grad, h16.grad_a16(x, a, G, ei, M, kind, w), f"{what} grad_a")
        # the float32 entry on the widened rows: g' = G16.float() * node_scale, Y16.float(), T16.float()
        o, C = mmf.ops, x.shape[1]
        gp = (Gd.float() * ns.unsqueeze(1)).contiguous()
        x32, y32, t32 = xd.detach().float().contiguous(), Y.float().contiguous(), c_t.float().contiguous()
        ga = torch.empty((plan.num_pairs,), dtype=torch.float32, device="cuda")
        o._call("mmf_pair_weight_grad", ga.device, o._p(plan.eptr), o._p(plan.emem), o._p(plan.epos), o._p(gp), o._p(x32), C, o._p(y32), o._p(t32), N, M,
                C, plan.num_pairs, o._p(ga))
        equal(ad.grad, ga, f"{what} grad_a")
    return out.detach(), Y


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [8, 66, 256, 520])
@pytest.mark.parametrize("kind", KINDS)
def test_pairs_forward_and_gradients(mmf, base, kind, C, weighted):
    N, M = base["N"], base["M"]
    ei = np.concatenate([base["ei"], base["ei"][:, :5]], axis=1)               # five pairs twice, with weights of their own on the copies
    w = base["w"] if weighted else None
    x = h16.features16(N, C, 31 + C, kind)
    a = hp.pair_weights(ei.shape[1], 32, signed=True)
    check_pairs(mmf, ei, N, M, x, a, kind, w, "count", bias=hr.features(1, C, 33)[0], what=f"count C={C}")
    a = hp.pair_weights(ei.shape[1], 34)
    check_pairs(mmf, ei, N, M, x, a, kind, w, "weight", bias=None if weighted else hr.features(1, C, 35)[0], what=f"weight C={C}", scales=weighted)
    # ones reproduce the plain 16-bit call
    ones = torch.ones(ei.shape[1], device="cuda")
    plan = mmf.incidence_pair_plan(dev(ei), N, M, None if w is None else dev(w))
    xd = dev16(x, kind)
    plain = mmf.hypergraph_propagate_16(xd, plan=plan, return_edge_features=True)
    for normalization in ("count", "weight"):
        got = mmf.hypergraph_propagate_pairs_16(xd, ones, plan=plan, normalization=normalization, return_edge_features=True)
        for g, p in zip(got, plain):
            equal(g, p, f"ones, {normalization}")


@pytest.mark.parametrize("kind", KINDS)
def test_pairs_on_hubs_and_the_refusal_under_weight(mmf, kind):
    ei = hr.hub_incidence()
    N, M, C = 1200, 1100, 8
    check_pairs(mmf, ei, N, M, h16.features16(N, C, 36, kind), hp.pair_weights(ei.shape[1], 37, signed=True), kind, None, "count", what="hubs")
    plan = mmf.incidence_pair_plan(dev(ei), N, M)
    with pytest.raises(ValueError, match="requires grad under normalization='weight'"):
        mmf.hypergraph_propagate_pairs_16(dev16(h16.features16(N, C, 36, kind), kind), torch.ones(ei.shape[1], device="cuda", requires_grad=True),
                                          plan=plan, normalization="weight")


# ---- readout --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 8, 24, 256, 520])
@pytest.mark.parametrize("kind", KINDS)
def test_readout_equals_the_float32_call_on_the_widened_x(mmf, kind, C):
    ptr = rr.offsets(rr.EDGE_SIZES)                                           # empty, 1, 63 / 64 / 65, several chunks, one long segment
    N, S = int(ptr[-1]), ptr.size - 1
    x = h16.features16(N, C, 41 + C, kind)
    gate = rr.gates(N, 42)
    plan = mmf.readout_plan(ptr=ptr.tolist())
    xd, gd = dev16(x, kind).requires_grad_(), dev(gate).requires_grad_()
    got = mmf.hg16._Readout16.apply(xd, gd, plan)
    x32, g32 = xd.detach().float().requires_grad_(), gd.detach().clone().requires_grad_()
    ref = mmf.readout._Readout.apply(x32, g32, plan)
    for g, r, name in zip(got, ref, ("out", "alpha", "seg_max", "seg_sum")):
        equal(g.detach(), r.detach(), name)
    want = h16.readout16(x, gate, ptr)
    for g, w_, name in zip(got, want, ("out", "alpha", "seg_max", "seg_sum")):
        same32(g, w_, name)
    G = rr.features(S, C, 43)
    got[0].backward(dev(G))
    ref[0].backward(dev(G))
    equal(xd.grad, x32.grad.to(T[kind]), "grad_x")
    equal(gd.grad, g32.grad, "grad_gate")
    want_gx, want_gg = h16.readout_backward16(x, ptr, want[1], want[0], G, kind)
    same16(xd.grad, want_gx, kind, "grad_x")
    same32(gd.grad, want_gg, "grad_gate")
    # the public function: a 16-bit gate is widened, the gate's share of the backward is skipped without a gradient in it
    x2 = dev16(x, kind).requires_grad_()
    out, alpha = mmf.attention_readout_16(x2, dev(gate).to(T[kind]), ptr=ptr.tolist(), return_attention=True)
    ref_out, ref_alpha = mmf.attention_readout(x2.detach().float(), dev(gate).to(T[kind]).float(), ptr=ptr.tolist(), return_attention=True)
    assert out.dtype == torch.float32
    equal(out.detach(), ref_out, "out (16-bit gate)")
    equal(alpha, ref_alpha, "alpha (16-bit gate)")
    out.backward(dev(G))
    equal(x2.grad, (ref_alpha.unsqueeze(1) * dev(G)[dev(np.repeat(np.arange(S), np.diff(ptr)))]).to(T[kind]), "grad_x without the gate")


# ---- modules under autocast -----------------------------------------------------------------------------------------------------------
def cohort(mmf, C, seed):
    """Three graphs of 150 / 90 / 60 nodes: block-diagonal incidence with global ids, batch vector, features."""
    sizes, ms = (150, 90, 60), (100, 60, 40)
    v, e, n0, m0 = [], [], 0, 0
    for i, (n, m) in enumerate(zip(sizes, ms)):
        ei = hr.random_incidence(n, m, 5 * n, seed + i)
        v.append(ei[0] + n0)
        e.append(ei[1] + m0)
        n0, m0 = n0 + n, m0 + m
    ei = np.stack([np.concatenate(v), np.concatenate(e)]).astype(np.int64)
    batch = np.repeat(np.arange(3), sizes).astype(np.int64)
    return ei, n0, m0, batch, hr.features(n0, C, seed + 9)


@pytest.mark.parametrize("kind", KINDS)
def test_modules_under_autocast_equal_the_cast_compositions(mmf, kind, monkeypatch):
    dt = T[kind]
    ei, N, M, batch, x = cohort(mmf, 32, 50)
    eid, xd, bd = dev(ei), dev(x), dev(batch)
    torch.manual_seed(3)
    pw = dev(hp.pair_weights(ei.shape[1], 51))
    plan = mmf.incidence_pair_plan(eid, N, M)
    conv = mmf.HypergraphConv(32, 48).cuda().eval()
    pconv = mmf.PairWeightedHypergraphConv(32, 48).cuda().eval()
    att = mmf.HypergraphAttentionConv(32, 16, heads=3).cuda().eval()
    att_mean = mmf.HypergraphAttentionConv(32, 16, heads=2, concat=False, attention_mode="edge").cuda().eval()
    pool = mmf.GlobalAttention(torch.nn.Sequential(torch.nn.Linear(32, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))).cuda().eval()
    net = mmf.HypergraphNetwork(32, [48, 48], 48).cuda().eval()
    with torch.no_grad():
        for m_ in (conv, pconv, att, att_mean):
            m_.bias.normal_()                                                  # a bias that matters
        for c in net.convs:
            c.bias.normal_()
    hattr = dev(hr.features(M, 32, 52))

    def run():
        with torch.no_grad(), torch.autocast("cuda", dtype=dt):
            return [conv(xd, plan=plan), conv(xd, eid, num_edges=M), pconv(xd, pair_weight=pw, plan=plan), att(xd, eid, hyperedge_attr=hattr, plan=plan),
                    att_mean(xd, eid, hyperedge_attr=hattr, num_edges=M), pool(xd.to(dt), bd), net(xd, eid, bd), net(xd, eid, bd, return_attention=True)[1]]

    got = run()
    for o in got[:5]:
        assert o.dtype == dt                                                   # the conv outputs keep the autocast type
    assert got[0].shape == (N, 48) and got[3].shape == (N, 48) and got[4].shape == (N, 16)
    assert got[5].dtype == torch.float32 and got[6].dtype == torch.float32 and got[6].shape == (3, 48)
    equal(got[0], got[1], "plan and edge_index")
    calls = {"plain": 0, "pairs": 0, "readout": 0}

    def plain_c(x16, edge_index=None, *, plan=None, num_edges=None, hyperedge_weight=None, bias=None, return_edge_features=False):
        calls["plain"] += 1
        p = plan if plan is not None else mmf.incidence_plan(edge_index, x16.shape[0], num_edges, hyperedge_weight)
        return comp_plain(mmf, x16, p, bias)[0]

    def pairs_c(x16, a, *, plan, normalization="count", scales=None, bias=None, return_edge_features=False):
        calls["pairs"] += 1
        es, ns = (plan.edge_scale, plan.node_scale) if normalization == "count" else mmf.pair_scales(a, plan=plan)
        return comp_pairs(mmf, x16.contiguous(), a.contiguous(), plan, es, ns, bias)[0]

    def readout_c(x16, gate, ptr=None, batch=None, *, plan=None, size=None, return_attention=False):
        calls["readout"] += 1
        return mmf.attention_readout(x16.float(), gate.float(), ptr=ptr, batch=batch, plan=plan, size=size, return_attention=return_attention)

    monkeypatch.setattr(mmf.hg16, "hypergraph_propagate_16", plain_c)
    monkeypatch.setattr(mmf.hg16, "hypergraph_propagate_pairs_16", pairs_c)
    monkeypatch.setattr(mmf.hg16, "attention_readout_16", readout_c)
    want = run()
    monkeypatch.undo()
    assert calls == {"plain": 2 + 2 * len(net.convs), "pairs": 1 + 3 + 2, "readout": 3}           # every 16-bit operator was replaced
    for g, w_, name in zip(got, want, ("HypergraphConv", "HypergraphConv (edge_index)", "PairWeightedHypergraphConv", "HypergraphAttentionConv",
                                       "HypergraphAttentionConv (mean)", "GlobalAttention", "HypergraphNetwork", "HypergraphNetwork alpha")):
        equal(g, w_, name)
    # float32 inputs take today's path
    assert conv(xd, plan=plan).dtype == torch.float32 and pool(xd, bd).dtype == torch.float32
    # a HypergraphConv checkpoint loads, and one training step runs: finite gradients in every parameter
    fresh = mmf.HypergraphConv(32, 48).cuda().eval()
    fresh.load_state_dict(conv.state_dict())
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        equal(fresh(xd, plan=plan), got[0], "a HypergraphConv checkpoint, loaded and run under autocast")
    pconv.load_state_dict(conv.state_dict())                                   # and into the pair-weighted layer, whose keys are the same
    train = mmf.HypergraphNetwork(32, [48, 48], 48).cuda().train()
    train.load_state_dict(net.state_dict())
    with torch.autocast("cuda", dtype=dt):
        token = train(xd, eid, bd)
        loss = token.float().square().mean()
    loss.backward()
    for name, p in train.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
    assert float(train.convs[0].lin.weight.grad.abs().max()) > 0
    att.train()
    with torch.autocast("cuda", dtype=dt):
        att(xd, eid, hyperedge_attr=hattr, plan=plan).float().square().mean().backward()
    for name, p in att.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


# ---- the stream contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_backward_on_a_busy_side_stream(mmf, kind):
    """Forward and backward of all three functions enqueue on the caller's stream only and return while the gate in front of their
    inputs is still closed; the bits are those of the idle default stream and of the restatement."""
    import streamgate as sg
    N, M, E, C = 2000, 1500, 30000, 64
    ptr = [0, 700, 700, 1300, N]

    def make_inputs(which):
        s = 0 if which == "truth" else 50
        return [torch.from_numpy(hr.random_incidence(N, M, E, 61 + s)), torch.from_numpy(h16.features16(N, C, 62 + s, kind)).to(T[kind]),
                torch.from_numpy(hr.weights(M, 63 + s)), torch.from_numpy(hp.pair_weights(E, 64 + s)), torch.from_numpy(rr.gates(N, 65 + s)),
                torch.from_numpy(h16.features16(N, C, 66 + s, kind)).to(T[kind]), torch.from_numpy(hr.features(1, C, 67 + s)[0])]

    def entry(ei, x, w, a, gate, G, bias):
        plan = mmf.incidence_pair_plan(ei, N, M, w, check=False)
        rp = mmf.readout_plan(ptr=ptr, device=x.device)
        x1, b1 = x.clone().requires_grad_(), bias.clone().requires_grad_()
        out, Y = mmf.hypergraph_propagate_16(x1, plan=plan, bias=b1, return_edge_features=True)
        out.backward(G)
        x2, a2 = x.clone().requires_grad_(), a.clone().requires_grad_()
        po = mmf.hypergraph_propagate_pairs_16(x2, a2, plan=plan, bias=bias)
        po.backward(G)
        x3, g3 = x.clone().requires_grad_(), gate.clone().requires_grad_()
        tok = mmf.attention_readout_16(x3, g3, plan=rp)
        tok.backward(tok.detach())
        return [out.detach(), Y, x1.grad, b1.grad, po.detach(), x2.grad, a2.grad, tok.detach(), x3.grad, g3.grad]

    def reference(ei, x, w, a, gate, G, bias):
        def verdict(got):
            want, want_y = h16.propagate16(x, ei, M, kind, w, bias)
            tok = h16.readout16(x, gate, np.array(ptr))[0]
            return (sg.diff(got[0], want, "out") + sg.diff(got[1], want_y, "Y") +
                    sg.diff(got[2], h16.propagate16(G, ei, M, kind, w, transpose=True)[0], "grad_x") +
                    sg.diff(got[4], h16.propagate_pairs16(x, a, ei, M, kind, w, bias=bias)[0], "out (pairs)") +
                    sg.diff(got[6], h16.grad_a16(x, a, G, ei, M, kind, w), "grad_a") + sg.diff(got[7], tok, "token"))
        return verdict

    sg.run_gated(entry, make_inputs, reference, name=f"hg16 {kind}: propagate, pairs, readout, forward and backward", nonsync=True, calls=2)
