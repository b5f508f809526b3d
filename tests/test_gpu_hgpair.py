"""Pair-weighted hypergraph propagation and the softmax over pairs on the GPU (mmf.hgpair, include/ext/mmf_hg_hgpair.h, DESIGN.md
§4.37): the pair plan has the arrays of the plain plan and the positions of a stable sort; out, Y, both scale vectors, grad_x, grad_a,
alpha and grad_score have the BITS of the numpy restatement (tests/hgpair_restate.py) on every path of the kernels (float4 / scalar,
one wave per row / several rows per wave, column chunks, id blocks of 64, batches of 8, softmax rows around the wave size); ones
reproduce hypergraph_propagate; everything stays within the derived bounds of float64; the two modules are the float64 composition
of their definition within a bound derived from the operator bounds; the entries keep the stream contract (tests/streamgate.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hgconv_restate as hr      # noqa: E402
import hgpair_restate as hp      # noqa: E402

pytestmark = pytest.mark.gpu
EPS = hp.EPS


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got: torch.Tensor, want: np.ndarray, what: str):
    g = got.detach().cpu().numpy()
    assert g.shape == want.shape and g.dtype == np.float32, (what, g.shape, want.shape, g.dtype)
    bad = int(np.count_nonzero(hp.bits(g) != hp.bits(want)))
    assert bad == 0, f"{what}: {bad} of {g.size} values differ from the restatement (max |diff| {np.nanmax(np.abs(g - want)):.3e})"


def check_plan(mmf, ei, N, M, w=None, check=True):
    """The pair plan on the device against the restatement and against the plain plan; returns (plan, restated plan)."""
    plan = mmf.incidence_pair_plan(dev(ei), N, M, None if w is None else dev(w), check=check)
    plain = mmf.incidence_plan(dev(ei), N, M, None if w is None else dev(w), check=check)
    for name in ("eptr", "emem", "nptr", "nmem", "edge_scale", "node_scale", "status"):
        assert torch.equal(getattr(plan, name), getattr(plain, name)), name
    pl = hp.plan(ei, N, M, w)
    n = int(pl["eptr"][-1])
    for name in ("epos", "npos"):
        got = getattr(plan, name).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got[:n], pl[name]) and not got[n:].any(), name
    return plan, pl


def check(mmf, ei, N, M, x, a, w=None, what="", x_dev=None, grads=True, G=None):
    """Forward in both normalisations (out, Y, scales), the gradient in x in both and in a under "count", against the restatement."""
    plan, pl = check_plan(mmf, ei, N, M, w)
    G = hr.features(N, x.shape[1], 77) if G is None else G
    for mode in ("count", "weight"):
        xd = (dev(x) if x_dev is None else x_dev).detach().requires_grad_(grads)
        ad = dev(a).requires_grad_(grads and mode == "count")
        out, Y = mmf.hypergraph_propagate_pairs(xd, ad, plan=plan, normalization=mode, return_edge_features=True)
        want, want_y = hp.propagate(x, a, ei, M, w, mode, pl=pl)
        same_bits(Y, want_y, f"{what} {mode} Y")
        same_bits(out, want, f"{what} {mode} out")
        if mode == "weight":
            es, ns = mmf.pair_scales(dev(a), plan=plan)
            wes, wns = hp.scales(pl, a, "weight")
            same_bits(es, wes, f"{what} edge_scale")
            same_bits(ns, wns, f"{what} node_scale")
            out2 = mmf.hypergraph_propagate_pairs(xd.detach(), dev(a), plan=plan, normalization=mode, scales=(es, ns))
            assert torch.equal(out2, out.detach())
        if grads:
            out.backward(dev(G))
            want_gx, _ = hp.propagate(G, a, ei, M, w, mode, transpose=True, pl=pl)
            same_bits(xd.grad, want_gx, f"{what} {mode} grad_x")
            if mode == "count":
                same_bits(ad.grad, hp.grad_a(x, a, G, ei, M, w, pl=pl), f"{what} grad_a")
    return plan, pl


BASE = dict(N=300, M=200, E=1500)


@pytest.fixture(scope="module")
def base():
    ei = hr.random_incidence(BASE["N"], BASE["M"], BASE["E"], 1)
    return ei, hr.weights(BASE["M"], 2), hp.pair_weights(BASE["E"], 3, signed=False)


# ---- bits on every path of the kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 16, 64, 65, 256, 300])
@pytest.mark.parametrize("weighted", [False, True])
def test_bits_over_channel_counts(mmf, base, C, weighted):
    ei, w, a = base
    check(mmf, ei, BASE["N"], BASE["M"], hr.features(BASE["N"], C, 3 + C), a, w if weighted else None, f"C={C}")


@pytest.mark.parametrize("C", [64, 256, 6])
def test_hub_rows_next_to_rows_of_degree_one(mmf, C):
    ei = hr.hub_incidence()
    N, M = 1200, 1100
    a = hp.pair_weights(ei.shape[1], 4)
    check(mmf, ei, N, M, hr.features(N, C, 11), a, None, "hubs")
    check(mmf, ei, N, M, hr.features(N, C, 11), a, hr.weights(M, 12), "hubs, weighted")


@pytest.mark.parametrize("C", [4, 32, 256, 7])
def test_degrees_around_the_batch_and_the_id_block(mmf, C):
    ei = hr.degree_incidence()
    N, M = 110, 10 + 70 * 6
    a = hp.pair_weights(ei.shape[1], 5)
    check(mmf, ei, N, M, hr.features(N, C, 13), a, None, "degrees")
    check(mmf, ei, N, M, hr.features(N, C, 13), a, hr.weights(M, 14), "degrees, weighted")


@pytest.mark.parametrize("weighted", [False, True])
def test_empty_rows_give_zeros(mmf, weighted):
    N, M = 50, 40
    ei = hr.random_incidence(N, 31, 260, 4)
    ei = ei[:, (ei[0] != 9) & (ei[1] != 17)]
    ei = np.concatenate([ei, np.array([[3], [30]])], axis=1)
    x, w, a = hr.features(N, 20, 5), hr.weights(M, 6), hp.pair_weights(ei.shape[1], 7)
    plan, pl = check(mmf, ei, N, M, x, a, w if weighted else None, "empty rows")
    out, Y = mmf.hypergraph_propagate_pairs(dev(x), dev(a), plan=plan, normalization="weight", return_edge_features=True)
    assert not out[9].any() and not Y[17].any() and not Y[31:].any() and Y.shape == (M, 20)
    es, ns = mmf.pair_scales(dev(a), plan=plan)
    assert float(es[17]) == 0.0 and float(ns[9]) == 0.0


def test_one_pair_three_times_with_three_weights(mmf):
    """The copies of a repeated pair sit in ascending column order: three weights whose float32 sum depends on the order."""
    N, M = 30, 12
    ei = hr.random_incidence(N, M, 90, 7)
    ei = ei[:, ei[1] != 2]                                                    # hyperedge 2 holds the three copies alone: B_2 is their chain
    cut = 40
    ei = np.concatenate([ei[:, :cut], np.array([[4], [2]]), ei[:, cut:cut + 10], np.array([[4], [2]]), ei[:, cut + 10:], np.array([[4], [2]])], axis=1)
    cols = np.nonzero((ei[0] == 4) & (ei[1] == 2))[0]
    assert cols.tolist() == [cut, cut + 11, ei.shape[1] - 1]
    x = hr.features(N, 8, 8)
    results = []
    for trio in ([1.0, 2.0 ** -24, 2.0 ** -24], [2.0 ** -24, 2.0 ** -24, 1.0]):
        a = hp.pair_weights(ei.shape[1], 9)
        a[cols] = np.array(trio, dtype=np.float32)
        plan, pl = check(mmf, ei, N, M, x, a, hr.weights(M, 9), "triple pair")
        s = int(plan.eptr[2]) + plan.emem[int(plan.eptr[2]):int(plan.eptr[3])].tolist().index(4)
        assert plan.epos[s:s + 3].tolist() == cols.tolist()
        results.append(mmf.pair_scales(dev(a), plan=plan)[0])
    assert not torch.equal(results[0], results[1])                            # column order decided the chain


def test_out_of_range_ids_are_flagged_left_out_and_get_zeros(mmf):
    N, M = 60, 45
    good = hr.random_incidence(N, M, 400, 29)
    bad = np.array([[N, 5, -1, 2 ** 40, 7, -(2 ** 62)], [3, M, 4, 6, -9, M + 100]], dtype=np.int64)
    ei = np.concatenate([good[:, :100], bad[:, :3], good[:, 100:250], bad[:, 3:], good[:, 250:]], axis=1)
    E = ei.shape[1]
    valid = np.concatenate([np.arange(100), np.arange(103, 253), np.arange(256, 406)])
    x, w, a, s = hr.features(N, 33, 30), hr.weights(M, 31), hp.pair_weights(E, 32, signed=True), hp.scores(E, 33)
    plan, pl = check_plan(mmf, ei, N, M, w, check=False)
    assert plan.status.tolist() == [100, 101] and int(plan.eptr[-1]) == int(plan.nptr[-1]) == 400
    assert sorted(plan.epos[:400].tolist()) == valid.tolist() and sorted(plan.npos[:400].tolist()) == valid.tolist()
    xd, ad = dev(x).requires_grad_(), dev(a).requires_grad_()
    out, Y = mmf.hypergraph_propagate_pairs(xd, ad, plan=plan, return_edge_features=True)
    want, want_y = hp.propagate(x, a[valid], good, M, w)                      # the restatement on the valid pairs alone
    same_bits(Y, want_y, "valid pairs only, Y")
    same_bits(out, want, "valid pairs only, out")
    G = hr.features(N, 33, 34)
    out.backward(dev(G))
    ga = hp.grad_a(x, a, G, ei, M, w, pl=pl)
    same_bits(ad.grad, ga, "grad_a")
    assert not ad.grad[[100, 101, 102, 253, 254, 255]].any() and bool(ad.grad[valid].abs().min() > 0)
    for group in ("edge", "node"):
        sd = dev(s).requires_grad_()
        alpha = mmf.pair_softmax(sd, plan=plan, group=group)
        ptr, pos = hp.group_of(pl, group)
        want_alpha = hp.softmax(s, ptr, pos, E)
        same_bits(alpha, want_alpha, f"alpha {group}")
        assert not alpha[[100, 101, 102, 253, 254, 255]].any()
        alpha.backward(dev(G[:, 0].repeat(7)[:E].copy()))
        same_bits(sd.grad, hp.softmax_backward(want_alpha, G[:, 0].repeat(7)[:E], ptr, pos, E), f"grad_score {group}")
        assert not sd.grad[[100, 101, 102, 253, 254, 255]].any()
    with pytest.raises(ValueError, match=r"edge_index\[0, 100\] is no node id in \[0, 60\)"):
        plan.check()
    with pytest.raises(ValueError, match=r"edge_index\[0, 100\]"):
        mmf.incidence_pair_plan(dev(ei), N, M)
    for cols in (bad, np.zeros((2, 0), dtype=np.int64)):                      # every pair bad, and no pair at all
        p = mmf.incidence_pair_plan(dev(cols), N, M, check=False)
        assert not p.eptr.any() and not p.nptr.any() and not p.epos.any() and not p.npos.any()
        av = torch.ones(cols.shape[1], device="cuda")
        o, y = mmf.hypergraph_propagate_pairs(dev(x), av, plan=p, return_edge_features=True)
        assert not o.any() and not y.any() and not mmf.pair_softmax(av, plan=p).any()


def test_x_as_a_slice_of_a_larger_tensor(mmf, base):
    ei, w, a = base
    N, M = BASE["N"], BASE["M"]
    big = torch.from_numpy(hr.features(N + 20, 100, 15)).cuda()
    for what, view in (("rows 10.. of [N + 20, 100]", big[10:10 + N]), ("columns 4..68: pitch 100, aligned", big[:N, 4:68]),
                       ("columns 1..65: pitch 100, unaligned", big[:N, 1:65]), ("columns 0..3", big[5:5 + N, 0:3]),
                       ("one column", big[:N, 7:8]), ("every second column: copied", big[:N, ::2][:, :32])):
        check(mmf, ei, N, M, view.cpu().numpy(), a, w, what, x_dev=view)


# ---- softmax --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["edge", "node"])
def test_softmax_rows_around_the_wave(mmf, group):
    """Rows of 0, 1, 7, 8, 9, 63, 64, 65 and 1000 slots, on either side, with random scores, scores of +-80, all-equal scores, +-0."""
    ei, N, M = hp.row_sizes_incidence()
    if group == "node":
        ei, N, M = ei[::-1].copy(), M, N
    E = ei.shape[1]
    perm = np.random.RandomState(41).permutation(E)
    ei = ei[:, perm]
    plan, pl = check_plan(mmf, ei, N, M)
    ptr, pos = hp.group_of(pl, group)
    assert sorted(set(np.diff(ptr).tolist())) == [0, 1, 7, 8, 9, 63, 64, 65, 1000]
    g = hr.features(E, 1, 42)[:, 0].copy()
    for what, s in (("random", hp.scores(E, 43)), ("+-80", np.where(np.arange(E) % 3 == 0, 80.0, -80.0).astype(np.float32)),
                    ("equal", np.full(E, 1.5, dtype=np.float32)), ("+-0", np.where(np.arange(E) % 2 == 0, 0.0, -0.0).astype(np.float32))):
        sd = dev(s).requires_grad_()
        alpha = mmf.pair_softmax(sd, plan=plan, group=group)
        want = hp.softmax(s, ptr, pos, E)
        same_bits(alpha, want, f"alpha {group} {what}")
        alpha.backward(dev(g))
        same_bits(sd.grad, hp.softmax_backward(want, g, ptr, pos, E), f"grad_score {group} {what}")
        a64, tol, _ = hp.softmax64(s, ptr, pos, E)
        err = np.abs(alpha.detach().cpu().numpy().astype(np.float64) - a64)
        g64, tol_g = hp.softmax_backward64(s, g, ptr, pos, E)
        err_g = np.abs(sd.grad.cpu().numpy().astype(np.float64) - g64)
        print(f"{group} {what}: alpha max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}, "
              f"grad_score max err / bound = {np.max(err_g / np.maximum(tol_g, 1e-300)):.3f}")
        assert (err <= tol).all() and (err_g <= tol_g).all()
        assert torch.equal(mmf.pair_softmax(dev(s), plan=plan, group=group), alpha.detach())       # from call to call


# ---- order, repetition, ones ----------------------------------------------------------------------------------------------------------
def test_shuffled_columns_and_repeated_calls_give_the_same_bits(mmf):
    N, M, C = 300, 200, 96
    ei = hr.random_incidence(N, M, 1500, 1)
    ei = ei[:, np.unique(ei[0] * M + ei[1], return_index=True)[1]]            # duplicate-free: the order of the columns must not matter
    E = ei.shape[1]
    a, s, w, x = hp.pair_weights(E, 2, signed=True), hp.scores(E, 3), hr.weights(M, 4), dev(hr.features(N, C, 16))
    G = dev(hr.features(N, C, 17))
    results = []
    for perm in (np.arange(E), np.random.RandomState(17).permutation(E), np.arange(E)[::-1].copy(), np.arange(E)):
        plan = mmf.incidence_pair_plan(dev(ei[:, perm]), N, M, dev(w))
        xd, ad, sd = x.clone().requires_grad_(), dev(a[perm]).requires_grad_(), dev(s[perm]).requires_grad_()
        out, Y = mmf.hypergraph_propagate_pairs(xd, ad, plan=plan, return_edge_features=True)
        out.backward(G)
        ow = mmf.hypergraph_propagate_pairs(x, dev(a[perm]).abs(), plan=plan, normalization="weight")
        alpha = mmf.pair_softmax(sd, plan=plan, group="edge")
        alpha.backward(dev(a[perm]))
        inv = torch.from_numpy(np.argsort(perm)).cuda()
        results.append([out.detach(), Y, xd.grad, ad.grad[inv], ow, alpha.detach()[inv], sd.grad[inv]])
    for r in results[1:]:
        for got, want in zip(r, results[0]):
            assert torch.equal(got, want)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [5, 64, 300])
def test_ones_reproduce_hypergraph_propagate(mmf, base, weighted, C):
    ei, w, _ = base
    N, M = BASE["N"], BASE["M"]
    ei = np.concatenate([ei, ei[:, :9]], axis=1)
    plan = mmf.incidence_pair_plan(dev(ei), N, M, dev(w) if weighted else None)
    x = dev(hr.features(N, C, 50)).requires_grad_()
    want, want_y = mmf.hypergraph_propagate(x, plan=plan, return_edge_features=True)          # a pair plan serves the unweighted layer
    G = dev(hr.features(N, C, 51))
    want.backward(G)
    want_gx = x.grad.clone()
    ones = torch.ones(ei.shape[1], device="cuda")
    for mode in ("count", "weight"):
        x.grad = None
        out, Y = mmf.hypergraph_propagate_pairs(x, ones, plan=plan, normalization=mode, return_edge_features=True)
        out.backward(G)
        assert torch.equal(out, want) and torch.equal(Y, want_y) and torch.equal(x.grad, want_gx), mode


# ---- float64 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_forward_and_gradients_within_the_derived_bounds(mmf, base, weighted):
    ei, w, a = base
    w = w if weighted else None
    N, M, C = BASE["N"], BASE["M"], 40
    ei = np.concatenate([ei, ei[:, :9]], axis=1)
    x, G = hr.features(N, C, 24), hr.features(N, C, 25)
    plan = mmf.incidence_pair_plan(dev(ei), N, M, None if w is None else dev(w))
    for mode, av in (("count", hp.pair_weights(ei.shape[1], 26, signed=True)), ("weight", hp.pair_weights(ei.shape[1], 26))):
        xd, ad = dev(x).requires_grad_(), dev(av).requires_grad_(mode == "count")
        out = mmf.hypergraph_propagate_pairs(xd, ad, plan=plan, normalization=mode)
        out.backward(dev(G))
        d = hp.dense64(ei, av, N, M, w, mode)
        err = np.abs(out.detach().cpu().numpy().astype(np.float64) - d["P"] @ x.astype(np.float64))
        tol = hp.bound(ei, av, x, N, M, w, mode)
        err_x = np.abs(xd.grad.cpu().numpy().astype(np.float64) - d["P"].T @ G.astype(np.float64))
        tol_x = hp.bound(ei, av, G, N, M, w, mode, transpose=True)
        print(f"weighted={weighted} {mode}: forward max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}, "
              f"grad_x max err / bound = {np.max(err_x / np.maximum(tol_x, 1e-300)):.3f}")
        assert (err <= tol).all() and (err_x <= tol_x).all()
        if mode == "count":
            want, tol_a = hp.grad_a64(ei, av, x, G, N, M, w)
            err_a = np.abs(ad.grad.cpu().numpy().astype(np.float64) - want)
            print(f"    grad_a max err / bound = {np.max(err_a / np.maximum(tol_a, 1e-300)):.3f}")
            assert (err_a <= tol_a).all()
    with pytest.raises(ValueError, match="requires grad under normalization='weight'"):
        mmf.hypergraph_propagate_pairs(dev(x), dev(a[:1]).repeat(ei.shape[1]).requires_grad_(), plan=plan, normalization="weight")


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def lin64(x, W):
    """(x W^T in float64 on the float32 operands, the bound of a float32 product with sums in any order or fused: (in + 1) eps |x| |W|^T)."""
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    return x64 @ W64.T, (x.shape[1] + 1) * EPS * (np.abs(x64) @ np.abs(W64).T)


def attention64(x, ea, ei, M, w, W, att, bias, mode, heads, concat, slope):
    """The float64 composition of HypergraphAttentionConv's definition and a first-order bound of the float32 module against it:
      * xh, eh = lin(x), lin(hyperedge_attr): d_xh, d_eh from lin64;
      * score = leaky_relu(<xh, att_x> + <eh, att_e>): each dot of F terms in float32 (F + 1) eps |.|.|att|, plus |att| . d_xh (d_eh),
        one add and the leaky_relu's multiply two roundings more; leaky_relu has slope <= 1: d_s per pair;
      * alpha = softmax: hp.softmax64's relative bound rho, plus the scores' perturbation: a softmax moves by at most
        expm1(2 max d_s) relatively (numerator and denominator each by exp(+-max d_s));
      * out_h = P_alpha xh_h: hp.bound for the float32 operator on the float32 alpha and xh, plus |P| d_xh for the input, plus alpha's
        relative error twice (it enters both gather steps) on |P| |xh|;
      * concat / mean (one rounding per head and the divide) and the bias add: (heads + 2) eps |out|.
    Second-order terms are covered by the factor 1 + 2^-6."""
    N, F = x.shape[0], W.shape[0] // heads
    xh, d_xh = lin64(x, W)
    eh, d_eh = lin64(ea, W)
    ok = (ei[0] >= 0) & (ei[0] < N) & (ei[1] >= 0) & (ei[1] < M)
    assert ok.all()
    pl = hp.plan(ei, N, M, w)
    ptr, pos = hp.group_of(pl, "edge" if mode == "node" else "node")
    E = ei.shape[1]
    outs, tols = [], []
    for h in range(heads):
        ax, ae = att[0, h, :F].astype(np.float64), att[0, h, F:].astype(np.float64)
        xs, es = xh[:, h * F:(h + 1) * F], eh[:, h * F:(h + 1) * F]
        sx, se = xs @ ax, es @ ae
        d_sx = (F + 1) * EPS * (np.abs(xs) @ np.abs(ax)) + d_xh[:, h * F:(h + 1) * F] @ np.abs(ax)
        d_se = (F + 1) * EPS * (np.abs(es) @ np.abs(ae)) + d_eh[:, h * F:(h + 1) * F] @ np.abs(ae)
        pre = sx[ei[0]] + se[ei[1]]
        score = np.where(pre > 0, pre, slope * pre)
        d_s = d_sx[ei[0]] + d_se[ei[1]] + 2 * EPS * (np.abs(sx[ei[0]]) + np.abs(se[ei[1]]))
        alpha, _, rho = hp.softmax64(score, ptr, pos, E)
        rel = float(rho.max()) + float(np.expm1(2 * float(d_s.max())))
        flush = 2 * (int(np.diff(ptr).max()) + 1) * hp.FLUSH * E * float(np.abs(xs).max())      # rows below -87: absolute, on every pair
        d = hp.dense64(ei, alpha, N, M, w, "count")
        outs.append(d["P"] @ xs)
        op = hp.bound(ei, alpha, xs, N, M, w, "count")
        tols.append(op + d["P"] @ d_xh[:, h * F:(h + 1) * F] + 2 * rel * (d["P"] @ np.abs(xs)) + flush)
    out = np.concatenate(outs, axis=1) if concat else np.mean(outs, axis=0)
    tol = np.concatenate(tols, axis=1) if concat else np.mean(tols, axis=0)
    out = out + bias.astype(np.float64)
    return out, (tol + (heads + 2) * EPS * np.abs(out)) * (1 + 2.0 ** -6)


@pytest.mark.parametrize("heads,concat", [(1, True), (3, True), (3, False)])
@pytest.mark.parametrize("mode", ["node", "edge"])
def test_hypergraph_attention_conv_against_the_float64_composition(mmf, base, heads, concat, mode):
    ei, w, _ = base
    N, M, Cin, F = BASE["N"], BASE["M"], 24, 10
    torch.manual_seed(heads + 10 * concat)
    conv = mmf.HypergraphAttentionConv(Cin, F, attention_mode=mode, heads=heads, concat=concat).cuda()
    with torch.no_grad():
        conv.bias.copy_(torch.linspace(-1, 1, conv.bias.numel()))
    x, ea = hr.features(N, Cin, 60), hr.features(M, Cin, 61)
    xd = dev(x).requires_grad_()
    plan = mmf.incidence_pair_plan(dev(ei), N, M, dev(w))
    y = conv(xd, dev(ei), hyperedge_attr=dev(ea), plan=plan)
    assert y.shape == (N, heads * F if concat else F)
    assert torch.equal(y, conv(xd, dev(ei), dev(w), dev(ea), num_edges=M))    # a plan of its own per call
    want, tol = attention64(x, ea, ei, M, w, conv.lin.weight.detach().cpu().numpy(), conv.att.detach().cpu().numpy(),
                            conv.bias.detach().cpu().numpy(), mode, heads, concat, 0.2)
    err = np.abs(y.detach().cpu().numpy().astype(np.float64) - want)
    print(f"heads={heads} concat={concat} mode={mode}: max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()
    y.sum().backward()
    for p in (conv.lin.weight, conv.att, conv.bias):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0)
    assert xd.grad is not None and bool(xd.grad.abs().sum() > 0)
    with pytest.raises(ValueError, match="hyperedge_attr"):
        conv(xd, dev(ei), plan=plan)
    conv.train()
    conv.dropout = 0.5
    assert conv(xd, dev(ei), hyperedge_attr=dev(ea), plan=plan).shape == y.shape


@pytest.mark.parametrize("normalization", ["weight", "count"])
def test_pair_weighted_conv_against_the_float64_composition(mmf, base, normalization):
    ei, w, a = base
    N, M = BASE["N"], BASE["M"]
    torch.manual_seed(0)
    conv = mmf.PairWeightedHypergraphConv(48, 20, normalization=normalization).cuda()
    conv.load_state_dict(mmf.HypergraphConv(48, 20).state_dict())             # a HypergraphConv checkpoint loads
    with torch.no_grad():
        conv.bias.copy_(torch.linspace(-1, 1, 20))
    x = hr.features(N, 48, 28)
    y = conv(dev(x), dev(ei), dev(a), dev(w), num_edges=M)
    plan = mmf.incidence_pair_plan(dev(ei), N, M, dev(w))
    assert torch.equal(conv(dev(x), pair_weight=dev(a), plan=plan), y)
    h = torch.nn.functional.linear(dev(x), conv.lin.weight)
    assert torch.equal(y, mmf.hypergraph_propagate_pairs(h, dev(a), plan=plan, normalization=normalization) + conv.bias)
    h64, d_h = lin64(x, conv.lin.weight.detach().cpu().numpy())
    d = hp.dense64(ei, a, N, M, w, normalization)
    want = d["P"] @ h64 + conv.bias.detach().cpu().numpy().astype(np.float64)
    # the operator's bound on lin(x), the input's error through |P_a|, one rounding for the bias add
    tol = (hp.bound(ei, a, h64, N, M, w, normalization) + d["P"] @ d_h + EPS * np.abs(want)) * (1 + 2.0 ** -6)
    err = np.abs(y.detach().cpu().numpy().astype(np.float64) - want)
    print(f"PairWeightedHypergraphConv {normalization}: max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()
    y.sum().backward()
    assert conv.lin.weight.grad is not None and conv.bias.grad is not None and bool(conv.lin.weight.grad.abs().sum() > 0)
    with pytest.raises(ValueError, match="plain IncidencePlan"):
        conv(dev(x), pair_weight=dev(a), plan=mmf.incidence_plan(dev(ei), N, M))


# ---- the stream contract --------------------------------------------------------------------------------------------------------------
def test_plan_forward_and_backward_on_a_busy_side_stream(mmf):
    """Plan build, both operators and both backwards enqueue on the caller's stream only and return while the gate in front of their
    inputs is still closed; the bits are those of the idle default stream and of the restatement."""
    import streamgate as sg
    N, M, E, C = 2000, 1500, 30000, 64

    def make_inputs(kind):
        s = 0 if kind == "truth" else 50
        return [torch.from_numpy(hr.random_incidence(N, M, E, 32 + s)), torch.from_numpy(hr.features(N, C, 33 + s)),
                torch.from_numpy(hr.weights(M, 34 + s)), torch.from_numpy(hp.pair_weights(E, 35 + s)), torch.from_numpy(hp.scores(E, 36 + s)),
                torch.from_numpy(hr.features(N, C, 37 + s))]

    def entry(ei, x, w, a, s, G):
        plan = mmf.incidence_pair_plan(ei, N, M, w, check=False)
        xd, ad, sd = x.clone().requires_grad_(), a.clone().requires_grad_(), s.clone().requires_grad_()
        out, Y = mmf.hypergraph_propagate_pairs(xd, ad, plan=plan, return_edge_features=True)
        out.backward(G)
        ow = mmf.hypergraph_propagate_pairs(x, a, plan=plan, normalization="weight")
        alpha = mmf.pair_softmax(sd, plan=plan, group="edge")
        alpha.backward(a)
        return [out.detach(), Y, xd.grad, ad.grad, ow, alpha.detach(), sd.grad, plan.status, plan.epos, plan.npos]

    def reference(ei, x, w, a, s, G):
        def verdict(got):
            pl = hp.plan(ei, N, M, w)
            want, want_y = hp.propagate(x, a, ei, M, w, pl=pl)
            gx, _ = hp.propagate(G, a, ei, M, w, transpose=True, pl=pl)
            alpha = hp.softmax(s, pl["eptr"], pl["epos"], E)
            return (sg.diff(got[0], want, "out") + sg.diff(got[1], want_y, "Y") + sg.diff(got[2], gx, "grad_x") +
                    sg.diff(got[3], hp.grad_a(x, a, G, ei, M, w, pl=pl), "grad_a") +
                    sg.diff(got[4], hp.propagate(x, a, ei, M, w, "weight", pl=pl)[0], "out (weight)") + sg.diff(got[5], alpha, "alpha") +
                    sg.diff(got[6], hp.softmax_backward(alpha, a, pl["eptr"], pl["epos"], E), "grad_score") +
                    sg.diff(got[7], np.array([-1, -1]), "status") + sg.diff(got[8], pl["epos"].astype(np.int32), "epos") +
                    sg.diff(got[9], pl["npos"].astype(np.int32), "npos"))
        return verdict

    sg.run_gated(entry, make_inputs, reference, name="hgpair plan + propagate + softmax, forward and backward", nonsync=True, calls=2)
