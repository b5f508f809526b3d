"""Pair-weighted hypergraph propagation and the softmax over pairs without a GPU (include/ext/mmf_hg_hgpair.h,
multimodal-fusion_amd/hgpair.py): the header and the export list, the package-level names and signatures, the numpy
restatement (tests/hgpair_restate.py) against the dense float64 operator within its derived bounds, with ones against
hgconv_restate bit for bit, every ValueError the Python layer raises before any device work, the host checks of the C entries, and
that the refusals of the attention mode in hgconv and HypergraphNetwork still hold."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hgconv_restate as hr      # noqa: E402
import hgpair_restate as hp      # noqa: E402
from test_hgconv_cpu import CASES  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ext", "mmf_hg_hgpair.h")
ENTRIES = {"mmf_incidence_pair_plan", "mmf_pair_scales", "mmf_hypergraph_propagate_pairs", "mmf_pair_weight_grad", "mmf_pair_softmax",
           "mmf_pair_softmax_backward"}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, library, binding, package ------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.HGPAIR_EXPORTS) == ENTRIES
    for name, v in vars(mmf._lib).items():                                   # no other export list binds the names
        if name != "HGPAIR_EXPORTS" and isinstance(v, list) and all(isinstance(e, str) for e in v):
            assert not set(v) & declared, name
    assert mmf._lib.ABI_VERSION == 3 and mmf._lib.lib().mmf_version() == 3    # an addition
    L = mmf._lib.lib()
    for name in ENTRIES:
        assert getattr(L, name).restype is ctypes.c_int
    assert len(L.mmf_incidence_pair_plan.argtypes) == 16 and len(L.mmf_hypergraph_propagate_pairs.argtypes) == 21
    assert len(L.mmf_pair_scales.argtypes) == 14 and len(L.mmf_pair_weight_grad.argtypes) == 15
    assert len(L.mmf_pair_softmax.argtypes) == 8 and len(L.mmf_pair_softmax_backward.argtypes) == 9
    for words in ("HGPAIR_EXPORTS", "sequential f32 chain", "no fma", "2^31", "SortPairs", "ascending column order", "Workspace:", "dot64",
                  "cexp", "never synchronises", "transpose"):
        assert words in hdr, words
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_hgpair", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("ext", "mmf_hg_hgpair.h")) for h in b.HEADERS) and "mmf_hgshare.h" in b.HEADERS
    assert all(os.path.exists(h if os.path.isabs(h) else os.path.join(ROOT, "multimodal-fusion_amd", "csrc", h)) for h in b.HEADERS)
    assert "mmf_hgpair.hip" in b.SOURCES and "mmf_hgpair.hip" not in b.EXTRA_FLAGS and "-ffp-contract=off" in b.FLAGS
    assert '#include "../../include/ext/mmf_hg_hgpair.h"' in open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_host.h")).read()


def test_package_names_and_signatures(mmf):
    from importlib import import_module
    m = import_module("multimodal_fusion_amd.hgpair")
    assert mmf.hgpair is m and "hgpair" in mmf.__all__ and "mmf.hgpair.*" in mmf.__doc__
    for name in ("incidence_pair_plan", "IncidencePairPlan", "pair_scales", "hypergraph_propagate_pairs", "pair_softmax",
                 "PairWeightedHypergraphConv", "HypergraphAttentionConv"):
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
    assert issubclass(m.IncidencePairPlan, mmf.hgconv.IncidencePlan)
    assert str(inspect.signature(m.incidence_pair_plan)) == str(inspect.signature(mmf.hgconv.incidence_plan)).replace("IncidencePlan", "IncidencePairPlan")
    sig = inspect.signature(m.hypergraph_propagate_pairs)
    assert list(sig.parameters)[:5] == ["x", "pair_weight", "plan", "normalization", "return_edge_features"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    assert sig.parameters["normalization"].default == "count" and sig.parameters["return_edge_features"].default is False
    sig = inspect.signature(m.pair_softmax)
    assert list(sig.parameters) == ["score", "plan", "group"] and sig.parameters["group"].default == "edge"
    assert sig.parameters["plan"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(m.PairWeightedHypergraphConv.__init__).parameters)[1:] == ["in_channels", "out_channels", "bias", "normalization"]
    assert inspect.signature(m.PairWeightedHypergraphConv.__init__).parameters["normalization"].default == "weight"
    assert list(inspect.signature(m.PairWeightedHypergraphConv.forward).parameters)[1:] == ["x", "hyperedge_index", "pair_weight", "hyperedge_weight",
                                                                                              "num_edges", "plan"]
    init = inspect.signature(m.HypergraphAttentionConv.__init__).parameters
    assert list(init)[1:] == ["in_channels", "out_channels", "attention_mode", "heads", "concat", "negative_slope", "dropout", "bias"]
    assert (init["attention_mode"].default, init["heads"].default, init["concat"].default, init["negative_slope"].default,
            init["dropout"].default, init["bias"].default) == ("node", 1, True, 0.2, 0.0, True)
    assert list(inspect.signature(m.HypergraphAttentionConv.forward).parameters)[1:] == ["x", "hyperedge_index", "hyperedge_weight", "hyperedge_attr",
                                                                                           "num_edges", "plan"]


def test_modules_without_a_device(mmf):
    torch.manual_seed(0)
    conv = mmf.PairWeightedHypergraphConv(16, 8)
    assert sorted(conv.state_dict()) == ["bias", "lin.weight"] and conv.lin.weight.shape == (8, 16) and not conv.bias.any()
    conv.load_state_dict(mmf.HypergraphConv(16, 8).state_dict())              # a HypergraphConv checkpoint loads
    assert sorted(mmf.PairWeightedHypergraphConv(4, 4, bias=False).state_dict()) == ["lin.weight"]
    with pytest.raises(ValueError, match="unknown normalization"):
        mmf.PairWeightedHypergraphConv(4, 4, normalization="sym")
    with pytest.raises(ValueError, match="pair_weight is required"):
        conv(torch.zeros(3, 16), torch.zeros(2, 1, dtype=torch.int64))
    att = mmf.HypergraphAttentionConv(16, 8, heads=3)
    sd = att.state_dict()
    assert sorted(sd) == ["att", "bias", "lin.weight"]
    assert sd["lin.weight"].shape == (24, 16) and sd["att"].shape == (1, 3, 16) and sd["bias"].shape == (24,) and not sd["bias"].any()
    assert att.lin.bias is None
    lim_w, lim_a = (6.0 / (24 + 16)) ** 0.5, (6.0 / (3 + 16)) ** 0.5          # glorot over the last two dimensions
    assert 0.5 * lim_w < float(sd["lin.weight"].abs().max()) <= lim_w and 0.5 * lim_a < float(sd["att"].abs().max()) <= lim_a
    assert mmf.HypergraphAttentionConv(16, 8, heads=3, concat=False).bias.shape == (8,)
    assert sorted(mmf.HypergraphAttentionConv(4, 4, bias=False).state_dict()) == ["att", "lin.weight"]
    with pytest.raises(ValueError, match="attention_mode"):
        mmf.HypergraphAttentionConv(4, 4, attention_mode="both")
    with pytest.raises(ValueError, match="hyperedge_attr"):
        att(torch.zeros(3, 16), torch.zeros(2, 1, dtype=torch.int64))


def test_the_existing_refusals_still_hold(mmf):
    with pytest.raises(NotImplementedError):
        mmf.HypergraphConv(4, 4, use_attention=True)
    with pytest.raises(NotImplementedError):
        mmf.HypergraphConv(4, 4, heads=2)
    with pytest.raises(NotImplementedError):
        mmf.HypergraphConv(4, 4)(torch.zeros(3, 4), torch.zeros(2, 1, dtype=torch.int64), hyperedge_attr=torch.zeros(1, 4))
    with pytest.raises(NotImplementedError):
        mmf.HypergraphNetwork(8, [8, 4], 2, use_attention=True)
    with pytest.raises(ValueError, match="requires grad"):
        mmf.incidence_plan(torch.zeros(2, 1, dtype=torch.int64), 3, 1, torch.ones(1, requires_grad=True))
    with pytest.raises(ValueError, match="requires grad"):
        mmf.incidence_pair_plan(torch.zeros(2, 1, dtype=torch.int64), 3, 1, torch.ones(1, requires_grad=True))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def case(N, M, E, seed):
    ei = hr.random_incidence(N, M, E, seed)
    return np.concatenate([ei, ei[:, :5]], axis=1)                            # some pairs twice, with weights of their own


@pytest.mark.parametrize("N,M,E,seed", CASES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("normalization", ["count", "weight"])
def test_restatement_against_the_dense_float64_operator(N, M, E, seed, weighted, normalization):
    ei = case(N, M, E, seed)
    x = hr.features(N, 9, 10 + seed)
    w = hr.weights(M, 20 + seed) if weighted else None
    a = hp.pair_weights(ei.shape[1], 40 + seed, signed=normalization == "count")
    out, Y = hp.propagate(x, a, ei, M, w, normalization)
    d = hp.dense64(ei, a, N, M, w, normalization)
    err = np.abs(out.astype(np.float64) - d["P"] @ x.astype(np.float64))
    tol = hp.bound(ei, a, x, N, M, w, normalization)
    print(f"N={N} M={M} weighted={weighted} {normalization}: forward max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()
    G = hr.features(N, 9, 30 + seed)
    gx, _ = hp.propagate(G, a, ei, M, w, normalization, transpose=True)
    err = np.abs(gx.astype(np.float64) - d["P"].T @ G.astype(np.float64))
    tol = hp.bound(ei, a, G, N, M, w, normalization, transpose=True)
    print(f"    grad_x max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()
    if normalization == "count":
        ga = hp.grad_a(x, a, G, ei, M, w)
        want, tol = hp.grad_a64(ei, a, x, G, N, M, w)
        err = np.abs(ga.astype(np.float64) - want)
        print(f"    grad_a max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert (err <= tol).all()
        # and grad_a64 is the derivative: a central difference of sum(G * P_a x) in float64 at three columns
        for p in (0, ei.shape[1] // 2, ei.shape[1] - 1):
            h = 1e-6
            ap, am = a.astype(np.float64).copy(), a.astype(np.float64).copy()
            ap[p] += h
            am[p] -= h
            f = [float((G * (hp.dense64(ei, t, N, M, w)["P"] @ x.astype(np.float64))).sum()) for t in (ap, am)]
            assert abs((f[0] - f[1]) / (2 * h) - want[p]) <= 1e-6 * (1 + abs(want[p])), p


@pytest.mark.parametrize("N,M,E,seed", CASES)
@pytest.mark.parametrize("weighted", [False, True])
def test_with_ones_the_restatement_is_hgconv_restate_bit_for_bit(N, M, E, seed, weighted):
    ei = case(N, M, E, seed)
    x = hr.features(N, 6, 50 + seed)
    w = hr.weights(M, 60 + seed) if weighted else None
    ones = np.ones(ei.shape[1], dtype=np.float32)
    want, want_y = hr.propagate(x, ei, M, w)
    want_t, want_ty = hr.propagate(x, ei, M, w, transpose=True)
    for normalization in ("count", "weight"):
        out, Y = hp.propagate(x, ones, ei, M, w, normalization)
        assert np.array_equal(hp.bits(out), hp.bits(want)) and np.array_equal(hp.bits(Y), hp.bits(want_y)), normalization
        gx, T = hp.propagate(x, ones, ei, M, w, normalization, transpose=True)
        assert np.array_equal(hp.bits(gx), hp.bits(want_t)) and np.array_equal(hp.bits(T), hp.bits(want_ty)), normalization


def test_restatement_positions_are_a_stable_sort():
    ei = np.array([[4, 1, 4, 9, 4, 0, -1, 2], [2, 2, 2, 0, 2, 7, 1, 1]], dtype=np.int64)      # (4, 2) three times; 9 and 7 and -1 out of range
    pl = hp.plan(ei, 5, 3)
    assert pl["eptr"].tolist() == [0, 0, 1, 5] and pl["emem"].tolist() == [2, 1, 4, 4, 4] and pl["epos"].tolist() == [7, 1, 0, 2, 4]
    assert pl["nptr"].tolist() == [0, 0, 1, 2, 2, 5] and pl["nmem"].tolist() == [2, 1, 2, 2, 2] and pl["npos"].tolist() == [1, 7, 0, 2, 4]
    # the order of the copies decides the chain: three weights that do not commute under float32 addition
    a = np.zeros(8, dtype=np.float32)
    a[[0, 2, 4]] = [1.0, 2.0 ** -24, 2.0 ** -24]
    x = np.ones((5, 1), dtype=np.float32)
    _, Y = hp.propagate(x, a, ei, 3)
    b = a.copy()
    b[[0, 2, 4]] = [2.0 ** -24, 2.0 ** -24, 1.0]
    _, Yb = hp.propagate(x, b, ei, 3)
    assert Y[2, 0] != Yb[2, 0]


@pytest.mark.parametrize("group", ["edge", "node"])
def test_softmax_restatement_against_float64(group):
    ei, N, M = hp.row_sizes_incidence()
    E = ei.shape[1]
    pl = hp.plan(ei, N, M)
    ptr, pos = hp.group_of(pl, group)
    for what, s in (("random", hp.scores(E, 1)), ("+-80", np.where(np.arange(E) % 3 == 0, 80.0, -80.0).astype(np.float32)),
                    ("equal", np.full(E, 1.5, dtype=np.float32)), ("+-0", np.where(np.arange(E) % 2 == 0, 0.0, -0.0).astype(np.float32))):
        alpha = hp.softmax(s, ptr, pos, E)
        want, tol, _ = hp.softmax64(s, ptr, pos, E)
        err = np.abs(alpha.astype(np.float64) - want)
        print(f"{group} {what}: alpha max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert (err <= tol).all()
        sums = np.zeros(ptr.size - 1)
        np.add.at(sums, np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), alpha[pos[:int(ptr[-1])]].astype(np.float64))
        assert np.allclose(sums[np.diff(ptr) > 0], 1.0, atol=1e-4)
        g = hr.features(E, 1, 2)[:, 0]
        grad = hp.softmax_backward(alpha, g, ptr, pos, E)
        want_g, tol_g = hp.softmax_backward64(s, g, ptr, pos, E)
        err = np.abs(grad.astype(np.float64) - want_g)
        print(f"    grad_score max err / bound = {np.max(err / np.maximum(tol_g, 1e-300)):.3f}")
        assert (err <= tol_g).all()


# ---- the Python layer's refusals, before any device work ------------------------------------------------------------------------------
def test_value_errors_need_no_device(mmf, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    m = mmf.hgpair
    status = torch.full((2,), -1, dtype=torch.int64)
    plan = m.IncidencePairPlan(6, 3, 4, *[torch.zeros(1)] * 6, None, status, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    plain = mmf.hgconv.IncidencePlan(6, 3, 4, *[torch.zeros(1)] * 6, None, status)
    x, a = torch.zeros(6, 4), torch.ones(4)
    for fn, arg, name in ((lambda t, **kw: m.hypergraph_propagate_pairs(x, t, **kw), a, "pair_weight"), (m.pair_softmax, a, "score"),
                          (m.pair_scales, a, "pair_weight")):
        with pytest.raises(ValueError, match=f"{name} must be float32"):
            fn(arg.double(), plan=plan)
        with pytest.raises(ValueError, match=f"{name} must be float32"):
            fn(arg.half(), plan=plan)
        with pytest.raises(ValueError, match=f"{name} has 5 entries, the plan was built for 4 pairs"):
            fn(torch.ones(5), plan=plan)
        with pytest.raises(ValueError, match=r"float32 vector \[E\]"):
            fn(torch.ones(4, 1), plan=plan)
        with pytest.raises(ValueError, match=f"{name} is on meta, the plan on cpu"):
            fn(torch.ones(4, device="meta"), plan=plan)
        with pytest.raises(ValueError, match="plain IncidencePlan"):
            fn(arg, plan=plain)
        with pytest.raises(ValueError, match="must be an IncidencePairPlan"):
            fn(arg, plan=None)
    with pytest.raises(ValueError, match="unknown normalization 'sym'"):
        m.hypergraph_propagate_pairs(x, a, plan=plan, normalization="sym")
    with pytest.raises(ValueError, match="unknown group 'both'"):
        m.pair_softmax(a, plan=plan, group="both")
    with pytest.raises(ValueError, match="x must be float32"):
        m.hypergraph_propagate_pairs(x.double(), a, plan=plan)
    with pytest.raises(ValueError, match=r"float32 tensor \[N, C\]"):
        m.hypergraph_propagate_pairs(x[0], a, plan=plan)
    with pytest.raises(ValueError, match="built for 6 nodes, x has 5 rows"):
        m.hypergraph_propagate_pairs(x[:5], a, plan=plan)
    with pytest.raises(ValueError, match="is on cpu, x on meta"):
        m.hypergraph_propagate_pairs(torch.zeros(6, 4, device="meta"), a, plan=plan)
    with pytest.raises(ValueError, match="requires grad under normalization='weight'"):
        m.hypergraph_propagate_pairs(x, a.clone().requires_grad_(), plan=plan, normalization="weight")
    with pytest.raises(ValueError, match="scales belong to normalization='weight'"):
        m.hypergraph_propagate_pairs(x, a, plan=plan, scales=(torch.zeros(3), torch.zeros(6)))
    with pytest.raises(ValueError, match=r"shape \[2, E\]"):
        m.incidence_pair_plan(torch.zeros(4, dtype=torch.int64), 6)
    with pytest.raises(ValueError, match="must be int64"):
        m.incidence_pair_plan(torch.zeros(2, 4, dtype=torch.int32), 6)
    with pytest.raises(ValueError, match="hyperedge_weight has 2 entries for 3 hyperedges"):
        m.incidence_pair_plan(torch.zeros(2, 4, dtype=torch.int64), 6, 3, torch.ones(2))
    # valid calls on host tensors reach the package's device error, not a CPU path
    for call in (lambda: m.hypergraph_propagate_pairs(x, a, plan=plan), lambda: m.hypergraph_propagate_pairs(x, a, plan=plan, normalization="weight"),
                 lambda: m.pair_softmax(a, plan=plan), lambda: m.pair_softmax(a, plan=plan, group="node"), lambda: m.pair_scales(a, plan=plan),
                 lambda: m.incidence_pair_plan(torch.zeros(2, 4, dtype=torch.int64), 6, 3)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    # a pair plan is an IncidencePlan: the unweighted propagation takes it as far as the same device error
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmf.hypergraph_propagate(x, plan=plan)
    bad = m.IncidencePairPlan(5, 3, 4, *[torch.zeros(1)] * 6, None, torch.tensor([3, -1]), None, None)
    with pytest.raises(ValueError, match=r"edge_index\[0, 3\] is no node id in \[0, 5\)"):
        bad.check()


# ---- the C entries' host checks (host buffers stand in for device pointers; device 63 does not exist) -----------------------------------
def test_c_entries_check_their_arguments_before_the_device(mmf):
    L = mmf._lib.lib()
    inv, uns, hip = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED, mmf._lib.MMF_E_HIP
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)

    def err():
        return L.mmf_last_error().decode()

    def plan(E=4, N=3, M=2, ei=b, epos=b, npos=b, status=b, dev=63):
        return L.mmf_incidence_pair_plan(ei, E, N, M, None, b, b, epos, b, b, npos, b, b, status, dev, None)
    assert plan(dev=-1) == uns and "no CPU path" in err() and err().startswith("incidence_pair_plan:")
    assert plan(E=-1) == inv and err().startswith("incidence_pair_plan:") and plan(N=-2) == inv
    for kw in (dict(ei=None), dict(epos=None), dict(npos=None), dict(status=None)):
        assert plan(**kw) == inv and "NULL" in err(), kw
    assert plan(E=1 << 31) == uns and "2^31" in err() and plan(M=1 << 31) == uns
    assert plan() == hip                                                      # a clean call gets as far as the device

    def sc(E=4, N=3, M=2, a=b, es=b, dev=63):
        return L.mmf_pair_scales(b, b, b, b, b, a, None, N, M, E, es, b, dev, None)
    assert sc(dev=-1) == uns and err().startswith("pair_scales:") and sc(N=-1) == inv and sc(a=None) == inv and sc(es=None) == inv
    assert sc(E=1 << 31) == uns and sc() == hip

    def prop(N=3, M=2, C=4, E=4, stride=4, x=b, Y=b, a=b, ns=b, tr=0, dev=63):
        return L.mmf_hypergraph_propagate_pairs(b, b, b, b, b, b, b, ns, None, a, E, x, stride, N, M, C, Y, b, tr, dev, None)
    assert prop(dev=-1) == uns and err().startswith("hypergraph_propagate_pairs:")
    assert prop(C=-1) == inv and prop(stride=3) == inv and err().startswith("hypergraph_propagate_pairs:") and prop(E=-1) == inv
    for kw in (dict(x=None), dict(Y=None), dict(a=None), dict(ns=None)):
        assert prop(**kw) == inv and "NULL" in err(), kw
    assert prop(N=1 << 31) == uns and prop(C=1 << 31, stride=1 << 31) == uns and prop(E=1 << 31) == uns
    assert prop() == hip and prop(ns=None, tr=1) == hip                       # the transposed form takes no node scale

    def wg(N=3, M=2, C=4, E=4, stride=4, gp=b, ga=b, dev=63):
        return L.mmf_pair_weight_grad(b, b, b, gp, b, stride, b, b, N, M, C, E, ga, dev, None)
    assert wg(dev=-1) == uns and err().startswith("pair_weight_grad:") and wg(C=-1) == inv and wg(stride=3) == inv
    assert wg(gp=None) == inv and wg(ga=None) == inv and wg(M=1 << 31) == uns and wg() == hip

    def sm(rows=3, E=4, ptr=b, score=b, alpha=b, dev=63):
        return L.mmf_pair_softmax(ptr, b, rows, E, score, alpha, dev, None)
    assert sm(dev=-1) == uns and err().startswith("pair_softmax:") and sm(rows=-1) == inv and sm(E=-1) == inv
    assert sm(ptr=None) == inv and sm(score=None) == inv and sm(alpha=None) == inv and sm(rows=1 << 31) == uns and sm() == hip

    def smb(rows=3, E=4, ptr=b, g=b, out=b, dev=63):
        return L.mmf_pair_softmax_backward(ptr, b, rows, E, b, g, out, dev, None)
    assert smb(dev=-1) == uns and err().startswith("pair_softmax_backward:") and smb(rows=-1) == inv
    assert smb(ptr=None) == inv and smb(g=None) == inv and smb(out=None) == inv and smb(E=1 << 31) == uns and smb() == hip


def test_the_kernel_file_abstains():
    src = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_hgpair.hip")).read()
    from test_stream_arguments_cpu import strip_comments
    code = strip_comments(src)
    assert not re.findall(r"\batomic\w+", code)                               # no atomics at all: the status words are mmf_hgconv.hip's
    for word in ("fmaf", "__fma", "expf", "exp2f", "__expf", "hipMalloc", "Synchronize", "hipMemcpy"):
        assert word not in code, word
    assert "SortPairs" in code and "ro_cexp" in code and "ro_tree" in code


# ---- documents ------------------------------------------------------------------------------------------------------------------------
def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.index("## 4.36") < design.index("## 4.37") < design.index("\n## 5")
    sec = design.split("## 4.37", 1)[1].split("\n## 5", 1)[0]
    for words in ("mmf_incidence_pair_plan", "mmf_hypergraph_propagate_pairs", "mmf_pair_softmax", "SortPairs", "dot64", "cexp", "Refus", "VGPR",
                  "hgpair_timing", "Not measured", "Left"):
        assert words in sec, words
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "hypergraph_propagate_pairs" in readme and "pair_softmax" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "from multimodal_fusion_amd.hgpair import" in integ
    assert os.path.exists(os.path.join(ROOT, "scripts", "hgpair_timing.py"))
    assert "hgpair_timing" in open(os.path.join(ROOT, "scripts", "README.md")).read()
    assert "hgpair_timing" in open(os.path.join(ROOT, "profiles", "README.md")).read()
