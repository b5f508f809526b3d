"""Hypergraph propagation without a GPU (include/ext/mmf_hg_hgconv.h, multimodal-fusion_amd/hgconv.py): the header and
the export list, the package-level names, the numpy restatement (tests/hgconv_restate.py) against the dense float64 operator within a
derived bound and under a permutation of the columns, every ValueError the Python layer raises before any device work, knn_incidence,
the host checks of the C entries, and the documents."""
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

HEADER = os.path.join(ROOT, "include", "ext", "mmf_hg_hgconv.h")
ENTRIES = {"mmf_incidence_plan_bytes", "mmf_incidence_plan", "mmf_csr_gather_sum", "mmf_hypergraph_propagate"}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, library, binding, package ------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.HGCONV_EXPORTS) == ENTRIES
    for name, v in vars(mmf._lib).items():                                   # no other export list binds the names
        if name != "HGCONV_EXPORTS" and isinstance(v, list) and all(isinstance(e, str) for e in v):
            assert not set(v) & declared, name
    assert mmf._lib.ABI_VERSION == 3 and mmf._lib.lib().mmf_version() == 3    # an addition
    L = mmf._lib.lib()
    for name in ENTRIES:
        assert getattr(L, name).restype is ctypes.c_int
    assert len(L.mmf_incidence_plan.argtypes) == 14 and len(L.mmf_hypergraph_propagate.argtypes) == 17
    assert len(L.mmf_csr_gather_sum.argtypes) == 12 and len(L.mmf_incidence_plan_bytes.argtypes) == 4
    for words in ("HGCONV_EXPORTS", "sequential f32 chain", "no fma", "2^31", "status int64 [2]", "none synchronises", "transpose"):
        assert words in hdr, words
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_hgconv", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("ext", "mmf_hg_hgconv.h")) for h in b.HEADERS) and all(os.path.exists(h) for h in b.HEADERS if os.path.isabs(h))
    assert "mmf_hgconv.hip" in b.SOURCES and "mmf_hgconv.hip" not in b.EXTRA_FLAGS and "-ffp-contract=off" in b.FLAGS
    assert '#include "../../include/ext/mmf_hg_hgconv.h"' in open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_host.h")).read()


def test_package_exports_the_module_and_its_four_names(mmf):
    from importlib import import_module
    m = import_module("multimodal_fusion_amd.hgconv")
    assert mmf.hgconv is m and "hgconv" in mmf.__all__ and "mmf.hgconv.*" in mmf.__doc__
    for name in ("incidence_plan", "hypergraph_propagate", "knn_incidence", "HypergraphConv"):
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
    assert "HypergraphConv" not in mmf.build_hypergraph.__all__
    sig = inspect.signature(m.incidence_plan)
    assert list(sig.parameters)[:4] == ["edge_index", "num_nodes", "num_edges", "hyperedge_weight"]
    assert sig.parameters["num_edges"].default is None and sig.parameters["hyperedge_weight"].default is None
    sig = inspect.signature(m.hypergraph_propagate)
    assert list(sig.parameters) == ["x", "edge_index", "plan", "num_edges", "hyperedge_weight", "return_edge_features"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    assert list(inspect.signature(m.knn_incidence).parameters) == ["idx", "include_self"]
    assert list(inspect.signature(m.HypergraphConv.__init__).parameters)[1:5] == ["in_channels", "out_channels", "use_attention", "bias"]
    fwd = inspect.signature(m.HypergraphConv.forward).parameters
    assert list(fwd)[1:4] == ["x", "hyperedge_index", "hyperedge_weight"] and "plan" in fwd


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
CASES = [(40, 30, 200, 1), (64, 5, 300, 2), (7, 50, 60, 3), (120, 120, 900, 4)]


@pytest.mark.parametrize("N,M,E,seed", CASES)
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_against_the_dense_float64_operator(N, M, E, seed, weighted):
    """|restatement - P @ x| <= (max B_e + max D-degree + 4) 2^-24 (P @ |x|) per element: two sequential chains (each term meets at most
    B_e - 1, resp. degree - 1, rounded adds) plus the roundings of the two reciprocals and of the scale multiplies."""
    ei = hr.random_incidence(N, M, E, seed)
    ei = np.concatenate([ei, ei[:, :5]], axis=1)                              # some pairs twice
    x = hr.features(N, 9, 10 + seed)
    w = hr.weights(M, 20 + seed) if weighted else None
    out, Y = hr.propagate(x, ei, M, w)
    P, max_b, max_deg = hr.dense_operator(ei, N, M, w)
    assert (P >= 0).all()
    want = P @ x.astype(np.float64)
    tol = hr.bound(P, x, max_b, max_deg)
    err = np.abs(out.astype(np.float64) - want)
    print(f"N={N} M={M} E={ei.shape[1]} weighted={weighted}: max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()
    # and the transposed form against P^T g
    g = hr.features(N, 9, 30 + seed)
    gx, _ = hr.propagate(g, ei, M, w, transpose=True)
    err_t = np.abs(gx.astype(np.float64) - P.T @ g.astype(np.float64))
    assert (err_t <= hr.bound(P.T, g, max_b, max_deg)).all()
    # isolated rows give zeros
    assert not out[np.bincount(ei[0], minlength=N) == 0].any() and not Y[np.bincount(ei[1], minlength=M) == 0].any()


@pytest.mark.parametrize("N,M,E,seed", CASES)
def test_restatement_does_not_depend_on_the_order_of_the_columns(N, M, E, seed):
    ei = hr.random_incidence(N, M, E, seed)
    ei = np.concatenate([ei, ei[:, :7]], axis=1)
    x, w = hr.features(N, 5, seed), hr.weights(M, seed)
    perm = np.random.RandomState(99 + seed).permutation(ei.shape[1])
    for ww in (None, w):
        a, ya = hr.propagate(x, ei, M, ww)
        b, yb = hr.propagate(x, ei[:, perm], M, ww)
        assert np.array_equal(hr.bits(a), hr.bits(b)) and np.array_equal(hr.bits(ya), hr.bits(yb))


def test_restatement_leaves_out_of_range_pairs_out():
    ei = hr.random_incidence(20, 10, 80, 5)
    bad = np.array([[-1, 20, 3, 4], [2, 3, -7, 10]], dtype=np.int64)
    x = hr.features(20, 4, 6)
    a, ya = hr.propagate(x, ei, 10)
    b, yb = hr.propagate(x, np.concatenate([bad[:, :2], ei, bad[:, 2:]], axis=1), 10)
    assert np.array_equal(hr.bits(a), hr.bits(b)) and np.array_equal(hr.bits(ya), hr.bits(yb))


# ---- the Python layer's refusals, before any device work ------------------------------------------------------------------------------
def test_value_errors_need_no_device(mmf, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    m = mmf.hgconv
    x = torch.zeros(6, 4)
    ei = torch.tensor([[0, 1, 2, 5], [0, 0, 1, 2]])
    with pytest.raises(ValueError, match="x must be float32"):
        m.hypergraph_propagate(x.double(), ei)
    with pytest.raises(ValueError, match="x must be float32"):
        m.hypergraph_propagate(x.half(), ei)
    with pytest.raises(ValueError, match=r"shape \[2, E\]"):
        m.hypergraph_propagate(x, ei.t().contiguous())
    with pytest.raises(ValueError, match=r"shape \[2, E\]"):
        m.incidence_plan(ei[0], 6)
    with pytest.raises(ValueError, match="must be contiguous"):
        m.hypergraph_propagate(x, torch.zeros(4, 2, dtype=torch.int64).t())
    with pytest.raises(ValueError, match="must be contiguous"):
        m.incidence_plan(torch.zeros(4, 2, dtype=torch.int64).t(), 6)
    with pytest.raises(ValueError, match="must be int64"):
        m.incidence_plan(ei.int(), 6)
    with pytest.raises(ValueError, match="hyperedge_weight has 2 entries for 3 hyperedges"):
        m.hypergraph_propagate(x, ei, num_edges=3, hyperedge_weight=torch.ones(2))
    with pytest.raises(ValueError, match="hyperedge_weight has 2 entries for 3 hyperedges"):
        m.incidence_plan(ei, 6, hyperedge_weight=torch.ones(2))              # num_edges = max + 1 = 3
    with pytest.raises(ValueError, match="requires grad"):
        m.hypergraph_propagate(x, ei, num_edges=3, hyperedge_weight=torch.ones(3, requires_grad=True))
    with pytest.raises(ValueError, match="requires grad"):
        m.incidence_plan(ei, 6, 3, torch.ones(3, requires_grad=True))
    with pytest.raises(ValueError, match="float32 vector"):
        m.incidence_plan(ei, 6, 3, torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="is on meta"):
        m.hypergraph_propagate(x, torch.zeros(2, 4, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="hyperedge_weight is on meta"):
        m.incidence_plan(ei, 6, 3, torch.ones(3, device="meta"))
    plan = m.IncidencePlan(5, 3, 4, *[torch.zeros(1)] * 6, None, torch.full((2,), -1, dtype=torch.int64))
    with pytest.raises(ValueError, match="built for 5 nodes, x has 6 rows"):
        m.hypergraph_propagate(x, plan=plan)
    with pytest.raises(ValueError, match="is on cpu, x on meta"):
        m.hypergraph_propagate(torch.zeros(5, 4, device="meta"), plan=plan)
    with pytest.raises(ValueError, match="either edge_index or plan"):
        m.hypergraph_propagate(x)
    with pytest.raises(ValueError, match="either edge_index or plan"):
        m.hypergraph_propagate(x, ei, plan=plan)
    with pytest.raises(ValueError, match=r"num_nodes must lie in \[0, 2\^31\)"):
        m.incidence_plan(ei, 2 ** 31)
    # a valid call on host tensors reaches the package's device error, not a CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.hypergraph_propagate(x, ei)
    # the plan's verdict on out-of-range ids: by column, read once
    for status, words in (([3, -1], r"edge_index\[0, 3\] is no node id in \[0, 5\)"), ([-1, 7], r"edge_index\[1, 7\] is no hyperedge id in \[0, 3\)"),
                          ([2, 1], r"edge_index\[0, 2\]")):
        bad = m.IncidencePlan(5, 3, 4, *[torch.zeros(1)] * 6, None, torch.tensor(status))
        with pytest.raises(ValueError, match=words):
            bad.check()
    assert plan.check() is plan and plan._checked


def test_hypergraph_conv_module_without_a_device(mmf):
    torch.manual_seed(0)
    conv = mmf.HypergraphConv(16, 8)
    assert sorted(conv.state_dict()) == ["bias", "lin.weight"]
    assert conv.lin.weight.shape == (8, 16) and conv.lin.bias is None and not conv.bias.any()
    a = (6.0 / 24) ** 0.5
    assert float(conv.lin.weight.detach().abs().max()) <= a and float(conv.lin.weight.detach().abs().max()) > 0.5 * a          # glorot
    assert sorted(mmf.HypergraphConv(4, 4, bias=False).state_dict()) == ["lin.weight"]
    with pytest.raises(NotImplementedError):
        mmf.HypergraphConv(4, 4, use_attention=True)
    with pytest.raises(NotImplementedError):
        mmf.HypergraphConv(4, 4, heads=2)
    with pytest.raises(NotImplementedError):
        conv(torch.zeros(3, 16), torch.zeros(2, 1, dtype=torch.int64), hyperedge_attr=torch.zeros(1, 16))


def test_knn_incidence_on_a_table_with_a_missing_entry(mmf):
    idx = torch.tensor([[1, 2], [0, -1], [2, 0], [3, 1]])
    ei = mmf.knn_incidence(idx)
    assert ei.dtype == torch.int64 and ei.is_contiguous()
    # row i's hyperedge is {i} ∪ idx[i]: -1 dropped, i itself once
    assert ei.tolist() == [[0, 1, 2, 1, 0, 2, 0, 3, 1], [0, 0, 0, 1, 1, 2, 2, 3, 3]]
    assert mmf.knn_incidence(idx, include_self=False).tolist() == [[1, 2, 0, 2, 0, 3, 1], [0, 0, 1, 2, 2, 3, 3]]
    assert mmf.knn_incidence(torch.zeros((0, 5), dtype=torch.int64)).shape == (2, 0)
    with pytest.raises(ValueError, match="int64"):
        mmf.knn_incidence(idx.float())
    # global ids of a batch: the incidence is block-diagonal because the ids are
    g = torch.tensor([[1], [0], [3], [2]])
    assert mmf.knn_incidence(g).tolist() == [[0, 1, 1, 0, 2, 3, 3, 2], [0, 0, 1, 1, 2, 2, 3, 3]]


# ---- the C entries' host checks (host buffers stand in for device pointers; device 63 does not exist) -----------------------------------
def test_c_entries_check_their_arguments_before_the_device(mmf):
    L = mmf._lib.lib()
    inv, uns, hip = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED, mmf._lib.MMF_E_HIP
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    out = (ctypes.c_int64 * 6)()
    assert L.mmf_incidence_plan_bytes(10, 5, 20, out) == 0 and list(out) == [48, 80, 88, 80, 20, 40]
    assert L.mmf_incidence_plan_bytes(-1, 5, 20, out) == inv and L.mmf_incidence_plan_bytes(10, 1 << 31, 20, out) == uns
    assert L.mmf_incidence_plan_bytes(10, 5, 20, None) == inv

    def plan(E=4, N=3, M=2, ei=b, status=b, dev=63):
        return L.mmf_incidence_plan(ei, E, N, M, None, b, b, b, b, b, b, status, dev, None)
    assert plan(dev=-1) == uns and "no CPU path" in L.mmf_last_error().decode()
    assert plan(E=-1) == inv and plan(N=-2) == inv and plan(ei=None) == inv and plan(status=None) == inv
    assert plan(E=1 << 31) == uns and "2^31" in L.mmf_last_error().decode() and L.mmf_last_error().decode().startswith("incidence_plan:")
    assert plan() == hip                                                      # a clean call gets as far as the device

    def prop(N=3, M=2, C=4, stride=4, x=b, Y=b, dev=63):
        return L.mmf_hypergraph_propagate(b, b, b, b, b, b, None, x, stride, N, M, C, Y, b, 0, dev, None)
    assert prop(dev=-1) == uns and prop(C=-1) == inv and prop(stride=3) == inv and prop(x=None) == inv and prop(Y=None) == inv
    assert prop(N=1 << 31) == uns and prop() == hip

    def gs(rows=3, C=4, ss=4, os_=4, ptr=b, dev=63):
        return L.mmf_csr_gather_sum(ptr, b, rows, b, ss, C, None, None, b, os_, dev, None)
    assert gs(dev=-1) == uns and gs(rows=-1) == inv and gs(ss=3) == inv and gs(os_=2) == inv and gs(ptr=None) == inv and gs() == hip


def test_the_kernel_file_has_no_float_atomics_and_checks_before_it_counts():
    src = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_hgconv.hip")).read()
    from test_stream_arguments_cpu import strip_comments
    code = strip_comments(src)
    atomics = re.findall(r"\batomic\w+\s*\(([^;]*);", code)
    assert len(atomics) == 2 and all("status" in a and "unsigned long long" in a for a in atomics)          # the two status words only
    keys = code.split("void hg_keys_kernel", 1)[1].split("\n}\n", 1)[0]
    assert keys.index("bad_v = v < 0 || v >= N") < keys.index("k_edge[j] =") and "ok ?" in keys
    assert "fmaf" not in code and "__fmaf" not in code and "hipMalloc" not in code and "Synchronize" not in code


# ---- documents ------------------------------------------------------------------------------------------------------------------------
def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design.split("## 4.35", 1)[1].split("\n## 5", 1)[0]
    for words in ("mmf_hypergraph_propagate", "mmf_incidence_plan", "order rule", "Hub rows", "Backward", "attention", "16-bit", "hgconv_timing"):
        assert words in sec, words
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "hypergraph_propagate" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "from multimodal_fusion_amd.hgconv import HypergraphConv" in integ and "cust_omics.py" in integ
    assert os.path.exists(os.path.join(ROOT, "scripts", "hgconv_timing.py"))
