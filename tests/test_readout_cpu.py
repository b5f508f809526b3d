"""The attention readout without a GPU (include/ext/mmf_hg_readout.h, multimodal-fusion_amd/readout.py and hypergraph_network.py,
DESIGN.md §4.36): the header and the export list, the package-level names and signatures, HypergraphNetwork's state-dict keys, the
canonical exponential's properties and its error on a sample, the numpy restatement (tests/readout_restate.py) against float64 within
the derived bounds, every ValueError the Python layer raises before any device work, the host checks of the C entries, the kernel
file's abstentions, and the documents."""
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
import readout_restate as rr      # noqa: E402

HEADER = os.path.join(ROOT, "include", "ext", "mmf_hg_readout.h")
ENTRIES = {"mmf_attention_readout_table", "mmf_attention_readout", "mmf_attention_readout_backward"}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, library, binding, package ------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.READOUT_EXPORTS) == ENTRIES
    for name, v in vars(mmf._lib).items():                                   # no other export list binds the names
        if name != "READOUT_EXPORTS" and isinstance(v, list) and all(isinstance(e, str) for e in v):
            assert not set(v) & declared, name
    assert not any(n.startswith("EXPORTS") and "READOUT" in n for n in vars(mmf._lib))
    assert mmf._lib.ABI_VERSION == 3 and mmf._lib.lib().mmf_version() == 3    # an addition
    assert int(re.search(r"^#define MMF_READOUT_CHUNK (\d+)$", hdr, re.M).group(1)) == rr.CHUNK == 64
    L = mmf._lib.lib()
    assert L.mmf_attention_readout_table.restype is ctypes.c_int64 and len(L.mmf_attention_readout_table.argtypes) == 4
    assert L.mmf_attention_readout.restype is ctypes.c_int and len(L.mmf_attention_readout.argtypes) == 15
    assert L.mmf_attention_readout_backward.restype is ctypes.c_int and len(L.mmf_attention_readout_backward.argtypes) == 15
    for words in ("READOUT_EXPORTS", "sequential chain", "no fma", "cexp(0) == 1.0f", "1e-16", "2^31", "dot64", "-87.0f", "0.693145751953125",
                  "synchronises", "{ segment id, first row }"):
        assert words in hdr, words
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_readout", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("ext", "mmf_hg_readout.h")) for h in b.HEADERS) and all(os.path.exists(h) for h in b.HEADERS if os.path.isabs(h))
    assert "mmf_readout.hip" in b.SOURCES and "mmf_readout.hip" not in b.EXTRA_FLAGS and "-ffp-contract=off" in b.FLAGS
    assert '#include "../../include/ext/mmf_hg_readout.h"' in open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_host.h")).read()


def test_package_exports_the_modules_and_their_names(mmf):
    from importlib import import_module
    m = import_module("multimodal_fusion_amd.readout")
    n = import_module("multimodal_fusion_amd.hypergraph_network")
    assert mmf.readout is m and "readout" in mmf.__all__ and "mmf.readout.*" in mmf.__doc__
    for name in ("attention_readout", "readout_plan", "GlobalAttention"):
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
    assert "HypergraphNetwork" in mmf.__all__ and mmf.HypergraphNetwork is n.HypergraphNetwork
    sig = inspect.signature(m.readout_plan)
    assert list(sig.parameters) == ["ptr", "batch", "rows", "size", "device"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("rows", "size", "device"))
    sig = inspect.signature(m.attention_readout)
    assert list(sig.parameters) == ["x", "gate", "ptr", "batch", "plan", "size", "return_attention"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("plan", "size", "return_attention"))
    assert list(inspect.signature(m.GlobalAttention.__init__).parameters)[1:] == ["gate_nn", "nn"]
    fwd = inspect.signature(m.GlobalAttention.forward).parameters
    assert list(fwd)[1:5] == ["x", "batch", "ptr", "size"] and fwd["plan"].kind is inspect.Parameter.KEYWORD_ONLY
    init = inspect.signature(n.HypergraphNetwork.__init__).parameters
    assert list(init)[1:] == ["input_dim", "hidden_dims", "output_dim", "dropout", "use_attention"]
    assert init["dropout"].default == 0.2 and init["use_attention"].default is False
    fwd = inspect.signature(n.HypergraphNetwork.forward).parameters
    assert list(fwd)[1:4] == ["x", "edge_index", "batch"]
    assert fwd["incidence"].kind is inspect.Parameter.KEYWORD_ONLY and fwd["readout"].kind is inspect.Parameter.KEYWORD_ONLY


def test_hypergraph_network_has_the_reference_modules_state_dict(mmf):
    net = mmf.HypergraphNetwork(32, [16, 12, 8], 10)
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    want = (["first_h.0.weight", "first_h.0.bias"] + [f"first_h.1.{k}" for k in bn] +
            ["convs.0.lin.weight", "convs.0.bias", "convs.1.lin.weight", "convs.1.bias", "output_layer.weight", "output_layer.bias",
             "attention_pool.gate_nn.0.weight", "attention_pool.gate_nn.0.bias", "attention_pool.gate_nn.2.weight", "attention_pool.gate_nn.2.bias"])
    sd = net.state_dict()
    assert sorted(sd) == sorted(want)
    shapes = {"first_h.0.weight": (16, 32), "convs.0.lin.weight": (12, 16), "convs.1.lin.weight": (8, 12), "convs.1.bias": (8,),
              "output_layer.weight": (10, 8), "attention_pool.gate_nn.0.weight": (4, 8), "attention_pool.gate_nn.2.weight": (1, 4)}
    for k, shp in shapes.items():
        assert tuple(sd[k].shape) == shp, k
    net.load_state_dict({k: torch.full_like(v, 2) for k, v in sd.items()})    # a checkpoint with those keys loads
    assert float(net.convs[1].bias.detach()[0]) == 2.0 and float(net.attention_pool.gate_nn[2].weight.detach()[0, 0]) == 2.0
    assert net.num_layers == 3 and net.hidden_dims == [16, 12, 8] and net.dropout == 0.2
    assert len(mmf.HypergraphNetwork(8, [8], 4).convs) == 0
    with pytest.raises(NotImplementedError):
        mmf.HypergraphNetwork(32, [16, 8], 10, use_attention=True)
    pool = mmf.GlobalAttention(torch.nn.Linear(4, 1), torch.nn.Linear(4, 3))
    assert sorted(pool.state_dict()) == ["gate_nn.bias", "gate_nn.weight", "nn.bias", "nn.weight"]


# ---- cexp -----------------------------------------------------------------------------------------------------------------------------
def test_cexp_properties():
    assert rr.cexp(np.float32(0.0)) == np.float32(1.0) and rr.cexp(np.float32(-0.0)) == np.float32(1.0)
    below = np.array([np.nextafter(np.float32(-87.0), np.float32(-np.inf)), -88.0, -1e4, -3e38], dtype=np.float32)
    assert not rr.cexp(below).any() and not np.signbit(rr.cexp(below)).any()
    edge = rr.cexp(np.float32(-87.0))
    assert edge >= np.finfo(np.float32).tiny and abs(float(edge) / np.exp(-87.0) - 1) < 1e-6          # a normal number
    t = np.linspace(-87.0, 0.0, 1 << 20).astype(np.float32)                   # spaced some 700 ulps of the result apart
    v = rr.cexp(t)
    assert (v[1:] >= v[:-1]).all() and (v >= np.finfo(np.float32).tiny).all() and v[-1] == 1.0
    assert rr.LN2_HI == np.float32(0.693145751953125) and float(rr.LN2_HI) == 0.693145751953125
    assert [float(c) for c in rr.COEF[:3]] == [1.0, 1.0, 0.5]


def test_cexp_against_float64_on_a_sample():
    """2^22 seeded values in four ranges plus the boundaries, in ulps of the correctly rounded result; the bound is the full sweep's
    (scripts/readout_exp_sweep.py), rounded up to the next half ulp."""
    rng = np.random.RandomState(0)
    q = 1 << 20
    t = np.concatenate([-87.0 * rng.rand(q), -rng.rand(q), -8.0 * rng.rand(q), -np.exp(-20.0 * rng.rand(q)),
                        [0.0, -0.0, -87.0, -86.99999, -0.5 * np.log(2.0), -np.log(2.0), -1e-30, -71.04561614990234]]).astype(np.float32)
    got = rr.cexp(t).astype(np.float64)
    want = np.exp(t.astype(np.float64))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    print(f"cexp on {t.size} values: max error {err.max():.4f} ulp at t = {t[np.argmax(err)]!r}; CEXP_ULPS = {rr.CEXP_ULPS}")
    assert err.max() <= rr.CEXP_ULPS and rr.CEXP_ULPS * 2 == int(rr.CEXP_ULPS * 2)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
CASES = [(rr.EDGE_SIZES, 9, 1, 3.0), ((200,), 33, 2, 1.0), ((5, 0, 700, 64), 70, 3, 30.0), ((130, 1, 1), 4, 4, 0.01)]


@pytest.mark.parametrize("sizes,C,seed,scale", CASES)
def test_restatement_against_float64(sizes, C, seed, scale):
    ptr = rr.offsets(sizes)
    N = int(ptr[-1])
    x, gate = rr.features(N, C, seed), rr.gates(N, 10 + seed, scale)
    out, alpha, seg_max, seg_sum = rr.forward(x, gate, ptr)
    n = np.diff(ptr)
    for s in range(len(sizes)):                                               # alpha sums to 1
        a = alpha[ptr[s]:ptr[s + 1]].astype(np.float64)
        if n[s]:
            assert abs(a.sum() - 1.0) <= (n[s] + 2) * 2.0 ** -24, (s, a.sum())
            assert seg_max[s] == gate[ptr[s]:ptr[s + 1]].max() and seg_sum[s] >= 1.0
        else:
            assert not out[s].any() and seg_max[s] == -np.inf and seg_sum[s] == 0.0
    o64, a64 = rr.reference64(x, gate, ptr)
    err = np.abs(out.astype(np.float64) - o64)
    tol = rr.bound(x, gate, ptr)
    print(f"sizes={sizes} C={C}: forward max err / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all()
    G = rr.features(len(sizes), C, 20 + seed)
    gx, gg = rr.backward(x, ptr, alpha, out, G)
    gx64, gg64 = rr.backward64(x, gate, ptr, G)
    tol_x, tol_g = rr.bound_backward(x, gate, ptr, G)
    ex, eg = np.abs(gx - gx64), np.abs(gg - gg64)
    print(f"   backward: grad_x max err / bound = {np.max(ex / np.maximum(tol_x, 1e-300)):.3f}, grad_gate {np.max(eg / np.maximum(tol_g, 1e-300)):.3f}")
    assert (ex <= tol_x).all() and (eg <= tol_g).all()


def test_restatement_pieces():
    assert rr.chunk_table([0, 0, 130, 130, 131]).tolist() == [[1, 0], [1, 64], [1, 128], [3, 130]]
    assert rr.chunk_table([0]).shape == (0, 2) and rr.chunk_table([0, 0]).shape == (0, 2)
    a, b = rr.features(3, 150, 1), rr.features(3, 150, 2)
    assert np.allclose(rr.dot64(a, b), (a.astype(np.float64) * b).sum(1), rtol=0, atol=1e-4)
    assert rr.dot64(a[:, :1], b[:, :1])[0] == a[0, 0] * b[0, 0]
    # a maximum of -0 and +0 is +0, whatever the order
    for g in ([-0.0, 0.0], [0.0, -0.0]):
        _, _, m, _ = rr.forward(np.ones((2, 1), dtype=np.float32), np.array(g, dtype=np.float32), [0, 2])
        assert m[0] == 0 and not np.signbit(m[0])
    out, alpha, _, _ = rr.forward(np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.float32), [0, 0])
    assert out.shape == (1, 3) and alpha.shape == (0,)


# ---- the Python layer's refusals, before any device work ------------------------------------------------------------------------------
def test_value_errors_need_no_device(mmf, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    m = mmf.readout
    x, g = torch.zeros(6, 4), torch.zeros(6)
    with pytest.raises(ValueError, match="x must be float32"):
        m.attention_readout(x.double(), g)
    with pytest.raises(ValueError, match="x must be float32"):
        m.attention_readout(x.half(), g)
    with pytest.raises(ValueError, match=r"x must be a float32 tensor \[N, C\]"):
        m.attention_readout(x[0], g)
    with pytest.raises(ValueError, match="gate must be float32"):
        m.attention_readout(x, g.double())
    with pytest.raises(ValueError, match=r"gate must have shape \[N\] or \[N, 1\]"):
        m.attention_readout(x, torch.zeros(5))
    with pytest.raises(ValueError, match=r"gate must have shape \[N\] or \[N, 1\]"):
        m.attention_readout(x, torch.zeros(6, 2))
    with pytest.raises(ValueError, match="gate is on meta, x on cpu"):
        m.attention_readout(x, torch.zeros(6, device="meta"))
    with pytest.raises(ValueError, match="exactly one of ptr / batch"):
        m.attention_readout(x, g, ptr=[0, 6], batch=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="ptr must end at 6"):
        m.attention_readout(x, g, ptr=[0, 5])
    with pytest.raises(ValueError, match="ptr decreases"):
        m.attention_readout(x, g, ptr=[0, 4, 2, 6])
    with pytest.raises(ValueError, match="batch must be sorted"):
        m.attention_readout(x, g, batch=torch.tensor([0, 1, 0, 1, 1, 1]))
    with pytest.raises(ValueError, match="size = 1, but the description holds 2 segments"):
        m.attention_readout(x, g, ptr=[0, 3, 6], size=1)
    with pytest.raises(ValueError, match="size = 1, but the description holds 2 segments"):
        m.readout_plan(ptr=[0, 3, 6], size=1)
    with pytest.raises(ValueError, match="exactly one of ptr / batch"):
        m.readout_plan()
    plan = m.ReadoutPlan(torch.tensor([0, 2, 5]), torch.tensor([0, 2, 5]), torch.zeros((2, 2), dtype=torch.int32), 2)
    assert (plan.num_rows, plan.num_segments, plan.num_chunks) == (5, 2, 2)
    with pytest.raises(ValueError, match="built for 5 rows, x has 6"):
        m.attention_readout(x, g, plan=plan)
    with pytest.raises(ValueError, match="the plan is on cpu, x on meta"):
        m.attention_readout(torch.zeros(5, 4, device="meta"), torch.zeros(5, device="meta"), plan=plan)
    for extra in (dict(ptr=[0, 5]), dict(batch=torch.zeros(5, dtype=torch.int64)), dict(size=2)):
        with pytest.raises(ValueError, match="either plan or a description"):
            m.attention_readout(x[:5], g[:5], plan=plan, **extra)
    # valid calls on host tensors reach the package's device error, not a CPU path
    for kw in (dict(), dict(ptr=[0, 2, 6]), dict(batch=torch.tensor([0, 0, 1, 1, 1, 3]), size=5), dict(plan=m.ReadoutPlan(
            torch.tensor([0, 6]), torch.tensor([0, 6]), torch.zeros((1, 2), dtype=torch.int32), 1))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.attention_readout(x, g.reshape(6, 1), **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.readout_plan(ptr=[0, 3, 6], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmf.GlobalAttention(torch.nn.Linear(4, 1))(x)
    net = mmf.HypergraphNetwork(4, [4, 4], 2).eval()
    with pytest.raises(ValueError, match="pass edge_index or incidence"):
        net(x)


# ---- the C entries' host checks (host buffers stand in for device pointers; device 63 does not exist) -----------------------------------
def test_the_table_entry(mmf):
    L = mmf._lib.lib()
    inv, uns = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED

    def table(ptr, cap=None):
        p = (ctypes.c_int64 * len(ptr))(*ptr)
        n = L.mmf_attention_readout_table(p, len(ptr) - 1, None, 0)
        if n < 0:
            return n, None
        out = (ctypes.c_int32 * (2 * max(n, 1)))()
        got = L.mmf_attention_readout_table(p, len(ptr) - 1, out, n if cap is None else cap)
        return got, np.array(out[:2 * n], dtype=np.int32).reshape(-1, 2)

    for ptr in ([0, 0, 130, 130, 131], [0], [0, 0], [0, 64], [0, 65, 65, 1065], list(rr.offsets(rr.EDGE_SIZES))):
        n, tab = table(ptr)
        want = rr.chunk_table(ptr)
        assert n == want.shape[0] and np.array_equal(tab, want), ptr
    assert table([1, 5])[0] == inv and "must start at 0" in L.mmf_last_error().decode()
    assert L.mmf_last_error().decode().startswith("attention_readout_table:")
    assert table([0, 5, 3])[0] == inv and "decreases" in L.mmf_last_error().decode()
    assert table([0, 1 << 31])[0] == uns and "2^31" in L.mmf_last_error().decode()
    assert table([0, 200], cap=3)[0] == inv and "4 records" in L.mmf_last_error().decode()
    assert L.mmf_attention_readout_table(None, 1, None, 0) == inv
    p = (ctypes.c_int64 * 2)(0, 5)
    assert L.mmf_attention_readout_table(p, -1, None, 0) == inv and L.mmf_attention_readout_table(p, 1 << 31, None, 0) == uns


def test_device_entries_check_their_arguments_before_the_device(mmf):
    L = mmf._lib.lib()
    inv, uns, hip = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED, mmf._lib.MMF_E_HIP
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(x=b, stride=4, gate=b, ptr=b, tab=b, Q=2, N=100, S=2, C=4, out=b, alpha=b, mx=b, sm=b, dev=63):
        return L.mmf_attention_readout(x, stride, gate, ptr, tab, Q, N, S, C, out, alpha, mx, sm, dev, None)
    assert fwd(dev=-1) == uns and "no CPU path" in L.mmf_last_error().decode() and L.mmf_last_error().decode().startswith("attention_readout:")
    for kw in (dict(x=None), dict(gate=None), dict(ptr=None), dict(tab=None), dict(out=None), dict(alpha=None), dict(mx=None), dict(sm=None)):
        assert fwd(**kw) == inv and "NULL" in L.mmf_last_error().decode(), kw
    assert fwd(N=-1) == inv and fwd(S=-1) == inv and fwd(C=-1) == inv and fwd(Q=-1) == inv
    assert fwd(stride=3) == inv and "row pitch" in L.mmf_last_error().decode()
    assert fwd(Q=1) == inv and fwd(Q=101) == inv and "chunks cannot hold" in L.mmf_last_error().decode()
    assert fwd(N=1 << 31, Q=1 << 26) == uns and fwd(S=1 << 31) == uns and fwd(C=1 << 31, stride=1 << 31) == uns
    assert "2^31" in L.mmf_last_error().decode()
    assert fwd() == hip                                                       # a clean call gets as far as the device

    def bwd(x=b, stride=4, alpha=b, ptr=b, tab=b, Q=2, out=b, G=b, N=100, S=2, C=4, gx=b, gg=b, dev=63):
        return L.mmf_attention_readout_backward(x, stride, alpha, ptr, tab, Q, out, G, N, S, C, gx, gg, dev, None)
    assert bwd(dev=-1) == uns and L.mmf_last_error().decode().startswith("attention_readout_backward:") and "no CPU path" in L.mmf_last_error().decode()
    for kw in (dict(x=None), dict(alpha=None), dict(ptr=None), dict(tab=None), dict(out=None), dict(G=None), dict(gx=None)):
        assert bwd(**kw) == inv and "NULL" in L.mmf_last_error().decode(), kw
    assert bwd(N=-1) == inv and bwd(stride=3) == inv and bwd(Q=1) == inv and bwd(N=1 << 31, Q=1 << 26) == uns
    assert bwd() == hip and bwd(gg=None) == hip and bwd(gg=None, x=None, out=None) == hip       # without the gate's gradient x is not read


def test_the_kernel_file_abstains():
    src = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_readout.hip")).read()
    from test_stream_arguments_cpu import strip_comments
    code = strip_comments(src)
    atomics = re.findall(r"\batomic\w+", code)
    assert atomics == ["atomicMax"]                                           # the integer key of the maximum, nothing on floats
    for word in ("atomicAdd", "fmaf", "__fma", "expf", "exp2f", "__expf", "hipMalloc", "Synchronize", "hipMemcpy"):
        assert word not in code, word
    assert "MMF_READOUT_CHUNK == 64" in code and code.count("hipMemsetAsync") == 1


# ---- documents ------------------------------------------------------------------------------------------------------------------------
def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.index("## 4.35") < design.index("## 4.36") < design.index("\n## 5")
    sec = design.split("## 4.36", 1)[1].split("\n## 5", 1)[0]
    for words in ("mmf_attention_readout", "GlobalAttention", "cexp", "1.21", "CEXP_ULPS", "dot64", "Backward", "Refus", "readout_timing",
                  "Left", "VGPR", "HypergraphNetwork"):
        assert words in sec, words
    assert "§4.36" in design.split("## 4.35", 1)[1].split("## 4.36", 1)[0]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "attention_readout" in readme and "HypergraphNetwork" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Readout entries" in integ and "cust_omics.py" in integ
    assert "from multimodal_fusion_amd.readout import GlobalAttention" in integ
    for name in ("readout_timing.py", "readout_exp_sweep.py"):
        assert os.path.exists(os.path.join(ROOT, "scripts", name)), name
