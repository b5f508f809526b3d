"""The 16-bit combined top-k for any k without a GPU (mmf_simtopk_combined_fast_anyk, include/ext/mmf_hg_topk16_anyk.h, DESIGN.md
§4.33): the header and the export list, the entry's host checks in their order and wording before any device call, the k values on
both sides of the one-pass boundary reaching the device, the one-pass entries keeping their refusal, the host-only plan, the
router's decisions, the Python errors, the documents — and the numpy restatement of the ceiling and of the pass loop
(tests/combined16_anyk_restate.py) on the seeded inputs tests/test_gpu_simtopk_combined_fast_anyk.py runs."""
import ctypes
import inspect
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combined16_anyk_restate as ar   # noqa: E402

ENTRY, PLAN = "mmf_simtopk_combined_fast_anyk", "mmf_combined_fast_anyk_plan"
WHO = "simtopk_combined_fast_anyk"
HEADER = os.path.join(ROOT, "include", "ext", "mmf_hg_topk16_anyk.h")


def _mod():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16_anyk")


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, library, binding ---------------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.TOPK16_ANYK_EXPORTS) == {ENTRY, PLAN}
    assert '#include "mmf_hg_fast_anyk.h"' in hdr and "typedef struct" not in hdr          # the info struct is reused, not redeclared
    for name, v in vars(mmf._lib).items():                                                 # no other export list binds the two names
        if name != "TOPK16_ANYK_EXPORTS" and isinstance(v, list) and all(isinstance(e, str) for e in v):
            assert not set(v) & declared, name
    inc = os.path.join(ROOT, "include")
    for d in (inc, os.path.join(inc, "ext")):
        for h in os.listdir(d):
            if h.endswith(".h") and h != "mmf_hg_topk16_anyk.h":
                assert ENTRY + "(" not in open(os.path.join(d, h)).read(), h
    L = mmf._lib.lib()
    for name in mmf._lib.TOPK16_ANYK_EXPORTS:
        assert getattr(L, name).restype is ctypes.c_int
    assert list(L.mmf_simtopk_combined_fast_anyk.argtypes) == list(L.mmf_simtopk_combined.argtypes) + [ctypes.POINTER(mmf._lib.FastAnykInfo)]
    assert len(L.mmf_simtopk_combined_fast_anyk.argtypes) == 18
    assert L.mmf_combined_fast_anyk_plan.argtypes == L.mmf_fast_anyk_plan.argtypes
    assert mmf._lib.ABI_VERSION == 3 and L.mmf_version() == 3                               # an addition
    for words in ("bit for bit", "MMF_PREC_FAST_BF16", "MMF_ANYK_SHORT_DIV", "Host-synchronous", "TOPK16_ANYK_EXPORTS", "k + self <= 20",
                  "0 (automatic)\n * or a power of two"):
        assert words in hdr, words
    build = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py")).read()
    assert "mmf_hg_topk16_anyk.h" in build and "mmf_topk_anyk.hip" in build and "mmf_rerank_combined.h" in build
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_topk16_anyk", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mmf_scan_b16c.hip" not in b.EXTRA_FLAGS and "mmf_topk_anyk.hip" not in b.EXTRA_FLAGS      # both select on -inf: NaNs are honoured


def test_python_signatures(mmf):
    m = _mod()
    assert mmf.combined_topk16_anyk is m and "combined_topk16_anyk" in mmf.__all__ and "mmf.combined_topk16_anyk.*" in mmf.__doc__
    for name in ("simtopk_combined_fast_any_k", "combined_fast_anyk_plan", "build_topk_weighted_hypergraph_fast_any_k",
                 "build_topk_hypergraph_data_fast_any_k"):
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
    # the router carries the name of combined_topk_anyk's call, which keeps the package-level name
    assert mmf.simtopk_combined_any_k is mmf.combined_topk_anyk.simtopk_combined_any_k is not m.simtopk_combined_any_k
    sig = inspect.signature(m.simtopk_combined_fast_any_k)
    assert list(sig.parameters) == ["features", "positions", "lambda_h", "lambda_g", "k", "ptr", "batch", "exclude_self", "precision",
                                    "col_splits", "return_stats", "return_info", "profile"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [1.0, 1.0, 5, None, None, True, "fast", 0, False, False, False]
    rsig = inspect.signature(m.simtopk_combined_any_k)
    old = inspect.signature(mmf.combined_topk_anyk.simtopk_combined_any_k)
    assert [n for n in rsig.parameters if n != "precision"] == list(old.parameters) and rsig.parameters["precision"].default == "auto"
    for fn, ref in ((m.build_topk_weighted_hypergraph_fast_any_k, mmf.combined_topk_anyk.build_topk_weighted_hypergraph_any_k),
                    (m.build_topk_hypergraph_data_fast_any_k, mmf.combined_topk_anyk.build_topk_hypergraph_data_any_k)):
        assert list(inspect.signature(fn).parameters) == list(inspect.signature(ref).parameters) + ["precision"]
    assert list(inspect.signature(m.combined_fast_anyk_plan).parameters) == ["d", "k", "exclude_self"]


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan(mmf):
    plan = mmf.combined_fast_anyk_plan
    assert plan(512, 19, True) == {"multi_pass": False, "scan_kk": 20, "first_yield": 19, "min_passes": 1}
    assert plan(512, 20, True) == {"multi_pass": True, "scan_kk": 20, "first_yield": 19, "min_passes": 2}
    assert plan(512, 20, False) == {"multi_pass": False, "scan_kk": 20, "first_yield": 20, "min_passes": 1}
    assert plan(512, 21, False) == {"multi_pass": True, "scan_kk": 20, "first_yield": 20, "min_passes": 2}
    assert plan(40, 5, True) == {"multi_pass": False, "scan_kk": 6, "first_yield": 5, "min_passes": 1}
    assert plan(1536, 38, True) == {"multi_pass": True, "scan_kk": 20, "first_yield": 19, "min_passes": 2}
    assert plan(1536, 39, True) == {"multi_pass": True, "scan_kk": 20, "first_yield": 19, "min_passes": 3}
    assert plan(4096, 64, True) == {"multi_pass": True, "scan_kk": 20, "first_yield": 19, "min_passes": 4}     # ceil(64 / 19)
    assert plan(1, 64, False) == {"multi_pass": True, "scan_kk": 20, "first_yield": 20, "min_passes": 4}       # ceil(64 / 20)
    for d in (1, 40, 512, 1024, 1025, 4096):                      # one depth at every served d, and the restatement's plan
        for k in (1, 18, 19, 20, 21, 38, 39, 40, 41, 45, 64, 128, 500):
            for ex in (False, True):
                p = plan(d, k, ex)
                assert (p["scan_kk"], p["first_yield"], p["min_passes"]) == ar.plan(k, ex), (d, k, ex)
                assert p["multi_pass"] == (k + ex > 20)
    L = mmf._lib.lib()
    UNS, INV = mmf._lib.MMF_E_UNSUPPORTED, mmf._lib.MMF_E_INVALID
    assert L.mmf_combined_fast_anyk_plan(4097, 32, 0, None, None, None) == UNS and "d = 4097" in L.mmf_last_error().decode()
    assert L.mmf_combined_fast_anyk_plan(0, 5, 0, None, None, None) == INV
    assert L.mmf_combined_fast_anyk_plan(512, 0, 0, None, None, None) == INV
    assert L.mmf_combined_fast_anyk_plan(512, 64, 1, None, None, None) == 1 and L.mmf_combined_fast_anyk_plan(512, 5, 1, None, None, None) == 0
    for bad in [(4097, 32, False), (0, 5, True), (512, 0, True)]:
        with pytest.raises(ValueError, match="mmf_combined_fast_anyk_plan"):
            plan(*bad)


# ---- the entry's host checks, with host buffers standing in for device pointers -------------------------------------------------------
def _call(fn=ENTRY, **kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(F=b, P=b, n=4, d=4, dp=2, lh=1.0, lg=1.0, k=2, self=1, ptr=None, S=0, idx=b, val=b, opts=(2, 0, 0, 0, None), device=63, info=True)
    a.update(kw)
    ptr = a["ptr"]
    if ptr is not None:
        ptr = ctypes.cast((ctypes.c_int64 * len(ptr))(*ptr), ctypes.c_void_p)
    opts = a["opts"]
    if opts is not None:
        opts = ctypes.byref(mmf._lib.SimtopkOpts(*opts))
    args = [a["F"], a["P"], a["n"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], ptr, a["S"], a["idx"], a["val"], opts, None, a["device"], None]
    if fn == ENTRY:
        args.append(ctypes.byref(mmf._lib.FastAnykInfo()) if a["info"] else None)
    rc = getattr(L, fn)(*args)
    return rc, L.mmf_last_error().decode()


INVALID = [
    (dict(n=-1), "n must be >= 0 (got -1)"),
    (dict(d=0), "d must be at least 1 (got 0)"),
    (dict(dp=0), "dp must be at least 1 (got 0)"),
    (dict(k=0), "k must be at least 1 (got 0)"),
    (dict(lh=-0.5), "lambda_h must be finite and >= 0"),
    (dict(lh=float("inf")), "lambda_h must be finite and >= 0"),
    (dict(lg=-1.0), "lambda_g must be finite and >= 0"),
    (dict(lg=float("nan")), "lambda_g must be finite and >= 0"),
    (dict(F=None), "F is NULL"),
    (dict(P=None), "P is NULL"),
    (dict(idx=None), "out_idx is NULL"),
    (dict(val=None), "out_val is NULL"),
    (dict(ptr=None, S=2), "host offsets ptr_host[n_seg + 1]"),
    (dict(ptr=[0, 4], S=-1), "need n_seg >= 0"),
    (dict(ptr=[1, 2, 4], S=2), "ptr_host must start at 0"),
    (dict(ptr=[0, 3, 2, 4], S=3), "ptr_host decreases at segment 1"),
    (dict(ptr=[0, 1, 3], S=2), "ptr_host must end at 4 (got 3)"),
    (dict(opts=(7, 0, 0, 0, None)), "precision 7: MMF_PREC_AUTO, _EXACT, _FAST (f16 operands) or _FAST_BF16"),
    (dict(opts=(2, 0, -1, 0, None)), "col_splits must be 0 or a power of two (got -1)"),
    (dict(opts=(2, 0, 3, 0, None)), "col_splits must be 0 or a power of two (got 3)"),
    (dict(opts=(1, 0, 6, 0, None), ptr=[0, 1, 4], S=2), "col_splits must be 0 or a power of two (got 6)"),
]
UNSUPPORTED = [
    (dict(dp=9), "dp = 9 > 8 is not supported"),
    (dict(d=4097), "d = 4097 > 4096 is not supported (mmf_simtopk_combined takes any d)"),
    (dict(d=4097, k=64), "d = 4097 > 4096 is not supported"),
    (dict(n=1 << 31), "n must be < 2^31"),
    (dict(n=1 << 31, ptr=[0, 1 << 31], S=1), "n must be < 2^31"),
]


@pytest.mark.parametrize("kw,words", INVALID)
def test_entry_refuses_bad_arguments_before_any_device_call(mmf, kw, words):
    """A device id that does not exist: an argument error must win over the device's."""
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and msg.startswith(WHO + ":"), (rc, msg)


@pytest.mark.parametrize("kw,words", UNSUPPORTED)
def test_entry_refuses_what_it_does_not_support_before_any_device_call(mmf, kw, words):
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and words in msg and msg.startswith(WHO + ":"), (rc, msg)


def test_the_order_and_the_wording_of_the_checks(mmf):
    """The argument checks first, then the offsets, then what is unsupported, then the options — the order of the two one-pass
    entries, whose words the shared refusals repeat under the new name."""
    inv, uns = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    for kw in (dict(), dict(k=0), dict(F=None), dict(dp=9), dict(ptr=None, S=2), dict(d=4097), dict(k=64)):
        rc, msg = _call(device=-1, **kw)
        assert rc == uns and "no CPU path" in msg and msg.startswith(WHO + ":"), (rc, msg)
    assert _call(k=0, ptr=[1, 4], S=1)[1].count("k must be at least 1") == 1
    rc, msg = _call(ptr=[1, 4], S=1, dp=9)
    assert rc == inv and "must start at 0" in msg
    rc, msg = _call(dp=9, d=4097, opts=(7, 0, 0, 0, None))
    assert rc == uns and "dp = 9 > 8" in msg
    rc, msg = _call(d=4097, n=1 << 31, opts=(7, 0, 0, 0, None))
    assert rc == uns and "d = 4097" in msg
    rc, msg = _call(opts=(7, 0, 3, 0, None))
    assert rc == inv and "precision 7" in msg
    seg, one = "mmf_simtopk_combined_fast_segmented", "mmf_simtopk_combined_fast"
    shared = [(dict(n=-1), one), (dict(dp=0), one), (dict(lh=-1.0), one), (dict(val=None), one), (dict(dp=9), one), (dict(d=4097), one),
              (dict(opts=(7, 0, 0, 0, None)), one), (dict(ptr=[0, 1, 3], S=2), seg), (dict(ptr=[0, 4], S=1, opts=(2, 0, 3, 0, None)), seg),
              (dict(ptr=[0, 4], S=1, n=1 << 31), seg)]
    for kw, other in shared:
        rc_o, msg_o = _call(other, **kw)
        rc_n, msg_n = _call(**kw)
        assert rc_o == rc_n and rc_n < 0 and msg_n == msg_o.replace(other[4:], WHO, 1), (kw, msg_o, msg_n)


@pytest.mark.parametrize("k", [1, 18, 19, 20, 21, 38, 39, 45, 64, 200])
def test_every_k_reaches_the_device(mmf, k):
    """No refusal on either side of the one-pass boundary, with and without self, one graph or a batch, every precision: the call
    gets as far as the device (which is not there)."""
    for kw in (dict(), dict(self=0), dict(ptr=[0, 1, 4], S=2), dict(ptr=[0, 0, 4, 4], S=3, self=0), dict(opts=None), dict(opts=(0, 0, 0, 0, None)),
               dict(opts=(1, 0, 0, 0, None)), dict(opts=(3, 1, 4, 0, None)), dict(lh=0.0, lg=0.0), dict(dp=8, d=4096), dict(info=False),
               dict(opts=(2, 0, 32, 0, None)), dict(n=300), dict(n=300, ptr=[0, 100, 300], S=2)):
        rc, msg = _call(k=k, **kw)
        assert rc == mmf._lib.MMF_E_HIP, (k, kw, rc, msg)


def test_no_rows_are_a_no_op(mmf):
    assert _call(n=0)[0] == mmf._lib.MMF_OK
    assert _call(n=0, k=64, ptr=[0, 0, 0], S=2, F=None, P=None, idx=None, val=None)[0] == mmf._lib.MMF_OK


def test_the_one_pass_entries_keep_their_refusal(mmf):
    uns = mmf._lib.MMF_E_UNSUPPORTED
    for kw in (dict(k=20), dict(k=21, self=0)):
        rc, msg = _call("mmf_simtopk_combined_fast", **kw)
        assert rc == uns and msg == "simtopk_combined_fast: k + self = 21 > 20 is not supported (mmf_simtopk_combined takes up to 44)", msg
        rc, msg = _call("mmf_simtopk_combined_fast_segmented", ptr=[0, 1, 4], S=2, **kw)
        assert rc == uns and msg == "simtopk_combined_fast_segmented: k + self = 21 > 20 is not supported (mmf_simtopk_combined takes up to 44)", msg
    rc, msg = _call("mmf_simtopk_combined_fast", ptr=[0, 2, 4], S=2)
    assert rc == uns and "stays on mmf_simtopk_combined" in msg
    rc, msg = _call("mmf_simtopk_combined_anyk", opts=(2, 0, 0, 0, None), k=64)
    assert rc == uns and "the 16-bit combined scans stop at k + self = 20" in msg


# ---- the router and the Python errors -------------------------------------------------------------------------------------------------
def test_the_routers_decisions(mmf):
    m = _mod()
    fast, exact = "combined_topk16_anyk.simtopk_combined_fast_any_k", "combined_topk_anyk.simtopk_combined_any_k"
    for prec in ("fast", "fast_bf16"):
        for k in (5, 19, 20, 64):
            assert m.anyk_route(65536, 512, k, True, 1, prec) == fast
    for k in (5, 19, 20, 64, 200):
        assert m.anyk_route(65536, 512, k, True, 1, "exact") == exact
    # "auto": the f16 call only on the measured classes of _AUTO_SHAPES, never where one pass serves, never beyond d = 4096
    assert m._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "simtopk_combined_fast_anyk_timing.txt"))
    for dl, dh, kl, kh, nl, pl, sh in m._AUTO_SHAPES:
        assert 1 <= dl <= dh <= 4096 and 20 <= kl <= kh and nl >= pl >= 1 and sh >= 1 and nl >= pl * sh
        assert m.anyk_route(nl, dl, kh, True, sh, "auto") == fast and m.anyk_route(nl, dh, kl + 1, False, sh, "auto") == fast
    # the measured winners and losers of profiles/simtopk_combined_fast_anyk_timing.txt
    for n, d, k, segs, want in ((16384, 512, 32, 1, fast), (262144, 512, 64, 1, fast), (65536, 1536, 64, 1, fast), (65536, 1024, 45, 1, fast),
                                (262144, 512, 32, 16, fast), (262144, 1536, 32, 16, fast), (262144, 1536, 32, 64, fast),
                                (262144, 512, 32, 64, exact), (262144, 512, 32, 2048, exact), (262144, 512, 64, 16, exact),
                                (8192, 512, 32, 1, exact), (65536, 256, 32, 1, exact), (65536, 2048, 32, 1, exact), (65536, 512, 128, 1, exact),
                                (32768, 512, 32, 2, exact)):
        assert m.anyk_route(n, d, k, True, segs, "auto") == want, (n, d, k, segs)
    for k in (1, 5, 19):
        assert m.anyk_route(1 << 20, 1536, k, True, 1, "auto") == exact                            # one pass: the existing routes decide
    assert m.anyk_route(1 << 20, 1536, 20, False, 1, "auto") == exact
    assert m.anyk_route(1 << 20, 5000, 64, True, 1, "auto") == exact and m.anyk_route(100, 512, 64, True, 1, "auto") == exact
    assert m.anyk_route(65536, 512, 64, True, 1, "exact") == exact
    with pytest.raises(ValueError, match="unknown precision"):
        m.anyk_route(100, 40, 5, True, 1, "fastest")
    with pytest.raises(ValueError, match="k must be >= 1"):
        m.anyk_route(100, 40, 0, True, 1)


def test_wrappers_reject_bad_input_before_any_library_call(mmf, monkeypatch):
    m = _mod()

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    ptr = torch.tensor([0, 4, 10])
    for f in (m.simtopk_combined_fast_any_k, m.simtopk_combined_any_k, m.build_topk_weighted_hypergraph_fast_any_k,
              m.build_topk_hypergraph_data_fast_any_k):
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:9], k=64)
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:, 0], k=64, ptr=ptr)
        with pytest.raises(ValueError, match=r"k must be >= 1 \(got 0\)"):
            f(F, P, k=0)
        with pytest.raises(ValueError, match="unknown precision 'half'"):
            f(F, P, k=64, precision="half")
        with pytest.raises(ValueError, match="ptr"):
            f(F, P, k=64, ptr=ptr, batch=torch.zeros(10, dtype=torch.int64))
        with pytest.raises(ValueError, match="ptr must end at 10"):
            f(F, P, k=64, ptr=torch.tensor([0, 4, 9]))
        with pytest.raises(ValueError, match="batch must be sorted"):
            f(F, P, k=64, batch=torch.tensor([0, 0, 1, 0, 1, 1, 1, 1, 1, 1]))
    for f in (m.simtopk_combined_fast_any_k, m.simtopk_combined_any_k):
        for cs in (-1, 3, 6):
            with pytest.raises(ValueError, match="col_splits must be 0 or a power of two"):
                f(F, P, k=64, col_splits=cs)
    # the multi-pass call takes device tensors only, like the other any-k 16-bit calls
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.simtopk_combined_fast_any_k(F, P, k=64)


def test_without_a_gpu_every_function_raises_the_packages_error(monkeypatch):
    m = _mod()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    F, P = torch.zeros(8, 16), torch.zeros(8, 2)
    for fn in (lambda: m.simtopk_combined_fast_any_k(F, P, k=60), lambda: m.simtopk_combined_fast_any_k(F, P, k=5, ptr=[0, 3, 8]),
               lambda: m.simtopk_combined_any_k(F, P, k=60), lambda: m.simtopk_combined_any_k(F, P, k=60, precision="fast"),
               lambda: m.simtopk_combined_any_k(F, P, k=5, ptr=[0, 3, 8], precision="exact"),
               lambda: m.build_topk_weighted_hypergraph_fast_any_k(F, P, k=60), lambda: m.build_topk_hypergraph_data_fast_any_k(F, P, k=60, precision="fast")):
        with pytest.raises(RuntimeError, match="ROCm"):
            fn()


# ---- the sources, read statically -----------------------------------------------------------------------------------------------------
def _body(text, name):
    return text.split("int " + name + "(", 1)[1].split("\n}\n", 1)[0]


def test_entry_and_driver_name_the_callers_stream_and_nothing_blocks():
    from test_stream_arguments_cpu import BLOCKING, BLOCKING_ALLOWED, is_null, sources, stream_uses
    src = dict(sources())
    raw = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")).read()
    entry = _body(raw, ENTRY)
    first_device = min(entry.index(c) for c in ("run_simtopk_combined(", "run_segmented_exact(", "run_simtopk_combined_fast(", "r.call.begin()"))
    assert entry.index(".on_device()") < entry.index("set_error(") and entry.rindex("set_error(") < first_device
    assert entry.index("check_pow2_splits(") < first_device and "k + self = " not in entry       # no refusal names a limit on k
    assert not [m for m in BLOCKING.finditer(entry) if not m.group(1).endswith("Async")] and "hipStream" not in entry
    driver = _body(src["mmf_api.hip"], "combined_fast_anyk_run")
    assert not [m for m in BLOCKING.finditer(driver) if not m.group(1).endswith("Async")] and "hipDeviceSynchronize" not in driver
    for call in ("launch_scan_b16c_seg(", "launch_scan_b16c_seg_ceil(", "launch_scan_b16c_ceilings(", "launch_rerank_combined(", "launch_rerank_combined_ext(",
                 "launch_anyk_count(", "launch_anyk_emit(", "launch_floor_rebase(", "upload_table(s,", "anyk_short_div()", "MMF_FAST_ANYK_MAX_PASSES - 1"):
        assert call in driver, call
    # the work table, the gather table and the segment offsets are uploaded once, before the pass loop
    loop = driver.split("for (int pass = 1;", 1)
    assert len(loop) == 2 and loop[0].count("upload_table(s, d_sched") == 1 and "upload_table(s, d_sched" not in loop[1]
    assert "MMF_DEBUG_FLAG_ROWS" in _body(raw, "combined_fast_anyk_run")
    for name in ("mmf_scan_b16c.hip", "mmf_topk_anyk.hip", "mmf_rerank_combined.h"):
        assert not [m for m in BLOCKING.finditer(src[name]) if not m.group(1).endswith("Async")], name
        assert not [u for u in stream_uses() if u[0] == name and is_null(u[3])], name
    ext = [u for u in stream_uses() if u[0] == "mmf_topk_anyk.hip"]
    assert sorted(a[0] for _, _, what, _, a in ext if what == "hipLaunchKernelGGL") == ["(rerank_combined_kernel<false, true, true>)",
                                                                                       "(rerank_combined_kernel<true, true, true>)"]
    assert all(u[3] == "s" for u in ext)
    assert not [k for k in BLOCKING_ALLOWED if "anyk" in k[1] or "topk_anyk" in k[0]]          # the allow-list was not extended


def test_the_ceiling_flag_sits_where_the_design_says():
    k = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_scan_b16c.hip")).read()
    assert "template <bool F16, int CAP, bool SEG, bool CEIL>" in k and "scan_b16c_body<F16, CAP, SEG, false>(a);" in k
    assert "scan_b16c_body<F16, C_CAP_BIG, true, true>(a);" in k
    args = k.split("struct ScanB16CArgs {", 1)[1].split("};", 1)[0]
    assert args.rstrip().splitlines()[-1].strip().startswith("const float* ceil;")            # the last member: no existing argument moves
    body = k.split("void scan_b16c_body(", 1)[1]
    ceil_at = body.index("if constexpr (CEIL)")
    # stage (ii): after the keys (with their padding select) are formed, before the second test and the list code
    assert body.index("else keys(std::integral_constant<int, 8>{});") < ceil_at < body.index("const float m0k =") < body.index("list.offer_tile(")
    assert body.count("a.ceil[") == 2 and body.index("a.ceil[") > ceil_at                       # loaded inside the branch that needs it
    assert "Ceilings (mmf_simtopk_combined_fast_anyk" in k and "h + 3.1 u' |h|" in k            # the derivation, in the header


# ---- documents ------------------------------------------------------------------------------------------------------------------------
def test_design_readme_integration_and_scripts_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design.split("## 4.33", 1)[1].split("\n## 5", 1)[0]
    for words in ("mmf_simtopk_combined_fast_anyk", "Ceiling", "ghost", "Resources", "ScratchSize", "Measured", "Not measured", "Cut",
                  "scan_b16c_ceil_kernel", "launch_rerank_combined_ext", "MMF_ANYK_SHORT_DIV", "bench.py"):
        assert words in sec, words
    assert "§4.33" in design.split("## 8", 1)[1]                                                # the follow-up item is struck
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "simtopk_combined_fast_any_k" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = re.split(r"^## [0-9. ]*16-bit combined any-k entries$", integ, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = dict((m.group(1), (m.group(2), m.group(3))) for m in re.finditer(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", section, flags=re.M))
    from test_gpu_simtopk_combined_fast_anyk import SYNC
    assert rows == SYNC == {ENTRY: ("data-dependent", "the call")}, rows
    assert os.path.exists(os.path.join(ROOT, "scripts", "simtopk_combined_fast_anyk_timing.py"))
    assert ENTRY in open(os.path.join(ROOT, "profiles", "simtopk_combined_fast_anyk_timing.txt")).read()


# ---- the restatement: the ceiling and the pass loop on the GPU tests' own inputs ------------------------------------------------------
def test_the_ceiling_in_numpy():
    f = np.float32
    fk = np.array([-np.inf, -1000.0, -1.0, 0.0, 1e-6, -3e-30], f)
    m0 = np.array([1e-3, 1e-3, 1e-5, 1e-30, 1e-7, 1e-30], f)
    c = ar.ceiling(fk, m0)
    assert np.isneginf(c[0]) and c.dtype == np.float32
    h = fk[1:].astype(np.float64) + 0.5 * m0[1:].astype(np.float64)
    bound = h + 3.1 * ar.UP * np.abs(h)                                   # the real-number bound of the derivation
    assert np.all(c[1:].astype(np.float64) >= bound) and np.all(c[1:] > fk[1:])
    assert np.all(c[1:].astype(np.float64) - fk[1:] <= 0.5 * m0[1:] + 8 * 2.0 ** -24 * np.abs(h) + 3e-45)      # no wider than stated
    assert ar.anyk_yield([0, 0, 3, 5, 100], 4, 7) == (3, 3) and ar.anyk_yield([1, 0], 2, 0) == (0, 0) and ar.anyk_yield([0, 0, 0], 2, 0) == (2, 0)


def _report(tag, recs):
    for p, r in enumerate(recs, 1):
        finite = r["excess"][np.isfinite(r["excess"])]
        print(f"{tag} pass {p}: done {r['done']} yield {r['yield']} short {r['short']} flagged {int(r['flagged'].sum())}; closest approach "
              f"of a column after the floor to its ceiling {finite.max() if finite.size else float('nan'):.3e}; ghosts max {int(r['ghosts'].max())} "
              f"mean {r['ghosts'].mean():.2f}, smallest ghost slack {r['ghost_slack'].min():.3e}; largest band {int(r['band'].max())}")


def _check_1_and_2(tag, recs):
    assert recs, tag
    for r in recs:
        assert float(r["excess"].max()) <= 0.0, f"{tag}: a column that ranks after the floor lies above its ceiling — the derivation is wrong"
        assert float(r["ghost_slack"].min()) >= 0.0, f"{tag}: a ghost's key lies further from the ceiling than e0 + 3 u' |A|"
        assert bool(r["prefix"].all()), f"{tag}: ghosts are no prefix of the re-ranked row"


@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(ar.CLEAN))
def test_clean_inputs_no_column_after_the_floor_exceeds_its_ceiling_and_no_band_outgrows_the_lists(name, operand):
    F, P = ar.clean_inputs(name)
    for exclude_self, k in ((True, 64), (False, 45)):
        recs = ar.passes(F, P, ar.LH, ar.LG, k, operand, exclude_self=exclude_self)
        _report(f"{name} {operand} self={exclude_self}", recs)
        _check_1_and_2(f"{name} {operand}", recs)
        for r in recs:                                                     # (3): no row is flagged by the scan, in any pass
            assert int(r["band"].max()) <= ar.LIST_CAP and not r["flagged"].any()
            assert not r["finished_exact"] and 1 <= r["yield"] <= 20 - exclude_self and r["short"] <= F.shape[0] // 64
        assert sum(r["yield"] for r in recs) + (20 - exclude_self) == k and 1 + len(recs) >= ar.plan(k, exclude_self)[2]


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_ghost_input_has_ghosts_in_pass_1(operand):
    F, P = ar.ghost_inputs()
    recs = ar.passes(F, P, ar.GHOST_LH, ar.GHOST_LG, 45, operand)
    _report(f"ghost {operand}", recs)
    _check_1_and_2(f"ghost {operand}", recs)
    # (4): a row the scan cannot flag (its band fits the lists) has a ghost in pass 1, and the pass still yields
    assert bool(((recs[0]["ghosts"] >= 1) & ~recs[0]["flagged"]).any()) and not recs[0]["finished_exact"] and recs[0]["yield"] >= 1


def test_ragged_batch_with_batch_wide_maxima():
    """The batch of the GPU test: the scale and the maxima are the batch's (a wider m0: sound), the order, the floor and the band a
    segment's own; the segments short of k admissible columns are not scanned."""
    F, P = ar.clean_inputs("n700")
    ptr = [0, 0, 1, 38, 166, 295, 700]
    for operand in ("f16", "bf16"):
        recs = ar.passes(F, P, ar.LH, ar.LG, 32, operand, ptr=ptr)
        _report(f"ragged {operand}", recs)
        _check_1_and_2(f"ragged {operand}", recs)
        assert len(recs[0]["excess"]) == 37 + 128 + 129 + 405              # the served rows: segments of at least 33 rows
        # the segment of 37 rows has 17 columns left after the first pass, fewer than a pass is deep: the re-rank flags those of
        # its rows that fewer than two ghosts fill up; no other row is flagged
        assert 30 <= int(recs[0]["flagged"].sum()) <= 37 and not recs[0]["flagged"][37:].any() and recs[0]["yield"] == 13


@pytest.mark.parametrize("d", [128, 500])
@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_worst_case_rounding_rows_stay_under_their_ceilings(operand, d):
    """(5): tests/adversarial16.py's worst-case rounding rows — every component of a column rounds the same way, so the error of a
    (q, A) and of a (q, B) pair each come close to the bound with opposite signs — with pixel positions added."""
    F, P, lh, q_rows = ar.adversarial_inputs(operand, d)
    recs = ar.passes(F, P, lh, ar.LG, 45, operand)
    _report(f"adversarial {operand} d={d}", recs)
    _check_1_and_2(f"adversarial {operand} d={d}", recs)
    q = [float(r["excess"][q_rows].max()) for r in recs]
    print(f"adversarial {operand} d={d}: the q rows' closest approach per pass {q}")
