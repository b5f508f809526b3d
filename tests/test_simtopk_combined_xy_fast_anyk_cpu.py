"""The 16-bit combined top-k for two node sets and any k without a GPU (mmf_simtopk_combined_xy_fast_anyk,
include/ext/mmf_hg_topk16_xy_anyk.h): the header and the export list, the entry's host checks in
mmf_simtopk_combined_xy's order and wording before any device call, every k reaching the device, the Python errors, the routers'
decisions with the calls replaced by recorders, the sharded driver's shard-size error, the sources read statically, the documents —
and the numpy restatement of the ceiling per query and of the pass loop (tests/combined_xy_anyk_restate.py) on the seeded inputs
tests/test_gpu_simtopk_combined_xy_fast_anyk.py runs."""
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
import combined16_anyk_restate as ar      # noqa: E402
import combined_xy_anyk_restate as xa     # noqa: E402
import combined_xy_restate as xr          # noqa: E402

ENTRY, OLD = "mmf_simtopk_combined_xy_fast_anyk", "mmf_simtopk_combined_xy"
WHO = "simtopk_combined_xy_fast_anyk"
HEADER = os.path.join(ROOT, "include", "ext", "mmf_hg_topk16_xy_anyk.h")


def _mod():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16_xy_anyk")


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    return m


# ---- header, library, binding ---------------------------------------------------------------------------------------------------------
def test_header_and_exports(mmf):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(mmf_\w+)\(", hdr, re.M))
    assert declared == set(mmf._lib.TOPK16_XY_ANYK_EXPORTS) == {ENTRY}
    assert '#include "mmf_hg_fast_anyk.h"' in hdr and "typedef struct" not in hdr          # the info struct is reused, not redeclared
    for name, v in vars(mmf._lib).items():                                                 # no other export list binds the name
        if name != "TOPK16_XY_ANYK_EXPORTS" and isinstance(v, list) and all(isinstance(e, str) for e in v):
            assert not set(v) & declared, name
    inc = os.path.join(ROOT, "include")
    for d in (inc, os.path.join(inc, "ext")):
        for h in os.listdir(d):
            if h.endswith(".h") and h != "mmf_hg_topk16_xy_anyk.h":
                assert ENTRY + "(" not in open(os.path.join(d, h)).read(), h
    L = mmf._lib.lib()
    assert L.mmf_simtopk_combined_xy_fast_anyk.restype is ctypes.c_int
    assert list(L.mmf_simtopk_combined_xy_fast_anyk.argtypes) == list(L.mmf_simtopk_combined_xy.argtypes) + [ctypes.POINTER(mmf._lib.FastAnykInfo)]
    assert len(L.mmf_simtopk_combined_xy_fast_anyk.argtypes) == 21
    assert mmf._lib.ABI_VERSION == 3 and L.mmf_version() == 3                               # an addition
    for words in ("bit for bit", "MMF_PREC_FAST_BF16", "MMF_ANYK_SHORT_DIV", "MMF_DEBUG_FLAG_ROWS", "Host-synchronous", "Workspace",
                  "TOPK16_XY_ANYK_EXPORTS", "k + self <= 20", "or a power of two", "row slice", "union", "mmf_combined_fast_anyk_plan",
                  "uploaded once", "served exactly"):
        assert words in hdr, words
    assert "k + self = " not in hdr                                                         # no limit on k
    build = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py")).read()
    assert "mmf_hg_topk16_xy_anyk.h" in build
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_topk16_xy_anyk", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("ext", "mmf_hg_topk16_xy_anyk.h")) for h in b.HEADERS) and all(os.path.exists(h) for h in b.HEADERS if os.path.isabs(h))
    assert "mmf_scan_b16c.hip" not in b.EXTRA_FLAGS and "mmf_api.hip" not in b.EXTRA_FLAGS
    assert '#include "../../include/ext/mmf_hg_topk16_xy_anyk.h"' in open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_host.h")).read()


def test_python_signatures(mmf):
    m = _mod()
    assert mmf.combined_topk16_xy_anyk is m and "combined_topk16_xy_anyk" in mmf.__all__ and "mmf.combined_topk16_xy_anyk.*" in mmf.__doc__
    for name in ("simtopk_combined_xy_fast_any_k", "simtopk_combined_rows_fast_any_k"):
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
    # the routers carry the names of combined_topk_anyk's calls, which keep the package-level names
    assert mmf.simtopk_combined_xy_any_k is mmf.combined_topk_anyk.simtopk_combined_xy_any_k is not m.simtopk_combined_xy_any_k
    assert mmf.simtopk_combined_rows_any_k is mmf.combined_topk_anyk.simtopk_combined_rows_any_k is not m.simtopk_combined_rows_any_k
    sig = inspect.signature(m.simtopk_combined_xy_fast_any_k)
    assert list(sig.parameters) == ["q_features", "q_positions", "c_features", "c_positions", "lambda_h", "lambda_g", "k", "exclude_self",
                                    "row_offset", "col_offset", "precision", "col_splits", "return_stats", "return_info", "profile"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[7:])
    assert [sig.parameters[n].default for n in list(sig.parameters)[4:]] == [1.0, 1.0, 5, False, 0, 0, "fast", 0, False, False, False]
    rows = inspect.signature(m.simtopk_combined_rows_fast_any_k)
    assert list(rows.parameters)[:4] == ["features", "positions", "lo", "hi"] and rows.parameters["exclude_self"].default is True
    assert rows.parameters["precision"].default == "fast" and "return_info" in rows.parameters
    for router, old in ((m.simtopk_combined_xy_any_k, mmf.combined_topk_anyk.simtopk_combined_xy_any_k),
                        (m.simtopk_combined_rows_any_k, mmf.combined_topk_anyk.simtopk_combined_rows_any_k)):
        rsig = inspect.signature(router)
        assert [n for n in rsig.parameters if n != "precision"] == list(inspect.signature(old).parameters)
        assert rsig.parameters["precision"].default == "auto" and rsig.parameters["precision"].kind is inspect.Parameter.KEYWORD_ONLY
    from multimodal_fusion_amd import distributed
    sig = inspect.signature(distributed.sharded_simtopk_combined_fast_any_k)
    assert list(sig.parameters) == ["f_local", "p_local", "n_total", "lambda_h", "lambda_g", "k", "exclude_self", "precision", "group",
                                    "gather_output", "return_stats"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[3:]] == [1.0, 1.0, 5, True, "fast", None, False, False]
    # the exact sharded driver keeps its parameter list and its body's call
    old = inspect.signature(distributed.sharded_simtopk_combined_any_k)
    assert list(old.parameters) == ["f_local", "p_local", "n_total", "lambda_h", "lambda_g", "k", "exclude_self", "group", "gather_output", "return_stats"]
    assert "combined_topk_anyk.simtopk_combined_rows_any_k(" in inspect.getsource(distributed.sharded_simtopk_combined_any_k)
    assert "combined_topk16_xy_anyk.simtopk_combined_rows_fast_any_k(" in inspect.getsource(distributed.sharded_simtopk_combined_fast_any_k)


# ---- the entry's host checks, with host buffers standing in for device pointers -------------------------------------------------------
def _call(fn=ENTRY, **kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(Fq=b, Pq=b, nq=4, Fc=b, Pc=b, nc=6, d=4, dp=2, lh=1.0, lg=1.0, k=2, self=1, ro=0, co=0, idx=b, val=b, opts=(2, 0, 0, 0, None),
             device=63, info=True)
    a.update(kw)
    opts = a["opts"]
    if opts is not None:
        opts = ctypes.byref(mmf._lib.SimtopkOpts(*opts))
    args = [a["Fq"], a["Pq"], a["nq"], a["Fc"], a["Pc"], a["nc"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], a["ro"], a["co"], a["idx"],
            a["val"], opts, None, a["device"], None]
    if fn == ENTRY:
        args.append(ctypes.byref(mmf._lib.FastAnykInfo()) if a["info"] else None)
    rc = getattr(L, fn)(*args)
    return rc, L.mmf_last_error().decode()


# every refusal the new entry shares with mmf_simtopk_combined_xy: (arguments, words); compared message by message below
SHARED_INVALID = [
    (dict(nq=-1), "nq must be >= 0 (got -1)"),
    (dict(nc=-1), "nc must be >= 0 (got -1)"),
    (dict(d=0), "d must be at least 1 (got 0)"),
    (dict(dp=0), "dp must be at least 1 (got 0)"),
    (dict(k=0), "k must be at least 1 (got 0)"),
    (dict(ro=-1), "row_offset must be >= 0 (got -1)"),
    (dict(co=-5), "col_offset must be >= 0 (got -5)"),
    (dict(lh=-0.5), "lambda_h must be finite and >= 0"),
    (dict(lh=float("inf")), "lambda_h must be finite and >= 0"),
    (dict(lg=-1.0), "lambda_g must be finite and >= 0"),
    (dict(lg=float("nan")), "lambda_g must be finite and >= 0"),
    (dict(Fq=None), "Fq is NULL"),
    (dict(Pq=None), "Pq is NULL"),
    (dict(Fc=None), "Fc is NULL"),
    (dict(Pc=None), "Pc is NULL"),
    (dict(idx=None), "out_idx is NULL"),
    (dict(val=None), "out_val is NULL"),
    (dict(opts=(7, 0, 0, 0, None)), "precision 7: MMF_PREC_AUTO, _EXACT, _FAST (f16 operands) or _FAST_BF16"),
]
OWN_INVALID = [           # col_splits as the any-k 16-bit entries check it
    (dict(opts=(2, 0, -1, 0, None)), "col_splits must be 0 or a power of two (got -1)"),
    (dict(opts=(2, 0, 3, 0, None)), "col_splits must be 0 or a power of two (got 3)"),
    (dict(opts=(1, 0, 6, 0, None)), "col_splits must be 0 or a power of two (got 6)"),
]
SHARED_UNSUPPORTED = [
    (dict(dp=9), "dp = 9 > 8 is not supported"),
    (dict(d=4097), "d = 4097 > 4096 is not supported (MMF_PREC_EXACT takes any d)"),
    (dict(d=4097, opts=(3, 0, 0, 0, None)), "d = 4097 > 4096 is not supported (MMF_PREC_EXACT takes any d)"),
    (dict(nq=1 << 31), "row_offset + nq must be < 2^31"),
    (dict(ro=(1 << 31) - 4), "row_offset + nq must be < 2^31"),
    (dict(nc=1 << 31), "col_offset + nc must be < 2^31"),
    (dict(co=(1 << 31) - 6), "col_offset + nc must be < 2^31"),
]
OWN_UNSUPPORTED = [       # AUTO means FAST here, so it meets the 16-bit scan's limit on d; with k beyond one pass as well
    (dict(d=4097, opts=None), "d = 4097 > 4096 is not supported"),
    (dict(d=4097, opts=(0, 0, 0, 0, None), k=64), "d = 4097 > 4096 is not supported"),
]


@pytest.mark.parametrize("kw,words", SHARED_INVALID + OWN_INVALID)
def test_entry_refuses_bad_arguments_before_any_device_call(mmf, kw, words):
    """A device id that does not exist: an argument error must win over the device's."""
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and msg.startswith(WHO + ":"), (rc, msg)


@pytest.mark.parametrize("kw,words", SHARED_UNSUPPORTED + OWN_UNSUPPORTED)
def test_entry_refuses_what_it_does_not_support_before_any_device_call(mmf, kw, words):
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and words in msg and msg.startswith(WHO + ":"), (rc, msg)


@pytest.mark.parametrize("kw,words", SHARED_INVALID + SHARED_UNSUPPORTED)
def test_every_shared_refusal_is_the_one_pass_entrys_under_the_new_name(mmf, kw, words):
    rc_o, msg_o = _call(OLD, **kw)
    rc_n, msg_n = _call(**kw)
    assert rc_o == rc_n and rc_n < 0 and msg_n == msg_o.replace(OLD[4:], WHO, 1), (kw, msg_o, msg_n)


def test_the_order_of_the_checks(mmf):
    """mmf_simtopk_combined_xy's: the device first, then every MMF_E_INVALID (shapes, offsets, lambdas, pointers, precision,
    col_splits — in that order), then every MMF_E_UNSUPPORTED (dp, the 16-bit limit on d, the id ranges) — no k + self refusal."""
    inv, uns = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    for kw in (dict(), dict(k=0), dict(Fq=None), dict(dp=9), dict(nq=-1), dict(d=4097), dict(k=64)):
        rc, msg = _call(device=-1, **kw)
        assert rc == uns and "no CPU path" in msg and msg.startswith(WHO + ":"), (rc, msg)
    chain = [(dict(nq=-1), "nq must"), (dict(nc=-1), "nc must"), (dict(d=0), "d must"), (dict(dp=0), "dp must"), (dict(k=0), "k must"),
             (dict(ro=-1), "row_offset must"), (dict(co=-1), "col_offset must"), (dict(lh=-1.0), "lambda_h"), (dict(lg=-1.0), "lambda_g"),
             (dict(Fq=None), "Fq is NULL"), (dict(Pq=None), "Pq is NULL"), (dict(Fc=None), "Fc is NULL"), (dict(Pc=None), "Pc is NULL"),
             (dict(idx=None), "out_idx"), (dict(val=None), "out_val"), (dict(opts=(7, 0, 3, 0, None)), "precision 7"),
             (dict(opts=(2, 0, 3, 0, None)), "col_splits"), (dict(dp=9), "dp = 9 > 8"), (dict(d=4097), "d = 4097 > 4096"),
             (dict(ro=1 << 31), "row_offset + nq"), (dict(co=1 << 31), "col_offset + nc")]
    for i, (_, words) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):           # this mistake and every later one at once: this one is reported
            kw.update(later)
        rc, msg = _call(**kw)
        assert words in msg and rc == (inv if i < 17 else uns), (i, words, rc, msg)


@pytest.mark.parametrize("k", [1, 18, 19, 20, 21, 38, 39, 43, 44, 45, 64, 200])
def test_every_k_reaches_the_device(mmf, k):
    """No refusal on either side of the one-pass boundary or of the exact lists' 44, with and without self, every precision: the
    call gets as far as the device (which is not there)."""
    for kw in (dict(), dict(self=0), dict(opts=None), dict(opts=(0, 0, 0, 0, None)), dict(opts=(1, 0, 0, 0, None)), dict(opts=(3, 1, 4, 0, None)),
               dict(lh=0.0, lg=0.0), dict(dp=8, d=4096), dict(d=5000, opts=(1, 0, 0, 0, None)), dict(info=False), dict(opts=(2, 0, 32, 0, None)),
               dict(nq=300, nc=500), dict(ro=100, co=(1 << 31) - 7), dict(nc=0, Fc=None, Pc=None)):
        rc, msg = _call(k=k, **kw)
        assert rc == mmf._lib.MMF_E_HIP, (k, kw, rc, msg)


def test_no_queries_are_a_no_op_and_the_siblings_keep_their_refusals(mmf):
    assert _call(nq=0)[0] == mmf._lib.MMF_OK
    assert _call(nq=0, k=64, Fq=None, Pq=None, Fc=None, Pc=None, idx=None, val=None)[0] == mmf._lib.MMF_OK
    uns = mmf._lib.MMF_E_UNSUPPORTED
    rc, msg = _call(OLD, k=20)
    assert rc == uns and msg == "simtopk_combined_xy: k + self = 21 > 20 is not supported (MMF_PREC_EXACT takes up to 44)", msg
    rc, msg = _call(OLD, k=44, opts=(1, 0, 0, 0, None))
    assert rc == uns and "k + self = 45 > 44" in msg
    rc, msg = _call("mmf_simtopk_combined_xy_anyk", k=64)
    assert rc == uns and "the 16-bit combined scans stop at k + self = 20" in msg


# ---- the Python layer's argument errors, on the host ----------------------------------------------------------------------------------
def test_wrappers_reject_bad_input_before_any_library_call(mmf, monkeypatch):
    m = _mod()

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    G, Q = torch.randn(6, 8), torch.zeros(6, 2)
    for f in (m.simtopk_combined_xy_fast_any_k, m.simtopk_combined_xy_any_k):
        with pytest.raises(ValueError, match="must share Nq"):
            f(G, Q[:5], F, P, k=64)
        with pytest.raises(ValueError, match="must share Nc"):
            f(G, Q, F, P[:9], k=64)
        with pytest.raises(ValueError, match="must share D and dp"):
            f(G[:, :7], Q, F, P, k=64)
        with pytest.raises(ValueError, match=r"k must be >= 1 \(got 0\)"):
            f(G, Q, F, P, k=0)
        with pytest.raises(ValueError, match="unknown precision 'half'"):
            f(G, Q, F, P, k=64, precision="half")
        with pytest.raises(ValueError, match="col_splits must be >= 0"):
            f(G, Q, F, P, k=64, col_splits=-1)
        with pytest.raises(ValueError, match="row_offset and col_offset must be >= 0"):
            f(G, Q, F, P, k=64, row_offset=-1)
    for r in (m.simtopk_combined_rows_fast_any_k, m.simtopk_combined_rows_any_k):
        with pytest.raises(ValueError, match="must share N"):
            r(F, P[:9], 0, 4, k=64)
        for lo, hi in ((-1, 4), (5, 4), (0, 11)):
            with pytest.raises(ValueError, match="are no range of the 10 rows"):
                r(F, P, lo, hi, k=64)
        with pytest.raises(ValueError, match="unknown precision"):
            r(F, P, 0, 4, k=64, precision="f16")
    for cs in (3, 6):                                 # the 16-bit calls: 0 or a power of two, as the entry
        with pytest.raises(ValueError, match="col_splits must be 0 or a power of two"):
            m.simtopk_combined_xy_fast_any_k(G, Q, F, P, k=64, col_splits=cs)
        with pytest.raises(ValueError, match="col_splits must be 0 or a power of two"):
            m.simtopk_combined_rows_fast_any_k(F, P, 0, 4, k=64, col_splits=cs)
    # the multi-pass calls take device tensors only, like the other any-k 16-bit calls
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.simtopk_combined_xy_fast_any_k(G, Q, F, P, k=64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.simtopk_combined_rows_fast_any_k(F, P, 0, 4, k=64)


def test_without_a_gpu_every_function_raises_the_packages_error(monkeypatch):
    m = _mod()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    F, P = torch.zeros(80, 16), torch.zeros(80, 2)
    for fn in (lambda: m.simtopk_combined_xy_fast_any_k(F[:4], P[:4], F, P, k=60), lambda: m.simtopk_combined_rows_fast_any_k(F, P, 2, 6, k=60),
               lambda: m.simtopk_combined_xy_any_k(F[:4], P[:4], F, P, k=60), lambda: m.simtopk_combined_xy_any_k(F[:4], P[:4], F, P, k=60, precision="fast"),
               lambda: m.simtopk_combined_rows_any_k(F, P, 2, 6, k=60, precision="fast_bf16"), lambda: m.simtopk_combined_rows_any_k(F, P, 2, 6, k=60, precision="exact")):
        with pytest.raises(RuntimeError, match="ROCm"):
            fn()


def test_sharded_driver_checks_its_shard(mmf):
    from multimodal_fusion_amd.distributed import sharded_simtopk_combined_fast_any_k
    with pytest.raises(ValueError, match=r"rank 0: shards have 9 / 10 rows, expected 10"):
        sharded_simtopk_combined_fast_any_k(torch.zeros(9, 8), torch.zeros(10, 2), 10, k=45)
    with pytest.raises(ValueError, match=r"rank 0: shards have 10 / 10 rows, expected 12"):
        sharded_simtopk_combined_fast_any_k(torch.zeros(10, 8), torch.zeros(10, 2), 12, k=45)


# ---- the routers ------------------------------------------------------------------------------------------------------------------------
def test_the_routers_decisions(mmf):
    m = _mod()
    for prec in ("fast", "fast_bf16"):
        for k in (5, 19, 20, 64):
            assert m.xy_anyk_route(8192, 65536, 512, k, True, prec) == "fast"
    for k in (5, 19, 20, 64, 200):
        assert m.xy_anyk_route(8192, 65536, 512, k, True, "exact") == "exact"
    # "auto": the f16 call only on the measured classes of _AUTO_SHAPES, never where one pass serves, never beyond d = 4096
    assert m._AUTO_SHAPES == () or os.path.exists(os.path.join(ROOT, "profiles", "simtopk_combined_xy_fast_anyk_timing.txt"))
    for dl, dh, kl, kh, ql, cl in m._AUTO_SHAPES:
        assert 1 <= dl <= dh <= 4096 and 20 <= kl <= kh and ql >= 1 and cl > kh
        assert m.xy_anyk_route(ql, cl, dl, kh, True, "auto") == "fast" and m.xy_anyk_route(ql, cl, dh, kl + 1, False, "auto") == "fast"
    # the measured shapes of profiles/simtopk_combined_xy_fast_anyk_timing.txt, and what lies outside them
    for nq, nc, d, k, ex, want in ((8192, 65536, 512, 32, True, "fast"), (8192, 65536, 512, 64, True, "fast"), (32768, 262144, 512, 32, True, "fast"),
                                   (32768, 262144, 512, 64, True, "fast"), (16384, 65536, 512, 32, False, "fast"), (16384, 65536, 1536, 64, False, "fast"),
                                   (8192, 65536, 1536, 32, True, "fast"), (8192, 65536, 1024, 45, True, "fast"),
                                   (4096, 65536, 512, 32, True, "exact"), (8192, 32768, 512, 32, True, "exact"), (8192, 65536, 256, 32, True, "exact"),
                                   (8192, 65536, 2048, 32, True, "exact"), (8192, 65536, 512, 128, True, "exact"), (130, 260, 40, 45, True, "exact")):
        assert m.xy_anyk_route(nq, nc, d, k, ex, "auto") == want, (nq, nc, d, k)
    for k in (1, 5, 19):
        assert m.xy_anyk_route(1 << 20, 1 << 20, 1536, k, True, "auto") == "exact"                  # one pass: the existing routes decide
    assert m.xy_anyk_route(1 << 20, 1 << 20, 1536, 20, False, "auto") == "exact"
    assert m.xy_anyk_route(1 << 20, 1 << 20, 5000, 64, True, "auto") == "exact"
    with pytest.raises(ValueError, match="unknown precision"):
        m.xy_anyk_route(100, 100, 40, 5, True, "fastest")
    with pytest.raises(ValueError, match="k must be >= 1"):
        m.xy_anyk_route(100, 100, 40, 0, True)


class _Shape:
    """A stand-in for a tensor of a measured size: the routers look at shapes before they hand anything on."""
    def __init__(self, n, d):
        self.shape, self.device = (n, d), torch.device("cpu")

    def dim(self):
        return 2

    def __getitem__(self, s):
        lo, hi, _ = s.indices(self.shape[0])
        return _Shape(max(hi - lo, 0), self.shape[1])


@pytest.mark.parametrize("nq,nc,d,k,precision,want", [
    (8192, 65536, 512, 32, "auto", "fast:fast"), (8192, 65536, 512, 32, "exact", "exact"), (8192, 65536, 512, 32, "fast", "fast:fast"),
    (8192, 65536, 512, 32, "fast_bf16", "fast:fast_bf16"), (16384, 65536, 1536, 64, "auto", "fast:fast"), (32768, 262144, 512, 64, "auto", "fast:fast"),
    (130, 260, 40, 45, "auto", "exact"), (130, 260, 40, 45, "fast", "fast:fast"), (8192, 65536, 512, 19, "auto", "exact"),
    (8192, 65536, 2048, 32, "auto", "exact"), (8192, 65536, 4200, 32, "auto", "exact"), (8192, 65536, 512, 128, "auto", "exact"),
    (4096, 65536, 512, 32, "auto", "exact"), (8192, 65536, 512, 32, "fast_bf16", "fast:fast_bf16")])
def test_the_routers_call_what_the_route_says(mmf, monkeypatch, nq, nc, d, k, precision, want):
    """Both routers with the calls replaced by recorders: which one is called, and at which precision."""
    m = _mod()
    seen = []
    monkeypatch.setattr(m, "compute_device", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(m, "to_gpu", lambda t, dev: t)
    out = (torch.zeros(1), torch.zeros(1))
    monkeypatch.setattr(m, "simtopk_combined_xy_fast_any_k", lambda *a, **kw: seen.append("fast:" + kw["precision"]) or out)
    monkeypatch.setattr(m, "simtopk_combined_rows_fast_any_k", lambda *a, **kw: seen.append("fast:" + kw["precision"]) or out)
    monkeypatch.setattr(m.combined_topk_anyk, "simtopk_combined_xy_any_k", lambda *a, **kw: seen.append("exact") or out)
    monkeypatch.setattr(m.combined_topk_anyk, "simtopk_combined_rows_any_k", lambda *a, **kw: seen.append("exact") or out)
    m.simtopk_combined_xy_any_k(_Shape(nq, d), _Shape(nq, 2), _Shape(nc, d), _Shape(nc, 2), 0.5, 2e-7, k, exclude_self=True, precision=precision)
    m.simtopk_combined_rows_any_k(_Shape(nc, d), _Shape(nc, 2), 100, 100 + nq, 0.5, 2e-7, k, precision=precision)
    assert seen == [want, want], seen


# ---- the sources, read statically -----------------------------------------------------------------------------------------------------
def _body(text, name):
    return text.split("int " + name + "(", 1)[1].split("\n}\n", 1)[0]


def _offset(text, line):
    return sum(len(x) + 1 for x in text.split("\n")[:line - 1])


def test_entry_driver_and_launchers_name_the_callers_stream_and_nothing_blocks():
    from test_stream_arguments_cpu import BLOCKING, BLOCKING_ALLOWED, enclosing, is_null, sources, stream_uses
    src = dict(sources())
    raw = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")).read()
    entry = _body(raw, ENTRY)
    first_device = min(entry.index(c) for c in ("run_simtopk_combined_xy(", "r.call.begin()"))
    assert entry.index(".on_device()") < entry.index("set_error(") and entry.rindex("set_error(") < first_device
    assert entry.index("check_pow2_splits(") < first_device and "k + self = " not in entry       # no refusal names a limit on k
    assert not [m for m in BLOCKING.finditer(entry) if not m.group(1).endswith("Async")] and "hipStream" not in entry
    driver = _body(src["mmf_api.hip"], "combined_xy_fast_anyk_run")
    assert not [m for m in BLOCKING.finditer(driver) if not m.group(1).endswith("Async")] and "hipDeviceSynchronize" not in driver
    for call in ("launch_scan_b16c_xy(", "launch_scan_b16c_xy_ceil(", "launch_scan_b16c_xy_ceilings(", "launch_rerank_combined(", "launch_rerank_combined_ext(",
                 "launch_anyk_count(", "launch_anyk_emit(", "launch_anyk_iota(", "launch_scan_b16_audit(", "upload_table(s,", "anyk_short_div()",
                 "MMF_FAST_ANYK_MAX_PASSES - 1", "reset_b16_lists("):
        assert call in driver, call
    api = src["mmf_api.hip"]
    mine = [u for u in stream_uses() if u[0] == "mmf_api.hip" and enclosing(api, _offset(api, u[1])) == "combined_xy_fast_anyk_run"]
    assert mine and all(u[3] == "s" for u in mine) and not [u for u in mine if is_null(u[3])], mine
    # the work table and the identity table go to the device once, before the pass loop
    loop = driver.split("for (int pass = 1;", 1)
    assert len(loop) == 2 and loop[0].count("upload_table(s, d_sched") == 1 and "upload_table(s, d_sched" not in loop[1]
    assert loop[0].count("launch_anyk_iota(") == 1 and "launch_anyk_iota(" not in loop[1]
    assert "MMF_DEBUG_FLAG_ROWS" in _body(raw, "combined_xy_fast_anyk_run")
    # the new launchers: the ceiling kernel and the seed union / the ceilings kernel, on the stream they were given
    text = src["mmf_scan_b16c.hip"]
    for fn, kernels in (("launch_scan_b16c_xy_ceil", ["kern", "comb_seed_union_kernel"]), ("launch_scan_b16c_xy_ceilings", ["comb_ceil_kernel"])):
        mine = [u for u in stream_uses() if u[0] == "mmf_scan_b16c.hip" and enclosing(text, _offset(text, u[1])) == fn]
        assert [a[0] for _, _, what, _, a in mine if what == "hipLaunchKernelGGL"] == kernels, (fn, mine)
        assert all(u[3] == "s" for u in mine)
    launcher = _body(text, "launch_scan_b16c_xy_ceil")
    assert "scan_b16c_ceil_kernel<true> : scan_b16c_ceil_kernel<false>" in launcher and "a.ceil = ceil - list_row0;" in launcher
    assert "a.seed = pn.seed - list_row0;" in launcher
    # no new kernel, no new instantiation: the two templates and their instantiations are what they were
    assert text.count("__global__") == 4 and text.count("scan_b16c_body<") == 2
    assert not [m for m in BLOCKING.finditer(text) if not m.group(1).endswith("Async")]
    assert not [k for k in BLOCKING_ALLOWED if "xy" in k[1] or "anyk" in k[1]]                    # the allow-list was not extended


# ---- documents ------------------------------------------------------------------------------------------------------------------------
def test_design_readme_integration_and_scripts_name_the_feature(mmf):
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design.split("## 4.34", 1)[1].split("\n## 5", 1)[0]
    for words in (ENTRY, "Ceiling", "union", "ghost", "Resources", "Measured", "Not measured", "Cut", "launch_scan_b16c_xy_ceil",
                  "launch_scan_b16c_xy_ceilings", "launch_rerank_combined_ext", "MMF_ANYK_SHORT_DIV", "bench.py", "sharded_simtopk_combined_fast_any_k",
                  "function by function"):
        assert words in sec, words
    assert "§4.34" in design.split("## 4.33", 1)[1].split("## 4.34", 1)[0]                      # §4.33's cut list points here
    assert "§4.34" in design.split("## 8", 1)[1]                                                # the follow-up item is updated
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "simtopk_combined_xy_fast_any_k" in readme and "sharded_simtopk_combined_fast_any_k" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = re.split(r"^## [0-9. ]*16-bit two-set any-k entries$", integ, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = dict((m.group(1), (m.group(2), m.group(3))) for m in re.finditer(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", section, flags=re.M))
    from test_gpu_simtopk_combined_xy_fast_anyk import SYNC
    assert rows == SYNC == {ENTRY: ("data-dependent", "no host arguments")}, rows
    assert set(rows) == set(mmf._lib.TOPK16_XY_ANYK_EXPORTS)
    for script in ("simtopk_combined_xy_fast_anyk_timing.py", "shard_combined_fast_any_k.py"):
        assert os.path.exists(os.path.join(ROOT, "scripts", script)), script
    prof = open(os.path.join(ROOT, "profiles", "simtopk_combined_xy_fast_anyk_timing.txt")).read()
    assert ENTRY in prof and prof.count("have B's bits: True") == 10 and "have B's bits: False" not in prof


# ---- the restatement: the ceiling per query and the pass loop on the GPU tests' own inputs ----------------------------------------------
def _report(tag, recs):
    for p, r in enumerate(recs, 1):
        finite = r["excess"][np.isfinite(r["excess"])]
        print(f"{tag} pass {p}: done {r['done']} yield {r['yield']} short {r['short']} flagged {int(r['flagged'].sum())}; closest approach "
              f"of a candidate after the floor to its ceiling {finite.max() if finite.size else float('nan'):.3e}; ghosts max {int(r['ghosts'].max())} "
              f"mean {r['ghosts'].mean():.2f}, smallest ghost slack {r['ghost_slack'].min():.3e}; largest band {int(r['band'].max())}")


def _check_1_and_2(tag, recs):
    assert recs, tag
    for r in recs:
        assert float(r["excess"].max()) <= 0.0, f"{tag}: a candidate that ranks after the floor lies above its ceiling — the argument is wrong"
        assert float(r["ghost_slack"].min()) >= 0.0, f"{tag}: a ghost's key lies further from the ceiling than e0 + 3 u' |A|"
        assert bool(r["prefix"].all()), f"{tag}: ghosts are no prefix of the staged row"


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_clean_input_no_candidate_after_the_floor_exceeds_its_ceiling_and_no_band_outgrows_the_lists(operand):
    """R1, what the GPU test's clean assertions depend on: in every pass, for both self modes, no band under a ceiling holds more than
    32 columns, so the scan flags no query; at most nq // 64 fall short of a pass's yield."""
    (F, P), q, c = xa.clean_case()
    nq = q[1] - q[0]
    for exclude_self, k in ((True, 64), (False, 64), (True, 45)):
        recs = xa.passes(F, P, q, c, xa.LH, xa.LG, k, operand, exclude_self=exclude_self)
        _report(f"R1 {operand} self={exclude_self} k={k}", recs)
        _check_1_and_2(f"R1 {operand}", recs)
        for r in recs:
            assert int(r["band"].max()) <= xa.LIST_CAP and not r["flagged"].any()
            assert not r["finished_exact"] and 1 <= r["yield"] <= 20 - exclude_self and r["short"] <= nq // 64
        assert sum(r["yield"] for r in recs) + (20 - exclude_self) == k and 1 + len(recs) >= ar.plan(k, exclude_self)[2]


@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("name,exclude_self", [("R2", True), ("R2", False), ("R5", True), ("R6", False)])
def test_the_other_cases_stay_under_their_ceilings(name, exclude_self, operand):
    """The identity mid-range, the slice (the union is the candidates: the self call's m0) and d = 1536."""
    case = {c.name: c for c in xr.CASES}[name]
    F, P = xr.case_data(case)
    recs = xa.passes(F, P, case.q, case.c, xa.LH, xa.LG, 45, operand, exclude_self=exclude_self)
    _report(f"{name} {operand} self={exclude_self}", recs)
    _check_1_and_2(f"{name} {operand}", recs)
    assert sum(r["yield"] for r in recs) + (20 - exclude_self) == 45


def test_a_slice_of_everything_is_the_one_graph_restatement():
    """Queries = candidates = all rows: the union is the set itself, and the passes are combined16_anyk_restate's."""
    F, P = ar.clean_inputs("n300")
    mine = xa.passes(F, P, (0, 300), (0, 300), ar.LH, ar.LG, 45, "f16", exclude_self=True)
    theirs = ar.passes(F, P, ar.LH, ar.LG, 45, "f16")
    assert len(mine) == len(theirs)
    for a, b in zip(mine, theirs):
        assert a["yield"] == b["yield"] and a["short"] == b["short"] and a["done"] == b["done"]
        for name in ("excess", "ghosts", "band", "flagged", "prefix"):
            assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_ghost_input_has_ghosts_in_pass_1(operand):
    (F, P), q, c = xa.ghost_case()
    recs = xa.passes(F, P, q, c, ar.GHOST_LH, ar.GHOST_LG, 45, operand, exclude_self=True)
    _report(f"ghost {operand}", recs)
    _check_1_and_2(f"ghost {operand}", recs)
    # a query the scan cannot flag (its band fits the lists) has a ghost in pass 1, and the pass still yields
    assert bool(((recs[0]["ghosts"] >= 1) & ~recs[0]["flagged"]).any()) and not recs[0]["finished_exact"] and recs[0]["yield"] >= 1


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_tie_input_ties_across_the_first_floor(operand):
    F, P = xa.tie_inputs()
    (_, _), q, c = xa.clean_case()
    ridx, rval = xr.reference(F, P, q, c, 45, xa.LH, xa.LG)
    for r in xa.TIE_QUERIES:
        assert sorted(ridx[r, :15]) == list(xa.TIE_NEAR) and np.array_equal(ridx[r, 15:45], xa.TIE_GROUP)
    _, key, _ = xa.setup(F, P, q, c, xa.LH, xa.LG, operand)
    tie = key[0, xa.TIE_GROUP - c[0]]
    assert np.all(tie == tie[0]) and tie[0] < key[0, xa.TIE_NEAR - c[0]].min()
    recs = xa.passes(F, P, q, c, xa.LH, xa.LG, 64, operand)
    _report(f"ties {operand}", recs)
    _check_1_and_2(f"ties {operand}", recs)


def test_the_yield_rule_and_the_plan():
    assert ar.anyk_yield([0, 0, 3, 5, 100], 4, 7) == (3, 3) and ar.anyk_yield([1, 0], 2, 0) == (0, 0) and ar.anyk_yield([0, 0, 0], 2, 0) == (2, 0)
    import multimodal_fusion_amd as mmf
    for k in (19, 20, 21, 45, 64):
        for ex in (False, True):
            p = mmf.combined_fast_anyk_plan(512, k, ex)                   # the plan query of §4.33 answers for this entry too
            assert (p["scan_kk"], p["first_yield"], p["min_passes"]) == ar.plan(k, ex)
