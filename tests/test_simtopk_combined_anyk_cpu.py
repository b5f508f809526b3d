"""The combined top-k for any k without a GPU (include/ext/mmf_hg_topk_anyk.h): the header declares exactly the
two entries and names the contract, the library exports them and the binding registers them in a list of its own, every refusal of
both entries comes before a device call under the new names while k of any size gets as far as the missing device, the existing
entries still refuse k + self = 45 with their words, the routing rule and the Python argument errors are host functions, the
documents name the feature, and the static stream scan finds every launch of mmf_topk.hip on the caller's stream."""
import ctypes
import inspect
import os
import re
import sys
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_simtopk_combined_anyk", "mmf_simtopk_combined_xy_anyk"]
HEADER = os.path.join("ext", "mmf_hg_topk_anyk.h")
OTHER_LISTS = ["EXPORTS", "EXPORTS_COHORT", "EXPORTS_POOL", "EXPORTS_STREAM", "EXPORTS_TOPK", "EXPORTS_WIDE", "EXPORTS_WIDE_SEG",
               "EXPORTS_TOPK16", "EXPORTS_TOPK16_SEG", "EXPORTS_TOPK_XY", "EXPORTS_SEG_EXACT", "EXPORTS_KMEANS_RAGGED"]
INVALID, UNSUPPORTED = -1, -2


def _mmf():
    import multimodal_fusion_amd as m
    return m


def _ak():
    _mmf()
    return import_module("multimodal_fusion_amd.combined_topk_anyk")


def _declared(path):
    with open(os.path.join(ROOT, "include", path)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding, build ---------------------------------------------------------------------------------------
def test_header_declares_exactly_the_entries_and_names_the_contract():
    assert _declared(HEADER) == set(ENTRIES)
    inc = os.path.join(ROOT, "include")
    for base, _, files in os.walk(inc):
        for f in files:
            rel = os.path.relpath(os.path.join(base, f), inc)
            if rel != HEADER:
                assert not _declared(rel) & set(ENTRIES), rel
    with open(os.path.join(inc, HEADER)) as f:
        h = f.read()
    assert '#include "../mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")
    for words in ("key descending, reported id ascending", "bitwise the entries of mmf_sim_dense_combined", "k + self <= 44 the output is bit for bit",
                  "the first k columns of the k' result are the k result", "Any k >= 1", "before any device call",
                  "device_id < 0 ->\n * MMF_E_UNSUPPORTED first", "MMF_PREC_FAST / _FAST_BF16 return MMF_E_UNSUPPORTED", "EXPORTS_TOPK_ANYK",
                  "Host-synchronous", "then id -1 and value -inf"):
        assert words in h, words
    with open(os.path.join(inc, "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()


def test_library_and_binding_export_the_entries_from_a_list_of_their_own():
    mmf = _mmf()
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_TOPK_ANYK) == ENTRIES and all(hasattr(L, e) for e in ENTRIES)
    for name in OTHER_LISTS:
        assert not set(ENTRIES) & set(getattr(mmf._lib, name)), name
    lists = [n for n in vars(mmf._lib) if n.startswith("EXPORTS")]
    assert sorted(lists) == sorted(OTHER_LISTS + ["EXPORTS_TOPK_ANYK"])                  # disjoint from EVERY other list
    lib = mmf._lib.lib()
    assert tuple(lib.mmf_simtopk_combined_anyk.argtypes) == tuple(lib.mmf_simtopk_combined.argtypes)
    assert tuple(lib.mmf_simtopk_combined_xy_anyk.argtypes) == tuple(lib.mmf_simtopk_combined_xy.argtypes)
    assert lib.mmf_simtopk_combined_anyk.restype is ctypes.c_int and lib.mmf_simtopk_combined_xy_anyk.restype is ctypes.c_int
    assert mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_build_lists_the_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_topk_anyk", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", "ext", "mmf_hg_topk_anyk.h")) for h in b.HEADERS)


def test_module_and_functions_are_exported():
    mmf, ak = _mmf(), _ak()
    assert mmf.combined_topk_anyk is ak and "combined_topk_anyk" in mmf.__all__
    for name in ("anyk_route", "simtopk_combined_any_k", "simtopk_combined_xy_any_k", "simtopk_combined_rows_any_k",
                 "build_topk_weighted_hypergraph_any_k", "build_topk_hypergraph_data_any_k"):
        assert getattr(mmf, name) is getattr(ak, name) and name in mmf.__all__
    assert list(inspect.signature(ak.simtopk_combined_any_k).parameters) == list(inspect.signature(mmf.combined_topk.simtopk_combined).parameters)
    xy = mmf.combined_topk_xy
    for new, old in ((ak.simtopk_combined_xy_any_k, xy.simtopk_combined_xy), (ak.simtopk_combined_rows_any_k, xy.simtopk_combined_rows)):
        assert list(inspect.signature(new).parameters) == [p for p in inspect.signature(old).parameters if p != "precision"]
    for new, old in ((ak.build_topk_weighted_hypergraph_any_k, mmf.combined_topk.build_topk_weighted_hypergraph),
                     (ak.build_topk_hypergraph_data_any_k, mmf.combined_topk.build_topk_hypergraph_data)):
        assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters)
    from multimodal_fusion_amd import distributed
    assert list(inspect.signature(distributed.sharded_simtopk_combined_any_k).parameters) == \
        [p for p in inspect.signature(distributed.sharded_simtopk_combined).parameters if p not in ("precision", "op")]


# ---- the entries' host checks, with host buffers standing in for device pointers -------------------------------------------------
def _ptr(v):
    return None if v is None else ctypes.cast((ctypes.c_int64 * len(v))(*v), ctypes.c_void_p)


def _buf():
    return ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)


def _self(entry="mmf_simtopk_combined_anyk", **kw):
    mmf = _mmf()
    L = mmf._lib.lib()
    b = _buf()
    a = dict(F=b, P=b, n=8, d=600, dp=2, lh=0.5, lg=0.5, k=2, self=1, ptr=None, S=0, idx=b, val=b, opts=None, device=63)
    a.update(kw)
    opts = None if a["opts"] is None else ctypes.byref(mmf._lib.SimtopkOpts(*a["opts"]))
    rc = getattr(L, entry)(a["F"], a["P"], a["n"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], _ptr(a["ptr"]), a["S"],
                           a["idx"], a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


def _xy(entry="mmf_simtopk_combined_xy_anyk", **kw):
    mmf = _mmf()
    L = mmf._lib.lib()
    b = _buf()
    a = dict(Fq=b, Pq=b, nq=4, Fc=b, Pc=b, nc=8, d=600, dp=2, lh=0.5, lg=0.5, k=2, self=1, ro=0, co=0, idx=b, val=b, opts=None, device=63)
    a.update(kw)
    opts = None if a["opts"] is None else ctypes.byref(mmf._lib.SimtopkOpts(*a["opts"]))
    rc = getattr(L, entry)(a["Fq"], a["Pq"], a["nq"], a["Fc"], a["Pc"], a["nc"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], a["ro"],
                           a["co"], a["idx"], a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


SEG = dict(ptr=[0, 3, 8], S=2)
SELF = [
    (dict(n=-1), INVALID, "n must be >= 0"),
    (dict(d=0), INVALID, "d must be at least 1"),
    (dict(dp=0), INVALID, "dp must be at least 1"),
    (dict(k=0), INVALID, "k must be at least 1"),
    (dict(lh=-1.0), INVALID, "lambda_h must be finite"),
    (dict(lg=float("inf")), INVALID, "lambda_g must be finite"),
    (dict(lg=float("nan")), INVALID, "lambda_g must be finite"),
    (dict(F=None), INVALID, "F is NULL"),
    (dict(P=None), INVALID, "P is NULL"),
    (dict(idx=None), INVALID, "out_idx is NULL"),
    (dict(val=None), INVALID, "out_val is NULL"),
    (dict(ptr=None, S=2), INVALID, "host offsets ptr_host"),
    (dict(ptr=[1, 3, 8], S=2), INVALID, "ptr_host must start at 0"),
    (dict(ptr=[0, 9, 8], S=2), INVALID, "ptr_host decreases at segment 1"),
    (dict(ptr=[0, 3, 7], S=2), INVALID, "ptr_host must end at 8"),
    (dict(opts=(0, 0, -1, 0, None)), INVALID, "col_splits must be >= 0"),
    (dict(opts=(0, 0, 3, 0, None), **SEG), INVALID, "col_splits must be 0 or a power of two (got 3)"),
    (dict(dp=9), UNSUPPORTED, "dp = 9 > 8"),
    (dict(dp=9, k=200, **SEG), UNSUPPORTED, "dp = 9 > 8"),
    (dict(n=1 << 31), UNSUPPORTED, "n must be < 2^31"),
    (dict(opts=(2, 0, 0, 0, None)), UNSUPPORTED, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
    (dict(opts=(3, 0, 0, 0, None), **SEG), UNSUPPORTED, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
]
XY = [
    (dict(nq=-1), INVALID, "nq must be >= 0"),
    (dict(nc=-1), INVALID, "nc must be >= 0"),
    (dict(d=0), INVALID, "d must be at least 1"),
    (dict(dp=0), INVALID, "dp must be at least 1"),
    (dict(k=0), INVALID, "k must be at least 1"),
    (dict(ro=-1), INVALID, "row_offset must be >= 0"),
    (dict(co=-1), INVALID, "col_offset must be >= 0"),
    (dict(lh=float("nan")), INVALID, "lambda_h must be finite"),
    (dict(lg=-0.5), INVALID, "lambda_g must be finite"),
    (dict(Fq=None), INVALID, "Fq is NULL"),
    (dict(Pq=None), INVALID, "Pq is NULL"),
    (dict(Fc=None), INVALID, "Fc is NULL"),
    (dict(Pc=None), INVALID, "Pc is NULL"),
    (dict(idx=None), INVALID, "out_idx is NULL"),
    (dict(val=None), INVALID, "out_val is NULL"),
    (dict(opts=(9, 0, 0, 0, None)), INVALID, "precision 9"),
    (dict(opts=(0, 0, -2, 0, None)), INVALID, "col_splits must be >= 0"),
    (dict(dp=9), UNSUPPORTED, "dp = 9 > 8"),
    (dict(opts=(2, 0, 0, 0, None)), UNSUPPORTED, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
    (dict(opts=(3, 0, 0, 0, None), k=100), UNSUPPORTED, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
    (dict(ro=(1 << 31) - 4), UNSUPPORTED, "row_offset + nq must be < 2^31"),
    (dict(co=(1 << 31) - 8), UNSUPPORTED, "col_offset + nc must be < 2^31"),
]


@pytest.mark.parametrize("kw,code,words", SELF)
def test_the_self_entry_refuses_before_any_device_call(kw, code, words):
    """A device id that does not exist: an argument error must win over the device's."""
    rc, msg = _self(**kw)
    assert rc == code and words in msg and msg.startswith("simtopk_combined_anyk:"), (rc, msg)


@pytest.mark.parametrize("kw,code,words", XY)
def test_the_two_set_entry_refuses_before_any_device_call(kw, code, words):
    rc, msg = _xy(**kw)
    assert rc == code and words in msg and msg.startswith("simtopk_combined_xy_anyk:"), (rc, msg)


def test_a_negative_device_is_refused_first():
    for kw in (dict(), dict(k=0), dict(ptr=None, S=2), dict(idx=None), dict(dp=9), dict(opts=(2, 0, 0, 0, None))):
        rc, msg = _self(device=-1, **kw)
        assert rc == UNSUPPORTED and "no CPU path" in msg and "simtopk_combined_anyk" in msg, (rc, msg)
    for kw in (dict(), dict(k=0), dict(Fq=None), dict(opts=(2, 0, 0, 0, None))):
        rc, msg = _xy(device=-1, **kw)
        assert rc == UNSUPPORTED and "no CPU path" in msg and "simtopk_combined_xy_anyk" in msg, (rc, msg)


@pytest.mark.parametrize("k", [44, 45, 200])
def test_any_k_reaches_the_device_and_no_rows_are_a_no_op(k):
    """k + self on either side of 44 and far beyond, one graph and offsets, AUTO and EXACT, power-of-two col_splits: the call gets
    as far as the device (which is not there)."""
    E_HIP = _mmf()._lib.MMF_E_HIP
    for kw in (dict(), dict(self=0), SEG, dict(opts=(1, 1, 8, 0, None), **SEG), dict(opts=(0, 0, 3, 0, None)), dict(ptr=[0, 0, 8], S=2)):
        rc, msg = _self(k=k, **kw)
        assert rc == E_HIP, (kw, rc, msg)
    for kw in (dict(), dict(self=0), dict(opts=(1, 0, 4, 0, None)), dict(nc=0, Fc=None, Pc=None), dict(ro=5, co=2)):
        rc, msg = _xy(k=k, **kw)
        assert rc == E_HIP, (kw, rc, msg)
    assert _self(k=k, n=0, F=None, P=None, idx=None, val=None)[0] == 0 and _self(k=k, n=0, ptr=[0, 0, 0], S=2, F=None, P=None)[0] == 0
    assert _xy(k=k, nq=0, Fq=None, Pq=None, idx=None, val=None)[0] == 0


def test_the_existing_entries_still_refuse_with_their_words():
    rc, msg = _self("mmf_simtopk_combined", k=44)
    assert rc == UNSUPPORTED and msg == "simtopk_combined: k + self = 45 > 44 is not supported (the multi-pass floors are a follow-up)", msg
    rc, msg = _self("mmf_simtopk_combined_segmented_exact", k=45, self=0, **SEG)
    assert rc == UNSUPPORTED and msg == "simtopk_combined_segmented_exact: k + self = 45 > 44 is not supported (the combined re-rank has no floors)", msg
    rc, msg = _xy("mmf_simtopk_combined_xy", k=44)
    assert rc == UNSUPPORTED and msg == "simtopk_combined_xy: k + self = 45 > 44 is not supported (the multi-pass floors are a follow-up)", msg
    E_HIP = _mmf()._lib.MMF_E_HIP
    assert _self("mmf_simtopk_combined", k=43)[0] == E_HIP and _xy("mmf_simtopk_combined_xy", k=44, self=0)[0] == E_HIP


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_the_routing_rule():
    ak = _ak()
    old = {False: "combined_topk.simtopk_combined", True: "segmented_exact.simtopk_combined_exact"}
    for segmented in (False, True):
        assert ak.anyk_route(43, True, segmented) == ak.anyk_route(44, False, segmented) == ak.anyk_route(1, True, segmented) == old[segmented]
        assert ak.anyk_route(44, True, segmented) == ak.anyk_route(45, False, segmented) == ak.anyk_route(4096, True, segmented) == "mmf_simtopk_combined_anyk"
    with pytest.raises(ValueError, match="k must be >= 1"):
        ak.anyk_route(0, True, False)
    assert ak.ONE_PASS_MAX == 44


def test_python_functions_refuse_on_the_host(monkeypatch):
    mmf, ak = _mmf(), _ak()
    from multimodal_fusion_amd import distributed
    monkeypatch.setattr(mmf._lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    F, P = torch.zeros(8, 16), torch.zeros(8, 2)
    bad = [(lambda: ak.simtopk_combined_any_k(F, P[:4], k=60), "must share N"),
           (lambda: ak.simtopk_combined_any_k(F, P, k=0), "k must be >= 1"),
           (lambda: ak.simtopk_combined_any_k(F, P, k=60, ptr=[0, 3, 7]), "ptr"),
           (lambda: ak.simtopk_combined_any_k(F, P, k=60, ptr=[0, 8], batch=torch.zeros(8, dtype=torch.int64)), "ptr"),
           (lambda: ak.simtopk_combined_any_k(F, P, k=60, col_splits=-1), "col_splits must be >= 0"),
           (lambda: ak.simtopk_combined_any_k(F, P, k=60, ptr=[0, 8], col_splits=3), "col_splits must be 0 or a power of two"),
           (lambda: ak.simtopk_combined_xy_any_k(F[:4], P[:3], F, P, k=60), "must share Nq"),
           (lambda: ak.simtopk_combined_xy_any_k(F[:4], P[:4], F, P[:, :1], k=60), "must share D and dp"),
           (lambda: ak.simtopk_combined_xy_any_k(F[:4], P[:4], F, P, k=0), "k must be >= 1"),
           (lambda: ak.simtopk_combined_xy_any_k(F[:4], P[:4], F, P, k=60, row_offset=-1), "row_offset and col_offset must be >= 0"),
           (lambda: ak.simtopk_combined_xy_any_k(F[:4], P[:4], F, P, k=60, col_splits=-1), "col_splits must be >= 0"),
           (lambda: ak.simtopk_combined_rows_any_k(F, P, 5, 3, k=60), "are no range"),
           (lambda: ak.simtopk_combined_rows_any_k(F, P, 0, 9, k=60), "are no range"),
           (lambda: ak.simtopk_combined_rows_any_k(F, P[:4], 0, 4, k=60), "must share N"),
           (lambda: ak.build_topk_weighted_hypergraph_any_k(F, P, k=0), "k must be >= 1"),
           (lambda: ak.build_topk_weighted_hypergraph_any_k(F, P, k=60, ptr=[0, 9]), "ptr"),
           (lambda: ak.build_topk_hypergraph_data_any_k(F, P[:4], k=60), "must share N"),
           (lambda: distributed.sharded_simtopk_combined_any_k(F[:4], P, 8, k=60), "shards have")]
    for fn, words in bad:
        with pytest.raises(ValueError, match=re.escape(words)):
            fn()


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU the functions run: tests/test_gpu_simtopk_combined_anyk.py")
def test_without_a_gpu_every_function_raises_the_packages_error():
    ak = _ak()
    from multimodal_fusion_amd import distributed
    F, P = torch.zeros(8, 16), torch.zeros(8, 2)
    for fn in (lambda: ak.simtopk_combined_any_k(F, P, k=60), lambda: ak.simtopk_combined_any_k(F, P, k=5), lambda: ak.simtopk_combined_any_k(F, P, k=60, ptr=[0, 3, 8]),
               lambda: ak.simtopk_combined_xy_any_k(F[:4], P[:4], F, P, k=60), lambda: ak.simtopk_combined_rows_any_k(F, P, 2, 6, k=60),
               lambda: ak.build_topk_weighted_hypergraph_any_k(F, P, k=60), lambda: ak.build_topk_hypergraph_data_any_k(F, P, k=60),
               lambda: distributed.sharded_simtopk_combined_any_k(F, P, 8, k=60)):
        with pytest.raises(RuntimeError, match="ROCm"):
            fn()


# ---- the re-rank and the drivers, read statically ------------------------------------------------------------------------------------
def test_every_launch_of_the_rerank_is_on_the_callers_stream_and_nothing_blocks():
    from test_stream_arguments_cpu import BLOCKING, enclosing, is_null, sources, stream_uses
    src = dict(sources())
    text, api = src["mmf_topk.hip"], src["mmf_api.hip"]
    uses = [u for u in stream_uses() if u[0] == "mmf_topk.hip"]
    launched = [a[0] for _, _, what, _, a in uses if what == "hipLaunchKernelGGL"]
    assert sorted(launched) == sorted(["rerank_combined_kernel<true>", "rerank_combined_kernel<false>", "(rerank_combined_kernel<true, true>)",
                                       "(rerank_combined_kernel<false, true>)"]), launched
    assert all(u[3] == "s" for u in uses) and not [u for u in uses if is_null(u[3])]
    assert not [m for m in BLOCKING.finditer(text) if not m.group(1).endswith("Async")]
    # the launcher still refuses gathered and permuted rows, and no longer refuses a pass
    launcher = text.split("int launch_rerank_combined(", 1)[1].split("\n}\n", 1)[0]
    assert "p.row_ids || p.perm" in launcher and "p.out_off != 0" in launcher.split("const bool pass")[1].split("\n")[0]
    assert "p.out_off != 0 ||" not in launcher.split("const bool pass")[0]
    # both entries: every refusal before the device is touched, nothing blocking, no stream of their own
    raw = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")).read()
    for name, first_device_call in (("mmf_simtopk_combined_anyk", "run_simtopk_combined("), ("mmf_simtopk_combined_xy_anyk", "run_simtopk_combined_xy(")):
        body = raw.split("int " + name + "(", 1)[1].split("\n}\n", 1)[0]
        assert body.index(".on_device()") < body.index("set_error(") and body.rindex("set_error(") < body.index(first_device_call), name
        assert not [m for m in BLOCKING.finditer(body) if not m.group(1).endswith("Async")] and "hipStream" not in body, name
    body = raw.split("int mmf_simtopk_combined_anyk(", 1)[1].split("\n}\n", 1)[0]
    assert body.rindex("set_error(") < body.index("r.call.begin()") < body.index("run_segmented_exact(")
    assert "k + self" not in body.replace("k + self = 20", "")                             # no limit on k is left in it
    # the drivers carve the floors their passes need
    for fn in ("run_simtopk_combined", "run_simtopk_combined_xy"):
        assert "B.carve(ws, ex.rows_total, ex.list_words, ex.cap(), ex.floors());" in api.split("int " + fn + "(", 1)[1].split("\n}\n", 1)[0], fn
    assert enclosing(api, api.index("run_segmented_exact(r, true, ptr_host, ptr_host, n_segments, opts, P, (int)dp, lambda_g)")) is not None


# ---- documents -----------------------------------------------------------------------------------------------------------------------
def _table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Any-k top-k entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_table_equals_the_gpu_tests_table():
    from test_gpu_simtopk_combined_anyk import SYNC
    rows = _table()
    assert rows == SYNC, (rows, SYNC)
    assert set(rows) == set(_mmf()._lib.EXPORTS_TOPK_ANYK)


def test_design_readme_and_scripts_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = " ".join(design.split("### 4.23", 1)[1].split("\n## ", 1)[0].split())          # the section, line breaks aside
    for words in ("Contract", "mmf_simtopk_combined_anyk", "mmf_simtopk_combined_xy_anyk", "floor_key_out", "out_off", "kernel-resource-usage",
                  "instruction for instruction identical", "Measurements", "simtopk_combined_anyk_timing.txt", "Cut", "one rank"):
        assert words in sec, words
    assert "\n| t5 " in design.split("## 4", 1)[0] and "combined_topk_anyk" in design.split("## 4", 1)[0]      # §1's table has the row
    for path, words in (("README.md", ["combined_topk_anyk", "simtopk_combined_any_k", "simtopk_combined_anyk_timing"]),
                        (os.path.join("scripts", "README.md"), ["simtopk_combined_anyk_timing.py"]),
                        (os.path.join("scripts", "simtopk_combined_anyk_timing.py"), ["mmf_simtopk_combined_anyk", "bit for bit"]),
                        (os.path.join("multimodal-fusion_amd", "csrc", "mmf_host.h"), ["floor_key_out / floor_id_out"])):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for w in words:
            assert w in text, (path, w)
    assert os.path.exists(os.path.join(ROOT, "profiles", "simtopk_combined_anyk_timing.txt"))
