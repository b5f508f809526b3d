"""The wide 16-bit cross-segment top-k without a GPU (include/ext/mmf_hg_cross_segw.h): the header declares exactly
the two new entries, the library exports them and the binding registers them in a list of its own, the entry runs its host checks
before any device call and names itself, the Python functions raise their argument errors on the host and the router takes the
route it documents, the work table — queried on the host — equals a restatement of its rule and, independently, covers for every
row each admissible column exactly once and no excluded one once the mask is applied, and the Gaussian inputs of
tests/test_gpu_cross_segments_wide.py satisfy the band condition under which the scan may flag no row."""
import ctypes
import functools
import inspect
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import scan16_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join("ext", "mmf_hg_cross_segw.h")
ENTRIES = ["mmf_simtopk_cross_segments_wide", "mmf_cross_segments_wide_table"]
INVALID, UNSUPPORTED = -1, -2
SPILL = 192                      # overflow-list slots per row: what the re-rank's 1024 candidates per row leave to the lists


def _mmf():
    import multimodal_fusion_amd as m
    return m


def _declared(path):
    with open(os.path.join(ROOT, "include", path)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- 1. header ------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_new_entries_and_no_version():
    assert _declared(HEADER) == set(ENTRIES)
    inc = os.path.join(ROOT, "include")
    for base, _, files in os.walk(inc):
        for f in files:
            rel = os.path.relpath(os.path.join(base, f), inc)
            if rel != HEADER:
                assert not _declared(rel) & set(ENTRIES), rel
    with open(os.path.join(inc, HEADER)) as f:
        h = f.read()
    assert '#include "../mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "") and "#define MMF_ABI" not in h
    for words in ("bit for bit", "no -1 / -inf fill", "before any device call", "1024 < d <= 4096", "k <= 20",
                  "key descending, then id ascending", "power of two", "Host only", "Host-synchronous: once per call",
                  "select_wait_event is refused", "query_order is ignored", "does NOT forward to mmf_simtopk_cross_segments_fast"):
        assert words in h, words


# ---- 2. exports -----------------------------------------------------------------------------------------------------------------
def test_library_and_binding_export_the_entries_from_a_list_of_their_own():
    mmf = _mmf()
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.CROSS_SEGW_EXPORTS) == ENTRIES and all(hasattr(L, e) for e in ENTRIES)
    for name in (n for n in vars(mmf._lib) if n.isupper() and "EXPORTS" in n and n != "CROSS_SEGW_EXPORTS"):
        assert not set(ENTRIES) & set(getattr(mmf._lib, name)), name
    lib = mmf._lib.lib()
    assert list(lib.mmf_simtopk_cross_segments_wide.argtypes) == list(lib.mmf_simtopk_cross_segments_fast.argtypes)
    assert list(lib.mmf_cross_segments_wide_table.argtypes) == list(lib.mmf_cross_segments_fast_table.argtypes)
    assert lib.mmf_simtopk_cross_segments_wide.restype is ctypes.c_int and lib.mmf_cross_segments_wide_table.restype is ctypes.c_int64
    assert mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_build_lists_the_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_cross_segw", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", HEADER)) for h in b.HEADERS)


def test_module_and_functions_are_exported():
    mmf = _mmf()
    cs = import_module("multimodal_fusion_amd.cross_segments_wide")
    assert mmf.cross_segments_wide is cs and "cross_segments_wide" in mmf.__all__ and "mmf.cross_segments_wide.*" in mmf.__doc__
    for name in ("simtopk_cross_segments_wide", "cross_segments_wide_table", "cross_segments_route"):
        assert getattr(mmf, name) is getattr(cs, name) and name in mmf.__all__
    assert mmf.simtopk_cross_segments is mmf.cross_segments.simtopk_cross_segments                 # the package name stays the exact call
    base = ["X", "Y", "ptr", "batch", "y_ptr", "y_batch", "metric", "lam", "k", "precision", "col_splits", "return_stats", "profile"]
    assert list(inspect.signature(cs.simtopk_cross_segments_wide).parameters) == base
    assert list(inspect.signature(cs.simtopk_cross_segments).parameters) == base
    assert inspect.signature(cs.simtopk_cross_segments_wide).parameters["precision"].default == "fast"
    assert inspect.signature(cs.simtopk_cross_segments).parameters["precision"].default == "auto"
    assert list(inspect.signature(cs.cross_segments_wide_table).parameters) == ["ptr", "y_ptr", "d", "k", "col_splits"]
    assert list(inspect.signature(cs.cross_segment_knn_edges).parameters) == ["X", "ptr", "batch", "k", "precision"]
    assert list(inspect.signature(cs.link_slides).parameters) == ["out", "k", "precision"]
    for fn in (cs.cross_segment_knn_edges, cs.link_slides):
        p = inspect.signature(fn).parameters["precision"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "exact"
    # the narrow module keeps its own router and signatures
    cs16 = mmf.cross_segments16
    assert list(inspect.signature(cs16.simtopk_cross_segments).parameters) == base and cs16.simtopk_cross_segments is not cs.simtopk_cross_segments


# ---- 3. the entry's host checks, with host buffers standing in for device pointers ----------------------------------------------
def _ptr(v):
    return None if v is None else ctypes.cast((ctypes.c_int64 * len(v))(*v), ctypes.c_void_p)


def _buf():
    return ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)


def _entry(**kw):
    mmf = _mmf()
    L = mmf._lib.lib()
    b = _buf()
    a = dict(X=b, n=8, Y=None, m=0, d=1100, dtype=0, metric=1, lam=1.0, k=2, xp=[0, 3, 8], yp=None, S=2, idx=b, val=b, opts=None, device=63)
    a.update(kw)
    opts = None if a["opts"] is None else ctypes.byref(mmf._lib.SimtopkOpts(*a["opts"]))
    rc = L.mmf_simtopk_cross_segments_wide(a["X"], a["n"], a["Y"], a["m"], a["d"], a["dtype"], a["metric"], a["lam"], a["k"], _ptr(a["xp"]),
                                           _ptr(a["yp"]), a["S"], a["idx"], a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


REFUSALS = [
    (dict(n=-1), INVALID, "bad shape"),
    (dict(d=0), INVALID, "bad shape"),
    (dict(dtype=7), INVALID, "bad in_dtype 7"),
    (dict(X=None), INVALID, "X is NULL"),
    (dict(n=1 << 31, xp=[0, 3, 1 << 31]), UNSUPPORTED, "n and m must be < 2^31"),
    (dict(metric=9), INVALID, "bad metric"),
    (dict(metric=4), INVALID, "bad metric"),
    (dict(metric=3, lam=0.0), INVALID, "MMF_RBF needs lambda > 0"),
    (dict(k=0), INVALID, "k must be >= 1"),
    (dict(xp=[1, 3, 8]), INVALID, "x_ptr must start at 0"),
    (dict(xp=[0, 5, 3, 8], S=3), INVALID, "x_ptr decreases at segment 1"),
    (dict(xp=[0, 3, 7]), INVALID, "x_ptr must end at 8"),
    (dict(xp=None), INVALID, "host offsets x_ptr"),
    (dict(Y=_buf(), m=6, yp=[0, 2, 5]), INVALID, "y_ptr must end at 6"),
    (dict(Y=_buf(), m=6, yp=None), INVALID, "host offsets y_ptr"),
    (dict(opts=(0, 0, 3, 0, None)), INVALID, "col_splits must be 0 or a power of two (got 3)"),
    (dict(opts=(2, 0, -2, 0, None)), INVALID, "col_splits must be 0 or a power of two"),
    (dict(opts=(7, 0, 0, 0, None)), INVALID, "bad precision 7"),
    (dict(opts=(2, 0, 0, 0, 1)), UNSUPPORTED, "select_wait_event is not supported"),
    # the shapes the wide scan does not serve: FAST / FAST_BF16 refuse and name d and k — also where the narrow scan would serve
    (dict(opts=(2, 0, 0, 0, None), d=600), UNSUPPORTED, "does not support d = 600, k = 2"),
    (dict(opts=(3, 0, 0, 0, None), d=600), UNSUPPORTED, "does not support d = 600, k = 2"),
    (dict(opts=(2, 0, 0, 0, None), d=1024), UNSUPPORTED, "does not support d = 1024, k = 2"),
    (dict(opts=(3, 0, 0, 0, None), d=4097), UNSUPPORTED, "does not support d = 4097, k = 2"),
    (dict(opts=(2, 0, 0, 0, None), n=60, xp=[0, 30, 60], k=21), UNSUPPORTED, "does not support d = 1100, k = 21"),
    (dict(opts=(3, 0, 0, 0, None), n=60, xp=[0, 30, 60], k=21), UNSUPPORTED, "does not support d = 1100, k = 21"),
    (dict(idx=None), INVALID, "NULL output"),
    (dict(val=None), INVALID, "NULL output"),
    # segment 1 has 5 of the 8 rows: 3 admissible columns; segment 0 has 5
    (dict(k=4), INVALID, "segment 1 has 3 admissible columns (m = 8 minus its own 5 rows of Y), k = 4"),
    (dict(k=6, opts=(3, 0, 0, 0, None)), INVALID, "segment 0 has 5 admissible columns (m = 8 minus its own 3 rows of Y), k = 6"),
    (dict(xp=[0, 8], S=1, k=1), INVALID, "segment 0 has 0 admissible columns"),
    (dict(Y=_buf(), m=6, yp=[0, 1, 6], k=2), INVALID, "segment 1 has 1 admissible columns (m = 6 minus its own 5 rows of Y), k = 2"),
]


@pytest.mark.parametrize("kw,code,words", REFUSALS)
def test_the_entry_refuses_before_any_device_call(kw, code, words):
    """A device id that does not exist: an argument error must win over the device's."""
    rc, msg = _entry(**kw)
    assert rc == code and words in msg and "simtopk_cross_segments_wide" in msg, (rc, msg)


def test_every_refusal_of_the_exact_entry_appears_under_the_new_name():
    """The same arguments through mmf_simtopk_cross_segments: wherever it refuses, the new entry refuses with the same status and the
    same words after the entry's name (the exact entry has its own words for the 16-bit precisions, which the new entry serves)."""
    mmf = _mmf()
    L = mmf._lib.lib()
    seen = 0
    for kw, _, _ in REFUSALS:
        a = dict(X=_buf(), n=8, Y=None, m=0, d=1100, dtype=0, metric=1, lam=1.0, k=2, xp=[0, 3, 8], yp=None, S=2, idx=_buf(), val=_buf(),
                 opts=None, device=63)
        a.update(kw)
        if a["opts"] is not None and a["opts"][0] in (2, 3, 7):
            continue
        opts = None if a["opts"] is None else ctypes.byref(mmf._lib.SimtopkOpts(*a["opts"]))
        rc = L.mmf_simtopk_cross_segments(a["X"], a["n"], a["Y"], a["m"], a["d"], a["dtype"], a["metric"], a["lam"], a["k"], _ptr(a["xp"]),
                                          _ptr(a["yp"]), a["S"], a["idx"], a["val"], opts, None, a["device"], None)
        exact = L.mmf_last_error().decode()
        got_rc, got = _entry(**kw)
        if rc in (INVALID, UNSUPPORTED) and "select_wait_event" not in got:
            seen += 1
            assert got_rc == rc and got == exact.replace("simtopk_cross_segments:", "simtopk_cross_segments_wide:"), (kw, exact, got)
    assert seen >= 20


def test_a_negative_device_is_refused_first():
    for kw in (dict(), dict(k=0), dict(xp=[1, 3, 8]), dict(idx=None), dict(opts=(0, 0, 3, 0, None)), dict(opts=(2, 0, 0, 0, None), d=600),
               dict(k=6), dict(n=-1), dict(opts=(7, 0, 0, 0, None))):
        rc, msg = _entry(device=-1, **kw)
        assert rc == UNSUPPORTED and "no CPU path" in msg and "simtopk_cross_segments_wide" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """Every precision, dtype and metric, both list capacities, power-of-two col_splits, AUTO on shapes the wide scan does not serve
    (the exact driver: d = 600, which the narrow scan would serve, d = 5000 and k = 21), EXACT, an empty segment on either side: the
    call gets as far as the device (which is not there)."""
    E_HIP = _mmf()._lib.MMF_E_HIP
    big = [0, 100, 300]
    for kw in (dict(), dict(k=3), dict(opts=(0, 1, 8, 0, None)), dict(opts=(1, 0, 0, 0, None)), dict(opts=(2, 0, 16, 0, None)),
               dict(opts=(3, 0, 2, 1, None)), dict(d=1025), dict(d=2560), dict(d=4096), dict(dtype=1), dict(dtype=2), dict(metric=0),
               dict(metric=2), dict(metric=3, lam=0.5), dict(n=300, xp=big, k=20), dict(opts=(2, 0, 0, 0, None), n=300, xp=big, k=20),
               dict(d=600), dict(opts=(0, 0, 0, 0, None), d=600), dict(d=5000), dict(opts=(0, 0, 0, 0, None), d=5000),
               dict(opts=(1, 0, 0, 0, None), d=600), dict(opts=(1, 0, 0, 0, None), n=300, xp=big, k=100),
               dict(n=300, xp=big, k=21), dict(xp=[0, 4, 4, 8], S=3, k=4), dict(Y=_buf(), m=6, yp=[0, 3, 6], k=3),
               dict(Y=_buf(), m=6, yp=[0, 6, 6], xp=[0, 0, 8], k=6)):
        rc, msg = _entry(**kw)
        assert rc == E_HIP, (kw, rc, msg)
    assert _entry(n=0, xp=[0, 0, 0])[0] == 0 and _entry(n=0, xp=[0], S=0, X=None, idx=None, val=None)[0] == 0
    assert _entry(n=0, xp=[0, 0, 0], Y=_buf(), m=6, yp=[0, 2, 6], k=20)[0] == 0


def test_the_entry_makes_every_refusal_before_the_first_device_call_and_keeps_the_other_entries():
    with open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")) as f:
        raw = f.read()
    body = raw.split("int mmf_simtopk_cross_segments_wide(", 1)[1].split("\n}\n", 1)[0]
    assert body.index(".on_device()") < body.index("set_error(") and body.rindex("set_error(") < body.index("run_segmented_exact(")
    # the one driver of both one-pass 16-bit entries, on its wide side: the literal `true`
    wide_call = "run_cross_segments16(r, self, x_ptr_host, y_ptr_host, n_segments, opts, true)"
    narrow_call = "run_cross_segments16(r, self, x_ptr_host, y_ptr_host, n_segments, opts, false)"
    assert body.count("run_cross_segments16(") == 1 and body.index("run_segmented_exact(") < body.index(wide_call)
    assert "hipStream" not in body and "hipMemcpy" not in body and "hipDeviceSynchronize" not in body
    assert "run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true)" in body
    assert narrow_call not in body and "scan_bf16_supported" not in body                        # AUTO does not forward to the narrow entry
    table = raw.split("int64_t mmf_cross_segments_wide_table(", 1)[1].split("\n}\n", 1)[0]
    assert "hip" not in table and "Call(" not in table                                          # host only
    assert "run_cross_segments_wide" not in raw and raw.count("static int run_cross_segments16(") == 1
    driver = raw.split("static int run_cross_segments16(", 1)[1].split("\n}\n", 1)[0]
    assert driver.count("launch_scan_b16w_xseg(") == 1 and driver.count("launch_scan_b16_xseg(") == 1
    assert driver.count("launch_select(") == 1 and driver.count("launch_scan_b16_audit(") == 1
    assert driver.count("upload_table(") == 2 and driver.count("flags.read(") == 1 and driver.count("cross_flagged(") == 1
    assert driver.count("hipStreamSynchronize") == 1 and driver.index("if (fallback_rows > 0) {") < driver.index("hipStreamSynchronize")
    assert "(hipStream_t)0" not in driver and "hipMemcpy(" not in driver and "hipMemset(" not in driver
    # the two older entries keep their refusals
    exact = raw.split("int mmf_simtopk_cross_segments(", 1)[1].split("\n}\n", 1)[0]
    assert "no 16-bit scan serves the cross-segment entry yet" in exact
    narrow = raw.split("int mmf_simtopk_cross_segments_fast(", 1)[1].split("\n}\n", 1)[0]
    assert "scan_bf16_supported(d, k, in_dtype)" in narrow and narrow_call in narrow and wide_call not in narrow


# ---- 5. Python: ValueErrors on the host, and the router's route -------------------------------------------------------------------
def _host_only(monkeypatch, mmf):
    monkeypatch.setattr(mmf.ops, "fast_scan_supported", lambda d, k, e=True: (d <= 1024 and k <= 20) or (d <= 512 and k <= 44))
    monkeypatch.setattr(mmf.wide_scan, "wide_scan_supported", lambda d, k, e=True: 1024 < d <= 4096 and k + bool(e) <= 20)
    monkeypatch.setattr(mmf._lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))


def test_python_functions_refuse_on_the_host(monkeypatch):
    mmf = _mmf()
    cs = mmf.cross_segments_wide
    X = torch.zeros(8, 1100)
    sf = torch.zeros(36, 1100)
    out = dict(super_features=sf, group_ptr=torch.tensor([0, 12, 24, 36]), node_ptr=torch.tensor([0, 20, 45, 60]))
    served = mmf.wide_scan.wide_scan_supported
    _host_only(monkeypatch, mmf)
    wide, route = cs.simtopk_cross_segments_wide, cs.simtopk_cross_segments
    bad = [(lambda: wide(X, ptr=[0, 3, 7], k=2), "ptr"),
           (lambda: wide(X, ptr=[0, 3, 8], k=0), "k must be >= 1"),
           (lambda: wide(X, ptr=[0, 3, 8], col_splits=3, k=2), "col_splits must be 0 or a power of two"),
           (lambda: wide(X, ptr=[0, 3, 8], col_splits=-4, k=2), "col_splits must be 0 or a power of two"),
           (lambda: wide(X, ptr=[0, 3, 8], y_ptr=[0, 8]), "y_ptr / y_batch need Y"),
           (lambda: wide(X, torch.zeros(4, 8), ptr=[0, 8], y_ptr=[0, 4]), "share device, dtype and feature dim"),
           (lambda: wide(torch.zeros(8), ptr=[0, 8]), "2-D"),
           (lambda: wide(X, ptr=[0, 3, 8], metric="manhattan", k=2), "unknown metric"),
           (lambda: wide(X, ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns (m = 8 minus its own 5 rows of Y), k = 4"),
           (lambda: wide(X, batch=torch.tensor([0, 0, 0, 1, 1, 1, 1, 1]), k=6), "segment 0 has 5 admissible columns"),
           (lambda: wide(X, torch.zeros(6, 1100), ptr=[0, 3, 8], y_ptr=[0, 1, 6], k=2), "segment 1 has 1 admissible columns"),
           (lambda: wide(X, k=1), "ptr"),
           (lambda: wide(X, ptr=[0, 3, 8], k=2, precision="exact"), "precision must be 'fast' or 'fast_bf16'"),
           (lambda: wide(X, ptr=[0, 3, 8], k=2, precision="auto"), "precision must be 'fast' or 'fast_bf16'"),
           (lambda: wide(torch.zeros(8, 600), ptr=[0, 3, 8], k=2), "does not serve d = 600, k = 2"),
           (lambda: wide(torch.zeros(8, 4200), ptr=[0, 3, 8], k=2, precision="fast_bf16"), "does not serve d = 4200, k = 2"),
           (lambda: wide(torch.zeros(60, 1100), ptr=[0, 30, 60], k=21), "does not serve d = 1100, k = 21"),
           (lambda: route(X, ptr=[0, 3, 8], k=2, precision="bf16"), "unknown precision"),
           (lambda: route(X, ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns"),
           (lambda: route(X, ptr=[0, 3, 8], k=4, precision="fast"), "segment 1 has 3 admissible columns"),
           (lambda: route(torch.zeros(8, 64), ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns"),
           # neither scan serves: the narrow call's words
           (lambda: route(torch.zeros(8, 4200), ptr=[0, 3, 8], k=2, precision="fast"), "simtopk_cross_segments_fast: the 16-bit scan does not serve d = 4200, k = 2"),
           (lambda: route(torch.zeros(60, 1100), ptr=[0, 30, 60], k=21, precision="fast_bf16"), "simtopk_cross_segments_fast: the 16-bit scan does not serve d = 1100, k = 21"),
           (lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], precision="fast"), "precision must be 'exact' or 'auto'"),
           (lambda: cs.cross_segment_knn_edges(X, precision="auto"), "needs ptr or batch"),
           (lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], k=4, precision="auto"), "segment 1 has 3 admissible columns"),
           (lambda: cs.link_slides(out, precision="fast"), "precision must be 'exact' or 'auto'"),
           (lambda: cs.link_slides({"super_features": sf}, precision="auto"), "needs the dict of build_cohort_hypergraphs"),
           (lambda: cs.link_slides(out, k=25, precision="auto"), "segment 0 has 24 admissible columns")]
    for fn, words in bad:
        with pytest.raises(ValueError, match=re.escape(words)):
            fn()
    # the narrow module's router still refuses d = 1100 under "fast"
    with pytest.raises(ValueError, match=re.escape("does not serve d = 1100, k = 2")):
        mmf.cross_segments16.simtopk_cross_segments(X, ptr=[0, 3, 8], k=2, precision="fast")
    monkeypatch.undo()
    assert mmf.wide_scan.wide_scan_supported is served
    for call in (lambda: wide(X, ptr=[0, 3, 8], k=3), lambda: route(X, ptr=[0, 3, 8], k=3), lambda: route(X, ptr=[0, 3, 8], k=3, precision="fast"),
                 lambda: route(torch.zeros(8, 64), ptr=[0, 3, 8], k=3), lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], k=3, precision="auto")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_the_router_takes_the_documented_route(monkeypatch):
    """Per (d, k, precision), with the three calls replaced by recorders.  "auto" where only the wide scan serves follows
    cross_segments_wide.AUTO_TAKES_WIDE, the record of DESIGN.md §4.26's measurement."""
    mmf = _mmf()
    cs = mmf.cross_segments_wide
    _host_only(monkeypatch, mmf)
    calls = []

    def recorder(name):
        def f(X, Y=None, **kw):
            calls.append((name, kw.get("precision")))
            return name
        return f
    monkeypatch.setattr(mmf.cross_segments, "simtopk_cross_segments", recorder("exact"))
    monkeypatch.setattr(mmf.cross_segments16, "simtopk_cross_segments_fast", recorder("narrow"))
    monkeypatch.setattr(cs, "simtopk_cross_segments_wide", recorder("wide"))
    auto_wide = ("wide", "fast") if cs.AUTO_TAKES_WIDE else ("exact", None)
    want = {(600, 5, "auto"): ("narrow", "fast"), (600, 5, "fast"): ("narrow", "fast"), (600, 5, "fast_bf16"): ("narrow", "fast_bf16"),
            (600, 5, "exact"): ("exact", None), (300, 44, "auto"): ("narrow", "fast"), (600, 21, "auto"): ("exact", None),
            (600, 21, "fast"): ("narrow", "fast"), (1024, 20, "auto"): ("narrow", "fast"),
            (1025, 5, "auto"): auto_wide, (1100, 20, "auto"): auto_wide, (4096, 5, "auto"): auto_wide,
            (1100, 5, "fast"): ("wide", "fast"), (1100, 20, "fast_bf16"): ("wide", "fast_bf16"), (4096, 1, "fast"): ("wide", "fast"),
            (1100, 5, "exact"): ("exact", None), (1100, 21, "auto"): ("exact", None), (1100, 21, "fast"): ("narrow", "fast"),
            (4097, 5, "auto"): ("exact", None), (4097, 5, "fast"): ("narrow", "fast"), (4097, 5, "exact"): ("exact", None)}
    for (d, k, precision), (name, passed) in want.items():
        calls.clear()
        assert cs.simtopk_cross_segments(torch.zeros(4, d), ptr=[0, 2, 4], k=k, precision=precision) == name, (d, k, precision)
        assert calls == [(name, passed)], (d, k, precision, calls)
        assert cs.cross_segments_route(d, k, precision) == name


# ---- 4. the work table, queried on the host ---------------------------------------------------------------------------------------
OFFSETS = [0, 100, 137, 437, 565, 700]                      # the GPU tests' segments: every bound off a tile edge
THREE = [50, 40, 0, 300, 129, 1, 500]                       # block 0 (rows 0 .. 128) holds segments 0, 1 and 3
WHOLE = [128, 400, 572]                                     # segment 1 holds blocks 1 .. 3 whole: hole = tiles 1 .. 4 of 10
ALIGNED = [256, 128, 0, 512, 128, 1024, 128]                # every bound a multiple of 128
ONE_BIG = [2990, 20]                                        # a single segment covering all but k = 20 rows ...
ONE_BIG_LAST = [20, 1500]                                   # ... and the other way round: the hole runs to the end of Y
TWO_SIDED = ([40, 0, 129, 5, 257, 1, 300, 32], [300, 7, 33, 0, 128, 256, 4, 1000])      # segment 1: no queries; segment 3: no rows of Y


def _offsets(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def _sizes(offsets):
    return [b - a for a, b in zip(offsets[:-1], offsets[1:])]


CASES = [(_sizes(OFFSETS), None), (THREE, None), (WHOLE, None), (ALIGNED, None), (ONE_BIG, None), (ONE_BIG_LAST, None), TWO_SIDED]
IDS = ["gpu offsets", "three segments in a block", "whole blocks", "aligned", "one big segment", "one big last segment", "two-sided"]


def _segment_of(xp, row):
    return max(s for s in range(len(xp) - 1) if xp[s] <= row < xp[s + 1])


def _restated(xp, yp, k, forced):
    """{first row of a block: [(t0, t1, w0, w1), ...] in slot order} and lists, from §4.26's rule restated."""
    cap = 16 if k <= 11 else 32
    n, m = xp[-1], yp[-1]
    T = -(-m // 256) * 2
    max_r = 1
    while 2 * (2 * max_r + 1) * cap <= 1024 - SPILL:
        max_r *= 2
    geo = {}
    for r0 in range(0, n, 128):
        s0, s1 = _segment_of(xp, r0), _segment_of(xp, min(r0 + 128, n) - 1)
        ulo, uhi = yp[s0], yp[s1 + 1]
        h0 = h1 = 0
        if s0 == s1:
            h0 = -(-ulo // 128)
            h1 = max(h0, T if uhi == m else uhi // 128)
        geo[r0] = (h0, h1, ulo // 128, -(-uhi // 128) if uhi > ulo else ulo // 128)
    fill = 1
    while len(geo) * fill < 256 and fill < max_r:
        fill *= 2
    blocks, most = {}, 1
    for r0, (h0, h1, w0, w1) in geo.items():
        adm = T - (h1 - h0)
        if adm <= 0:
            continue
        want = forced if forced > 0 else min(fill, max(1, adm // 8))       # automatic: no run shorter than 8 tiles
        r = 1
        while 2 * r <= want and 2 * r <= adm and 2 * r <= max_r:
            r *= 2
        tps = -(-adm // r)
        runs = []
        for a0 in range(0, adm, tps):
            a1 = min(a0 + tps, adm)
            if h1 == h0 or a1 <= h0:
                runs.append((a0, a1))
            elif a0 >= h0:
                runs.append((a0 + h1 - h0, a1 + h1 - h0))
            else:
                runs += [(a0, h0), (h1, a1 + h1 - h0)]
        out = []
        for t0, t1 in runs:
            if t0 >= t1:
                continue
            e0, e1 = max(w0, t0), min(w1, t1)
            out.append((t0, t1, e0, e1) if e0 < e1 else (t0, t1, t0, t0))
        blocks[r0] = out
        most = max(most, len(out))
    return blocks, 2 * most, cap


def _blocks_of(table):
    """{row0: [(number, t0, t1, w0, w1)] sorted} from the entries (layout of mmf_hg_cross_segw.h)."""
    got = {}
    for qpos, row0, nq, t0, t1, w0, slot, w1 in table.tolist():
        assert qpos == row0 and slot % 2 == 0
        got.setdefault(row0, []).append((slot // 2, t0, t1, w0, w1))
    return {r: sorted(v) for r, v in got.items()}


@pytest.mark.parametrize("forced", [0, 1, 2, 4, 8, 16])
@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("xs,ys", CASES, ids=IDS)
def test_the_table_is_the_restated_rule_and_covers_every_admissible_column_once(xs, ys, k, forced):
    mmf = _mmf()
    xp = _offsets(xs)
    yp = xp if ys is None else _offsets(ys)
    n, m = xp[-1], yp[-1]
    table, lists = mmf.cross_segments_wide_table(xp, None if ys is None else yp, d=1536, k=k, col_splits=forced)
    assert table.dtype == torch.int32 and table.shape[1] == 8
    want, want_lists, cap = _restated(xp, yp, k, forced)
    assert lists == want_lists and lists % 2 == 0 and lists * cap <= 1024 - SPILL
    T = -(-m // 256) * 2
    for qpos, row0, nq, t0, t1, w0, slot, w1 in table.tolist():
        assert qpos == row0 and row0 % 128 == 0 and nq == min(128, n - row0) and nq >= 1
        assert 0 <= t0 < t1 <= T and t0 <= w0 <= w1 <= t1 and 0 <= slot and slot % 2 == 0 and slot + 1 < lists
    got = _blocks_of(table)
    for r, v in got.items():
        assert [e[0] for e in v] == list(range(len(v))), "list slots of a block are not 0, 2, .. in tile order"
    assert {r: [e[1:] for e in v] for r, v in got.items()} == want
    assert sorted(got) == [r for r in range(0, n, 128) if want.get(r)], "a row block with admissible tiles and no entry"
    lengths = [e[4] - e[3] for e in table.tolist()]
    assert lengths == sorted(lengths, reverse=True), "the entries do not come longest run first"
    cap_r = 16 if k <= 11 else 8
    assert lists <= 2 * (cap_r + 1)
    if forced and forced <= cap_r:
        assert lists <= 2 * forced + 2                            # + 1 entry where a run spans a hole
    # independently of the rule: for every row, the tiles of its block's entries minus the columns the mask removes (inside the
    # entry's window, the row's own segment) are every admissible column exactly once and no excluded one; outside the window no
    # tile of an entry holds a column that any row of the block excludes
    for r0 in range(0, n, 128):
        tiles = [(t, w0 <= t < w1) for _, t0, t1, w0, w1 in got.get(r0, []) for t in range(t0, t1)]
        assert len(tiles) == len({t for t, _ in tiles}), "a tile is in two entries of a block"
        segs = sorted({_segment_of(xp, i) for i in range(r0, min(r0 + 128, n))})
        for s in segs:                                            # the rows of a block that share a segment share the answer
            lo, hi = yp[s], yp[s + 1]
            seen = []
            for t, masked in tiles:
                cols = range(t * 128, min((t + 1) * 128, m))
                if masked:
                    seen += [j for j in cols if not lo <= j < hi]
                else:
                    assert not any(lo <= j < hi for j in cols), f"block {r0}, segment {s}: tile {t} holds excluded columns outside the mask window"
                    seen += list(cols)
            assert len(seen) == len(set(seen)) == m - (hi - lo), f"block {r0}, segment {s}: admissible columns missing or doubled"


def test_a_hole_inside_a_run_and_at_a_run_edge_and_the_automatic_rule():
    mmf = _mmf()
    entries = lambda t, row0: [list(e[1:]) for e in _blocks_of(t)[row0]]          # noqa: E731  (t0, t1, w0, w1) in slot order
    # m = 1100: 10 tiles (m_pad = 1280).  Segment 1 = rows 128 .. 528 swallows tiles 1 .. 4; tile 4 (rows 512 .. 640) straddles its end
    xp = _offsets(WHOLE)
    t, lists = mmf.cross_segments_wide_table(xp, d=1100, k=5, col_splits=1)
    assert entries(t, 256) == [[0, 1, 0, 0], [4, 10, 4, 5]] and lists == 4                       # one run across the hole
    assert entries(t, 0) == [[1, 10, 1, 1]]                                                      # segment 0 = tile 0: a hole at the front edge
    assert entries(t, 512) == [[0, 10, 1, 9]]                                                    # rows 512 .. 640: segments 1 and 2, no hole
    assert entries(t, 640) == [[0, 5, 4, 5]]                                                     # segment 2 runs to the end of Y: hole 5 .. 10
    t, lists = mmf.cross_segments_wide_table(xp, d=1100, k=5, col_splits=2)
    assert entries(t, 128) == [[0, 1, 0, 0], [4, 7, 4, 5], [7, 10, 7, 7]] and lists == 6         # the hole inside the first of two runs
    assert entries(t, 0) == [[1, 6, 1, 1], [6, 10, 6, 6]]
    t, lists = mmf.cross_segments_wide_table(xp, d=1100, k=5, col_splits=8)                      # 7 admissible tiles: four runs of two
    assert entries(t, 384) == [[0, 1, 0, 0], [4, 5, 4, 5], [5, 7, 5, 5], [7, 9, 7, 7], [9, 10, 9, 9]] and lists == 10
    # the hole exactly between two runs: [512, 1024, 512] at two runs of 4 tiles, hole = tiles 4 .. 12
    t, lists = mmf.cross_segments_wide_table(_offsets([512, 1024, 512]), d=1100, k=5, col_splits=2)
    assert entries(t, 512) == [[0, 4, 0, 0], [12, 16, 12, 12]] and lists == 4
    # automatic: 9 row blocks ask for 32 runs (9 x 32 >= 256), the capacity allows 16, runs of 8 tiles allow one here
    t, lists = mmf.cross_segments_wide_table(xp, d=1100, k=5)
    assert lists == 4 and all(len(v) <= 2 for v in _blocks_of(t).values())
    # 64 x 1024 rows: 512 row blocks fill the chip with one run each
    t, lists = mmf.cross_segments_wide_table(_offsets([1024] * 64), d=1536, k=5)
    assert lists == 4 and t.shape[0] == 512 + 62 * 8
    # 8 x 1024 rows: 64 blocks x 4 runs = 256; 56 admissible tiles make runs of 14
    t, lists = mmf.cross_segments_wide_table(_offsets([1024] * 8), d=1536, k=5)
    assert lists == 10 and max(e[4] - e[3] for e in t.tolist()) == 14
    # k = 20 (32-entry lists): at most 8 runs, forced or not
    t, lists = mmf.cross_segments_wide_table(_offsets([1024] * 2), d=1536, k=20, col_splits=16)
    assert lists == 16
    t, lists = mmf.cross_segments_wide_table(_offsets([1024] * 2), d=1536, k=5, col_splits=16)
    assert lists == 16                                            # 8 admissible tiles: 8 runs


def test_the_table_query_refuses_bad_arguments():
    mmf = _mmf()
    for kw, words in ((dict(ptr=[1, 4]), "x_ptr must start at 0"), (dict(ptr=[0, 4, 2]), "decreases"), (dict(ptr=[0, 4], k=0), "k must be >= 1"),
                      (dict(ptr=[0, 4], col_splits=3), "power of two"), (dict(ptr=[0, 4], y_ptr=[0, 2, 4]), "the same S on both sides")):
        with pytest.raises(ValueError, match=words):
            mmf.cross_segments_wide_table(kw.pop("ptr"), d=1536, **kw)
    for d, k in ((600, 5), (1100, 21), (4097, 5)):
        with pytest.raises(RuntimeError, match=f"does not serve d = {d}, k = {k}"):
            mmf.cross_segments_wide_table([0, 300, 600], d=d, k=k)
    L = mmf._lib.lib()
    small = (ctypes.c_int32 * 8)()
    rc = L.mmf_cross_segments_wide_table(_ptr([0, 300, 600]), None, 2, 1536, 5, 0, ctypes.cast(small, ctypes.c_void_p), 1, None)
    assert rc == INVALID and "entries needed" in L.mmf_last_error().decode() and "cross_segments_wide_table" in L.mmf_last_error().decode()
    table, lists = mmf.cross_segments_wide_table([0], d=1536, k=5)                              # no segments: no entries
    assert table.shape == (0, 8) and lists == 2
    table, _ = mmf.cross_segments_wide_table([0, 300], d=1536, k=5)                             # one segment: nothing is admissible
    assert table.shape == (0, 8)


def test_the_narrow_table_is_unchanged_by_the_shared_geometry():
    """cross_seg16_table shares its block geometry and run cutting with the wide table: one of its pinned results, again."""
    mmf = _mmf()
    t, _ = mmf.cross_segments_fast_table(_offsets([100, 200, 212]), d=600, k=5, col_splits=1)
    assert sorted(e[:8] for e in t.tolist()) == [[0, 0, 128, 0, 16, 0, 0, 10], [128, 128, 128, 0, 4, 0, 3, 4], [128, 128, 128, 9, 16, 1, 9, 10],
                                                 [256, 256, 128, 0, 16, 0, 3, 16], [384, 384, 128, 0, 10, 0, 9, 10]]


# ---- 6. the band condition of the GPU tests' data ---------------------------------------------------------------------------------
# tests/test_gpu_cross_segments_wide.py imports everything below: the rows, the kernel table and the band count.
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# (d, k, metric, row dtype): d = 1100 pads to 1152 and d = 1300 to 1408; k = 5 takes the 16-entry lists and k = 20 the 32-entry
# ones; the four metrics and the three row dtypes rotate over the rows
TABLE = [(1100, 5, "cosine", "f32"), (1100, 20, "dot", "f16"), (1100, 5, "rbf", "bf16"), (1100, 20, "neg_sq_l2", "f32"),
         (1300, 5, "neg_sq_l2", "f16"), (1300, 20, "rbf", "f32"), (1300, 5, "dot", "f32"), (1300, 20, "cosine", "bf16")]


def gauss(n, d, seed, dtype="f32"):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, d).astype(np.float32)).to(DTYPES[dtype])


@functools.lru_cache(maxsize=None)
def table_rows(d, dtype):
    """The n = 700 Gaussian rows of the kernel-table test (CPU tensor of `dtype`; never written)."""
    return gauss(OFFSETS[-1], d, 700 + d, dtype)


def band_sizes_outside(X, xp, metric, operand, kk):
    """band_sizes of tests/test_gpu_wide_scan.py (the margin formula in the header of mmf_scan_b16w.hip, G in float64) with the band
    taken over each row's ADMISSIBLE columns: the kk-th best G and the count skip the columns of the row's own segment.  Scale and
    maxima are taken over all rows, as the call takes them (plain images of all of X)."""
    f = np.float32
    X = np.ascontiguousarray(X.float().numpy(), f)
    d = X.shape[1]
    dp = (d + 127) // 128 * 128
    scal = R.row_scalars(X, metric)
    scale = R.common_scale(float(R.sq_norms(X).max()), metric)
    u = ((X / scal[:, None]).astype(f) if metric == R.COSINE else X) * scale
    u = u.astype(f)
    z = u.astype(np.float16).astype(f) if operand == "f16" else R.bf16_to_f32(R.round_bf16(u))
    z64, u64 = z.astype(np.float64), u.astype(np.float64)
    norm = lambda v: np.sqrt((v * v).sum(axis=1).astype(f)) * R.UP   # noqa: E731
    zn, rn, un = norm(z64), norm((z - u).astype(np.float64)), norm(u64)
    cb = (f(-0.5) * scal * scale * scale).astype(f) if metric in (R.NEG_SQ_L2, R.RBF) else np.zeros(X.shape[0], f)
    ZB, RB, UB, CB = zn.max(), rn.max(), un.max(), np.abs(cb).max()
    g_acc, g_chain = f(dp + 8) * R.EPS24, f(d + 2) * R.EPS24
    e1 = rn * ZB + un * RB + g_acc * (zn * ZB + CB)
    if metric == R.DOT:
        e2 = g_chain * un * UB
    elif metric == R.COSINE:
        e2 = (g_chain + f(4.7683716e-7)) * un * UB * f(1.01)
    else:
        e2 = g_chain * un * UB + f(2.3841858e-7) * (un * un + UB * UB)
    margin = (f(2.0) * (e1 + e2) * f(1.001) + f(1e-30)).astype(np.float64)
    G = cb.astype(np.float64)[None, :] + z64 @ z64.T
    if xp is not None:
        seg = np.searchsorted(np.asarray(xp), np.arange(X.shape[0]), side="right") - 1
        G[seg[:, None] == seg[None, :]] = -np.inf
    t = -np.partition(-G, kk - 1, axis=1)[:, kk - 1]
    return (G >= (t - margin)[:, None]).sum(axis=1)


def test_the_band_count_is_the_wide_scans_helper_when_nothing_is_excluded():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_wide_scan import band_sizes
    X = table_rows(1100, "f32")[:200]
    for metric, operand, kk in (("cosine", "f16", 6), ("neg_sq_l2", "bf16", 20)):
        assert np.array_equal(band_sizes_outside(X, None, metric, operand, kk), band_sizes(X, metric, operand, kk))


@pytest.mark.parametrize("d,k,metric,dtype", TABLE)
def test_no_row_of_the_gpu_table_has_a_band_beyond_its_lists_with_f16_operands(d, k, metric, dtype):
    """'band <= capacity => never flagged' (header of mmf_scan_b16w.hip; §4.26 Margin: over the admissible columns): with f16
    operands every row of the GPU kernel table has at most 16 (k = 5) / 32 (k = 20) columns in its band, so fallback_rows == 0 there
    is a claim about the scan, not about the data."""
    cap = 16 if k <= 11 else 32
    band = band_sizes_outside(table_rows(d, dtype), OFFSETS, metric, "f16", k)
    print(f"d {d} k {k} {metric} {dtype}: largest band {int(band.max())} of capacity {cap}")
    assert band.min() >= k and band.max() <= cap
