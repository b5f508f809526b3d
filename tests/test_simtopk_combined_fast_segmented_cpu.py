"""The segmented 16-bit top-k of the combined similarity without a GPU (mmf_simtopk_combined_fast_segmented,
include/ext/mmf_hg_topk16_seg.h): the header declares exactly the one entry, the library exports it and the
binding registers it in a list of its own, the entry runs its host checks before any device call and names the argument, the
Python layer raises its argument errors on the host, the static stream scan reads the new launcher and driver, the documents name
the feature, and on every batch of the GPU capacity test no row's restated band (tests/combined16_seg_restate.py) exceeds its
list capacity."""
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
ENTRY = "mmf_simtopk_combined_fast_segmented"
HEADER = os.path.join(ROOT, "include", "ext", "mmf_hg_topk16_seg.h")


def _mod():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16_segmented")


def _declared(path):
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding ----------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_and_no_other_header_does():
    assert _declared(HEADER) == {ENTRY}
    inc = os.path.join(ROOT, "include")
    for h in os.listdir(inc):
        if h.endswith(".h"):
            assert ENTRY not in _declared(os.path.join(inc, h)), h
    with open(HEADER) as f:
        h = f.read()
    assert '#include "../mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    for words in ("bit for bit", "k + self <= 20", "1 <= d <= 4096", "dp <= 8", "MMF_PREC_FAST_BF16", "Host-synchronous",
                  "multiple of 128", "0 (automatic: at most two) or a power of two", "id -1 and value -inf"):
        assert words in h, words
    with open(os.path.join(inc, "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()                  # additions only


def test_library_and_binding_export_the_entry_from_a_list_of_its_own():
    import multimodal_fusion_amd as mmf
    lb = mmf._lib
    L = ctypes.CDLL(lb.SO_PATH)
    assert list(lb.EXPORTS_TOPK16_SEG) == [ENTRY] and hasattr(L, ENTRY)
    assert list(lb.EXPORTS_TOPK16) == ["mmf_simtopk_combined_fast"]
    others = (set(lb.EXPORTS) | set(lb.EXPORTS_COHORT) | set(lb.EXPORTS_POOL) | set(lb.EXPORTS_STREAM) | set(lb.EXPORTS_TOPK)
              | set(lb.EXPORTS_WIDE) | set(lb.EXPORTS_WIDE_SEG) | set(lb.EXPORTS_TOPK16))
    assert ENTRY not in others
    fn = getattr(lb.lib(), ENTRY)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17
    assert list(fn.argtypes) == list(lb.lib().mmf_simtopk_combined.argtypes)
    assert lb.ABI_VERSION == 3 and lb.lib().mmf_version() == 3


def test_build_lists_the_new_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_topk16_seg", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", "ext", "mmf_hg_topk16_seg.h")) for h in b.HEADERS)
    assert "mmf_scan_b16c.hip" in b.SOURCES and "mmf_scan_b16c.hip" not in b.EXTRA_FLAGS


def test_module_and_functions_are_exported():
    import multimodal_fusion_amd as mmf
    m = _mod()
    assert "combined_topk16_segmented" in mmf.__all__ and mmf.combined_topk16_segmented is m
    names = {"simtopk_combined_fast_segmented", "build_topk_weighted_hypergraph_fast_segmented", "build_topk_hypergraph_data_fast"}
    for name in names:
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
        assert not hasattr(mmf.ops, name) and not hasattr(mmf.combined_topk, name) and not hasattr(mmf.combined_topk16, name)
    public = {n for n, fn in inspect.getmembers(m, inspect.isfunction) if fn.__module__ == m.__name__ and not n.startswith("_")}
    assert public == names
    sig = inspect.signature(m.simtopk_combined_fast_segmented)
    assert list(sig.parameters) == ["features", "positions", "lambda_h", "lambda_g", "k", "ptr", "batch", "exclude_self", "precision",
                                    "col_splits", "return_stats", "profile"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [1.0, 1.0, 5, None, None, True, "auto", 0, False, False]
    sig = inspect.signature(m.build_topk_weighted_hypergraph_fast_segmented)
    assert list(sig.parameters) == ["features", "positions", "lambda_h", "lambda_g", "k", "device", "ptr", "batch", "precision"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("ptr", "batch", "precision"))
    assert sig.parameters["precision"].default == "auto"
    sig = inspect.signature(m.build_topk_hypergraph_data_fast)
    assert list(sig.parameters) == ["features", "positions", "lambda_h", "lambda_g", "k", "use_pooling", "device", "ptr", "batch", "precision"]


# ---- the entry's host checks, with host buffers standing in for device pointers ------------------------------------------
def _call(**kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(F=b, P=b, n=4, d=4, dp=2, lh=1.0, lg=1.0, k=2, self=1, ptr=[0, 1, 4], S=2, idx=b, val=b, opts=(2, 0, 0, 0, None), device=63)
    a.update(kw)
    ptr = a["ptr"]
    if ptr is not None:
        ptr = ctypes.cast((ctypes.c_int64 * len(ptr))(*ptr), ctypes.c_void_p)
    opts = a["opts"]
    if opts is not None:
        opts = ctypes.byref(mmf._lib.SimtopkOpts(*opts))
    rc = getattr(L, ENTRY)(a["F"], a["P"], a["n"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], ptr, a["S"], a["idx"], a["val"], opts,
                           None, a["device"], None)
    return rc, L.mmf_last_error().decode()


INVALID = [
    (dict(F=None), "F is NULL"),
    (dict(P=None), "P is NULL"),
    (dict(idx=None), "out_idx is NULL"),
    (dict(val=None), "out_val is NULL"),
    (dict(n=-1), "n must be >= 0"),
    (dict(d=0), "d must be at least 1"),
    (dict(dp=0), "dp must be at least 1"),
    (dict(k=0), "k must be at least 1"),
    (dict(lh=-0.5), "lambda_h must be finite and >= 0"),
    (dict(lh=float("inf")), "lambda_h must be finite and >= 0"),
    (dict(lg=-1.0), "lambda_g must be finite and >= 0"),
    (dict(lg=float("nan")), "lambda_g must be finite and >= 0"),
    (dict(ptr=None, S=2), "host offsets ptr_host[n_seg + 1]"),
    (dict(ptr=None, S=0), "host offsets ptr_host[n_seg + 1]"),
    (dict(ptr=[0, 4], S=-1), "need n_seg >= 0"),
    (dict(ptr=[1, 2, 4]), "ptr_host must start at 0"),
    (dict(ptr=[0, 3, 2, 4], S=3), "ptr_host decreases at segment 1"),
    (dict(ptr=[0, 1, 3]), "ptr_host must end at 4 (got 3)"),
    (dict(opts=(7, 0, 0, 0, None)), "precision 7"),
    (dict(opts=(2, 0, -1, 0, None)), "col_splits must be 0 or a power of two (got -1)"),
    (dict(opts=(2, 0, 3, 0, None)), "col_splits must be 0 or a power of two (got 3)"),
    (dict(opts=(1, 0, 6, 0, None)), "col_splits must be 0 or a power of two (got 6)"),
]
UNSUPPORTED = [
    (dict(dp=9), "dp = 9 > 8"),
    (dict(k=20), "k + self = 21 > 20"),
    (dict(k=21, self=0), "k + self = 21 > 20"),
    (dict(d=4097), "d = 4097 > 4096"),
    (dict(n=1 << 31, ptr=[0, 1 << 31], S=1), "n must be < 2^31"),
]


@pytest.mark.parametrize("kw,words", INVALID)
def test_entry_refuses_bad_arguments_before_any_device_call(kw, words):
    """A device id that does not exist: an argument error must win over the device's."""
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and "simtopk_combined_fast_segmented" in msg, (rc, msg)


@pytest.mark.parametrize("kw,words", UNSUPPORTED)
def test_entry_refuses_what_it_does_not_support_before_any_device_call(kw, words):
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and words in msg and "simtopk_combined_fast_segmented" in msg, (rc, msg)


def test_the_order_of_the_checks():
    """The argument checks first, then the offsets, then what is unsupported, then the options — the order of
    mmf_simtopk_combined_fast with mmf_simtopk_combined's offsets check in the place of its ragged-batch refusal."""
    import multimodal_fusion_amd as mmf
    inv, uns = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    assert _call(k=0, ptr=[1, 4], S=1)[1].count("k must be at least 1") == 1
    rc, msg = _call(ptr=[1, 4], S=1, dp=9)
    assert rc == inv and "must start at 0" in msg
    rc, msg = _call(dp=9, opts=(7, 0, 0, 0, None))
    assert rc == uns and "dp = 9 > 8" in msg
    rc, msg = _call(opts=(7, 0, 3, 0, None))
    assert rc == inv and "precision 7" in msg


def test_entry_refuses_a_negative_device_first():
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(k=0), dict(F=None), dict(dp=9), dict(ptr=None), dict(d=4097)):
        rc, msg = _call(device=-1, **kw)
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and "no CPU path" in msg and "simtopk_combined_fast_segmented" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """Every precision, zero lambdas, the limits themselves, empty segments, forced splits: the call gets as far as the device
    (which is not there).  n == 0 returns before it."""
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(opts=None), dict(opts=(0, 0, 0, 0, None)), dict(opts=(1, 0, 0, 0, None)), dict(opts=(3, 1, 4, 0, None)),
               dict(lh=0.0, lg=0.0), dict(k=19), dict(k=20, self=0), dict(dp=8), dict(d=4096), dict(ptr=[0, 0, 4, 4], S=3),
               dict(ptr=[0, 4], S=1), dict(opts=(2, 0, 32, 0, None))):
        rc, msg = _call(**kw)
        assert rc == mmf._lib.MMF_E_HIP, (kw, rc, msg)
    assert _call(n=0, ptr=[0], S=0)[0] == mmf._lib.MMF_OK
    assert _call(n=0, ptr=[0, 0, 0], S=2, F=None, P=None, idx=None, val=None)[0] == mmf._lib.MMF_OK


def test_the_one_graph_entry_still_refuses_a_ragged_batch():
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    b = ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)
    ptr = ctypes.cast((ctypes.c_int64 * 3)(0, 2, 4), ctypes.c_void_p)
    rc = L.mmf_simtopk_combined_fast(b, b, 4, 4, 2, 1.0, 1.0, 2, 1, ptr, 2, b, b, None, None, 63, None)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and "stays on mmf_simtopk_combined" in L.mmf_last_error().decode()


# ---- the Python layer's argument errors, on the host ------------------------------------------------------------------
def test_wrapper_rejects_bad_input_before_any_library_call(monkeypatch):
    import multimodal_fusion_amd as mmf
    m = _mod()

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    ptr = torch.tensor([0, 4, 10])
    for f in (m.simtopk_combined_fast_segmented, m.build_topk_weighted_hypergraph_fast_segmented, m.build_topk_hypergraph_data_fast):
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:9], ptr=ptr)
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:, 0], ptr=ptr)
        with pytest.raises(ValueError, match=r"k must be >= 1 \(got 0\)"):
            f(F, P, k=0, ptr=ptr)
        with pytest.raises(ValueError, match="unknown precision 'half'"):
            f(F, P, precision="half", ptr=ptr)
        with pytest.raises(ValueError, match="give exactly one of ptr / batch"):
            f(F, P)
        with pytest.raises(ValueError, match="give exactly one of ptr / batch"):
            f(F, P, ptr=ptr, batch=torch.zeros(10, dtype=torch.int64))
        with pytest.raises(ValueError, match="ptr must end at 10"):
            f(F, P, ptr=torch.tensor([0, 4, 9]))
        with pytest.raises(ValueError, match="ptr decreases"):
            f(F, P, ptr=torch.tensor([0, 6, 4, 10]))
        with pytest.raises(ValueError, match="batch must be sorted"):
            f(F, P, batch=torch.tensor([0, 0, 1, 0, 1, 1, 1, 1, 1, 1]))
        with pytest.raises(ValueError, match=f.__name__ + ":"):
            f(F, P, ptr=torch.tensor([1, 10]))
    for cs in (-1, 3, 6):
        with pytest.raises(ValueError, match="col_splits must be 0 or a power of two"):
            m.simtopk_combined_fast_segmented(F, P, ptr=ptr, col_splits=cs)


def test_without_a_gpu_the_wrapper_raises(monkeypatch):
    m = _mod()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    for f in (m.simtopk_combined_fast_segmented, m.build_topk_weighted_hypergraph_fast_segmented):
        with pytest.raises(RuntimeError, match="ROCm"):
            f(F, P, ptr=[0, 4, 10])


# ---- static stream scan ------------------------------------------------------------------------------------------------
def _body(text, name):
    return text.split("int " + name + "(", 1)[1].split("\n}\n", 1)[0]


def _offset(text, line):
    return sum(len(x) + 1 for x in text.split("\n")[:line - 1])


def test_launcher_and_driver_name_the_callers_stream_and_nothing_blocks():
    from test_stream_arguments_cpu import BLOCKING, BLOCKING_ALLOWED, enclosing, is_null, sources, stream_uses
    src = dict(sources())
    text, api = src["mmf_scan_b16c.hip"], src["mmf_api.hip"]
    for inst in ("scan_b16c_kernel<true, CAP, true>", "scan_b16c_kernel<false, CAP, true>", "launch_b16c_t<C_CAP_SMALL, true>",
                 "launch_b16c_t<C_CAP_BIG, true>", "template <bool F16, int CAP, bool SEG = false>"):
        assert inst in text, inst
    # the launcher: both launches (the scan through launch_b16c_t, the seed union) on the stream it was given
    mine = [u for u in stream_uses() if u[0] == "mmf_scan_b16c.hip" and enclosing(text, _offset(text, u[1])) == "launch_scan_b16c_seg"]
    assert [a[0] for _, _, what, _, a in mine if what == "hipLaunchKernelGGL"] == ["comb_seed_union_kernel"]
    assert all(u[3] == "s" for u in mine)
    launcher = _body(text, "launch_scan_b16c_seg")
    assert "launch_b16c_t<C_CAP_SMALL, true>(a, p.f16, grid, s)" in launcher and "launch_b16c_t<C_CAP_BIG, true>(a, p.f16, grid, s)" in launcher
    assert not [u for u in stream_uses() if u[0] == "mmf_scan_b16c.hip" and is_null(u[3])]
    assert not [m for m in BLOCKING.finditer(text) if not m.group(1).endswith("Async")]
    # the driver: every runtime call is asynchronous and names the call's stream; one explicit synchronisation, taken only when
    # more than 1024 rows were flagged (the clean path's one synchronisation is FlagBlock::read's)
    body = _body(api, "run_simtopk_combined_fast_segmented")
    assert not [m for m in BLOCKING.finditer(body) if not m.group(1).endswith("Async")]
    assert body.count("hipStreamSynchronize(s)") == 1 and body.index("if (h_fail > peek)") < body.index("hipStreamSynchronize(s)")
    assert body.count("flags.read(") == 1 and "hipDeviceSynchronize" not in body
    for call in ("launch_scan_b16c_seg(", "launch_rerank_combined(", "launch_scan_b16_audit(", "launch_prep_half_gather(", "upload_table(s,"):
        assert call in body, call
    assert body.count("launch_prep_half_gather(") == 1 and body.count("launch_scan_b16c_seg(") == 1
    raw = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")).read()
    assert "MMF_DEBUG_FLAG_ROWS" in _body(raw, "run_simtopk_combined_fast_segmented")
    mine = [u for u in stream_uses() if u[0] == "mmf_api.hip" and enclosing(api, _offset(api, u[1])) == "run_simtopk_combined_fast_segmented"]
    assert len(mine) >= 10 and all(u[3] == "s" for u in mine), mine
    assert not [k for k in BLOCKING_ALLOWED if "combined" in k[1] or "b16c" in k[1]]          # the allow-list was not extended


def test_the_pinned_files_and_the_one_graph_driver_are_not_edited():
    csrc = os.path.join(ROOT, "multimodal-fusion_amd", "csrc")
    for name in ("mmf_scan_b16w.hip", "mmf_scan_bf16.hip", "mmf_scan_f32.hip", "mmf_select.hip", "mmf_topk.hip", "mmf_prep.hip"):
        with open(os.path.join(csrc, name)) as f:
            src = f.read()
        assert "b16c" not in src and "combined_fast" not in src, name
    with open(os.path.join(csrc, "mmf_api.hip")) as f:
        api = f.read()
    one = _body(api, "run_simtopk_combined_fast")
    assert "launch_scan_b16c(sp, sc, splits, L, pnl, s, &grid)" in one and "_seg" not in one and "sched" not in one
    with open(os.path.join(csrc, "mmf_scan_b16c.hip")) as f:
        k = f.read()
    assert k.index("const int32_t* sched;") > k.index("float* margin_out;") and "sched;" in k.split("float* margin_out;", 1)[1].split("};", 1)[0]


# ---- documents -------------------------------------------------------------------------------------------------------
def _seg_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Segmented 16-bit top-k entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_table_equals_the_gpu_tests_table():
    from test_gpu_simtopk_combined_fast_segmented import SYNC
    import multimodal_fusion_amd as mmf
    rows = _seg_table()
    assert rows == SYNC == {ENTRY: ("data-dependent", "the call")}, (rows, SYNC)
    assert set(rows) == set(mmf._lib.EXPORTS_TOPK16_SEG)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    one_graph = re.search(r"^## [0-9. ]*16-bit top-k entries$", text, flags=re.M)
    assert one_graph and one_graph.start() < text.index("Segmented 16-bit top-k entries")       # a section of its own, after it


def test_design_readme_and_scripts_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design.split("## 4.18", 1)[1]
    for words in ("Contract", "Kernel flag and table", "Margin", "superset", "Resources", "ScratchSize", "Measurements", "Decisions",
                  "MMF_PREC_AUTO", "Cut", "instruction for instruction"):
        assert words in sec, words
    assert "simtopk_combined_fast_segmented" in design.split("## 4", 1)[0]          # §1's table has the row
    assert "§4.18" in design.split("## 4.17", 1)[1].split("## 4.18", 1)[0]          # §4.17's Cut points here
    with open(os.path.join(ROOT, "README.md")) as f:
        r = f.read()
    assert "simtopk_combined_fast_segmented" in r and "build_topk_weighted_hypergraph_fast_segmented" in r
    assert os.path.exists(os.path.join(ROOT, "scripts", "simtopk_combined_fast_segmented_timing.py"))
    with open(os.path.join(ROOT, "profiles", "simtopk_combined_fast_segmented_timing.txt")) as f:
        assert "simtopk_combined_fast_segmented" in f.read()


# ---- the capacity condition of the GPU test, on the CPU ----------------------------------------------------------------
def test_the_restatement_of_one_segment_is_the_one_graph_restatement():
    import combined16_restate as cr
    import combined16_seg_restate as sr
    F, P, ptr = sr.batch([0, 200, 0], 40, 2, 3)
    assert ptr.tolist() == [0, 0, 200, 200]
    F1, P1 = cr.make_data(200, 40, 2, 4)
    assert np.array_equal(F, F1) and np.array_equal(P, P1)
    for operand in ("f16", "bf16"):
        a, b = sr.bands_segmented(F, P, ptr, 0.5, 2e-7, 6, operand), cr.bands(F, P, 0.5, 2e-7, 6, operand)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_no_band_of_the_capacity_batches_exceeds_its_capacity(operand):
    """What tests/test_gpu_simtopk_combined_fast_segmented.py's capacity test relies on: with scale, maxima and the largest pn taken
    over the whole batch, no row's band inside its own segment holds more columns than its lists."""
    import combined16_restate as cr
    import combined16_seg_restate as sr
    from test_gpu_simtopk_combined_fast_segmented import CAPACITY_BATCHES, CAP_SEED, LG, LH
    for sizes, d, dp in CAPACITY_BATCHES:
        F, P, ptr = sr.batch(sizes, d, dp, CAP_SEED)
        for kk in (6, 11, 12, 20):
            _, _, cnt = sr.bands_segmented(F, P, ptr, LH, LG, kk, operand)
            cap = cr.capacity(kk)
            print(f"{sizes} d {d} dp {dp} {operand} k + self {kk}: largest band {int(cnt.max())} of {cap}")
            assert int((cnt > cap).sum()) == 0, (sizes, d, kk)
