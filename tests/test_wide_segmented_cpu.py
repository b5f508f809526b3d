"""The segmented wide 16-bit scan without a GPU (include/mmf_hg_wide_seg.h): the header declares exactly the one
entry, the library exports it and the binding registers it in a list of its own, the entry runs its host checks before any device
call and names itself, the Python wrapper raises its argument errors on the host, INTEGRATION.md's table has the entry's row, and
every kernel launch the feature adds is on the caller's stream."""
import ctypes
import inspect
import os
import re
import sys
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_simtopk_segmented_wide"]
OTHER_HEADERS = ["mmf_hg.h", "mmf_hg_pool.h", "mmf_hg_stream.h", "mmf_hg_topk.h", "mmf_hg_wide.h"]
SYNC_WIDE_SEG = {"mmf_simtopk_segmented_wide": ("data-dependent", "until the call returns")}


def _ws():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.wide_scan")


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding, build ------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry():
    assert _declared("mmf_hg_wide_seg.h") == set(ENTRIES)
    for h in OTHER_HEADERS:
        assert not _declared(h) & set(ENTRIES), h
    with open(os.path.join(ROOT, "include", "mmf_hg_wide_seg.h")) as f:
        h = f.read()
    assert '#include "mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    for words in ("bit for bit", "row_offset = x_ptr[s] and col_offset = y_ptr[s]", "1024 < d <= 4096", "k + self <= 20",
                  "power of two", "select_wait_event is refused", "before any device call", "device_id < 0 -> MMF_E_UNSUPPORTED first"):
        assert words in h, words                                                                         # the contract
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()                                                 # additions only


def test_library_and_binding_export_the_entry_from_a_list_of_its_own():
    import multimodal_fusion_amd as mmf
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_WIDE_SEG) == ENTRIES and hasattr(L, ENTRIES[0])
    assert list(mmf._lib.EXPORTS_WIDE) == ["mmf_wide_scan_supported", "mmf_wide_scan_list_capacity"]   # still the two queries
    others = (set(mmf._lib.EXPORTS) | set(mmf._lib.EXPORTS_COHORT) | set(mmf._lib.EXPORTS_POOL) | set(mmf._lib.EXPORTS_STREAM)
              | set(mmf._lib.EXPORTS_TOPK) | set(mmf._lib.EXPORTS_WIDE))
    assert not set(ENTRIES) & others
    lib = mmf._lib.lib()
    fn = lib.mmf_simtopk_segmented_wide
    assert fn.restype is ctypes.c_int and tuple(fn.argtypes) == tuple(lib.mmf_simtopk_segmented.argtypes) and len(fn.argtypes) == 19
    assert mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_build_lists_the_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_wide_seg", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", "mmf_hg_wide_seg.h")) for h in b.HEADERS)
    assert any(h.endswith(os.path.join("include", "mmf_hg_wide.h")) for h in b.HEADERS) and "mmf_scan_b16w.hip" in b.SOURCES


def test_the_function_lives_in_wide_scan_and_adds_no_top_level_name():
    import multimodal_fusion_amd as mmf
    ws = _ws()
    assert mmf.wide_scan is ws and mmf.simtopk_segmented is mmf.ops.simtopk_segmented
    sig = inspect.signature(ws.simtopk_segmented)
    assert list(sig.parameters) == ["X", "Y", "ptr", "batch", "y_ptr", "y_batch", "metric", "lam", "k", "exclude_self", "precision",
                                    "col_splits", "return_stats", "profile"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    assert sig.parameters["precision"].default == "auto" and sig.parameters["col_splits"].default == 0
    ops_sig = inspect.signature(mmf.ops.simtopk_segmented)
    assert [n for n in sig.parameters if n != "col_splits"] == list(ops_sig.parameters)
    assert "col_splits" not in ops_sig.parameters and not hasattr(mmf.ops, "wide_scan")


# ---- the entry's host checks, with host buffers standing in for device pointers ------------------------------------------
def _call(**kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(X=b, n=8, Y=None, m=0, d=1536, dtype=0, metric=1, lam=1.0, k=2, self=1, xp=[0, 3, 8], yp=None, S=2, idx=b, val=b,
             opts=None, device=63)
    a.update(kw)
    xp, yp = a["xp"], a["yp"]
    xp = None if xp is None else ctypes.cast((ctypes.c_int64 * len(xp))(*xp), ctypes.c_void_p)
    yp = None if yp is None else ctypes.cast((ctypes.c_int64 * len(yp))(*yp), ctypes.c_void_p)
    opts = a["opts"]
    if opts is not None:
        opts = ctypes.byref(mmf._lib.SimtopkOpts(*opts))
    rc = L.mmf_simtopk_segmented_wide(a["X"], a["n"], a["Y"], a["m"], a["d"], a["dtype"], a["metric"], a["lam"], a["k"], a["self"], xp, yp,
                                      a["S"], a["idx"], a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


EVENT = ctypes.c_void_p(8)          # any non-NULL select_wait_event
INVALID = [
    (dict(xp=[1, 3, 8]), "x_ptr must start at 0"),
    (dict(xp=[0, 5, 3, 8], S=3), "x_ptr decreases at segment 1"),
    (dict(xp=[0, 3, 7]), "x_ptr must end at 8"),
    (dict(xp=None), "host offsets x_ptr"),
    (dict(Y=ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p), m=6, yp=[0, 2, 5]), "y_ptr must end at 6"),
    (dict(k=0), "k must be >= 1"),
    (dict(idx=None), "NULL output"),
    (dict(val=None), "NULL output"),
    (dict(opts=(0, 0, 3, 0, None)), "col_splits must be 0 or a power of two (got 3)"),
    (dict(opts=(2, 0, -2, 0, None)), "col_splits must be 0 or a power of two"),
]
UNSUPPORTED = [
    (dict(d=512, opts=(0, 0, 2, 0, None)), "col_splits and select_wait_event are not supported"),      # outside the wide range
    (dict(opts=(1, 0, 2, 0, None)), "col_splits and select_wait_event are not supported"),             # exact: the narrow entry's options
    (dict(opts=(0, 0, 0, 0, EVENT)), "select_wait_event is not supported"),
    (dict(d=512, opts=(0, 0, 0, 0, EVENT)), "select_wait_event"),
    (dict(k=20, opts=(2, 0, 0, 0, None)), "does not support d = 1536, k = 20"),                        # k + self = 21
    (dict(k=21, self=0, opts=(3, 0, 0, 0, None)), "does not support"),
    (dict(d=4097, opts=(2, 0, 0, 0, None)), "does not support d = 4097"),
    (dict(d=4097, opts=(3, 0, 0, 0, None)), "does not support d = 4097"),
    (dict(k=44), "k + self = 45 > 44"),
]


@pytest.mark.parametrize("kw,words", INVALID)
def test_entry_refuses_bad_arguments_before_any_device_call(kw, words):
    """A device id that does not exist: an argument error must win over the device's."""
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and "simtopk_segmented_wide" in msg, (rc, msg)


@pytest.mark.parametrize("kw,words", UNSUPPORTED)
def test_entry_refuses_what_it_does_not_support_before_any_device_call(kw, words):
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and words in msg and "simtopk_segmented_wide" in msg, (rc, msg)


def test_entry_refuses_a_negative_device_first():
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(k=0), dict(xp=[1, 3, 8]), dict(idx=None), dict(opts=(0, 0, 3, 0, None)), dict(d=4097, opts=(2, 0, 0, 0, None))):
        rc, msg = _call(device=-1, **kw)
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and "no CPU path" in msg and "simtopk_segmented_wide" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """Power-of-two col_splits in the wide range, every precision, k + self = 20, the narrow range without options: the call gets as
    far as the device (which is not there).  n == 0 returns before it."""
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(opts=(0, 0, 4, 0, None)), dict(opts=(2, 1, 16, 0, None)), dict(opts=(3, 0, 1, 0, None)), dict(opts=(1, 0, 0, 0, None)),
               dict(k=19), dict(d=512), dict(d=4096), dict(d=4097), dict(xp=[0, 0, 8])):
        rc, msg = _call(**kw)
        assert rc == mmf._lib.MMF_E_HIP, (kw, rc, msg)
    assert _call(n=0, xp=[0, 0, 0])[0] == mmf._lib.MMF_OK
    assert _call(n=0, xp=[0], S=0, X=None, idx=None, val=None)[0] == mmf._lib.MMF_OK


def test_the_narrow_entry_keeps_its_texts():
    """mmf_simtopk_segmented shares the body: its name in its messages, col_splits refused at every d."""
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)
    xp = ctypes.cast((ctypes.c_int64 * 3)(0, 3, 8), ctypes.c_void_p)
    for d in (512, 1536):
        opts = mmf._lib.SimtopkOpts(0, 0, 2, 0, None)
        rc = L.mmf_simtopk_segmented(buf, 8, None, 0, d, 0, 1, 1.0, 2, 1, xp, None, 2, buf, buf, ctypes.byref(opts), None, 63, None)
        msg = L.mmf_last_error().decode()
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and msg == "simtopk_segmented: col_splits and select_wait_event are not supported", (rc, msg)
    # ... and outside the wide scan's shapes the wide entry says the same under its own name
    opts = mmf._lib.SimtopkOpts(0, 0, 2, 0, None)
    rc = L.mmf_simtopk_segmented_wide(buf, 8, None, 0, 512, 0, 1, 1.0, 2, 1, xp, None, 2, buf, buf, ctypes.byref(opts), None, 63, None)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED
    assert L.mmf_last_error().decode() == "simtopk_segmented_wide: col_splits and select_wait_event are not supported"


# ---- the wrapper's argument errors, on the host ---------------------------------------------------------------------
def test_wrapper_rejects_bad_input_before_any_library_call(monkeypatch):
    import multimodal_fusion_amd as mmf
    f = _ws().simtopk_segmented

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    X = torch.randn(10, 1536)
    with pytest.raises(ValueError, match="expected a 2-D"):
        f(X[0], ptr=[0, 10])
    with pytest.raises(ValueError, match="must share device, dtype and feature dim"):
        f(X, torch.randn(4, 1535), ptr=[0, 10], y_ptr=[0, 4])
    with pytest.raises(ValueError, match=r"k must be >= 1 \(got 0\)"):
        f(X, ptr=[0, 10], k=0)
    with pytest.raises(ValueError, match="unknown precision 'half'"):
        f(X, ptr=[0, 10], precision="half")
    with pytest.raises(ValueError, match=r"col_splits must be 0 or a power of two \(got 3\)"):
        f(X, ptr=[0, 10], col_splits=3)
    with pytest.raises(ValueError, match="y_ptr / y_batch need Y"):
        f(X, ptr=[0, 10], y_ptr=[0, 10])
    with pytest.raises(ValueError, match=r"ptr must end at 10 \(got 9\)"):
        f(X, ptr=[0, 4, 9])
    with pytest.raises(ValueError, match="ptr must start at 0"):
        f(X, ptr=[1, 10])
    with pytest.raises(ValueError, match="batch must be sorted"):
        f(X, batch=torch.tensor([0, 0, 1, 0, 1, 1, 2, 2, 2, 2]))
    with pytest.raises(ValueError):
        f(X, ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long))


def test_without_a_gpu_the_wrapper_raises():
    f = _ws().simtopk_segmented
    X = torch.randn(10, 1536)
    for kw in (dict(ptr=[0, 4, 10]), dict(ptr=[0, 10], precision="fast", col_splits=2), dict(batch=torch.zeros(10, dtype=torch.long))):
        with pytest.raises(RuntimeError, match="ROCm"):
            f(X, **kw)
    with pytest.raises(RuntimeError, match="ROCm"):
        f(X, torch.randn(6, 1536), ptr=[0, 4, 10], y_ptr=[0, 6, 6])


# ---- documents -------------------------------------------------------------------------------------------------------
def _wide_seg_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Wide segmented entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_table_has_exactly_the_new_entrys_row():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import multimodal_fusion_amd as mmf
    rows = _wide_seg_table()
    assert rows == SYNC_WIDE_SEG, rows
    assert set(rows) == set(mmf._lib.EXPORTS_WIDE_SEG)
    from test_stream_arguments_cpu import integration_table
    assert integration_table()["mmf_simtopk_segmented"] == rows["mmf_simtopk_segmented_wide"]        # as the narrow entry
    from test_simtopk_combined_cpu import _topk_table
    from test_super_patch_stats_streamed_cpu import _stream_table
    from test_super_patches_segmented_cpu import _pool_table
    from test_wsi_tma_segmented_cpu import _cohort_table
    assert not (set(integration_table()) | set(_cohort_table()) | set(_pool_table()) | set(_stream_table()) | set(_topk_table())) & set(rows)


def test_new_kernel_launches_are_on_the_callers_stream():
    """The static scan of tests/test_stream_arguments_cpu.py over the wide scan's file: the segmented launcher's two launches (the SEG
    instantiations through launch_b16w_t, the threshold union) pass the caller's stream like the plain launcher's, nothing in the
    file blocks, and the shared body in mmf_api.hip reaches the launcher with the call's stream."""
    from test_stream_arguments_cpu import BLOCKING, is_null, sources, stream_uses
    uses = [u for u in stream_uses() if u[0] == "mmf_scan_b16w.hip"]
    launches = [u for u in uses if u[2] == "hipLaunchKernelGGL"]
    assert len(launches) == 3 and not [u for u in uses if is_null(u[3])]          # launch_b16w_t's, and one union per launcher
    assert sum("wide_seed_union_kernel" in u[4][0] for u in launches) == 2
    text = dict(sources())["mmf_scan_b16w.hip"]
    assert not [m for m in BLOCKING.finditer(text) if not m.group(1).endswith("Async")]
    assert "launch_b16w_t<W_CAP_SMALL, true>(a, p.f16, grid, s)" in text and "launch_b16w_t<W_CAP_BIG, true>(a, p.f16, grid, s)" in text
    assert "scan_b16w_kernel<true, CAP, SEG>" in text and "scan_b16w_kernel<false, CAP, SEG>" in text
    api = dict(sources())["mmf_api.hip"]
    assert "launch_scan_b16w_seg(sp, d_sched, grid, lists, L, pn, s)" in api and "const hipStream_t s = r.call.s;" in api
    assert not [u for u in stream_uses() if u[0] == "mmf_api.hip" and is_null(u[3])]


def test_design_readme_and_scripts_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design.split("4.16", 1)[1]
    for words in ("SEG", "work table", "Column splits", "scratch", "instruction", "Measurements", "Routing", "Cuts"):
        assert words in sec, words
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "wide_scan.simtopk_segmented" in f.read()
    with open(os.path.join(ROOT, "scripts", "README.md")) as f:
        assert "wide_segmented_timing.py" in f.read()
    assert os.path.exists(os.path.join(ROOT, "scripts", "wide_segmented_timing.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "wide_segmented_timing.txt"))
