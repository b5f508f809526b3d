"""Streamed super-patch statistics without a GPU: include/mmf_hg_stream.h declares exactly the two streaming entries, the library
exports them and the binding registers them in a fourth list that shares no name with the other three, the entry runs its host
checks before any device call and names the argument, the workspace formula has no term in n^2 beyond the median's own 5 %, the
Python wrapper raises its argument errors on the host, and INTEGRATION.md's streaming table equals the GPU test's."""
import ctypes
import os
import re
import sys
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_super_patch_stats_streamed", "mmf_super_patch_stats_streamed_bytes"]
MIB, GIB = 1 << 20, 1 << 30


def _sps():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.super_patch_stats")


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding ----------------------------------------------------------------------------------------
def test_stream_header_declares_exactly_the_two_entries():
    assert _declared("mmf_hg_stream.h") == set(ENTRIES)
    assert not _declared("mmf_hg.h") & set(ENTRIES) and not _declared("mmf_hg_pool.h") & set(ENTRIES)
    with open(os.path.join(ROOT, "include", "mmf_hg_stream.h")) as f:
        h = f.read()
    assert '#include "mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    assert "preprocess_hypergraph.py:172-197" in h                       # the reference lines the entry replaces
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()                  # additions only


def test_library_and_binding_export_the_entries_from_a_fourth_list():
    import multimodal_fusion_amd as mmf
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_STREAM) == ENTRIES
    assert not set(ENTRIES) & (set(mmf._lib.EXPORTS) | set(mmf._lib.EXPORTS_COHORT) | set(mmf._lib.EXPORTS_POOL))
    for name in ENTRIES:
        assert hasattr(L, name), name
    fn = mmf._lib.lib().mmf_super_patch_stats_streamed
    assert fn.restype is ctypes.c_int and tuple(fn.argtypes[-2:]) == (ctypes.c_int, ctypes.c_void_p) and len(fn.argtypes) == 15
    size = mmf._lib.lib().mmf_super_patch_stats_streamed_bytes
    assert size.restype is ctypes.c_int64 and list(size.argtypes) == [ctypes.c_int64] * 5
    assert mmf._lib.ABI_VERSION == 3 and mmf._lib.lib().mmf_version() == 3
    assert "super_patch_stats" in mmf.__all__ and mmf.super_patch_stats is _sps()


def test_build_lists_the_new_source_and_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mmf_stream_stats.hip" in b.SOURCES and any(h.endswith(os.path.join("include", "mmf_hg_stream.h")) for h in b.HEADERS)


# ---- the entry's host checks, with host buffers standing in for device pointers ------------------------------------------
def _call(**kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(F=b, P=b, n=4, d=4, dp=2, order=b, offsets=b, n_clusters=2, panel_rows=0, intra=b, k_stats=b, device=63)
    a.update(kw)
    rc = L.mmf_super_patch_stats_streamed(a["F"], a["P"], a["n"], a["d"], a["dp"], 1.0, 1.0, a["order"], a["offsets"], a["n_clusters"],
                                          a["panel_rows"], a["intra"], a["k_stats"], a["device"], None)
    return rc, L.mmf_last_error().decode()


BAD_ARGS = [
    (dict(n=1), "n must be at least 2"),
    (dict(n=0), "n must be at least 2"),
    (dict(d=0), "d must be at least 1"),
    (dict(dp=0), "dp must be at least 1"),
    (dict(n_clusters=0), "n_clusters must be at least 1"),
    (dict(F=None), "F is NULL"),
    (dict(P=None), "P is NULL"),
    (dict(k_stats=None), "k_stats is NULL"),
    (dict(offsets=None), "offsets is NULL"),
    (dict(intra=None), "intra_mean is NULL"),
]


@pytest.mark.parametrize("kw,words", BAD_ARGS)
def test_entry_refuses_bad_arguments_before_any_device_call(kw, words):
    """A device id that does not exist: an argument error must win over the device's."""
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and "super_patch_stats_streamed" in msg, (rc, msg)


def test_entry_refuses_a_negative_device_first():
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(n=1), dict(F=None)):
        rc, msg = _call(device=-1, **kw)
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and "no CPU path" in msg, (rc, msg)


def test_without_order_the_clusters_are_not_looked_at():
    """order == NULL: n_clusters, offsets and intra_mean may be anything; the call gets as far as the device (which is not there)."""
    import multimodal_fusion_amd as mmf
    rc, msg = _call(order=None, offsets=None, intra=None, n_clusters=0)
    assert rc == mmf._lib.MMF_E_HIP, (rc, msg)


# ---- the workspace: pure host arithmetic ----------------------------------------------------------------------------
def test_workspace_does_not_grow_with_n_squared(monkeypatch):
    monkeypatch.delenv("MMF_MEDIAN_RADIX", raising=False)
    ws = _sps().streamed_workspace_bytes
    assert ws(262144, 512, 2, 100, 0) < 4 * GIB <= 262144 ** 2 * 4 // 64         # K itself would be 256 GiB
    assert ws(65536, 512, 2, 100) < 4 * GIB
    n, R = 4096, 128
    median = n * n // 20 * 4 + MIB                                       # the one-sweep buffer: 5 % of the values
    assert ws(n, 32, 2, 8, R) < 4 * R * n + 4 * n * 64 + median + 32 * MIB
    # the terms per row (include/mmf_hg_stream.h): 4 bytes of squared norm, 8 of row sum, 4 of cluster id, 4 of member position
    assert ws(2 * n, 32, 2, 8, R) - ws(n, 32, 2, 8, R) < 4 * R * n + 4 * n * 64 + 3 * median + 8 * MIB + 20 * n
    got = [ws(n, 32, 2, 8, r) for r in (1, 128, 129, 333, 1024, n, 2 * n)]
    assert got == sorted(got) and got[0] == got[1] and got[-1] == got[-2] and got[1] < got[2]          # at least 128, at most n rows
    assert ws(n, 32, 2, 8, 0) == ws(n, 32, 2, 8, n)                    # about 1 GiB would be 65536 rows: capped at n
    assert ws(n, 32, 2, 8, R) == ws(n, 32, 2, 3000, R)                 # nothing per cluster
    assert ws(300, 16, 2, 4) < 300 * 300 * 4 + 2 * MIB                   # a small block is stored: its n^2 floats and little else


def test_workspace_in_the_current_environment(monkeypatch):
    """The size is the size of the path the call would take: with MMF_MEDIAN_RADIX there is no one-sweep buffer."""
    ws = _sps().streamed_workspace_bytes
    monkeypatch.delenv("MMF_MEDIAN_RADIX", raising=False)
    sweep = ws(8192, 64, 2, 8, 128)
    monkeypatch.setenv("MMF_MEDIAN_RADIX", "1")
    radix = ws(8192, 64, 2, 8, 128)
    assert 0 < sweep - radix and abs((sweep - radix) - 8192 * 8192 // 20 * 4) < 4 * MIB


def test_workspace_size_rejects_bad_sizes():
    ws = _sps().streamed_workspace_bytes
    for args, words in (((1, 8, 2, 4), "at least 2 rows"), ((8, 0, 2, 4), "D >= 1"), ((8, 8, 0, 4), "dp >= 1"), ((8, 8, 2, 4, -1), "panel_rows")):
        with pytest.raises(ValueError, match=words):
            ws(*args)


# ---- the wrapper's argument errors, on the host ---------------------------------------------------------------------
def test_wrapper_rejects_bad_input_before_any_library_call(monkeypatch):
    import multimodal_fusion_amd as mmf
    f = _sps().super_patch_stats_streamed

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    order, offs = torch.arange(10), torch.zeros(5, dtype=torch.long)
    with pytest.raises(RuntimeError, match="ROCm"):                       # CPU tensors: the package has no CPU path
        f(F, P, order, offs, 4)
    with pytest.raises(RuntimeError, match="ROCm"):
        f(F, P, None, None, 0)
    with pytest.raises(ValueError, match="all tensors must share a device"):
        f(F, P.to("meta"), order, offs, 4)
    with pytest.raises(ValueError, match="all tensors must share a device"):
        f(F, P, order.to("meta"), offs, 4)
    with pytest.raises(ValueError, match=r"order must hold 10 rows and offsets 5 entries \(got 9 and 5\)"):
        f(F, P, order[:9], offs, 4)
    with pytest.raises(ValueError, match=r"offsets 5 entries \(got 10 and 4\)"):
        f(F, P, order, offs[:4], 4)
    with pytest.raises(ValueError, match=r"offsets 5 entries \(got 10 and None\)"):
        f(F, P, order, None, 4)
    with pytest.raises(ValueError, match="must share N"):
        f(F, P[:9], order, offs, 4)
    with pytest.raises(ValueError, match="at least 2 rows"):
        f(F[:1], P[:1], None, None, 0)
    with pytest.raises(ValueError, match="bad n_clusters 0"):
        f(F, P, order, offs, 0)
    with pytest.raises(ValueError, match="panel_rows must be >= 0"):
        f(F, P, order, offs, 4, panel_rows=-3)


def test_cohort_functions_take_the_budget_and_report_the_streamed_groups():
    import inspect
    import multimodal_fusion_amd as mmf
    sig = inspect.signature(mmf.cohort.build_cohort_hypergraphs)
    last = list(sig.parameters.values())[-1]
    assert last.name == "budget_bytes" and last.kind is inspect.Parameter.KEYWORD_ONLY and last.default is None
    assert mmf.super_patches.STREAM_MIN_VALUES == 1 << 22
    # no new public function in the two modules whose functions are pinned one gated case each
    for mod, names in ((mmf.super_patches, {"group_plan", "segment_sort_segmented", "pool_super_patches_segmented",
                                            "aggregate_wsi_super_patches_segmented"}), (mmf.cohort, {"build_cohort_hypergraphs"})):
        public = {n for n, fn in inspect.getmembers(mod, inspect.isfunction) if fn.__module__ == mod.__name__ and not n.startswith("_")}
        assert public == names, (mod.__name__, public)
    assert mmf.super_patches.group_plan([10, 20, 30, 100, 10], 6000) == [(0, 3), (3, 4), (4, 5)]          # still drops the flag


# ---- documents -------------------------------------------------------------------------------------------------------
def _stream_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Streaming entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_stream_table_equals_the_gpu_tests_table():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_super_patch_stats_streamed import SYNC_STREAM
    import multimodal_fusion_amd as mmf
    rows = _stream_table()
    assert rows == SYNC_STREAM == {"mmf_super_patch_stats_streamed": ("data-dependent", "—")}, (rows, SYNC_STREAM)
    assert set(rows) == {e for e in mmf._lib.EXPORTS_STREAM if not e.endswith("_bytes")}          # the size query takes no stream
    from test_stream_arguments_cpu import integration_table
    from test_super_patches_segmented_cpu import _pool_table
    from test_wsi_tma_segmented_cpu import _cohort_table
    assert not (set(integration_table()) | set(_cohort_table()) | set(_pool_table())) & set(rows)


def test_new_kernels_are_launched_on_the_callers_stream():
    """The static scan of tests/test_stream_arguments_cpu.py reads the new file too: no launch on the null stream, no blocking
    call, and the carried kernels are really launched."""
    from test_stream_arguments_cpu import stream_uses, is_null
    uses = [u for u in stream_uses() if u[0] in ("mmf_stream_stats.hip", "mmf_edges.hip")]
    launched = " ".join(a[0] for _, _, what, _, a in uses if what == "hipLaunchKernelGGL")
    for kernel in ("stream_member_pos_kernel", "stream_row_sums_kernel", "bracket_sweep_kernel<true>", "bracket_sweep_kernel<false>",
                   "stats_partial_kernel<true>", "stats_partial_kernel<false>", "stat_lanes_init_kernel", "stat_lanes_finish_kernel"):
        assert kernel in launched, kernel
    mine = [u for u in uses if u[0] == "mmf_stream_stats.hip"]
    assert len(mine) >= 5 and not [u for u in uses if is_null(u[3])]


def test_design_readme_and_header_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        sec = f.read().split("4.13", 1)[1]
    for words in ("Contract", "two assignments", "carried", "Workspace", "recomput"):
        assert words in sec, words
    with open(os.path.join(ROOT, "README.md")) as f:
        r = f.read()
    assert "super_patch_stats_streamed" in r and "budget_bytes" in r
