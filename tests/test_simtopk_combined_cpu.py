"""Top-k of the combined similarity without a GPU: include/mmf_hg_topk.h declares exactly the one entry, the library exports it and
the binding registers it in a fifth list that shares no name with the other four, the entry runs its host checks before any
device call and names the argument, the Python wrapper raises its argument errors on the host, INTEGRATION.md's top-k table
equals the GPU test's, and ops.py keeps the public functions it had."""
import ctypes
import inspect
import os
import re
import sys
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_simtopk_combined"]
OTHER_HEADERS = ["mmf_hg.h", "mmf_hg_pool.h", "mmf_hg_stream.h"]


def _ct():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk")


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding ----------------------------------------------------------------------------------------
def test_topk_header_declares_exactly_the_one_entry():
    assert _declared("mmf_hg_topk.h") == set(ENTRIES)
    for h in OTHER_HEADERS:
        assert not _declared(h) & set(ENTRIES), h
    with open(os.path.join(ROOT, "include", "mmf_hg_topk.h")) as f:
        h = f.read()
    assert '#include "mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    assert "similarity_kernel.py:88-124" in h                             # the reference lines of the similarity it ranks
    for words in ("key_ij = eh + eg", "val_ij = expf(eh) * expf(eg)", "global column id ascending", "-1 and value -inf"):
        assert words in h, words                                          # the arithmetic contract
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()                  # additions only


def test_library_and_binding_export_the_entry_from_a_fifth_list():
    import multimodal_fusion_amd as mmf
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_TOPK) == ENTRIES
    others = set(mmf._lib.EXPORTS) | set(mmf._lib.EXPORTS_COHORT) | set(mmf._lib.EXPORTS_POOL) | set(mmf._lib.EXPORTS_STREAM)
    assert not set(ENTRIES) & others
    assert hasattr(L, ENTRIES[0])
    fn = mmf._lib.lib().mmf_simtopk_combined
    assert fn.restype is ctypes.c_int and tuple(fn.argtypes[-2:]) == (ctypes.c_int, ctypes.c_void_p) and len(fn.argtypes) == 17
    assert mmf._lib.ABI_VERSION == 3 and mmf._lib.lib().mmf_version() == 3


def test_build_lists_the_new_source_and_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mmf_topk.hip" in b.SOURCES and any(h.endswith(os.path.join("include", "mmf_hg_topk.h")) for h in b.HEADERS)


def test_module_and_functions_are_exported_and_ops_is_unchanged():
    import multimodal_fusion_amd as mmf
    ct = _ct()
    assert "combined_topk" in mmf.__all__ and mmf.combined_topk is ct
    for name in ("simtopk_combined", "build_topk_weighted_hypergraph", "build_topk_hypergraph_data"):
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(ct, name), name
    public = {n for n, fn in inspect.getmembers(ct, inspect.isfunction) if fn.__module__ == ct.__name__ and not n.startswith("_")}
    assert public == {"simtopk_combined", "build_topk_weighted_hypergraph", "build_topk_hypergraph_data"}
    sig = inspect.signature(ct.simtopk_combined)
    assert list(sig.parameters) == ["features", "positions", "lambda_h", "lambda_g", "k", "ptr", "batch", "exclude_self", "col_splits",
                                    "return_stats", "profile"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    assert list(inspect.signature(ct.build_topk_weighted_hypergraph).parameters) == ["features", "positions", "lambda_h", "lambda_g", "k",
                                                                                    "device", "ptr", "batch"]
    assert len(import_module("multimodal_fusion_amd.build_hypergraph").__all__) == 17
    # ops.py: every public function has a gated case in tests/test_gpu_stream_contract.py; the new ones live elsewhere
    ops_public = {n for n, fn in inspect.getmembers(mmf.ops, inspect.isfunction) if fn.__module__ == mmf.ops.__name__ and not n.startswith("_")}
    assert ops_public == {
        "simtopk", "simtopk_segmented", "last_query_order", "sim_dense", "sim_dense_stats", "sim_dense_combined", "edge_cosine",
        "topk_merge", "offdiag_lower_median", "lower_median", "array_stats", "threshold_edges", "combined_offdiag_median",
        "combined_threshold_edges", "sim_dense_combined_segmented", "offdiag_lower_median_segmented", "threshold_edges_segmented",
        "padded_dim", "fast_scan_supported", "row_scalars", "prep_rows", "simtopk_prepared", "simtopk_panels", "segment_sort",
        "segment_mean", "segment_offdiag_mean", "clique_pairs", "knn_pairs", "knn_clique_edges", "kmeans_fit", "kmeans_fit_segmented"}


# ---- the entry's host checks, with host buffers standing in for device pointers ------------------------------------------
def _call(**kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(F=b, P=b, n=4, d=4, dp=2, lh=1.0, lg=1.0, k=2, self=1, ptr=None, S=0, idx=b, val=b, opts=None, device=63)
    a.update(kw)
    ptr = a["ptr"]
    if ptr is not None:
        ptr = ctypes.cast((ctypes.c_int64 * len(ptr))(*ptr), ctypes.c_void_p)
    opts = a["opts"]
    if opts is not None:
        opts = ctypes.byref(mmf._lib.SimtopkOpts(*opts))
    rc = L.mmf_simtopk_combined(a["F"], a["P"], a["n"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], ptr, a["S"], a["idx"],
                                a["val"], opts, None, a["device"], None)
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
    (dict(ptr=None, S=2), "host offsets ptr_host"),
    (dict(ptr=[1, 4], S=1), "ptr_host must start at 0"),
    (dict(ptr=[0, 3, 2, 4], S=3), "ptr_host decreases at segment 1"),
    (dict(ptr=[0, 2, 3], S=2), "ptr_host must end at 4"),
    (dict(opts=(1, 0, -1, 0, None)), "col_splits must be >= 0"),
]
UNSUPPORTED = [
    (dict(dp=9), "dp = 9 > 8"),
    (dict(k=44), "k + self = 45 > 44"),
    (dict(k=45, self=0), "k + self = 45 > 44"),
    (dict(n=1 << 31), "n must be < 2^31"),
    (dict(opts=(2, 0, 0, 0, None)), "precision 2"),
]


@pytest.mark.parametrize("kw,words", INVALID)
def test_entry_refuses_bad_arguments_before_any_device_call(kw, words):
    """A device id that does not exist: an argument error must win over the device's."""
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and "simtopk_combined" in msg, (rc, msg)


@pytest.mark.parametrize("kw,words", UNSUPPORTED)
def test_entry_refuses_what_it_does_not_support_before_any_device_call(kw, words):
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and words in msg and "simtopk_combined" in msg, (rc, msg)


def test_entry_refuses_a_negative_device_first():
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(k=0), dict(F=None), dict(dp=9)):
        rc, msg = _call(device=-1, **kw)
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and "no CPU path" in msg and "simtopk_combined" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """Zero lambdas, k + self = 44, an empty segment, dp = 8: the call gets as far as the device (which is not there).  n == 0 returns
    before it."""
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(lh=0.0, lg=0.0), dict(k=43), dict(k=44, self=0), dict(dp=8), dict(ptr=[0, 0, 1, 4], S=3),
               dict(opts=(0, 1, 3, 0, None))):
        rc, msg = _call(**kw)
        assert rc == mmf._lib.MMF_E_HIP, (kw, rc, msg)
    assert _call(n=0)[0] == mmf._lib.MMF_OK and _call(n=0, F=None, P=None, idx=None, val=None, ptr=[0], S=0)[0] == mmf._lib.MMF_OK


# ---- the wrapper's argument errors, on the host ---------------------------------------------------------------------
def test_wrapper_rejects_bad_input_before_any_library_call(monkeypatch):
    import multimodal_fusion_amd as mmf
    ct = _ct()

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    for f in (ct.simtopk_combined, ct.build_topk_weighted_hypergraph, ct.build_topk_hypergraph_data):
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:9])
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:, 0])
        with pytest.raises(ValueError, match=r"k must be >= 1 \(got 0\)"):
            f(F, P, k=0)
        with pytest.raises(ValueError, match="give exactly one of ptr / batch"):
            f(F, P, ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long))
        with pytest.raises(ValueError, match=r"ptr must end at 10 \(got 9\)"):
            f(F, P, ptr=[0, 4, 9])
        with pytest.raises(ValueError, match="ptr must start at 0"):
            f(F, P, ptr=[1, 10])
        with pytest.raises(ValueError, match="segment 1: ptr decreases"):
            f(F, P, ptr=[0, 6, 4, 10])
        with pytest.raises(ValueError, match="batch must be sorted"):
            f(F, P, batch=torch.tensor([0, 0, 1, 0, 1, 1, 2, 2, 2, 2]))
        with pytest.raises(ValueError, match="batch must hold one segment id per row"):
            f(F, P, batch=torch.zeros(9, dtype=torch.long))


def test_without_a_gpu_the_wrapper_raises(monkeypatch):
    ct = _ct()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    for f in (ct.simtopk_combined, ct.build_topk_weighted_hypergraph, ct.build_topk_hypergraph_data):
        with pytest.raises(RuntimeError, match="ROCm"):
            f(F, P)
        with pytest.raises(RuntimeError, match="ROCm"):
            f(F, P, ptr=[0, 4, 10])


# ---- documents -------------------------------------------------------------------------------------------------------
def _topk_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Top-k entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_topk_table_equals_the_gpu_tests_table():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_simtopk_combined import SYNC_TOPK
    import multimodal_fusion_amd as mmf
    rows = _topk_table()
    assert rows == SYNC_TOPK == {"mmf_simtopk_combined": ("once", "the call")}, (rows, SYNC_TOPK)
    assert set(rows) == set(mmf._lib.EXPORTS_TOPK)
    from test_stream_arguments_cpu import integration_table
    from test_super_patch_stats_streamed_cpu import _stream_table
    from test_super_patches_segmented_cpu import _pool_table
    from test_wsi_tma_segmented_cpu import _cohort_table
    assert not (set(integration_table()) | set(_cohort_table()) | set(_pool_table()) | set(_stream_table())) & set(rows)


def test_new_kernels_are_launched_on_the_callers_stream():
    """The static scan of tests/test_stream_arguments_cpu.py reads the new file too: the re-rank is launched on the caller's stream,
    nothing in it blocks, and the driver's fills are asynchronous."""
    from test_stream_arguments_cpu import BLOCKING, is_null, sources, stream_uses
    uses = [u for u in stream_uses() if u[0] == "mmf_topk.hip"]
    launched = " ".join(a[0] for _, _, what, _, a in uses if what == "hipLaunchKernelGGL")
    assert "rerank_combined_kernel<true>" in launched and "rerank_combined_kernel<false>" in launched
    assert uses and not [u for u in uses if is_null(u[3])]
    text = dict(sources())["mmf_topk.hip"]
    assert not [m for m in BLOCKING.finditer(text) if not m.group(1).endswith("Async")]
    scan = dict(sources())["mmf_scan_f32.hip"]
    assert "launch_f32_t<MODE_SCAN, 16, false, true>" in scan and "launch_f32_t<MODE_SCAN, 48, false, true>" in scan


def test_design_readme_and_header_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design.split("4.14", 1)[1]
    for words in ("Contract", "key_ij = eh + eg", "pos_exponent", "Re-rank", "instructions per pair", "Measurements"):
        assert words in sec, words
    assert "simtopk_combined" in design.split("## 4", 1)[0]               # §1's table has the row
    with open(os.path.join(ROOT, "README.md")) as f:
        r = f.read()
    assert "simtopk_combined" in r and "build_topk_weighted_hypergraph" in r
    assert os.path.exists(os.path.join(ROOT, "scripts", "simtopk_combined_timing.py"))
