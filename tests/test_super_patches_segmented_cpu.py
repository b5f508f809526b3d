"""Segmented super-patch aggregation and the cohort chain without a GPU: include/mmf_hg_pool.h declares exactly the two pooling
entries, the library exports them and the binding registers them in a third list that shares no name with the other two, both
entries run their host checks before any device call, every argument error of super_patches.py and cohort.py is raised on the
host and names the first bad slide, the group plan is weighted_hypergraph's, and INTEGRATION.md's pooling table equals the GPU
test's."""
import ctypes
import os
import re
import sys
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_segment_sort_segmented", "mmf_super_patches_segmented"]
FNS = ["segment_sort_segmented", "pool_super_patches_segmented", "aggregate_wsi_super_patches_segmented", "build_cohort_hypergraphs"]


def _sp():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.super_patches")


def _co():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.cohort")


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding ----------------------------------------------------------------------------------------
def test_pool_header_declares_exactly_the_two_entries():
    assert _declared("mmf_hg_pool.h") == set(ENTRIES)
    assert not _declared("mmf_hg.h") & set(ENTRIES)                     # mmf_hg.h stays what the two pinned lists say
    with open(os.path.join(ROOT, "include", "mmf_hg_pool.h")) as f:
        h = f.read()
    assert '#include "mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    assert "preprocess_hypergraph.py:157-197" in h                       # the reference lines the entries replace
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()                  # additions only


def test_library_and_binding_export_the_entries_from_a_third_list():
    import multimodal_fusion_amd as mmf
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_POOL) == ENTRIES
    assert not set(ENTRIES) & (set(mmf._lib.EXPORTS) | set(mmf._lib.EXPORTS_COHORT))
    for name in ENTRIES:
        assert hasattr(L, name), name
        fn = getattr(mmf._lib.lib(), name)
        assert fn.restype is ctypes.c_int and tuple(fn.argtypes[-2:]) == (ctypes.c_int, ctypes.c_void_p), name
    assert len(mmf._lib.lib().mmf_segment_sort_segmented.argtypes) == 11
    assert len(mmf._lib.lib().mmf_super_patches_segmented.argtypes) == 17
    assert mmf._lib.ABI_VERSION == 3 and mmf._lib.lib().mmf_version() == 3


def test_build_lists_the_new_source_and_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mmf_pool.hip" in b.SOURCES and any(h.endswith(os.path.join("include", "mmf_hg_pool.h")) for h in b.HEADERS)


def _calls():
    """name -> call(ptr, n_seg, device_id): n = 4 rows, 2 clusters; host buffers stand in for device pointers."""
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    return L, mmf._lib, {
        "mmf_segment_sort_segmented": lambda p, S, dev=0: L.mmf_segment_sort_segmented(b, 4, p, S, 2, b, b, b, b, dev, None),
        "mmf_super_patches_segmented": lambda p, S, dev=0: L.mmf_super_patches_segmented(b, b, 4, 4, 2, p, S, 2, b, b, b, b, b, b, b, dev, None),
        "mmf_super_patches_segmented without K": lambda p, S, dev=0: L.mmf_super_patches_segmented(b, b, 4, 4, 2, p, S, 2, b, b, None, b, b,
                                                                                                   None, None, dev, None),
    }


def test_entries_refuse_a_negative_device_first():
    L, m, calls = _calls()
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    bad = (ctypes.c_int64 * 3)(1, 2, 4)                # a malformed table too: the device is still the first objection
    for name, call in calls.items():
        for p, S in ((vp((ctypes.c_int64 * 2)(0, 4)), 1), (vp(bad), 2), (None, 0)):
            assert call(p, S, -1) == m.MMF_E_UNSUPPORTED, (name, L.mmf_last_error())
            assert b"no CPU path" in L.mmf_last_error(), (name, L.mmf_last_error())


def test_entries_refuse_bad_offsets_before_any_device_call():
    """The three malformed tables of tests/test_entry_checks_cpu.py, with a device id that does not exist."""
    L, m, calls = _calls()
    late, decreasing, short = (ctypes.c_int64 * 3)(1, 2, 4), (ctypes.c_int64 * 4)(0, 3, 2, 4), (ctypes.c_int64 * 3)(0, 2, 3)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    for name, call in calls.items():
        assert call(vp(late), 2, 63) == m.MMF_E_INVALID and b"must start at 0" in L.mmf_last_error(), (name, L.mmf_last_error())
        assert call(vp(decreasing), 3, 63) == m.MMF_E_INVALID, (name, "decreasing", L.mmf_last_error())
        assert b"segment 1" in L.mmf_last_error(), (name, L.mmf_last_error())
        assert call(vp(short), 2, 63) == m.MMF_E_INVALID and b"must end at 4" in L.mmf_last_error(), (name, L.mmf_last_error())
        assert call(None, 1, 63) == m.MMF_E_INVALID, name
    # the limits, still on the host: 16384 clusters per segment, G < 2^31; with K every segment needs a row
    buf = (ctypes.c_int64 * 8)()
    b = vp(buf)
    ok = vp((ctypes.c_int64 * 2)(0, 4))
    assert L.mmf_segment_sort_segmented(b, 4, ok, 1, 16385, b, b, b, b, 63, None) == m.MMF_E_UNSUPPORTED
    assert b"16384" in L.mmf_last_error()
    assert L.mmf_segment_sort_segmented(b, 4, ok, 1, 0, b, b, b, b, 63, None) == m.MMF_E_INVALID
    hole = vp((ctypes.c_int64 * 4)(0, 2, 2, 4))
    assert calls["mmf_segment_sort_segmented"](hole, 3, 63) != m.MMF_E_INVALID                       # an empty segment sorts to nothing
    assert calls["mmf_super_patches_segmented"](hole, 3, 63) == m.MMF_E_INVALID and b"segment 1 has 0 rows" in L.mmf_last_error()


def test_package_exports_and_mirror_package_is_unchanged():
    import multimodal_fusion_amd as mmf
    for fn in FNS[:3]:
        assert fn in mmf.__all__ and getattr(mmf, fn) is getattr(_sp(), fn), fn
    assert "build_cohort_hypergraphs" in mmf.__all__ and mmf.build_cohort_hypergraphs is _co().build_cohort_hypergraphs
    assert "super_patches" in mmf.__all__ and "cohort" in mmf.__all__ and mmf.super_patches is _sp() and mmf.cohort is _co()
    for fn in FNS:
        assert not hasattr(mmf.ops, fn), fn                       # ops.py's functions are pinned by the stream-contract test
    bh = import_module("multimodal_fusion_amd.build_hypergraph")
    assert not set(FNS) & set(bh.__all__) and len(bh.__all__) == 17


# ---- host-side argument errors: 10 patches of D = 8 on the CPU ----------------------------------------------------------
BAD_PTR = [
    (dict(ptr=[0, 5, 9]), r"slide 1: ptr must end at 10 \(got 9\)"),
    (dict(ptr=[1, 5, 10]), "slide 0: ptr must start at 0"),
    (dict(ptr=[0, 6, 4, 10]), "slide 1: ptr decreases"),
    (dict(ptr=[0, 6, 6, 10]), "slide 1 has 0 rows in ptr, need at least 1"),
    (dict(batch=torch.tensor([0, 0, 0, 1, 1, 1, 0, 1, 1, 1])), "slide 0: batch must be sorted"),
    (dict(batch=torch.tensor([0, 0, 0, 0, 0, 2, 2, 2, 2, 2])), "slide 1 has 0 rows in batch"),
    (dict(batch=torch.zeros(9, dtype=torch.long)), r"batch must hold one slide id per row \(10\)"),
    (dict(ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long)), "exactly one of ptr / batch"),
    (dict(), "exactly one of ptr / batch"),
]


@pytest.mark.parametrize("kw,match", BAD_PTR)
def test_aggregate_rejects_bad_slides_on_the_host(kw, match):
    with pytest.raises(ValueError, match=match):
        _sp().aggregate_wsi_super_patches_segmented(torch.randn(10, 8), torch.zeros(10, 2), 2, **kw)
    if "has 0 rows" not in match:                                    # an empty slide sorts to nothing
        with pytest.raises(ValueError, match=match):
            _sp().segment_sort_segmented(torch.zeros(10, dtype=torch.long), 2, **kw)


def test_aggregate_rejects_bad_shapes_and_cluster_counts_on_the_host():
    sp = _sp()
    F, P, ok = torch.randn(10, 8), torch.zeros(10, 2), dict(ptr=[0, 6, 10])
    with pytest.raises(ValueError, match="slide 0: wsi_features have 10 rows, wsi_positions 9"):
        sp.aggregate_wsi_super_patches_segmented(F, P[:9], 2, **ok)
    with pytest.raises(ValueError, match="must be 2-D"):
        sp.aggregate_wsi_super_patches_segmented(F[:, 0], P, 2, **ok)
    with pytest.raises(ValueError, match=r"slide 1: n_samples=4 should be >= n_clusters=5\."):       # what scikit-learn raises
        sp.aggregate_wsi_super_patches_segmented(F, P, 5, **ok)
    with pytest.raises(ValueError, match=r"slide 0: n_samples=6 should be >= n_clusters=0\."):
        sp.aggregate_wsi_super_patches_segmented(F, P, 0, **ok)
    with pytest.raises(ValueError, match="slide 1: wsi_similarity_flat .* holds 51 values, the blocks of the slides 52"):
        sp.aggregate_wsi_super_patches_segmented(F, P, 2, wsi_similarity_flat=torch.rand(51), **ok)
    with pytest.raises(ValueError, match="slide 1: wsi_similarity_flat must be the flat 1-D buffer"):
        sp.aggregate_wsi_super_patches_segmented(F, P, 2, wsi_similarity_flat=torch.rand(4, 13), **ok)
    big = dict(ptr=[0, 20000, 40000])
    with pytest.raises(ValueError, match="slide 0: at most 16384 clusters per slide"):
        sp.aggregate_wsi_super_patches_segmented(torch.zeros(40000, 1), torch.zeros(40000, 2), 16385, **big)


def test_sort_and_pooling_reject_bad_input_on_the_host():
    sp = _sp()
    lab, ok = torch.zeros(10, dtype=torch.long), dict(ptr=[0, 6, 10])
    with pytest.raises(ValueError, match="flat 1-D"):
        sp.segment_sort_segmented(lab.view(2, 5), 2, **ok)
    with pytest.raises(ValueError, match=r"slide 0: n_clusters must lie in \[1, 16384\] \(got 0\)"):
        sp.segment_sort_segmented(lab, 0, **ok)
    with pytest.raises(ValueError, match=r"n_clusters must lie in \[1, 16384\] \(got 16385\)"):
        sp.segment_sort_segmented(lab, 16385, **ok)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    order, offsets = torch.arange(10), torch.zeros(5, dtype=torch.long)
    with pytest.raises(ValueError, match="slide 0: features .* and positions .* must share N"):
        sp.pool_super_patches_segmented(F, P[:9], order, offsets, 2, **ok)
    with pytest.raises(ValueError, match="slide 1: ptr decreases"):
        sp.pool_super_patches_segmented(F, P, order, offsets, 2, ptr=[0, 6, 4, 10])
    with pytest.raises(ValueError, match=r"order must hold 10 rows and offsets 5 entries \(got 9 and 5\)"):
        sp.pool_super_patches_segmented(F, P, order[:9], offsets, 2, **ok)
    with pytest.raises(ValueError, match=r"offsets 5 entries \(got 10 and 4\)"):
        sp.pool_super_patches_segmented(F, P, order, offsets[:4], 2, **ok)
    with pytest.raises(ValueError, match="slide 1: K_flat holds 50 values, the blocks of the slides 52"):
        sp.pool_super_patches_segmented(F, P, order, offsets, 2, K_flat=torch.rand(50), **ok)
    with pytest.raises(ValueError, match="slide 1 has 0 rows in ptr"):                      # with K every slide needs a row
        sp.pool_super_patches_segmented(F, P, order, torch.zeros(7, dtype=torch.long), 2, ptr=[0, 6, 6, 10], K_flat=torch.rand(52))


BAD_COHORT = [
    (dict(wsi_ptr=[0, 5, 9], tma_ptr=[0, 3, 6]), r"slide 1: wsi_ptr must end at 10 \(got 9\)"),
    (dict(wsi_ptr=[0, 6, 4, 10], tma_ptr=[0, 2, 4, 6]), "slide 1: wsi_ptr decreases"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 4, 3, 6]), "slide 1: tma_ptr decreases"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 6, 6]), "slide 1 has no TMA rows"),
    (dict(wsi_ptr=[0, 3, 6, 10], tma_batch=torch.tensor([0, 0, 0, 2, 2, 2])), "slide 1 has no TMA rows"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 5]), r"slide 1: tma_ptr must end at 6 \(got 5\)"),
    (dict(wsi_ptr=[0, 5, 10]), "exactly one of tma_ptr / tma_batch"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 2, 4, 6]), "slide 2: wsi describes 2 slides, tma 3"),
    (dict(wsi_ptr=[0, 8, 10], tma_ptr=[0, 3, 6]), r"slide 1: n_samples=2 should be >= n_clusters=3\."),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6], num_groups=4), r"slide 0: n_samples=3 should be >= n_clusters=4\."),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 5, 6], hypergraph_k=4), "slide 1: Expected n_neighbors <= n_samples_fit, but n_neighbors = 5"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 5, 6], num_hyperedges=5), r"slide 1: n_samples=4 should be >= n_clusters=5\."),
]


@pytest.mark.parametrize("kw,match", BAD_COHORT)
def test_cohort_chain_rejects_bad_input_on_the_host(kw, match):
    args = dict(num_wsi_super_patches=3, num_groups=2, hypergraph_k=2, num_hyperedges=2)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _co().build_cohort_hypergraphs(torch.randn(10, 8), torch.zeros(10, 2), torch.randn(6, 8), **args)


def test_cohort_chain_rejects_different_feature_widths():
    with pytest.raises(ValueError, match="slide 0: wsi_features have D=8, tma_features D=7"):
        _co().build_cohort_hypergraphs(torch.randn(10, 8), torch.zeros(10, 2), torch.randn(6, 7), wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6])
    with pytest.raises(ValueError, match="must be 2-D"):
        _co().build_cohort_hypergraphs(torch.randn(10, 8), torch.zeros(10), torch.randn(6, 8), wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6])


def test_valid_input_reaches_the_device_check(monkeypatch):
    """With nothing to object to, CPU tensors fail at the device, not at an argument: no host path computes anything."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    sp = _sp()
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    with pytest.raises(RuntimeError, match="ROCm"):
        sp.aggregate_wsi_super_patches_segmented(F, P, 2, ptr=[0, 6, 10])
    with pytest.raises(RuntimeError, match="ROCm"):
        sp.aggregate_wsi_super_patches_segmented(F, P, 2, wsi_similarity_flat=torch.rand(52), batch=torch.tensor([0] * 6 + [1] * 4))
    with pytest.raises(RuntimeError, match="ROCm"):
        sp.segment_sort_segmented(torch.zeros(10, dtype=torch.long), 2, ptr=[0, 6, 6, 10])
    with pytest.raises(RuntimeError, match="ROCm"):
        sp.pool_super_patches_segmented(F, P, torch.arange(10), torch.zeros(5, dtype=torch.long), 2, ptr=[0, 6, 10], K_flat=torch.rand(52))
    with pytest.raises(RuntimeError, match="ROCm"):
        _co().build_cohort_hypergraphs(F, P, torch.randn(6, 8), wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6], num_wsi_super_patches=3,
                                       num_groups=2, hypergraph_k=2, num_hyperedges=2)


# ---- pure functions --------------------------------------------------------------------------------------------------
def test_group_plan_for_a_hand_written_list():
    sp = _sp()
    # blocks of 400, 1600, 3600, 40000, 400, 400, 6400, 100 bytes against 6000: 400 + 1600 + 3600 fit, the next block alone is
    # larger than the budget and runs alone, 400 + 400 fit and 6400 does not join them (and is itself too large), 100 is the rest
    sizes = [10, 20, 30, 100, 10, 10, 40, 5]
    assert sp.group_plan(sizes, 6000) == [(0, 3), (3, 4), (4, 6), (6, 7), (7, 8)]
    assert sp.group_plan(sizes, 1 << 40) == [(0, 8)]
    assert sp.group_plan(sizes, 1) == [(s, s + 1) for s in range(8)]                     # every slide alone: none is dropped
    assert sp.group_plan([30, 30, 30], 7200) == [(0, 2), (2, 3)]                         # exactly the budget still fits
    assert sp.group_plan([], 100) == []
    # consecutive, complete, in order
    plan = sp.group_plan([7, 300, 12, 12, 250, 3], 300000)
    assert [a for a, _ in plan] == [0] + [b for _, b in plan][:-1] and plan[-1][1] == 6
    from multimodal_fusion_amd.build_hypergraph import similarity_kernel
    assert similarity_kernel.STREAM_BYTES == 32 << 30                  # the default budget of aggregate_wsi_super_patches_segmented


# ---- documents -------------------------------------------------------------------------------------------------------
def _pool_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Pooling entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_pool_table_equals_the_gpu_tests_table():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_super_patches_segmented import SYNC_POOL
    import multimodal_fusion_amd as mmf
    rows = _pool_table()
    assert rows == SYNC_POOL, (rows, SYNC_POOL)
    assert set(rows) == set(mmf._lib.EXPORTS_POOL)                        # every entry of the third list has its row
    assert {s for s, _ in rows.values()} <= {"none", "once", "per iteration", "data-dependent"}
    # the two pinned tables and the third list do not overlap
    from test_stream_arguments_cpu import integration_table
    from test_wsi_tma_segmented_cpu import _cohort_table
    assert not (set(integration_table()) | set(_cohort_table())) & set(rows)


def test_new_kernels_are_launched_on_the_callers_stream():
    """The static scan of tests/test_stream_arguments_cpu.py reads csrc/mmf_pool.hip too: no launch on the null stream, no
    blocking call, and the new kernels are really launched from it."""
    from test_stream_arguments_cpu import stream_uses, is_null
    uses = [u for u in stream_uses() if u[0] == "mmf_pool.hip"]
    launched = " ".join(a[0] for _, _, what, _, a in uses if what == "hipLaunchKernelGGL")
    for kernel in ("pool_count_kernel", "pool_chunk_scan_kernel", "pool_tile_sum_kernel", "pool_tile_scan_kernel", "pool_offsets_kernel",
                   "pool_scatter_kernel", "pool_status_kernel", "pool_seg_of_kernel", "pool_row_sums_kernel", "pool_offdiag_final_kernel",
                   "pool_stats_partial_kernel"):
        assert kernel in launched, kernel
    assert uses and not [u for u in uses if is_null(u[3])]


def test_design_and_readme_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        d = f.read()
    sec = d.split("4.12", 1)[1]
    for heading in ("Contract", "Why the bits are the plain call's", "Resources", "Known cost", "Cut"):
        assert heading in sec, heading
    with open(os.path.join(ROOT, "README.md")) as f:
        r = f.read()
    assert "aggregate_wsi_super_patches_segmented" in r and "build_cohort_hypergraphs" in r
