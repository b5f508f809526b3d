"""Segmented WSI x TMA similarity, grouping and median edge filter without a GPU: the header declares the two cohort entries, the
library exports them and the binding registers them in its second list (which, with EXPORTS, is exactly what the header
declares), every argument error is raised on the host and names the first bad slide, the grouping-by-width plan and the
threshold rounding of the filter are what DESIGN.md §4.11 says, and INTEGRATION.md's cohort table equals the GPU test's."""
import ctypes
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_sim_dense_stats_segmented", "mmf_lower_median_segmented"]
FNS = ["sim_dense_stats_segmented", "lower_median_segmented", "compute_wsi_tma_similarity_segmented", "similarity_block",
       "group_by_similarity_segmented", "filter_edges_by_median_segmented"]


def _wt():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.wsi_tma_similarity")


def _declared():
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        h = f.read()
    for name in ENTRIES:
        assert f"int {name}(" in h, name
    assert "#define MMF_ABI_VERSION 3" in h                       # additions only
    assert "preprocess_hypergraph.py:248-265" in h and "preprocess_hypergraph.py:885-897" in h      # the reference lines they replace


def test_library_and_binding_export_the_entries():
    import multimodal_fusion_amd as mmf
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in mmf._lib.EXPORTS_COHORT and name not in mmf._lib.EXPORTS, name
        fn = getattr(mmf._lib.lib(), name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, name
    assert len(mmf._lib.lib().mmf_sim_dense_stats_segmented.argtypes) == 15
    assert len(mmf._lib.lib().mmf_lower_median_segmented.argtypes) == 6
    assert mmf._lib.ABI_VERSION == 3 and mmf._lib.lib().mmf_version() == 3


def test_the_two_lists_are_exactly_what_the_header_declares():
    """The gap a second list opens: an entry bound in neither list, or a stale name in one, fails here."""
    import multimodal_fusion_amd as mmf
    both = list(mmf._lib.EXPORTS) + list(mmf._lib.EXPORTS_COHORT)
    assert len(both) == len(set(both))
    assert set(both) == _declared(), sorted(set(both) ^ _declared())
    assert list(mmf._lib.EXPORTS_COHORT) == ENTRIES


def test_entries_have_no_cpu_path():
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_float * 16)()
    st = (ctypes.c_double * 5)()
    ptr = (ctypes.c_int64 * 2)(0, 4)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    rc = L.mmf_sim_dense_stats_segmented(vp(buf), 4, vp(buf), 4, 4, 0, mmf._lib.RBF_DIRECT, 1.0, vp(ptr), vp(ptr), 1, vp(buf), vp(st), -1, None)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and b"no CPU path" in L.mmf_last_error()
    rc = L.mmf_lower_median_segmented(vp(buf), vp(ptr), 1, vp(buf), -1, None)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and b"no CPU path" in L.mmf_last_error()


def test_c_entries_check_their_tables_before_any_device_work():
    """Host pointers stand in for device ones: every one of these returns from the host checks, naming the first bad segment."""
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf, st = (ctypes.c_float * 64)(), (ctypes.c_double * 10)()
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)   # noqa: E731

    def stats(xp, yp, S, metric=mmf._lib.RBF_DIRECT, out=buf):
        return L.mmf_sim_dense_stats_segmented(vp(buf), 4, vp(buf), 6, 4, 0, metric, 1.0, vp(xp), vp(yp), S, vp(out) if out else None,
                                               vp(st), 0, None)
    cases = [((i64(0, 2, 4), i64(0, 6, 6), 2), b"segment 1 has 0 rows in y_ptr"),
             ((i64(0, 0, 4), i64(0, 3, 6), 2), b"segment 0 has 0 rows in x_ptr"),
             ((i64(0, 3, 2, 4), i64(0, 2, 4, 6), 3), b"x_ptr decreases at segment 1"),
             ((i64(1, 2, 4), i64(0, 3, 6), 2), b"x_ptr must start at 0"),
             ((i64(0, 2, 3), i64(0, 3, 6), 2), b"x_ptr must end at 4"),
             ((i64(0, 2, 4), i64(0, 3, 5), 2), b"y_ptr must end at 6")]
    for args, msg in cases:
        assert stats(*args) == mmf._lib.MMF_E_INVALID and msg in L.mmf_last_error(), (msg, L.mmf_last_error())
    for metric in (mmf._lib.DOT, mmf._lib.COSINE, mmf._lib.NEG_SQ_L2, mmf._lib.RBF):
        assert stats(i64(0, 2, 4), i64(0, 3, 6), 2, metric=metric) == mmf._lib.MMF_E_UNSUPPORTED
    assert stats(i64(0, 2, 4), i64(0, 3, 6), 2, out=None) == mmf._lib.MMF_E_UNSUPPORTED
    med = lambda p, S: L.mmf_lower_median_segmented(vp(buf), vp(p), S, vp(buf), 0, None)   # noqa: E731
    assert med(i64(0, 3, 3, 5), 3) == mmf._lib.MMF_E_INVALID and b"segment 1 has 0 rows" in L.mmf_last_error()
    assert med(i64(0, 3, 2), 2) == mmf._lib.MMF_E_INVALID and b"decreases at segment 1" in L.mmf_last_error()
    assert med(i64(2, 3), 1) == mmf._lib.MMF_E_INVALID and b"must start at 0" in L.mmf_last_error()


def test_package_exports_and_mirror_package_is_unchanged():
    import multimodal_fusion_amd as mmf
    for fn in FNS:
        assert fn in mmf.__all__ and getattr(mmf, fn) is getattr(_wt(), fn), fn
        assert not hasattr(mmf.ops, fn), fn                       # ops.py's functions are pinned by the stream-contract test
    bh = import_module("multimodal_fusion_amd.build_hypergraph")
    for fn in FNS:
        assert fn not in bh.__all__
    assert len(bh.__all__) == 17


# ---- host-side argument errors: 10 wsi rows and 6 tma rows of D = 8 on the CPU ---------------------------------------
BAD_SIDES = [
    (dict(wsi_ptr=[0, 5, 9], tma_ptr=[0, 3, 6]), r"slide 1: wsi_ptr must end at 10 \(got 9\)"),
    (dict(wsi_ptr=[1, 5, 10], tma_ptr=[0, 3, 6]), "slide 0: wsi_ptr must start at 0"),
    (dict(wsi_ptr=[0, 6, 4, 10], tma_ptr=[0, 2, 4, 6]), "slide 1: wsi_ptr decreases"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 4, 3, 6]), "slide 1: tma_ptr decreases"),
    (dict(wsi_ptr=[0, 5, 5, 10], tma_ptr=[0, 2, 4, 6]), "slide 1 has 0 rows in wsi_ptr, need at least 1"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 6, 6]), "slide 1 has 0 rows in tma_ptr, need at least 1"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 5]), r"slide 1: tma_ptr must end at 6 \(got 5\)"),
    (dict(wsi_batch=torch.tensor([0, 0, 0, 1, 1, 1, 0, 1, 1, 1]), tma_ptr=[0, 3, 6]), "slide 0: wsi_batch must be sorted"),
    (dict(wsi_ptr=[0, 5, 10], tma_batch=torch.tensor([-1, 0, 0, 0, 1, 1])), "slide -1: tma_batch must be non-negative"),
    (dict(wsi_ptr=[0, 3, 5, 10], tma_batch=torch.tensor([0, 0, 0, 2, 2, 2])), "slide 1 has 0 rows in tma_batch"),
    (dict(wsi_batch=torch.zeros(9, dtype=torch.long), tma_ptr=[0, 6]), r"wsi_batch must hold one slide id per row \(10\)"),
    (dict(wsi_ptr=[0, 5, 10], wsi_batch=torch.zeros(10, dtype=torch.long), tma_ptr=[0, 3, 6]), "exactly one of wsi_ptr / wsi_batch"),
    (dict(wsi_ptr=[0, 5, 10]), "exactly one of tma_ptr / tma_batch"),
    (dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 2, 4, 6]), "slide 2: wsi describes 2 slides, tma 3"),
    (dict(wsi_ptr=[0, 5, 10], tma_batch=torch.zeros(6, dtype=torch.long)), "slide 1: wsi describes 2 slides, tma 1"),
]


@pytest.mark.parametrize("kw,match", BAD_SIDES)
def test_similarity_rejects_bad_input_on_the_host(kw, match):
    wt = _wt()
    with pytest.raises(ValueError, match=match):
        wt.compute_wsi_tma_similarity_segmented(torch.randn(10, 8), torch.zeros(10, 2), torch.randn(6, 8), **kw)
    xy = {k.replace("wsi_", "x_").replace("tma_", "y_"): v for k, v in kw.items()}
    with pytest.raises(ValueError, match=match.replace("wsi_", "x_").replace("tma_", "y_").replace("wsi describes", "x describes")
                       .replace("tma ", "y ")):
        wt.sim_dense_stats_segmented(torch.randn(10, 8), torch.randn(6, 8), **xy)


def test_similarity_rejects_different_feature_widths_and_metrics():
    wt = _wt()
    with pytest.raises(ValueError, match="slide 0: wsi_features have D=8, tma_features D=7"):
        wt.compute_wsi_tma_similarity_segmented(torch.randn(10, 8), None, torch.randn(6, 7), wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6])
    with pytest.raises(ValueError, match="slide 0: X has D=8, Y has D=7"):
        wt.sim_dense_stats_segmented(torch.randn(10, 8), torch.randn(6, 7), x_ptr=[0, 5, 10], y_ptr=[0, 3, 6])
    with pytest.raises(ValueError, match="2-D"):
        wt.compute_wsi_tma_similarity_segmented(torch.randn(10), None, torch.randn(6, 7), wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6])
    with pytest.raises(ValueError, match="only metric='rbf_direct'"):
        wt.sim_dense_stats_segmented(torch.randn(10, 8), torch.randn(6, 8), x_ptr=[0, 10], y_ptr=[0, 6], metric="rbf")
    with pytest.raises(ValueError, match="unknown metric"):
        wt.sim_dense_stats_segmented(torch.randn(10, 8), torch.randn(6, 8), x_ptr=[0, 10], y_ptr=[0, 6], metric="l1")


@pytest.mark.parametrize("kw,match", [
    (dict(ptr=[0, 5, 9]), r"slide 1: ptr must end at 10 \(got 9\)"),
    (dict(ptr=[1, 5, 10]), "slide 0: ptr must start at 0"),
    (dict(ptr=[0, 6, 4, 10]), "slide 1: ptr decreases"),
    (dict(ptr=[0, 6, 6, 10]), "slide 1 has 0 rows in ptr, need at least 1"),
    (dict(batch=torch.tensor([0, 0, 0, 1, 1, 1, 0, 1, 1, 1])), "slide 0: batch must be sorted"),
    (dict(batch=torch.tensor([0, 0, 0, 0, 0, 2, 2, 2, 2, 2])), "slide 1 has 0 rows in batch"),
    (dict(ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long)), "exactly one"),
    (dict(), "exactly one"),
])
def test_median_rejects_bad_input_on_the_host(kw, match):
    with pytest.raises(ValueError, match=match):
        _wt().lower_median_segmented(torch.rand(10), **kw)
    with pytest.raises(ValueError, match="flat 1-D"):
        _wt().lower_median_segmented(torch.rand(2, 5), ptr=[0, 10])


def test_grouping_rejects_bad_input_on_the_host():
    wt = _wt()
    S_flat = torch.rand(5 * 3 + 5 * 3)
    ok = dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6])
    with pytest.raises(ValueError, match="^Unknown grouping method: knn$"):               # the mirror's error, before anything else
        wt.group_by_similarity_segmented(S_flat, 2, method="knn", **ok)
    with pytest.raises(ValueError, match=r"slide 1: n_samples=2 should be >= n_clusters=3\."):
        wt.group_by_similarity_segmented(torch.rand(8 * 3 + 2 * 3), 3, wsi_ptr=[0, 8, 10], tma_ptr=[0, 3, 6])
    with pytest.raises(ValueError, match=r"slide 0: n_samples=5 should be >= n_clusters=0\."):
        wt.group_by_similarity_segmented(S_flat, 0, **ok)
    with pytest.raises(ValueError, match="slide 1: S_flat holds 29 values, the blocks of the slides 30"):
        wt.group_by_similarity_segmented(S_flat[:29], 2, **ok)
    with pytest.raises(ValueError, match="flat 1-D"):
        wt.group_by_similarity_segmented(S_flat.view(10, 3), 2, **ok)
    with pytest.raises(ValueError, match="slide 1: wsi_ptr decreases"):
        wt.group_by_similarity_segmented(S_flat, 2, wsi_ptr=[0, 6, 4, 10], tma_ptr=[0, 2, 4, 6])
    with pytest.raises(ValueError, match="slide 2: wsi describes 2 slides, tma 3"):
        wt.group_by_similarity_segmented(S_flat, 2, wsi_ptr=[0, 5, 10], tma_ptr=[0, 2, 4, 6])
    with pytest.raises(ValueError, match="exactly one of tma_ptr / tma_batch"):
        wt.group_by_similarity_segmented(S_flat, 2, wsi_ptr=[0, 5, 10])


def test_filter_rejects_bad_input_on_the_host():
    wt = _wt()
    ei, ew = torch.zeros((2, 10), dtype=torch.int64), torch.rand(10)
    with pytest.raises(ValueError, match="slide 1 has no edges"):
        wt.filter_edges_by_median_segmented(ei, ew, [0, 4, 4, 10], 0.5)
    with pytest.raises(ValueError, match="slide 0 has no edges"):
        wt.filter_edges_by_median_segmented(ei[:, :0], ew[:0], [0, 0], 0.5)
    with pytest.raises(ValueError, match=r"slide 1: edge_ptr must end at 10 \(got 9\)"):
        wt.filter_edges_by_median_segmented(ei, ew, [0, 4, 9], 0.5)
    with pytest.raises(ValueError, match="slide 1: edge_ptr decreases"):
        wt.filter_edges_by_median_segmented(ei, ew, [0, 6, 4, 10], 0.5)
    with pytest.raises(ValueError, match=r"edge_index \[2, E\] and edge_weights \[E\]"):
        wt.filter_edges_by_median_segmented(ei[:, :9], ew, [0, 10], 0.5)


def test_valid_input_reaches_the_device_check(monkeypatch):
    """With nothing to object to, CPU tensors fail at the device, not at an argument: no host path computes anything."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    wt = _wt()
    ok = dict(wsi_ptr=[0, 5, 10], tma_ptr=[0, 3, 6])
    with pytest.raises(RuntimeError, match="ROCm"):
        wt.compute_wsi_tma_similarity_segmented(torch.randn(10, 8), torch.zeros(10, 2), torch.randn(6, 8), **ok)
    with pytest.raises(RuntimeError, match="ROCm"):
        wt.sim_dense_stats_segmented(torch.randn(10, 8), torch.randn(6, 8), x_ptr=[0, 5, 10], y_ptr=[0, 3, 6])
    with pytest.raises(RuntimeError, match="ROCm"):
        wt.lower_median_segmented(torch.rand(10), ptr=[0, 4, 10])
    with pytest.raises(RuntimeError, match="ROCm"):
        wt.group_by_similarity_segmented(torch.rand(30), 2, **ok)
    with pytest.raises(RuntimeError, match="ROCm"):
        wt.filter_edges_by_median_segmented(torch.zeros((2, 10), dtype=torch.int64), torch.rand(10), [0, 4, 10], 0.5)


# ---- pure functions --------------------------------------------------------------------------------------------------
def test_width_plan_groups_slides_by_tma_count():
    wt = _wt()
    # repeated widths out of order, one unique width
    n_sizes, m_sizes = [5, 7, 4, 9, 6, 3], [40, 16, 40, 33, 16, 40]
    plan = wt.width_plan(n_sizes, m_sizes)
    assert [f["width"] for f in plan] == [40, 16, 33]                      # order of first appearance
    assert [f["slides"] for f in plan] == [[0, 2, 5], [1, 4], [3]]
    assert [f["fit_ptr"] for f in plan] == [[0, 5, 9, 12], [0, 7, 13], [0, 9]]
    assert [f["adjacent"] for f in plan] == [False, False, True]
    # every slide lands in exactly one fit, and the labels of fit rows fit_ptr[i]:fit_ptr[i+1] are the n_s labels of its slide
    seen = sorted(s for f in plan for s in f["slides"])
    assert seen == list(range(6))
    for f in plan:
        for i, s in enumerate(f["slides"]):
            assert f["fit_ptr"][i + 1] - f["fit_ptr"][i] == n_sizes[s] and m_sizes[s] == f["width"]
    # one width: one fit over adjacent slides (a view of S_flat, no copy)
    one = wt.width_plan([100] * 8, [64] * 8)
    assert len(one) == 1 and one[0]["slides"] == list(range(8)) and one[0]["adjacent"] and one[0]["fit_ptr"][-1] == 800
    # all widths distinct: S fits of one slide each
    many = wt.width_plan([4, 5, 6], [7, 8, 9])
    assert [f["slides"] for f in many] == [[0], [1], [2]] and all(f["adjacent"] for f in many)
    # adjacent runs that do not start at slide 0
    run = wt.width_plan([3, 4, 5, 6], [9, 8, 8, 8])
    assert [(f["slides"], f["adjacent"]) for f in run] == [([0], True), ([1, 2, 3], True)]
    assert wt.width_plan([], []) == []


def test_similarity_block_is_a_view():
    wt = _wt()
    sizes = [(2, 3), (1, 1), (4, 2)]
    s_ptr = [0, 6, 7, 15]
    flat = torch.arange(15, dtype=torch.float32)
    for s, (n_s, m_s) in enumerate(sizes):
        b = wt.similarity_block(flat, s_ptr, sizes, s)
        assert b.shape == (n_s, m_s) and b.data_ptr() == flat[s_ptr[s]:].data_ptr()
        assert b.reshape(-1).tolist() == list(range(s_ptr[s], s_ptr[s + 1]))


def test_threshold_rounding_is_torchs_own_scalar_comparison():
    """`weights >= median.item() * ratio` (the reference's line) compares an f32 tensor with a Python float; the filter compares
    with the f32 rounding of that float64 product.  Element for element the same decisions, ties and neighbours included."""
    wt = _wt()
    rng = np.random.RandomState(5)
    med = torch.from_numpy(np.concatenate([rng.rand(300), [0.0, 1.0, 1e-30, 3e38, 0.1, 1 / 3]]).astype(np.float32))
    for ratio in (0.8, 1.0, 1.25, 0.1, 1 / 3, 7.0):
        thr64, thr32 = wt.median_thresholds(med, ratio)
        assert thr64.dtype == torch.float64 and thr32.dtype == torch.float32
        for i in range(med.numel()):
            t = med[i].item() * ratio                                      # the reference's Python float
            assert thr64[i].item() == t
            with np.errstate(over="ignore"):
                c = np.float32(t)                                          # 3e38 * 7 rounds to inf, as torch's rounding does
            w = torch.from_numpy(np.concatenate([rng.rand(64).astype(np.float32), np.array(
                [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf)),
                 np.nextafter(np.nextafter(c, np.float32(np.inf)), np.float32(np.inf))], np.float32)]))
            assert torch.equal(w >= t, w >= thr32[i]), (ratio, i)


def _cohort_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Cohort entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_cohort_table_equals_the_gpu_tests_table():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_wsi_tma_segmented import SYNC_COHORT
    import multimodal_fusion_amd as mmf
    rows = _cohort_table()
    assert rows == SYNC_COHORT, (rows, SYNC_COHORT)
    assert set(rows) == set(mmf._lib.EXPORTS_COHORT)                      # every entry of the second list has its row
    assert {s for s, _ in rows.values()} <= {"none", "once", "per iteration", "data-dependent"}
    # the pinned table of §6 and the second list do not overlap
    from test_stream_arguments_cpu import integration_table
    assert not set(integration_table()) & set(rows)


def test_new_code_names_the_callers_stream():
    """The static scan of tests/test_stream_arguments_cpu.py covers the new launches too: none on the null stream, no new
    blocking call, and the new kernels are really launched from the files the scan reads."""
    from test_stream_arguments_cpu import stream_uses, is_null
    launched = " ".join(a[0] for _, _, what, _, a in stream_uses() if what == "hipLaunchKernelGGL")
    for kernel in ("rbf_direct_pivot_seg_kernel", "DirectSegTables", "stats_final_seg_kernel", "stats_median_seg_kernel",
                   "seg_median_hist_kernel<FLAT>"):
        assert kernel in launched, kernel
    assert not [u for u in stream_uses() if is_null(u[3]) and not u[2].startswith("hipcub::")]
