"""Ragged-width segmented KMeans without a GPU (include/ext/mmf_hg_kmeans_ragged.h): the header declares exactly
the new entries, the library exports them and the binding registers them in a list of its own; the group planner — queried on the
host through mmf_kmeans_ragged_groups — keeps the lockstep limits and the padding rule; every argument error of the entry and of
the Python functions is raised before a device is needed and names the segment; and the driver returns labels, centres and info
in the caller's segment order (checked with a stubbed binding)."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join("ext", "mmf_hg_kmeans_ragged.h")
ENTRIES = ["mmf_kmeans_fit_ragged", "mmf_kmeans_ragged_groups"]
OTHER_LISTS = ["EXPORTS", "EXPORTS_COHORT", "EXPORTS_POOL", "EXPORTS_STREAM", "EXPORTS_TOPK", "EXPORTS_WIDE", "EXPORTS_WIDE_SEG",
               "EXPORTS_TOPK16", "EXPORTS_TOPK16_SEG", "EXPORTS_TOPK_XY", "EXPORTS_SEG_EXACT"]
INVALID, UNSUPPORTED = -1, -2


def _mmf():
    import multimodal_fusion_amd as m
    return m


def _kr():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.kmeans_ragged")


def _declared(path):
    with open(os.path.join(ROOT, "include", path)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding, build ------------------------------------------------------------------------------------
def test_header_declares_exactly_the_new_entries():
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
    for words in ("bit for bit", "never zero-padded", "rows local to the segment", "before any device call", "the first bad segment",
                  "device_id < 0 ->\n * MMF_E_UNSUPPORTED first", "exceed twice", "Host only", "once per Lloyd iteration"):
        assert words in h, words
    with open(os.path.join(inc, "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()


def test_library_and_binding_export_the_entries_from_a_list_of_their_own():
    mmf = _mmf()
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_KMEANS_RAGGED) == ENTRIES and all(hasattr(L, e) for e in ENTRIES)
    for name in OTHER_LISTS:
        assert not set(ENTRIES) & set(getattr(mmf._lib, name)), name
    lib = mmf._lib.lib()
    assert len(lib.mmf_kmeans_fit_ragged.argtypes) == 19 and lib.mmf_kmeans_fit_ragged.restype is ctypes.c_int
    assert len(lib.mmf_kmeans_ragged_groups.argtypes) == 8 and lib.mmf_kmeans_ragged_groups.restype is ctypes.c_int64
    assert mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_build_lists_the_header_and_the_integration_table_names_the_entries():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_kmeans_ragged", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", HEADER)) for h in b.HEADERS)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        section = re.split(r"^## [0-9. ]*Ragged KMeans entries$", f.read(), 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = dict(re.findall(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|", section, flags=re.M))
    assert rows == {"mmf_kmeans_fit_ragged": "per iteration", "mmf_kmeans_ragged_groups": "host only: no device, no stream"}


def test_module_and_functions_are_exported():
    mmf, kr = _mmf(), _kr()
    assert mmf.kmeans_ragged is kr and "kmeans_ragged" in mmf.__all__
    for name in ("kmeans_fit_ragged", "kmeans_fit_predict_ragged", "ragged_groups"):
        assert getattr(mmf, name) is getattr(kr, name) and name in mmf.__all__
    assert list(inspect.signature(kr.kmeans_fit_ragged).parameters) == ["V", "xoff", "rows", "widths", "n_clusters", "first_centres", "uniforms",
                                                                        "max_iter", "tol", "return_seeds"]
    sig = inspect.signature(kr.kmeans_fit_predict_ragged)
    assert list(sig.parameters) == ["V_flat", "n_clusters", "rows", "widths", "xoff", "n_init", "max_iter", "tol", "seed", "return_info"]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters)[2:])
    assert (sig.parameters["n_init"].default, sig.parameters["max_iter"].default, sig.parameters["tol"].default,
            sig.parameters["seed"].default, sig.parameters["xoff"].default) == (10, 300, 1e-4, 42, None)
    assert list(inspect.signature(kr.ragged_groups).parameters) == ["rows", "widths", "n_clusters", "n_init"]
    # the grouping step keeps its signature and width_plan
    wt = import_module("multimodal_fusion_amd.wsi_tma_similarity")
    assert list(inspect.signature(wt.group_by_similarity_segmented).parameters) == ["S_flat", "num_groups", "wsi_ptr", "wsi_batch", "tma_ptr",
                                                                                    "tma_batch", "method"]
    assert [f["width"] for f in wt.width_plan([3, 4, 5], [7, 9, 7])] == [7, 9]


# ---- the group planner ---------------------------------------------------------------------------------------------------
def _ds(w):
    return (w + 31) // 32 * 32


def _restated_groups(rows, widths, k, n_init=10):
    """The planner's rules without the scratch bound: at most 16384 restarts-times-clusters and fewer than 2^31 label slots per
    group; a group closes before a segment that would make sum rows * ds_g exceed twice sum rows * ds_own."""
    bounds, s0, n = [0], 0, len(rows)
    while s0 < n:
        s1, nr, dmax, own = s0 + 1, rows[s0], widths[s0], rows[s0] * _ds(widths[s0])
        while s1 < n:
            nr2, d2, own2 = nr + rows[s1], max(dmax, widths[s1]), own + rows[s1] * _ds(widths[s1])
            if (s1 + 1 - s0) * n_init * k > 16384 or nr2 * n_init >= 2 ** 31 or nr2 * _ds(d2) > 2 * own2:
                break
            nr, dmax, own, s1 = nr2, d2, own2, s1 + 1
        bounds.append(s1)
        s0 = s1
    ds = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        ds += [_ds(max(widths[a:b]))] * (b - a)
    return bounds, ds


PLANS = {
    "one_width": ([40, 100, 64], [64, 64, 64], 4),
    "case_1_of_the_gpu_test": ([12, 33, 40, 64, 100, 257, 300], [33, 130, 1, 65, 7, 31, 32], 10),
    "wide_block_in_the_middle": ([40] * 4, [8, 8, 2000, 8], 5),
    "wide_block_last": ([40] * 4, [8, 8, 8, 2000], 5),
    "wide_block_first": ([40, 40, 40], [2000, 8, 8], 5),
    "exactly_twice": ([10, 10], [32, 96], 3),            # 20 x 96 = 1920 <= 2 x (320 + 960) = 2560; and [32, 97]: 20 x 128 = 2560 <= 2 x 1600
    "segment_limit": ([15] * 170, [(5, 40, 70)[s % 3] for s in range(170)], 10),
    "segment_limit_k_100": ([120] * 40, [16, 48] * 20, 100),          # 16 segments of 1000 restart-clusters per group
    "1000_slides": (np.random.RandomState(1).randint(40, 501, 1000).tolist(), np.random.RandomState(2).randint(16, 201, 1000).tolist(), 10),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_planner_keeps_the_limits_and_the_padding_rule(name):
    kr = _kr()
    rows, widths, k = PLANS[name]
    for label, order in (("as given", np.arange(len(rows))), ("sorted", np.argsort((np.array(widths) + 31) // 32, kind="stable"))):
        r, w = np.array(rows)[order].tolist(), np.array(widths)[order].tolist()
        bounds, ds = kr.ragged_groups(r, w, k)
        assert (bounds, ds) == _restated_groups(r, w, k), (name, label)
        assert bounds[0] == 0 and bounds[-1] == len(r) and all(a < b for a, b in zip(bounds[:-1], bounds[1:]))
        for a, b in zip(bounds[:-1], bounds[1:]):
            assert (b - a) * 10 * k <= 16384 and len(set(ds[a:b])) == 1 and ds[a] == _ds(max(w[a:b]))
            assert sum(r[a:b]) * ds[a] <= 2 * sum(n * _ds(d) for n, d in zip(r[a:b], w[a:b])) or b - a == 1
    if name == "wide_block_in_the_middle":
        assert kr.ragged_groups(rows, widths, k) == ([0, 2, 4], [32, 32, 2016, 2016])
    if name == "segment_limit":
        assert kr.ragged_groups(rows, widths, k)[0] == [0, 163, 170]
    if name == "1000_slides":                              # sorted by internal width, the padding rule never cuts: only the segment limit does
        order = np.argsort((np.array(widths) + 31) // 32, kind="stable")
        b, _ = kr.ragged_groups(np.array(rows)[order], np.array(widths)[order], k)
        assert b == list(range(0, 1000, 163)) + [1000]


def test_planner_bounds_the_rows_and_the_scratch_of_a_group():
    kr = _kr()
    # the scratch bound (2 GiB per group): 200000 x 512 blocks are 400 MB of centred rows each, no other limit is near.  The label
    # rows alone take 16 n_init bytes per row, so a group under the scratch bound is under n_init * rows < 2^31 as well.
    bounds, ds = kr.ragged_groups([200_000] * 12, [512] * 12, 10)
    assert len(bounds) > 3 and all(2 <= b - a <= 4 for a, b in zip(bounds[:-2], bounds[1:-1])) and set(ds) == {512}
    bounds, _ = kr.ragged_groups([300_000_000] * 3, [1] * 3, 1, n_init=2)      # (the query allocates nothing)
    assert bounds == [0, 1, 2, 3]
    # one segment alone is always a group
    assert kr.ragged_groups([3_000_000], [4096], 10) == ([0, 1], [4096])


def test_planner_query_checks_its_arguments():
    kr = _kr()
    with pytest.raises(ValueError, match=r"segment 1: n_samples=3 should be >= n_clusters=4"):
        kr.ragged_groups([10, 3], [5, 5], 4)
    with pytest.raises(ValueError, match=r"segment 2: width 0 must be >= 1"):
        kr.ragged_groups([10, 10, 10], [5, 5, 0], 4)
    with pytest.raises(ValueError, match="widths must be a 1-D sequence of 2 entries"):
        kr.ragged_groups([10, 10], [5], 4)
    with pytest.raises(ValueError, match="n_seg >= 1"):
        kr.ragged_groups([], [], 4)
    with pytest.raises(RuntimeError, match="16384"):
        kr.ragged_groups([3000], [8], 2000)
    with pytest.raises(RuntimeError, match=r"segment 1: n_init \* n_samples must be < 2\^31"):
        kr.ragged_groups([10, 2 ** 31 // 10 + 1], [1, 1], 1)
    L = _mmf()._lib.lib()
    r = (ctypes.c_int64 * 2)(10, 10)
    assert L.mmf_kmeans_ragged_groups(ctypes.cast(r, ctypes.c_void_p), ctypes.cast(r, ctypes.c_void_p), 2, 2, 10, 2, None, None) == INVALID
    assert "kmeans_ragged_groups: NULL pointer" in L.mmf_last_error().decode()
    assert L.mmf_kmeans_ragged_groups(None, ctypes.cast(r, ctypes.c_void_p), 2, 2, 10, 2, ctypes.cast(r, ctypes.c_void_p), None) == INVALID
    assert L.mmf_kmeans_ragged_groups(ctypes.cast(r, ctypes.c_void_p), ctypes.cast(r, ctypes.c_void_p), 2, 2, 10, 65, ctypes.cast(r, ctypes.c_void_p),
                                      None) == UNSUPPORTED
    assert "trials = 65" in L.mmf_last_error().decode()


# ---- the entry's host checks, with host buffers standing in for device pointers --------------------------------------------
def _arr(v, ct=ctypes.c_int64):
    return None if v is None else ctypes.cast((ct * len(v))(*v), ctypes.c_void_p)


def _entry(**kw):
    L = _mmf()._lib.lib()
    buf = ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)
    a = dict(V=buf, n_values=200, xoff=[0, 100], rows=[10, 10], width=[10, 5], n_seg=2, k=3, n_init=2, trials=3, first=[0, 9, 5, 5],
             u=[0.5] * 12, max_iter=300, tol=1e-4, labels=buf, device=63)
    a.update(kw)
    rc = L.mmf_kmeans_fit_ragged(a["V"], a["n_values"], _arr(a["xoff"]), _arr(a["rows"]), _arr(a["width"]), a["n_seg"], a["k"], a["n_init"],
                                 a["trials"], _arr(a["first"]), _arr(a["u"], ctypes.c_double), a["max_iter"], a["tol"], a["labels"], None, None,
                                 None, a["device"], None)
    return rc, L.mmf_last_error().decode()


ENTRY_ERRORS = [
    (dict(device=-1), UNSUPPORTED, "device_id -1: no CPU path"),
    (dict(device=-1, rows=[1, 10]), UNSUPPORTED, "device_id -1"),                    # before every other check
    (dict(rows=[10, 2]), INVALID, "segment 1: n_samples=2 should be >= n_clusters=3."),
    (dict(width=[0, 5]), INVALID, "segment 0: width 0 must be >= 1"),
    (dict(xoff=[0, -1]), INVALID, "segment 1: block [-1, -1 + 10 x 5) outside the 200 values of V"),
    (dict(xoff=[0, 151]), INVALID, "segment 1: block [151, 151 + 10 x 5) outside the 200 values of V"),
    (dict(n_values=99), INVALID, "segment 0: block [0, 0 + 10 x 10) outside the 99 values of V"),
    (dict(first=[0, 9, 5, 10]), INVALID, "segment 1: first_centres[1] outside [0, n_samples)"),
    (dict(first=[-1, 9, 5, 5]), INVALID, "segment 0: first_centres[0] outside [0, n_samples)"),
    (dict(V=None), INVALID, "NULL pointer"),
    (dict(xoff=None), INVALID, "NULL pointer"),
    (dict(rows=None), INVALID, "NULL pointer"),
    (dict(width=None), INVALID, "NULL pointer"),
    (dict(first=None), INVALID, "NULL pointer"),
    (dict(u=None), INVALID, "NULL pointer"),
    (dict(labels=None), INVALID, "NULL pointer"),
    (dict(n_seg=0), INVALID, "n_seg >= 1"),
    (dict(k=0), INVALID, "n_clusters >= 1"),
    (dict(n_init=0), INVALID, "n_init >= 1"),
    (dict(trials=0), INVALID, "trials >= 1"),
    (dict(max_iter=0), INVALID, "max_iter >= 1"),
    (dict(tol=-1.0), INVALID, "tol >= 0"),
    (dict(trials=65), UNSUPPORTED, "trials = 65 above the supported 64"),
    (dict(k=9000, rows=[9000, 9000], xoff=[0, 0], width=[1, 1], n_values=9000), UNSUPPORTED, "n_init * n_clusters = 18000 above the supported 16384"),
    (dict(k=1, u=None, rows=[10, 2 ** 30], width=[1, 1], xoff=[0, 0], n_values=2 ** 30), UNSUPPORTED, "segment 1: n_init * n_samples must be < 2^31"),
]


@pytest.mark.parametrize("kw,rc,words", ENTRY_ERRORS, ids=[str(i) for i in range(len(ENTRY_ERRORS))])
def test_entry_checks_its_arguments_before_any_device_call(kw, rc, words):
    got, msg = _entry(**kw)
    assert got == rc and words in msg and msg.startswith("kmeans_fit_ragged: "), (got, msg)


# ---- the Python functions' host checks: raised on CPU tensors, before the "needs a ROCm device" error ------------------------
def test_python_argument_errors_need_no_device():
    kr = _kr()
    V = torch.rand(200)
    with pytest.raises(ValueError, match=r"kmeans_fit_predict_ragged: segment 1: n_samples=2 should be >= n_clusters=3"):
        kr.kmeans_fit_predict_ragged(V, 3, rows=[10, 2], widths=[10, 5])
    with pytest.raises(ValueError, match=r"kmeans_fit_predict_ragged: segment 0: width 0 must be >= 1"):
        kr.kmeans_fit_predict_ragged(V, 3, rows=[10, 10], widths=[0, 5])
    with pytest.raises(ValueError, match=r"segment 1: block \[100, 100 \+ 10 x 11\) outside the 200 values of V"):
        kr.kmeans_fit_predict_ragged(V, 3, rows=[10, 10], widths=[10, 11])
    with pytest.raises(ValueError, match=r"segment 0: block \[-4, "):
        kr.kmeans_fit_predict_ragged(V, 3, rows=[10, 10], widths=[10, 5], xoff=[-4, 100])
    with pytest.raises(ValueError, match="xoff must be a 1-D sequence of 2 entries"):
        kr.kmeans_fit_predict_ragged(V, 3, rows=[10, 10], widths=[10, 5], xoff=[0])
    with pytest.raises(ValueError, match="widths must be a 1-D sequence of 2 entries"):
        kr.kmeans_fit_predict_ragged(V, 3, rows=[10, 10], widths=[10])
    with pytest.raises(ValueError, match="at least one segment"):
        kr.kmeans_fit_predict_ragged(V, 3, rows=[], widths=[])
    with pytest.raises(ValueError, match="flat 1-D buffer"):
        kr.kmeans_fit_predict_ragged(V.view(20, 10), 3, rows=[10, 10], widths=[10, 5])
    with pytest.raises(ValueError, match=r"segment 0: n_samples=10 should be >= n_clusters=0"):
        kr.kmeans_fit_predict_ragged(V, 0, rows=[10, 10], widths=[10, 5])
    with pytest.raises(RuntimeError, match="ROCm device"):                 # a good call on a CPU tensor: only now the device error
        kr.kmeans_fit_predict_ragged(V, 3, rows=[10, 10], widths=[10, 5])
    # the thin binding
    first, u = np.zeros((2, 10), np.int64), np.full((10, 2, 3), 0.5)
    with pytest.raises(ValueError, match=r"kmeans_fit_ragged: segment 1: first_centres\[3\] outside \[0, n_samples\)"):
        bad = first.copy()
        bad[1, 3] = 10
        kr.kmeans_fit_ragged(V, [0, 100], [10, 10], [10, 5], 3, bad, u)
    with pytest.raises(ValueError, match=r"first_centres must be \[n_seg, n_init\]"):
        kr.kmeans_fit_ragged(V, [0, 100], [10, 10], [10, 5], 3, first[:1], u)
    with pytest.raises(ValueError, match=r"uniforms must be \[n_init, n_clusters - 1, trials\]"):
        kr.kmeans_fit_ragged(V, [0, 100], [10, 10], [10, 5], 3, first, u[:, :1])
    with pytest.raises(ValueError, match=r"segment 1: block \[195, "):
        kr.kmeans_fit_ragged(V, [0, 195], [10, 10], [10, 5], 3, first, u)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kr.kmeans_fit_ragged(V, [0, 100], [10, 10], [10, 5], 3, first, u)
    # the grouping step still raises its own errors first
    wt = import_module("multimodal_fusion_amd.wsi_tma_similarity")
    with pytest.raises(ValueError, match=r"slide 1: n_samples=2 should be >= n_clusters=3"):
        wt.group_by_similarity_segmented(torch.rand(5 * 4 + 2 * 7), 3, wsi_ptr=[0, 5, 7], tma_ptr=[0, 4, 11])


# ---- the driver's order of segments and the way back, with a stubbed binding ---------------------------------------------
def test_driver_sorts_by_internal_width_and_returns_the_callers_order(monkeypatch):
    kr = _kr()
    rows, widths = [12, 5, 9, 7, 6, 8], [70, 5, 33, 32, 200, 1]            # internal widths 96, 32, 64, 32, 224, 32
    xoff = [1000, 0, 3000, 5000, 7000, 9000]
    k, seen = 3, {}

    def stub(V, xo, r, w, n_clusters, first, u, *, max_iter, tol, return_seeds=False):
        seen.update(xoff=list(xo), rows=list(r), widths=list(w), first=np.array(first), u=u, max_iter=max_iter, tol=tol)
        # row j of the segment stored at xo[i] gets the label xo[i] + j; its centres and its inertia hold xo[i]
        labels = torch.cat([torch.arange(n, dtype=torch.int64) + int(x) for x, n in zip(xo, r)])
        cen = torch.cat([torch.full((n_clusters * int(ww),), float(x)) for x, ww in zip(xo, w)])
        info = [{"inertia": float(x), "ambiguous_draws": 0, "ambiguous_trials": 0} for x in xo]
        return labels, cen, info
    monkeypatch.setattr(kr, "kmeans_fit_ragged", stub)
    monkeypatch.setattr(kr.ops, "_need_gpu", lambda t, what: None)
    labels, centres, inertia, info = kr.kmeans_fit_predict_ragged(torch.zeros(12000), k, rows=rows, widths=widths, xoff=xoff, max_iter=7, tol=0.5,
                                                                  return_info=True)
    order = [1, 3, 5, 2, 0, 4]                                              # stable in the internal width
    assert seen["xoff"] == [xoff[s] for s in order] and seen["rows"] == [rows[s] for s in order] and seen["widths"] == [widths[s] for s in order]
    km = import_module("multimodal_fusion_amd.kmeans")
    first, u = km.segment_streams(42, 10, k, rows)                          # the stream depends on the rows only, and follows its segment
    assert np.array_equal(seen["first"], first[order]) and np.array_equal(seen["u"], u) and (seen["max_iter"], seen["tol"]) == (7, 0.5)
    want = torch.cat([torch.arange(n, dtype=torch.int64) + x for x, n in zip(xoff, rows)])
    assert torch.equal(labels, want)
    assert [tuple(c.shape) for c in centres] == [(k, w) for w in widths] and [float(c[0, 0]) for c in centres] == [float(x) for x in xoff]
    assert inertia.tolist() == [float(x) for x in xoff] and [i["inertia"] for i in info] == inertia.tolist()
    # already sorted: no indexed store, the binding's tensor is returned as it is
    labels2, _, _ = kr.kmeans_fit_predict_ragged(torch.zeros(12000), k, rows=[5, 7, 12], widths=[5, 32, 70], xoff=[0, 5000, 1000])
    assert seen["xoff"] == [0, 5000, 1000] and torch.equal(labels2, torch.cat([torch.arange(5), torch.arange(7) + 5000, torch.arange(12) + 1000]))
    # xoff None: the blocks back to back
    kr.kmeans_fit_predict_ragged(torch.zeros(12000), k, rows=[5, 7], widths=[40, 3])
    assert seen["xoff"] == [200, 0] and seen["widths"] == [3, 40]
