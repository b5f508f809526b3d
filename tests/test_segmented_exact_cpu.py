"""The segmented exact scan without a GPU (include/ext/mmf_hg_seg_exact.h): the header declares exactly the new
entries, the library exports them and the binding registers them in a list of its own, the entries run their host checks before
any device call and name themselves, the Python functions raise their argument errors on the host, and the work table — queried
on the host — covers every (query row, column tile) pair of every served segment exactly once."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_simtopk_segmented_exact", "mmf_simtopk_combined_segmented_exact", "mmf_segmented_exact_table"]
OTHER_LISTS = ["EXPORTS", "EXPORTS_COHORT", "EXPORTS_POOL", "EXPORTS_STREAM", "EXPORTS_TOPK", "EXPORTS_WIDE", "EXPORTS_WIDE_SEG",
               "EXPORTS_TOPK16", "EXPORTS_TOPK16_SEG", "EXPORTS_TOPK_XY"]
OPS_PUBLIC = ["Segments", "array_stats", "clique_pairs", "combined_offdiag_median", "combined_threshold_edges", "edge_cosine",
              "fast_scan_supported", "kmeans_fit", "kmeans_fit_segmented", "knn_clique_edges", "knn_pairs", "last_query_order",
              "lower_median", "offdiag_lower_median", "offdiag_lower_median_segmented", "padded_dim", "prep_rows", "row_scalars",
              "segment_mean", "segment_offdiag_mean", "segment_sort", "sim_dense", "sim_dense_combined", "sim_dense_combined_segmented",
              "sim_dense_stats", "simtopk", "simtopk_panels", "simtopk_prepared", "simtopk_segmented", "threshold_edges",
              "threshold_edges_segmented", "topk_merge"]


def _mmf():
    import multimodal_fusion_amd as m
    return m


def _declared(path):
    with open(os.path.join(ROOT, "include", path)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding, build ------------------------------------------------------------------------------------
def test_header_declares_exactly_the_new_entries():
    assert _declared(os.path.join("ext", "mmf_hg_seg_exact.h")) == set(ENTRIES)
    inc = os.path.join(ROOT, "include")
    for base, _, files in os.walk(inc):
        for f in files:
            rel = os.path.relpath(os.path.join(base, f), inc)
            if rel != os.path.join("ext", "mmf_hg_seg_exact.h"):
                assert not _declared(rel) & set(ENTRIES), rel
    with open(os.path.join(inc, "ext", "mmf_hg_seg_exact.h")) as f:
        h = f.read()
    assert '#include "../mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")
    for words in ("bit for bit", "row_offset = x_ptr[s], col_offset = y_ptr[s]", "k + self > 44 runs passes", "power of two",
                  "before any device call", "device_id < 0 -> MMF_E_UNSUPPORTED first", "k + self <= 44", "Host only"):
        assert words in h, words
    with open(os.path.join(inc, "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()


def test_library_and_binding_export_the_entries_from_a_list_of_their_own():
    mmf = _mmf()
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_SEG_EXACT) == ENTRIES and all(hasattr(L, e) for e in ENTRIES)
    for name in OTHER_LISTS:
        assert not set(ENTRIES) & set(getattr(mmf._lib, name)), name
    lib = mmf._lib.lib()
    assert tuple(lib.mmf_simtopk_segmented_exact.argtypes) == tuple(lib.mmf_simtopk_segmented.argtypes)
    assert tuple(lib.mmf_simtopk_combined_segmented_exact.argtypes) == tuple(lib.mmf_simtopk_combined.argtypes)
    assert lib.mmf_simtopk_segmented_exact.restype is ctypes.c_int and lib.mmf_segmented_exact_table.restype is ctypes.c_int64
    assert mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_build_lists_the_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_seg_exact", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", "ext", "mmf_hg_seg_exact.h")) for h in b.HEADERS)


def test_module_and_functions_are_exported_and_ops_is_unchanged():
    mmf = _mmf()
    se = import_module("multimodal_fusion_amd.segmented_exact")
    assert mmf.segmented_exact is se
    for name in ("simtopk_segmented_exact", "simtopk_combined_exact", "segmented_exact_table"):
        assert getattr(mmf, name) is getattr(se, name) and name in mmf.__all__
    assert "segmented_exact" in mmf.__all__ and mmf.simtopk_segmented is mmf.ops.simtopk_segmented      # the router is not the top-level name
    public = sorted(n for n, v in vars(mmf.ops).items() if not n.startswith("_") and getattr(v, "__module__", None) == mmf.ops.__name__)
    assert public == sorted(OPS_PUBLIC)
    sig = inspect.signature(se.simtopk_segmented_exact)
    assert list(sig.parameters) == ["X", "Y", "ptr", "batch", "y_ptr", "y_batch", "metric", "lam", "k", "exclude_self", "col_splits",
                                    "return_stats", "profile"]
    assert list(inspect.signature(se.simtopk_segmented).parameters) == list(inspect.signature(mmf.wide_scan.simtopk_segmented).parameters)
    assert list(inspect.signature(se.simtopk_combined_exact).parameters) == list(inspect.signature(mmf.combined_topk.simtopk_combined).parameters)


# ---- the entries' host checks, with host buffers standing in for device pointers ------------------------------------------
def _ptr(v):
    return None if v is None else ctypes.cast((ctypes.c_int64 * len(v))(*v), ctypes.c_void_p)


def _plain(**kw):
    mmf = _mmf()
    L = mmf._lib.lib()
    b = ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)
    a = dict(X=b, n=8, Y=None, m=0, d=600, dtype=0, metric=1, lam=1.0, k=2, self=1, xp=[0, 3, 8], yp=None, S=2, idx=b, val=b, opts=None, device=63)
    a.update(kw)
    opts = None if a["opts"] is None else ctypes.byref(mmf._lib.SimtopkOpts(*a["opts"]))
    rc = L.mmf_simtopk_segmented_exact(a["X"], a["n"], a["Y"], a["m"], a["d"], a["dtype"], a["metric"], a["lam"], a["k"], a["self"], _ptr(a["xp"]),
                                       _ptr(a["yp"]), a["S"], a["idx"], a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


def _combined(**kw):
    mmf = _mmf()
    L = mmf._lib.lib()
    b = ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)
    a = dict(F=b, P=b, n=8, d=600, dp=2, lh=0.5, lg=0.5, k=2, self=1, ptr=[0, 3, 8], S=2, idx=b, val=b, opts=None, device=63)
    a.update(kw)
    opts = None if a["opts"] is None else ctypes.byref(mmf._lib.SimtopkOpts(*a["opts"]))
    rc = L.mmf_simtopk_combined_segmented_exact(a["F"], a["P"], a["n"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], _ptr(a["ptr"]), a["S"],
                                                a["idx"], a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


INVALID = -1
UNSUPPORTED = -2
PLAIN = [
    (dict(xp=[1, 3, 8]), INVALID, "x_ptr must start at 0"),
    (dict(xp=[0, 5, 3, 8], S=3), INVALID, "x_ptr decreases at segment 1"),
    (dict(xp=[0, 3, 7]), INVALID, "x_ptr must end at 8"),
    (dict(xp=None), INVALID, "host offsets x_ptr"),
    (dict(Y=ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p), m=6, yp=[0, 2, 5]), INVALID, "y_ptr must end at 6"),
    (dict(k=0), INVALID, "k must be >= 1"),
    (dict(X=None), INVALID, "X is NULL"),
    (dict(idx=None), INVALID, "NULL output"),
    (dict(val=None), INVALID, "NULL output"),
    (dict(metric=9), INVALID, "bad metric"),
    (dict(opts=(0, 0, 3, 0, None)), INVALID, "col_splits must be 0 or a power of two (got 3)"),
    (dict(opts=(1, 0, -2, 0, None)), INVALID, "col_splits must be 0 or a power of two"),
    (dict(opts=(7, 0, 0, 0, None)), INVALID, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
    (dict(opts=(2, 0, 0, 0, None)), UNSUPPORTED, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
    (dict(opts=(3, 0, 0, 0, None)), UNSUPPORTED, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
]
COMBINED = [
    (dict(ptr=None), INVALID, "host offsets ptr_host"),
    (dict(ptr=[0, 9, 8]), INVALID, "ptr_host decreases at segment 1"),
    (dict(ptr=[0, 3, 7]), INVALID, "ptr_host must end at 8"),
    (dict(k=0), INVALID, "k must be at least 1"),
    (dict(dp=0), INVALID, "dp must be at least 1"),
    (dict(lh=-1.0), INVALID, "lambda_h must be finite"),
    (dict(P=None), INVALID, "P is NULL"),
    (dict(idx=None), INVALID, "out_idx is NULL"),
    (dict(opts=(0, 0, 6, 0, None)), INVALID, "col_splits must be 0 or a power of two (got 6)"),
    (dict(dp=9), UNSUPPORTED, "dp = 9 > 8"),
    (dict(k=44), UNSUPPORTED, "k + self = 45 > 44"),
    (dict(opts=(2, 0, 0, 0, None)), UNSUPPORTED, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
]


@pytest.mark.parametrize("kw,code,words", PLAIN)
def test_the_entry_refuses_before_any_device_call(kw, code, words):
    """A device id that does not exist: an argument error must win over the device's."""
    rc, msg = _plain(**kw)
    assert rc == code and words in msg and "simtopk_segmented_exact" in msg, (rc, msg)


@pytest.mark.parametrize("kw,code,words", COMBINED)
def test_the_combined_entry_refuses_before_any_device_call(kw, code, words):
    rc, msg = _combined(**kw)
    assert rc == code and words in msg and "simtopk_combined_segmented_exact" in msg, (rc, msg)


def test_a_negative_device_is_refused_first():
    for kw in (dict(), dict(k=0), dict(xp=[1, 3, 8]), dict(idx=None), dict(opts=(0, 0, 3, 0, None)), dict(opts=(2, 0, 0, 0, None))):
        rc, msg = _plain(device=-1, **kw)
        assert rc == UNSUPPORTED and "no CPU path" in msg and "simtopk_segmented_exact" in msg, (rc, msg)
    for kw in (dict(), dict(k=0), dict(ptr=None), dict(k=44)):
        rc, msg = _combined(device=-1, **kw)
        assert rc == UNSUPPORTED and "no CPU path" in msg and "simtopk_combined_segmented_exact" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """k + self beyond 44, every metric's dtype, power-of-two col_splits: the call gets as far as the device (which is not there)."""
    E_HIP = _mmf()._lib.MMF_E_HIP
    for kw in (dict(), dict(k=7), dict(k=100, xp=[0, 0, 8]), dict(opts=(1, 1, 8, 0, None)), dict(opts=(0, 0, 64, 0, None)), dict(d=5000), dict(dtype=1)):
        rc, msg = _plain(**kw)
        assert rc == E_HIP, (kw, rc, msg)
    assert _plain(n=0, xp=[0, 0, 0])[0] == 0 and _plain(n=0, xp=[0], S=0, X=None, idx=None, val=None)[0] == 0
    for kw in (dict(), dict(k=43), dict(k=44, self=0), dict(opts=(1, 0, 2, 0, None))):
        rc, msg = _combined(**kw)
        assert rc == E_HIP, (kw, rc, msg)
    assert _combined(n=0, ptr=[0, 0, 0], F=None, P=None, idx=None, val=None)[0] == 0


def test_python_functions_refuse_on_the_host(monkeypatch):
    mmf = _mmf()
    se = mmf.segmented_exact
    monkeypatch.setattr(mmf._lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    X, P = torch.zeros(8, 16), torch.zeros(8, 2)
    bad = [(lambda: se.simtopk_segmented_exact(X, ptr=[0, 3, 7]), "ptr"),
           (lambda: se.simtopk_segmented_exact(X, ptr=[0, 3, 8], k=0), "k must be >= 1"),
           (lambda: se.simtopk_segmented_exact(X, ptr=[0, 3, 8], col_splits=3), "col_splits must be 0 or a power of two"),
           (lambda: se.simtopk_segmented_exact(X, ptr=[0, 3, 8], y_ptr=[0, 8]), "y_ptr / y_batch need Y"),
           (lambda: se.simtopk_segmented_exact(X, torch.zeros(4, 8), ptr=[0, 8], y_ptr=[0, 4]), "share device, dtype and feature dim"),
           (lambda: se.simtopk_segmented_exact(torch.zeros(8), ptr=[0, 8]), "2-D"),
           (lambda: se.simtopk_combined_exact(X, P, k=0, ptr=[0, 8]), "k must be >= 1"),
           (lambda: se.simtopk_combined_exact(X, P), "needs ptr or batch"),
           (lambda: se.simtopk_combined_exact(X, P[:4], ptr=[0, 8]), "must share N"),
           (lambda: se.simtopk_combined_exact(X, P, ptr=[0, 8], col_splits=-4), "col_splits must be 0 or a power of two"),
           (lambda: se.simtopk_combined_exact(X, P, ptr=[0, 9]), "ptr"),
           (lambda: se.simtopk_segmented(X, ptr=[0, 8], precision="half"), "unknown precision")]
    for fn, words in bad:
        with pytest.raises(ValueError, match=re.escape(words)):
            fn()
    with pytest.raises(RuntimeError, match="no CPU path"):
        se.simtopk_segmented_exact(X, ptr=[0, 3, 8])


# ---- the work table, queried on the host ---------------------------------------------------------------------------------------
SIZES = [33, 0, 1, 257, 5, 6, 128, 31, 129, 32, 98, 385]
CROSS = ([40, 0, 129, 5, 257, 1, 300, 32], [300, 7, 33, 0, 128, 256, 4, 1000])
LARGE = [4096, 4096, 300, 4096, 4096]


def _offsets(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def _restated(xs, ys, xp, yp, k, exclude_self, forced):
    """(served segments, entry count, lists) from the rule of mmf_scan_f32.hip's seg_exact_table, restated."""
    kk = min(k + (1 if exclude_self else 0), 44)
    cap = 16 if kk <= 12 else 32 if kk <= 28 else 48
    max_r = 1
    while 2 * (2 * max_r) * cap <= 1024:
        max_r *= 2
    served = []
    for s, (n, m) in enumerate(zip(xs, ys)):
        overlap = exclude_self and xp[s] < yp[s] + m and xp[s] + n > yp[s]
        if n > 0 and m - (1 if overlap else 0) >= k:
            served.append(s)
    pairs = sum(-(-xs[s] // 128) * -(-ys[s] // 128) for s in served)
    per = max(1, -(-pairs // 1024))
    count, ranges = 0, 1
    for s in served:
        tiles = -(-ys[s] // 128)
        want = forced if forced > 0 else -(-tiles // per)
        r = 1
        while 2 * r <= want and 2 * r <= tiles and 2 * r <= max_r:
            r *= 2
        ranges = max(ranges, r)
        tps = -(-tiles // r)
        count += -(-xs[s] // 128) * -(-tiles // tps)
    return served, count, 2 * ranges, cap


@pytest.mark.parametrize("forced", [0, 1, 2, 4, 64])
@pytest.mark.parametrize("k,exclude_self", [(5, True), (12, True), (28, False), (50, True)])
@pytest.mark.parametrize("xs,ys", [(SIZES, None), CROSS, (LARGE, None)], ids=["ragged self", "cross", "large self"])
def test_the_table_covers_every_pair_of_every_served_segment_once(xs, ys, k, exclude_self, forced):
    mmf = _mmf()
    xp = _offsets(xs)
    yp = xp if ys is None else _offsets(ys)
    ys_ = xs if ys is None else ys
    table, lists = mmf.segmented_exact_table(xp, None if ys is None else yp, k=k, exclude_self=exclude_self, col_splits=forced)
    served, count, want_lists, cap = _restated(xs, ys_, xp, yp, k, exclude_self, forced)
    assert table.shape == (count, 8) and lists == want_lists and lists * cap <= 1024
    covered = {}
    slots = {}
    for seg, row0, nq, cbase, t0, t1, rng, ms in table.tolist():
        assert seg in served and 1 <= nq <= 128
        assert xp[seg] <= row0 and row0 + nq <= xp[seg + 1], "a block straddles a segment"
        assert (row0 - xp[seg]) % 128 == 0 and (nq == 128 or row0 + nq == xp[seg + 1])
        assert cbase == yp[seg] and ms == ys_[seg] and 0 <= t0 < t1 <= -(-ms // 128)
        assert cbase + (t1 - 1) * 128 < yp[-1] and (t1 - 1) * 128 < ms, "a tile starts past the candidates"
        assert 0 <= rng and 2 * rng + 1 < lists
        assert rng not in slots.setdefault(row0, set()), "two entries of a row block share a list slot"
        slots[row0].add(rng)
        for t in range(t0, t1):
            key = (row0, t)
            assert key not in covered, "a (row block, tile) pair is covered twice"
            covered[key] = nq
    want = {(xp[s] + r, t): min(128, xs[s] - r) for s in served for r in range(0, xs[s], 128) for t in range(-(-ys_[s] // 128))}
    assert covered == want
    unserved = set(range(len(xs))) - set(served)
    assert not unserved & {e[0] for e in table.tolist()}
    if forced in (1, 2, 4) and any(-(-ys_[s] // 128) >= forced for s in served):
        assert lists == 2 * forced


def test_the_table_query_refuses_bad_arguments():
    mmf = _mmf()
    for kw, words in ((dict(ptr=[1, 4]), "x_ptr must start at 0"), (dict(ptr=[0, 4, 2]), "decreases"), (dict(ptr=[0, 4], k=0), "k must be >= 1"),
                      (dict(ptr=[0, 4], col_splits=3), "power of two")):
        with pytest.raises(ValueError, match=words):
            mmf.segmented_exact_table(kw.pop("ptr"), **kw)
    L = mmf._lib.lib()
    small = (ctypes.c_int64 * 8)()
    rc = L.mmf_segmented_exact_table(_ptr([0, 300, 600]), None, 2, 5, 1, 0, ctypes.cast(small, ctypes.c_void_p), 1, None)
    assert rc == INVALID and "entries needed" in L.mmf_last_error().decode()


def test_design_readme_and_scripts_name_the_feature():
    for path, words in (("DESIGN.md", ["4.20", "mmf_simtopk_segmented_exact", "segmented_exact_timing.txt", "kernel-resource-usage"]),
                        ("README.md", ["segmented_exact", "segmented_exact_timing"]),
                        (os.path.join("scripts", "segmented_exact_timing.py"), ["--baseline-only", "simtopk_segmented_exact"])):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for w in words:
            assert w in text, (path, w)
    assert os.path.exists(os.path.join(ROOT, "profiles", "segmented_exact_timing.txt"))
