"""The 16-bit cross-segment top-k without a GPU (include/ext/mmf_hg_cross_seg16.h): the header declares exactly the
two new entries, the library exports them and the binding registers them in a list of its own, the entry runs its host checks
before any device call and names itself, the Python functions raise their argument errors on the host, and the work table — queried
on the host — equals a restatement of its rule and, independently, covers for every row each admissible column exactly once and no
excluded one once the mask is applied."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join("ext", "mmf_hg_cross_seg16.h")
ENTRIES = ["mmf_simtopk_cross_segments_fast", "mmf_cross_segments_fast_table"]
INVALID, UNSUPPORTED = -1, -2
SPILL = 192                      # overflow-list slots per row: what the re-rank's 1024 candidates per row leave to the lists


def _mmf():
    import multimodal_fusion_amd as m
    return m


def _declared(path):
    with open(os.path.join(ROOT, "include", path)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding, build ------------------------------------------------------------------------------------------
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
    for words in ("bit for bit", "key descending, then id ascending", "power of two", "before any device call", "no -1 / -inf fill",
                  "Host only", "Host-synchronous: once per call", "select_wait_event is refused", "query_order is ignored",
                  "MMF_PREC_AUTO means MMF_PREC_FAST", "d <= 1024 with k <= 20 and d <= 512 with k <= 44"):
        assert words in h, words


def test_library_and_binding_export_the_entries_from_a_list_of_their_own():
    mmf = _mmf()
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.CROSS_SEG16_EXPORTS) == ENTRIES and all(hasattr(L, e) for e in ENTRIES)
    for name in (n for n in vars(mmf._lib) if n.isupper() and "EXPORTS" in n and n != "CROSS_SEG16_EXPORTS"):
        assert not set(ENTRIES) & set(getattr(mmf._lib, name)), name
    lib = mmf._lib.lib()
    assert list(lib.mmf_simtopk_cross_segments_fast.argtypes) == list(lib.mmf_simtopk_cross_segments.argtypes)
    tab = list(lib.mmf_cross_segments_table.argtypes)
    assert list(lib.mmf_cross_segments_fast_table.argtypes) == tab[:3] + [ctypes.c_int64] + tab[3:]            # + d
    assert lib.mmf_simtopk_cross_segments_fast.restype is ctypes.c_int and lib.mmf_cross_segments_fast_table.restype is ctypes.c_int64
    assert mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_build_lists_the_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_cross_seg16", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", HEADER)) for h in b.HEADERS)


def test_module_and_functions_are_exported():
    mmf = _mmf()
    cs = import_module("multimodal_fusion_amd.cross_segments16")
    assert mmf.cross_segments16 is cs and "cross_segments16" in mmf.__all__ and "mmf.cross_segments16.*" in mmf.__doc__
    for name in ("simtopk_cross_segments_fast", "cross_segments_fast_table"):
        assert getattr(mmf, name) is getattr(cs, name) and name in mmf.__all__
    assert mmf.simtopk_cross_segments is mmf.cross_segments.simtopk_cross_segments                 # the package name stays the exact call
    base = ["X", "Y", "ptr", "batch", "y_ptr", "y_batch", "metric", "lam", "k", "precision", "col_splits", "return_stats", "profile"]
    assert list(inspect.signature(cs.simtopk_cross_segments_fast).parameters) == base
    assert list(inspect.signature(cs.simtopk_cross_segments).parameters) == base
    assert inspect.signature(cs.simtopk_cross_segments_fast).parameters["precision"].default == "fast"
    assert inspect.signature(cs.simtopk_cross_segments).parameters["precision"].default == "auto"
    assert list(inspect.signature(cs.cross_segments_fast_table).parameters) == ["ptr", "y_ptr", "d", "k", "col_splits"]
    assert list(inspect.signature(cs.cross_segment_knn_edges).parameters) == ["X", "ptr", "batch", "k", "precision"]
    assert list(inspect.signature(cs.link_slides).parameters) == ["out", "k", "precision"]
    for fn in (cs.cross_segment_knn_edges, cs.link_slides):
        p = inspect.signature(fn).parameters["precision"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "exact"


# ---- the entry's host checks, with host buffers standing in for device pointers ---------------------------------------------------
def _ptr(v):
    return None if v is None else ctypes.cast((ctypes.c_int64 * len(v))(*v), ctypes.c_void_p)


def _buf():
    return ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)


def _entry(**kw):
    mmf = _mmf()
    L = mmf._lib.lib()
    b = _buf()
    a = dict(X=b, n=8, Y=None, m=0, d=600, dtype=0, metric=1, lam=1.0, k=2, xp=[0, 3, 8], yp=None, S=2, idx=b, val=b, opts=None, device=63)
    a.update(kw)
    opts = None if a["opts"] is None else ctypes.byref(mmf._lib.SimtopkOpts(*a["opts"]))
    rc = L.mmf_simtopk_cross_segments_fast(a["X"], a["n"], a["Y"], a["m"], a["d"], a["dtype"], a["metric"], a["lam"], a["k"], _ptr(a["xp"]),
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
    # the shapes the 16-bit scan does not serve: FAST / FAST_BF16 refuse and name d and k
    (dict(opts=(2, 0, 0, 0, None), d=1100), UNSUPPORTED, "does not support d = 1100, k = 2"),
    (dict(opts=(3, 0, 0, 0, None), d=1100), UNSUPPORTED, "does not support d = 1100, k = 2"),
    (dict(opts=(2, 0, 0, 0, None), n=60, xp=[0, 30, 60], k=21), UNSUPPORTED, "does not support d = 600, k = 21"),
    (dict(opts=(2, 0, 0, 0, None), n=100, xp=[0, 50, 100], d=300, k=45), UNSUPPORTED, "does not support d = 300, k = 45"),
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
    assert rc == code and words in msg and "simtopk_cross_segments_fast" in msg, (rc, msg)


def test_a_negative_device_is_refused_first():
    for kw in (dict(), dict(k=0), dict(xp=[1, 3, 8]), dict(idx=None), dict(opts=(0, 0, 3, 0, None)), dict(opts=(2, 0, 0, 0, None), d=1100),
               dict(k=6), dict(n=-1)):
        rc, msg = _entry(device=-1, **kw)
        assert rc == UNSUPPORTED and "no CPU path" in msg and "simtopk_cross_segments_fast" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """Every precision, dtype and metric, the three list capacities, power-of-two col_splits, AUTO on a shape the scan does not serve
    (the exact driver), an empty segment on either side: the call gets as far as the device (which is not there)."""
    E_HIP = _mmf()._lib.MMF_E_HIP
    big = [0, 100, 300]
    for kw in (dict(), dict(k=3), dict(opts=(0, 1, 8, 0, None)), dict(opts=(1, 0, 0, 0, None)), dict(opts=(2, 0, 64, 0, None)),
               dict(opts=(3, 0, 2, 1, None)), dict(d=40), dict(d=300), dict(d=1024), dict(dtype=1), dict(dtype=2), dict(metric=0),
               dict(metric=2), dict(metric=3, lam=0.5), dict(n=300, xp=big, k=20), dict(n=300, xp=big, k=44, d=512),
               dict(d=5000), dict(opts=(0, 0, 0, 0, None), d=1100), dict(opts=(1, 0, 0, 0, None), n=300, xp=big, k=100),
               dict(n=300, xp=big, k=21), dict(xp=[0, 4, 4, 8], S=3, k=4), dict(Y=_buf(), m=6, yp=[0, 3, 6], k=3),
               dict(Y=_buf(), m=6, yp=[0, 6, 6], xp=[0, 0, 8], k=6)):
        rc, msg = _entry(**kw)
        assert rc == E_HIP, (kw, rc, msg)
    assert _entry(n=0, xp=[0, 0, 0])[0] == 0 and _entry(n=0, xp=[0], S=0, X=None, idx=None, val=None)[0] == 0
    assert _entry(n=0, xp=[0, 0, 0], Y=_buf(), m=6, yp=[0, 2, 6], k=20)[0] == 0


def test_the_entry_makes_every_refusal_before_the_first_device_call_and_keeps_the_exact_entry():
    with open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")) as f:
        raw = f.read()
    body = raw.split("int mmf_simtopk_cross_segments_fast(", 1)[1].split("\n}\n", 1)[0]
    assert body.index(".on_device()") < body.index("set_error(") and body.rindex("set_error(") < body.index("run_segmented_exact(")
    # the one driver of both one-pass 16-bit entries, on its narrow side: the literal `false`, behind this entry's own served test
    narrow_call = "run_cross_segments16(r, self, x_ptr_host, y_ptr_host, n_segments, opts, false)"
    assert body.count("run_cross_segments16(") == 1 and body.index("run_segmented_exact(") < body.index(narrow_call)
    assert "scan_bf16_supported(d, k, in_dtype)" in body
    assert "hipStream" not in body and "hipMemcpy" not in body and "hipDeviceSynchronize" not in body
    assert "run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true)" in body
    table = raw.split("int64_t mmf_cross_segments_fast_table(", 1)[1].split("\n}\n", 1)[0]
    assert "hip" not in table and "Call(" not in table                                          # host only
    assert "run_cross_segments_fast" not in raw and raw.count("static int run_cross_segments16(") == 1
    driver = raw.split("static int run_cross_segments16(", 1)[1].split("\n}\n", 1)[0]
    assert driver.count("launch_scan_b16_xseg(") == 1 and driver.count("launch_scan_b16w_xseg(") == 1
    assert driver.count("launch_select(") == 1 and driver.count("launch_scan_b16_audit(") == 1
    assert driver.count("upload_table(") == 2 and driver.count("flags.read(") == 1 and driver.count("cross_flagged(") == 1
    # one synchronisation (flags.read) when no row is flagged; the second one sits inside the flagged branch
    assert driver.count("hipStreamSynchronize") == 1 and driver.index("if (fallback_rows > 0) {") < driver.index("hipStreamSynchronize")
    # the exact entry still refuses the 16-bit precisions with its own words (tests/test_cross_segments_cpu.py pins them)
    exact = raw.split("int mmf_simtopk_cross_segments(", 1)[1].split("\n}\n", 1)[0]
    assert "no 16-bit scan serves the cross-segment entry yet" in exact


def test_python_functions_refuse_on_the_host(monkeypatch):
    mmf = _mmf()
    cs = mmf.cross_segments16
    X = torch.zeros(8, 16)
    sf = torch.zeros(36, 16)
    out = dict(super_features=sf, group_ptr=torch.tensor([0, 12, 24, 36]), node_ptr=torch.tensor([0, 20, 45, 60]))
    served = mmf.ops.fast_scan_supported
    monkeypatch.setattr(mmf.ops, "fast_scan_supported", lambda d, k, e=True: (d <= 1024 and k <= 20) or (d <= 512 and k <= 44))
    monkeypatch.setattr(mmf._lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    fast, route = cs.simtopk_cross_segments_fast, cs.simtopk_cross_segments
    bad = [(lambda: fast(X, ptr=[0, 3, 7], k=2), "ptr"),
           (lambda: fast(X, ptr=[0, 3, 8], k=0), "k must be >= 1"),
           (lambda: fast(X, ptr=[0, 3, 8], col_splits=3, k=2), "col_splits must be 0 or a power of two"),
           (lambda: fast(X, ptr=[0, 3, 8], col_splits=-4, k=2), "col_splits must be 0 or a power of two"),
           (lambda: fast(X, ptr=[0, 3, 8], y_ptr=[0, 8]), "y_ptr / y_batch need Y"),
           (lambda: fast(X, torch.zeros(4, 8), ptr=[0, 8], y_ptr=[0, 4]), "share device, dtype and feature dim"),
           (lambda: fast(torch.zeros(8), ptr=[0, 8]), "2-D"),
           (lambda: fast(X, ptr=[0, 3, 8], metric="manhattan", k=2), "unknown metric"),
           (lambda: fast(X, ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns (m = 8 minus its own 5 rows of Y), k = 4"),
           (lambda: fast(X, batch=torch.tensor([0, 0, 0, 1, 1, 1, 1, 1]), k=6), "segment 0 has 5 admissible columns"),
           (lambda: fast(X, torch.zeros(6, 16), ptr=[0, 3, 8], y_ptr=[0, 1, 6], k=2), "segment 1 has 1 admissible columns"),
           (lambda: fast(X, k=1), "ptr"),
           (lambda: fast(X, ptr=[0, 3, 8], k=2, precision="exact"), "precision must be 'fast' or 'fast_bf16'"),
           (lambda: fast(X, ptr=[0, 3, 8], k=2, precision="auto"), "precision must be 'fast' or 'fast_bf16'"),
           (lambda: fast(torch.zeros(8, 1100), ptr=[0, 3, 8], k=2), "does not serve d = 1100, k = 2"),
           (lambda: fast(torch.zeros(60, 600), ptr=[0, 30, 60], k=21), "does not serve d = 600, k = 21"),
           (lambda: fast(torch.zeros(100, 300), ptr=[0, 50, 100], k=45, precision="fast_bf16"), "does not serve d = 300, k = 45"),
           (lambda: route(X, ptr=[0, 3, 8], k=2, precision="bf16"), "unknown precision"),
           (lambda: route(X, ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns"),
           (lambda: route(torch.zeros(8, 1100), ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns"),        # auto -> exact: its checks
           (lambda: route(torch.zeros(8, 1100), ptr=[0, 3, 8], k=2, precision="fast"), "does not serve d = 1100, k = 2"),
           (lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], precision="fast"), "precision must be 'exact' or 'auto'"),
           (lambda: cs.cross_segment_knn_edges(X, precision="auto"), "needs ptr or batch"),
           (lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], k=4, precision="auto"), "segment 1 has 3 admissible columns"),
           (lambda: cs.link_slides(out, precision="fast"), "precision must be 'exact' or 'auto'"),
           (lambda: cs.link_slides({"super_features": sf}, precision="auto"), "needs the dict of build_cohort_hypergraphs"),
           (lambda: cs.link_slides(out, k=25, precision="auto"), "segment 0 has 24 admissible columns")]
    for fn, words in bad:
        with pytest.raises(ValueError, match=re.escape(words)):
            fn()
    monkeypatch.undo()
    assert mmf.ops.fast_scan_supported is served
    for call in (lambda: fast(X, ptr=[0, 3, 8], k=3), lambda: route(X, ptr=[0, 3, 8], k=3),
                 lambda: route(torch.zeros(8, 1100), ptr=[0, 3, 8], k=3), lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], k=3, precision="auto")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


# ---- the work table, queried on the host ---------------------------------------------------------------------------------------
# bounds off a tile edge, a block spanning three segments (rows 0 .. 256 hold segments 0, 1, 3), a segment holding whole blocks
RAGGED = [3, 150, 0, 260, 400, 31, 1, 456, 700]
ALIGNED = [256, 32, 0, 512, 64, 128, 1024, 32]              # every bound a multiple of 32, most of 256
ONE_BIG = [2990, 11]                                        # a single segment covering all but k = 11 rows ...
ONE_BIG_LAST = [7, 1500]                                    # ... and the other way round: the hole runs to the end of Y
TWO_SIDED = ([40, 0, 129, 5, 257, 1, 300, 32], [300, 7, 33, 0, 128, 256, 4, 1000])      # segment 1: no queries; segment 3: no rows of Y
CASES = [(RAGGED, None), (ALIGNED, None), (ONE_BIG, None), (ONE_BIG_LAST, None), TWO_SIDED]
IDS = ["ragged self", "aligned self", "one big segment", "one big last segment", "two-sided"]


def _offsets(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def _shape(d, k):
    """(padded dim, queries per block, list capacity) of the 16-bit scan for (d, k): DESIGN.md §4.1's kernel table."""
    dp = 128 if d <= 128 else 256 if d <= 256 else 512 if d <= 512 else 1024
    cap = 15 if dp > 512 or k <= 11 else 16 if k <= 20 else 32
    return dp, (256 if dp <= 512 else 128), cap


def _segment_of(xp, row):
    return max(s for s in range(len(xp) - 1) if xp[s] <= row < xp[s + 1])


def _restated(xp, yp, d, k, forced):
    """{first row of a block: [(t0, t1, w0, w1), ...] in slot order} and lists, from §4.25's rule restated."""
    dp, qt, cap = _shape(d, k)
    n, m = xp[-1], yp[-1]
    T = -(-m // 256) * 8
    max_r = 1
    while 2 * (2 * max_r + 1) * cap <= 1024 - SPILL:
        max_r *= 2
    geo = {}
    for r0 in range(0, n, qt):
        s0, s1 = _segment_of(xp, r0), _segment_of(xp, min(r0 + qt, n) - 1)
        ulo, uhi = yp[s0], yp[s1 + 1]
        h0 = h1 = 0
        if s0 == s1:
            h0 = -(-ulo // 32)
            h1 = max(h0, T if uhi == m else uhi // 32)
        geo[r0] = (h0, h1, ulo // 32, -(-uhi // 32) if uhi > ulo else ulo // 32)
    per = max(1, -(-sum(T - (h1 - h0) for h0, h1, _, _ in geo.values()) // 1024))
    blocks, most = {}, 1
    for r0, (h0, h1, w0, w1) in geo.items():
        adm = T - (h1 - h0)
        if adm <= 0:
            continue
        want = forced if forced > 0 else min(-(-adm // per), max(1, adm // 64))       # automatic: no run shorter than 64 tiles
        r = 1
        while 2 * r <= want and 2 * r <= adm and 2 * r <= max_r:
            r *= 2
        tps = -(-adm // r)
        assert tps * 32 * dp * 2 < 1 << 32
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
            e0, e1 = max(w0, t0), min(w1, t1)
            out.append((t0, t1, e0, e1) if e0 < e1 else (t0, t1, t0, t0))
        blocks[r0] = out
        most = max(most, len(out))
    return blocks, 2 * most, qt, cap


@pytest.mark.parametrize("forced", [0, 1, 2, 4, 8, 64])
@pytest.mark.parametrize("d,k", [(40, 5), (300, 20), (300, 44), (600, 5), (600, 20)])
@pytest.mark.parametrize("xs,ys", CASES, ids=IDS)
def test_the_table_is_the_restated_rule_and_covers_every_admissible_column_once(xs, ys, d, k, forced):
    mmf = _mmf()
    xp = _offsets(xs)
    yp = xp if ys is None else _offsets(ys)
    n, m = xp[-1], yp[-1]
    table, lists = mmf.cross_segments_fast_table(xp, None if ys is None else yp, d=d, k=k, col_splits=forced)
    assert table.dtype == torch.int32 and table.shape[1] == 8
    want, want_lists, qt, cap = _restated(xp, yp, d, k, forced)
    assert lists == want_lists and lists % 2 == 0 and lists * cap <= 1024 - SPILL
    got = {}
    for qpos, row0, nq, t0, t1, slot, w0, w1 in table.tolist():
        assert qpos == row0 and row0 % qt == 0 and nq == min(qt, n - row0) and nq >= 1
        assert 0 <= t0 < t1 <= -(-m // 256) * 8 and t0 <= w0 <= w1 <= t1 and 0 <= slot and 2 * slot + 1 < lists
        got.setdefault(row0, []).append((slot, t0, t1, w0, w1))
    got = {r: sorted(v) for r, v in got.items()}
    for r, v in got.items():
        assert [e[0] for e in v] == list(range(len(v))), "list slots of a block are not 0 .. count - 1 in tile order"
    assert {r: [e[1:] for e in v] for r, v in got.items()} == want
    assert sorted(got) == list(range(0, n, qt)), "a row block without an entry"
    lengths = [e[4] - e[3] for e in table.tolist()]
    assert lengths == sorted(lengths, reverse=True), "the entries do not come longest run first"
    if forced in (1, 2, 4, 8):
        assert lists in (2 * forced, 2 * forced + 2)              # + 1 entry where a run spans a hole
    # independently of the rule: for every row, the tiles of its block's entries minus the columns the mask removes (inside the
    # entry's window, the row's own segment) are every admissible column exactly once and no excluded one
    tiles_of = {r: [(t, w0 <= t < w1) for _, t0, t1, w0, w1 in v for t in range(t0, t1)] for r, v in got.items()}
    for r0, tiles in tiles_of.items():
        assert len(tiles) == len({t for t, _ in tiles}), "a tile is in two entries of a block"
        rows = range(r0, min(r0 + qt, n))
        segs = sorted({_segment_of(xp, i) for i in rows})
        for s in segs:                                            # the rows of a block that share a segment share the answer
            lo, hi = yp[s], yp[s + 1]
            seen = []
            for t, masked in tiles:
                cols = range(t * 32, min((t + 1) * 32, m))
                if masked:
                    seen += [j for j in cols if not lo <= j < hi]
                else:
                    assert not any(lo <= j < hi for j in cols), f"block {r0}, segment {s}: tile {t} holds excluded columns outside the mask window"
                    seen += list(cols)
            assert len(seen) == len(set(seen)) == m - (hi - lo), f"block {r0}, segment {s}: admissible columns missing or doubled"


def test_automatic_runs_fill_the_chip_but_stay_longer_than_the_threshold_exchange():
    """16684 rows: the rule for about 1024 workgroups alone would ask for 16 runs of 33 tiles; the automatic count stops at runs of 64
    tiles (the cadence at which the workgroups of a row block exchange thresholds), a forced count does not."""
    mmf = _mmf()
    xp = _offsets([4096, 4096, 300, 4096, 4096])
    for d, k in ((300, 5), (300, 44), (600, 20)):
        table, lists = mmf.cross_segments_fast_table(xp, d=d, k=k)
        want, want_lists, qt, _ = _restated(xp, xp, d, k, 0)
        got = {}
        for _, row0, _, t0, t1, slot, w0, w1 in table.tolist():
            got.setdefault(row0, []).append((slot, t0, t1, w0, w1))
        assert {r: [e[1:] for e in sorted(v)] for r, v in got.items()} == want and lists == want_lists
        assert lists in (16, 18)                                  # 8 runs of 66 tiles, 9 entries where one spans a hole
        whole = [t1 - t0 for v in want.values() if len(v) == 8 for t0, t1, _, _ in v]
        assert whole and min(whole) >= 64
        forced, _ = mmf.cross_segments_fast_table(xp, d=d, k=k, col_splits=16 if k <= 20 else 8)
        assert forced.shape[0] > table.shape[0] or k > 20


def test_a_hole_inside_a_run_and_at_a_run_edge_and_a_block_over_three_segments():
    mmf = _mmf()
    # d = 300: blocks of 256 rows; m = 2048 = 64 tiles.  Segment 1 = rows 512 .. 1024 swallows tiles 16 .. 32: 48 admissible tiles.
    xp = _offsets([512, 512, 1024])
    t, lists = mmf.cross_segments_fast_table(xp, d=300, k=5, col_splits=1)
    assert sorted(e[3:8] for e in t.tolist() if e[1] == 512) == [[0, 16, 0, 0, 0], [32, 64, 1, 32, 32]] and lists == 4     # one run across the hole
    t, lists = mmf.cross_segments_fast_table(xp, d=300, k=5, col_splits=2)
    assert sorted(e[3:8] for e in t.tolist() if e[1] == 768) == [[0, 16, 0, 0, 0], [32, 40, 1, 32, 32], [40, 64, 2, 40, 40]]
    assert sorted(e[3:8] for e in t.tolist() if e[1] == 0) == [[16, 40, 0, 16, 16], [40, 64, 1, 40, 40]]                   # hole at the front
    assert sorted(e[3:8] for e in t.tolist() if e[1] == 1024) == [[0, 16, 0, 0, 0], [16, 32, 1, 16, 16]] and lists == 6     # hole at the back
    # runs of 16 admissible tiles with the hole (tiles 16 .. 48) exactly at a run edge: no run is cut
    t, lists = mmf.cross_segments_fast_table(_offsets([512, 1024, 512]), d=300, k=5, col_splits=2)
    assert sorted(e[3:8] for e in t.tolist() if e[1] == 512) == [[0, 16, 0, 0, 0], [48, 64, 1, 48, 48]] and lists == 4
    # bounds off a tile edge (m = 512: 16 tiles): segment 1 = rows 100 .. 300 has the hole tiles [4, 9); the straddling tiles 3 and 9
    # are its mask window.  At 256 rows per block, block 0 spans segments 0 and 1: no hole, window = tiles [0, 10); block 1 spans 1 and
    # 2: window = tiles [3, 16).  At 128 rows per block, the blocks at rows 128 and 384 lie inside one segment each (segment 2 = rows
    # 300 .. 512 runs to the end of Y: hole [10, 16), window tile 9).
    t, lists = mmf.cross_segments_fast_table(_offsets([100, 200, 212]), d=40, k=5, col_splits=1)
    assert sorted(e[:8] for e in t.tolist()) == [[0, 0, 256, 0, 16, 0, 0, 10], [256, 256, 256, 0, 16, 0, 3, 16]] and lists == 2
    t, _ = mmf.cross_segments_fast_table(_offsets([100, 200, 212]), d=600, k=5, col_splits=1)                              # blocks of 128 rows
    assert sorted(e[:8] for e in t.tolist()) == [[0, 0, 128, 0, 16, 0, 0, 10], [128, 128, 128, 0, 4, 0, 3, 4], [128, 128, 128, 9, 16, 1, 9, 10],
                                                 [256, 256, 128, 0, 16, 0, 3, 16], [384, 384, 128, 0, 10, 0, 9, 10]]


def test_the_table_query_refuses_bad_arguments():
    mmf = _mmf()
    for kw, words in ((dict(ptr=[1, 4]), "x_ptr must start at 0"), (dict(ptr=[0, 4, 2]), "decreases"), (dict(ptr=[0, 4], k=0), "k must be >= 1"),
                      (dict(ptr=[0, 4], col_splits=3), "power of two"), (dict(ptr=[0, 4], y_ptr=[0, 2, 4]), "the same S on both sides")):
        with pytest.raises(ValueError, match=words):
            mmf.cross_segments_fast_table(kw.pop("ptr"), d=64, **kw)
    for d, k in ((1100, 5), (600, 21), (300, 45)):
        with pytest.raises(RuntimeError, match=f"does not serve d = {d}, k = {k}"):
            mmf.cross_segments_fast_table([0, 300, 600], d=d, k=k)
    L = mmf._lib.lib()
    small = (ctypes.c_int32 * 8)()
    rc = L.mmf_cross_segments_fast_table(_ptr([0, 300, 600]), None, 2, 64, 5, 0, ctypes.cast(small, ctypes.c_void_p), 1, None)
    assert rc == INVALID and "entries needed" in L.mmf_last_error().decode() and "cross_segments_fast_table" in L.mmf_last_error().decode()
    table, lists = mmf.cross_segments_fast_table([0], d=64, k=5)                                # no segments: no entries
    assert table.shape == (0, 8) and lists == 2
    table, _ = mmf.cross_segments_fast_table([0, 300], d=64, k=5)                               # one segment: nothing is admissible
    assert table.shape == (0, 8)


# ---- documents -----------------------------------------------------------------------------------------------------------------------
def test_design_and_readme_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = " ".join(design.split("### 4.25", 1)[1].split("\n## ", 1)[0].split())
    for words in ("Contract", "mmf_simtopk_cross_segments_fast", "cross_seg16_table", "XSEG", "mask window", "kernel-resource-usage",
                  "instruction for instruction", "Measurements", "Cuts", "No query order", "No symmetric"):
        assert words in sec, words
    assert "4.25" in design.split("## 8", 1)[1]
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "cross_segments16" in f.read()
