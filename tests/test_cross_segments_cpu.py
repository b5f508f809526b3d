"""The cross-segment top-k without a GPU (include/ext/mmf_hg_cross_seg.h): the header declares exactly the new
entries, the library exports them and the binding registers them in a list of its own, the entry runs its host checks before any
device call and names itself, the Python functions raise their argument errors on the host, and the work table — queried on the
host — covers every (query row, admissible column) pair exactly once and never a tile that lies wholly inside a row block's own
segment."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join("ext", "mmf_hg_cross_seg.h")
ENTRIES = ["mmf_simtopk_cross_segments", "mmf_cross_segments_table"]
INVALID, UNSUPPORTED = -1, -2


def _mmf():
    import multimodal_fusion_amd as m
    return m


def _declared(path):
    with open(os.path.join(ROOT, "include", path)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding, build ------------------------------------------------------------------------------------------
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
    for words in ("Bit for bit", "key descending, then id ascending", "k > 44 runs passes", "power of two", "before any device call",
                  "device_id < 0 -> MMF_E_UNSUPPORTED first", "no -1 / -inf fill", "fewer than k admissible", "Host only",
                  "Host-synchronous: once per call", "no exclude_self"):
        assert words in h, words
    with open(os.path.join(inc, "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()


def test_library_and_binding_export_the_entries_from_a_list_of_their_own():
    mmf = _mmf()
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.CROSS_SEG_EXPORTS) == ENTRIES and all(hasattr(L, e) for e in ENTRIES)
    for name in (n for n in vars(mmf._lib) if n.startswith("EXPORTS")):
        assert not set(ENTRIES) & set(getattr(mmf._lib, name)), name
    lib = mmf._lib.lib()
    seg = list(lib.mmf_simtopk_segmented_exact.argtypes)
    assert list(lib.mmf_simtopk_cross_segments.argtypes) == seg[:9] + seg[10:]                # the same list without exclude_self
    tab = list(lib.mmf_segmented_exact_table.argtypes)
    assert list(lib.mmf_cross_segments_table.argtypes) == tab[:4] + tab[5:]
    assert lib.mmf_simtopk_cross_segments.restype is ctypes.c_int and lib.mmf_cross_segments_table.restype is ctypes.c_int64
    assert mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_build_lists_the_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_cross_seg", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", HEADER)) for h in b.HEADERS)


def test_module_and_functions_are_exported():
    mmf = _mmf()
    cs = import_module("multimodal_fusion_amd.cross_segments")
    assert mmf.cross_segments is cs and "cross_segments" in mmf.__all__ and "mmf.cross_segments.*" in mmf.__doc__
    for name in ("simtopk_cross_segments", "cross_segments_table", "cross_segment_knn_edges"):
        assert getattr(mmf, name) is getattr(cs, name) and name in mmf.__all__
    assert list(inspect.signature(cs.simtopk_cross_segments).parameters) == ["X", "Y", "ptr", "batch", "y_ptr", "y_batch", "metric", "lam", "k",
                                                                            "col_splits", "return_stats", "profile"]
    assert list(inspect.signature(cs.cross_segments_table).parameters) == ["ptr", "y_ptr", "k", "col_splits"]
    assert list(inspect.signature(cs.cross_segment_knn_edges).parameters) == ["X", "ptr", "batch", "k"]
    assert list(inspect.signature(mmf.cohort.link_slides).parameters) == ["out", "k"]
    for fn in (cs.simtopk_cross_segments, cs.cross_segment_knn_edges):
        kinds = {n: p.kind for n, p in inspect.signature(fn).parameters.items()}
        assert all(kind is inspect.Parameter.KEYWORD_ONLY for n, kind in kinds.items() if n not in ("X", "Y"))


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
    rc = L.mmf_simtopk_cross_segments(a["X"], a["n"], a["Y"], a["m"], a["d"], a["dtype"], a["metric"], a["lam"], a["k"], _ptr(a["xp"]),
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
    (dict(opts=(1, 0, -2, 0, None)), INVALID, "col_splits must be 0 or a power of two"),
    (dict(opts=(7, 0, 0, 0, None)), INVALID, "only MMF_PREC_AUTO and MMF_PREC_EXACT"),
    (dict(opts=(2, 0, 0, 0, None)), UNSUPPORTED, "no 16-bit scan serves the cross-segment entry yet"),
    (dict(opts=(3, 0, 0, 0, None)), UNSUPPORTED, "no 16-bit scan serves the cross-segment entry yet"),
    (dict(idx=None), INVALID, "NULL output"),
    (dict(val=None), INVALID, "NULL output"),
    # segment 1 has 5 of the 8 rows: 3 admissible columns; segment 0 has 5
    (dict(k=4), INVALID, "segment 1 has 3 admissible columns (m = 8 minus its own 5 rows of Y), k = 4"),
    (dict(k=6), INVALID, "segment 0 has 5 admissible columns (m = 8 minus its own 3 rows of Y), k = 6"),
    (dict(xp=[0, 8], S=1, k=1), INVALID, "segment 0 has 0 admissible columns"),
    (dict(Y=_buf(), m=6, yp=[0, 1, 6], k=2), INVALID, "segment 1 has 1 admissible columns (m = 6 minus its own 5 rows of Y), k = 2"),
]


@pytest.mark.parametrize("kw,code,words", REFUSALS)
def test_the_entry_refuses_before_any_device_call(kw, code, words):
    """A device id that does not exist: an argument error must win over the device's."""
    rc, msg = _entry(**kw)
    assert rc == code and words in msg and "simtopk_cross_segments" in msg, (rc, msg)


def test_a_negative_device_is_refused_first():
    for kw in (dict(), dict(k=0), dict(xp=[1, 3, 8]), dict(idx=None), dict(opts=(0, 0, 3, 0, None)), dict(opts=(2, 0, 0, 0, None)), dict(k=6),
               dict(n=-1)):
        rc, msg = _entry(device=-1, **kw)
        assert rc == UNSUPPORTED and "no CPU path" in msg and "simtopk_cross_segments" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """Every dtype and metric, k beyond one pass, power-of-two col_splits, a segment without rows that nothing is asked of, a segment
    with no rows of Y: the call gets as far as the device (which is not there)."""
    E_HIP = _mmf()._lib.MMF_E_HIP
    big = [0, 100, 300]
    for kw in (dict(), dict(k=3), dict(opts=(1, 1, 8, 0, None)), dict(opts=(0, 0, 64, 0, None)), dict(d=5000), dict(dtype=1), dict(dtype=2),
               dict(metric=0), dict(metric=2), dict(metric=3, lam=0.5), dict(n=300, xp=big, k=100), dict(xp=[0, 4, 4, 8], S=3, k=4),
               dict(Y=_buf(), m=6, yp=[0, 3, 6], k=3), dict(Y=_buf(), m=6, yp=[0, 6, 6], xp=[0, 0, 8], k=6)):
        rc, msg = _entry(**kw)
        assert rc == E_HIP, (kw, rc, msg)
    assert _entry(n=0, xp=[0, 0, 0])[0] == 0 and _entry(n=0, xp=[0], S=0, X=None, idx=None, val=None)[0] == 0
    assert _entry(n=0, xp=[0, 0, 0], Y=_buf(), m=6, yp=[0, 2, 6], k=50)[0] == 0           # no rows: nothing is short of columns


def test_the_entry_makes_every_refusal_before_the_first_device_call_and_shares_the_driver():
    with open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")) as f:
        raw = f.read()
    body = raw.split("int mmf_simtopk_cross_segments(", 1)[1].split("\n}\n", 1)[0]
    assert body.index(".on_device()") < body.index("set_error(") and body.rindex("set_error(") < body.index("run_segmented_exact(")
    assert "hipStream" not in body and "hipMemcpy" not in body and "hipDeviceSynchronize" not in body
    assert "run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true)" in body
    table = raw.split("int64_t mmf_cross_segments_table(", 1)[1].split("\n}\n", 1)[0]
    assert "hip" not in table and "Call(" not in table                                         # host only


def test_python_functions_refuse_on_the_host(monkeypatch):
    mmf = _mmf()
    cs = mmf.cross_segments
    monkeypatch.setattr(mmf._lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    X = torch.zeros(8, 16)
    sf = torch.zeros(36, 16)
    out = dict(super_features=sf, group_ptr=torch.tensor([0, 12, 24, 36]), node_ptr=torch.tensor([0, 20, 45, 60]))
    bad = [(lambda: cs.simtopk_cross_segments(X, ptr=[0, 3, 7], k=2), "ptr"),
           (lambda: cs.simtopk_cross_segments(X, ptr=[0, 3, 8], k=0), "k must be >= 1"),
           (lambda: cs.simtopk_cross_segments(X, ptr=[0, 3, 8], col_splits=3, k=2), "col_splits must be 0 or a power of two"),
           (lambda: cs.simtopk_cross_segments(X, ptr=[0, 3, 8], col_splits=-4, k=2), "col_splits must be 0 or a power of two"),
           (lambda: cs.simtopk_cross_segments(X, ptr=[0, 3, 8], y_ptr=[0, 8]), "y_ptr / y_batch need Y"),
           (lambda: cs.simtopk_cross_segments(X, torch.zeros(4, 8), ptr=[0, 8], y_ptr=[0, 4]), "share device, dtype and feature dim"),
           (lambda: cs.simtopk_cross_segments(torch.zeros(8), ptr=[0, 8]), "2-D"),
           (lambda: cs.simtopk_cross_segments(X, ptr=[0, 3, 8], metric="manhattan", k=2), "unknown metric"),
           (lambda: cs.simtopk_cross_segments(X, ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns (m = 8 minus its own 5 rows of Y), k = 4"),
           (lambda: cs.simtopk_cross_segments(X, batch=torch.tensor([0, 0, 0, 1, 1, 1, 1, 1]), k=6), "segment 0 has 5 admissible columns"),
           (lambda: cs.simtopk_cross_segments(X, torch.zeros(6, 16), ptr=[0, 3, 8], y_ptr=[0, 1, 6], k=2), "segment 1 has 1 admissible columns"),
           (lambda: cs.simtopk_cross_segments(X, k=1), "ptr"),
           (lambda: cs.cross_segment_knn_edges(X), "needs ptr or batch"),
           (lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], k=0), "k must be >= 1"),
           (lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], k=4), "segment 1 has 3 admissible columns"),
           (lambda: cs.cross_segment_knn_edges(torch.zeros(8), ptr=[0, 8]), "2-D"),
           (lambda: cs.cross_segment_knn_edges(X, ptr=[0, 3, 9]), "ptr"),
           (lambda: mmf.cohort.link_slides({"super_features": sf}), "needs the dict of build_cohort_hypergraphs"),
           (lambda: mmf.cohort.link_slides([sf]), "needs the dict of build_cohort_hypergraphs"),
           (lambda: mmf.cohort.link_slides(dict(out, group_ptr=torch.tensor([0, 36]), node_ptr=torch.tensor([0, 60]))), "no other slide to link to"),
           (lambda: mmf.cohort.link_slides(dict(out, node_ptr=torch.tensor([0, 20, 45]))), "group_ptr and node_ptr [S + 1]"),
           (lambda: mmf.cohort.link_slides(dict(out, group_ptr=torch.tensor([0, 12, 24, 30]))), "link_slides"),
           (lambda: mmf.cohort.link_slides(dict(out, node_ptr=torch.tensor([0, 10, 45, 60]))), "fewer nodes than it has super patches"),
           (lambda: mmf.cohort.link_slides(out, k=0), "k must be >= 1"),
           (lambda: mmf.cohort.link_slides(out, k=25), "segment 0 has 24 admissible columns")]
    for fn, words in bad:
        with pytest.raises(ValueError, match=re.escape(words)):
            fn()
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU path"):
        cs.simtopk_cross_segments(X, ptr=[0, 3, 8], k=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cs.cross_segment_knn_edges(X, ptr=[0, 3, 8], k=3)


# ---- the work table, queried on the host ---------------------------------------------------------------------------------------
# bounds on a tile edge (128 | 256 ...), one off a tile edge, inside the first tile and inside the last, partial, tile; the 400- and the
# 385-row segments swallow whole tiles; the first and the last segment have rows
SIZES = [100, 400, 1, 0, 127, 128, 129, 385, 30]
ALIGNED = [128, 256, 0, 384, 128]                          # every bound on a tile edge, m a multiple of 128
TWO_SIDED = ([40, 0, 129, 5, 257, 1, 300, 32], [300, 7, 33, 0, 128, 256, 4, 1000])      # segment 1: no queries; segment 3: no rows of Y
LARGE = [4096, 4096, 300, 4096, 4096]


def _offsets(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def _restated(xs, xp, yp, k, forced):
    """{first row of a block: [(t0, t1), ...] in range order} and lists, from the rule of mmf_scan_f32.hip's cross_seg_table,
    restated: the tiles of all of Y without the block's hole, numbered without it, cut into R runs; a run across the hole is two."""
    kk = min(k, 44)
    cap = 16 if kk <= 12 else 32 if kk <= 28 else 48
    max_r = 1
    while 2 * (2 * max_r + 1) * cap <= 1024:
        max_r *= 2
    m = yp[-1]
    T = -(-m // 128)

    def hole(s):
        h0 = -(-yp[s] // 128)
        h1 = T if yp[s + 1] == m else yp[s + 1] // 128
        return h0, max(h0, h1)
    pairs = sum(-(-xs[s] // 128) * (T - (hole(s)[1] - hole(s)[0])) for s in range(len(xs)))
    per = max(1, -(-pairs // 1024))
    blocks, ranges = {}, 1
    for s, n in enumerate(xs):
        h0, h1 = hole(s)
        adm = T - (h1 - h0)
        if n == 0 or adm == 0:
            continue
        want = forced if forced > 0 else -(-adm // per)
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
        ranges = max(ranges, len(runs))
        for r0 in range(0, n, 128):
            blocks[xp[s] + r0] = runs
    return blocks, 2 * ranges, cap


@pytest.mark.parametrize("forced", [0, 1, 2, 4, 64])
@pytest.mark.parametrize("k", [5, 12, 28, 50])
@pytest.mark.parametrize("xs,ys", [(SIZES, None), (ALIGNED, None), TWO_SIDED, (LARGE, None)], ids=["ragged self", "aligned self", "two-sided", "large self"])
def test_the_table_covers_every_admissible_pair_once_and_no_excluded_tile(xs, ys, k, forced):
    mmf = _mmf()
    xp = _offsets(xs)
    yp = xp if ys is None else _offsets(ys)
    m = yp[-1]
    table, lists = mmf.cross_segments_table(xp, None if ys is None else yp, k=k, col_splits=forced)
    want_blocks, want_lists, cap = _restated(xs, xp, yp, k, forced)
    assert lists == want_lists and lists * cap <= 1024 and lists % 2 == 0
    got_blocks, nqs = {}, {}
    for seg, row0, nq, lo, t0, t1, rng, hi in table.tolist():
        assert xs[seg] > 0 and 1 <= nq <= 128, "a segment without rows made an entry"
        assert xp[seg] <= row0 and row0 + nq <= xp[seg + 1], "a block crosses a segment"
        assert (row0 - xp[seg]) % 128 == 0 and (nq == 128 or row0 + nq == xp[seg + 1])
        assert (lo, hi) == (yp[seg], yp[seg + 1]), "the bounds are not the segment's y_ptr pair"
        assert 0 <= t0 < t1 and (t1 - 1) * 128 < m, "a tile starts at or past m"
        for t in range(t0, t1):
            assert not (lo <= t * 128 and min((t + 1) * 128, m) <= hi and lo < hi), "a tile lies wholly inside the excluded range"
        assert 0 <= rng and 2 * rng + 1 < lists
        got_blocks.setdefault(row0, []).append((rng, t0, t1))
        assert nqs.setdefault(row0, nq) == nq
    # range numbers: distinct per block, 0 .. count - 1 in tile order; the runs are the restated rule's
    got_blocks = {row0: sorted(runs) for row0, runs in got_blocks.items()}
    for row0, runs in got_blocks.items():
        assert [r[0] for r in runs] == list(range(len(runs))), "list slots of a block are not distinct"
    assert {r: [(t0, t1) for _, t0, t1 in v] for r, v in got_blocks.items()} == want_blocks
    lengths = [e[5] - e[4] for e in table.tolist()]
    assert lengths == sorted(lengths, reverse=True), "the entries do not come longest run first"
    # every (query row, admissible column) pair is in exactly one entry: per block, the union of the entries' columns minus the
    # excluded range is every column outside the range, and no tile is in two entries
    for s, n in enumerate(xs):
        per_block = [got_blocks.get(xp[s] + r0, []) for r0 in range(0, n, 128)]
        assert all(runs == per_block[0] for runs in per_block), f"segment {s}: its blocks differ"
        assert [nqs.get(xp[s] + r0, 0) for r0 in range(0, n, 128)] == [min(128, n - r0) for r0 in range(0, n, 128)], f"segment {s}: rows missing"
        if n == 0:
            continue
        tiles = [t for _, t0, t1 in per_block[0] for t in range(t0, t1)]
        assert len(tiles) == len(set(tiles)), "a (row block, tile) pair is covered twice"
        cols = set()
        for t in tiles:
            cols.update(j for j in range(t * 128, min((t + 1) * 128, m)) if not yp[s] <= j < yp[s + 1])
        assert len(cols) == m - (yp[s + 1] - yp[s]), f"segment {s}: admissible columns missing"
    if forced in (1, 2, 4):
        assert lists in (2 * forced, 2 * forced + 2)          # + 1 range where a run spans a hole


def test_a_run_across_the_hole_is_two_entries_and_a_hole_at_a_run_edge_is_none():
    mmf = _mmf()
    # m = 1024: 8 tiles.  Segment 1 = rows 256..512 swallows tiles 2 and 3: 6 admissible tiles.
    xp = _offsets([256, 256, 512])
    t, lists = mmf.cross_segments_table(xp, k=5, col_splits=1)
    assert sorted(e[4:7] for e in t.tolist() if e[1] == 256) == [[0, 2, 0], [4, 8, 1]] and lists == 4          # one run, across the hole
    t, lists = mmf.cross_segments_table(xp, k=5, col_splits=2)
    assert sorted(e[4:7] for e in t.tolist() if e[1] == 256) == [[0, 2, 0], [4, 5, 1], [5, 8, 2]]              # runs of 3: the first spans it
    assert sorted(e[4:7] for e in t.tolist() if e[1] == 0) == [[2, 5, 0], [5, 8, 1]]                           # the hole at the front: none does
    assert sorted(e[4:7] for e in t.tolist() if e[1] == 512) == [[0, 2, 0], [2, 4, 1]] and lists == 6          # the hole at the back
    # segment 1 = rows 256..768 with runs of 2 admissible tiles: the hole (tiles 2 .. 5) sits exactly at a run edge
    t, lists = mmf.cross_segments_table(_offsets([256, 512, 256]), k=5, col_splits=2)
    assert sorted(e[4:7] for e in t.tolist() if e[1] == 256) == [[0, 2, 0], [6, 8, 1]] and lists == 4


def test_the_table_query_refuses_bad_arguments():
    mmf = _mmf()
    for kw, words in ((dict(ptr=[1, 4]), "x_ptr must start at 0"), (dict(ptr=[0, 4, 2]), "decreases"), (dict(ptr=[0, 4], k=0), "k must be >= 1"),
                      (dict(ptr=[0, 4], col_splits=3), "power of two"), (dict(ptr=[0, 4], y_ptr=[0, 2, 4]), "the same S on both sides")):
        with pytest.raises(ValueError, match=words):
            mmf.cross_segments_table(kw.pop("ptr"), **kw)
    L = mmf._lib.lib()
    small = (ctypes.c_int64 * 8)()
    rc = L.mmf_cross_segments_table(_ptr([0, 300, 600]), None, 2, 5, 0, ctypes.cast(small, ctypes.c_void_p), 1, None)
    assert rc == INVALID and "entries needed" in L.mmf_last_error().decode() and "cross_segments_table" in L.mmf_last_error().decode()
    table, lists = mmf.cross_segments_table([0], k=5)                                           # no segments: no entries
    assert table.shape == (0, 8) and lists == 2
    table, _ = mmf.cross_segments_table([0, 300], k=5)                                          # one segment: nothing is admissible
    assert table.shape == (0, 8)


# ---- documents -----------------------------------------------------------------------------------------------------------------------
def test_design_readme_integration_and_scripts_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = " ".join(design.split("### 4.24", 1)[1].split("\n## ", 1)[0].split())
    for words in ("Contract", "mmf_simtopk_cross_segments", "cross_seg_table", "XSEG", "over-read", "instruction for instruction identical",
                  "kernel-resource-usage", "Measurements", "cross_segments_timing.txt", "Cuts", "MMF_PREC_FAST"):
        assert words in sec, words
    assert "cross-segment" in design.split("## 8", 1)[1]                                        # the 16-bit follow-up is on the list
    for path, words in (("README.md", ["cross_segments", "simtopk_cross_segments", "cross_segments_timing"]),
                        ("INTEGRATION.md", ["mmf_simtopk_cross_segments", "mmf_hg_cross_seg.h"]),
                        (os.path.join("scripts", "cross_segments_timing.py"), ["simtopk_cross_segments", "bit for bit", "--baseline-only"])):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for w in words:
            assert w in text, (path, w)
    assert os.path.exists(os.path.join(ROOT, "profiles", "cross_segments_timing.txt"))
