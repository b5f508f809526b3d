"""The 16-bit scan's query-side list code files a visit's hits in per-lane rounds (SlotList::offer_tile, csrc/mmf_dev.h;
DESIGN.md §4.1): every lane folds its passing values into a 16-bit mask and a round takes the lowest set bit of every lane that
has one.  Planted rows drive the visits the rounds can get wrong — several hits of one lane in one tile, one hit in each lane
in different accumulator rows, a list that fills in the middle of a visit, crowded lists and the overflow path, the ragged last
tile and row block, the 16- and 32-entry lists and the split-k kernel — through the public entry with precision="fast", on the
plain path (its default column splits and one column range) and, where it applies, on the symmetric path (forced at this size
with MMF_SYMMETRIC=1, MMF_SYMMETRIC_G=1).  Ids and scores are compared bit for bit with the oracle; no row may be rescued by the
exact rescan unless the case says so.

Geometry the plants rely on (mmf_scan_bf16.hip): a workgroup owns a row block of 256 queries, a wave 32 consecutive ones; a tile
is 32 consecutive candidate rows; the two lanes of a query (l, l ^ 32) hold tile rows {0-7, 16-23} and {8-15, 24-31}.  With
G = 1 a row block is a super-block: the first symmetric launch scans its own and (even count) the antipodal row block, the
second one the (ns - 1) / 2 row blocks behind it, query side and candidate side at once."""
import functools
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

KEYS = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G")
LOW = list(range(8)) + list(range(16, 24))        # tile rows of a query's lower lane
HIGH = list(range(8, 16)) + list(range(24, 32))   # ... of its partner lane


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available()
    return m


@contextmanager
def switches(symmetric, G):
    old = {k: os.environ.get(k) for k in KEYS}
    for k, v in zip(KEYS, (symmetric, G)):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sym_grid(mmf, n, G):
    return 2 * mmf._lib.lib().mmf_debug_symmetric_schedule((n + 255) // 256, G, 0, None, 0)


class Rows:
    """Gaussian unit rows with planted neighbours: plant(q, rows, cosines) turns `rows` into unit rows whose cosine with row q
    is the given one (the rest of each is fresh noise orthogonal to q), far above anything the Gaussian rows reach (0.2)."""

    def __init__(self, n, d, seed):
        self.g = torch.Generator().manual_seed(seed)
        x = torch.randn((n, d), generator=self.g, dtype=torch.float64)
        self.X = x / x.norm(dim=1, keepdim=True)
        self.taken = set()

    def plant(self, q, rows, cosines):
        rows = [int(r) for r in rows]
        assert len(rows) == len(cosines) and not (self.taken & set(rows)) and q not in rows, (q, rows)
        self.taken |= set(rows) | {q}
        qv = self.X[q]
        for r, c in zip(rows, cosines):
            u = torch.randn(qv.shape, generator=self.g, dtype=torch.float64)
            u = u - (u @ qv) * qv
            self.X[r] = c * qv + (1.0 - c * c) ** 0.5 * u / u.norm()

    def done(self):
        return self.X.float().contiguous()


def falling(count, top=0.9, step=0.01):
    return [top - step * i for i in range(count)]


def tile(block, t):
    """First row of tile t (0..7) of row block `block`."""
    return 256 * block + 32 * t


@functools.lru_cache(maxsize=None)
def case(name):
    """(X on the host, k, oracle ids, oracle scores); built once."""
    k = 5
    if name == "several_hits_in_one_lane":
        # 3, 8 and 16 hits of ONE lane in one tile, and 16 in both lanes.  Queries of row block 8 with their tiles in row block 5
        # (second symmetric launch, query side), queries of row block 2 with theirs in row block 10 (first launch, antipodal).
        R = Rows(4096, 512, 11)
        for qb, cb in ((8, 5), (2, 10)):
            for i, rows in enumerate((LOW[:3], LOW[:8], LOW, list(range(32)))):
                R.plant(256 * qb + 37 * i + 5, [tile(cb, 2 * i) + r for r in rows], falling(len(rows)))
    elif name == "one_hit_per_lane":
        # the 32 queries of a wave have one hit each in one tile, each in another candidate row: one round
        R = Rows(4096, 512, 12)
        for qb, w, cb in ((8, 2, 6), (3, 1, 11)):
            for i in range(32):
                R.plant(256 * qb + 32 * w + i, [tile(cb, 3) + (7 * i + 3) % 32], [0.8 - 0.004 * i])
    elif name == "list_fills_mid_visit":
        # p earlier hits of the lower lane, one per tile, then a tile with 4 hits in that lane and 2 in its partner's: with
        # p = 12 .. 14 the list runs full inside the visit (a nearly full list is compacted on entry, which p = 14 meets).
        # Row block 8 walks the tiles of row blocks 4 .. 7 in the second launch; row block 1 its own and row block 9's in the first.
        R = Rows(4096, 512, 13)
        for j, p in enumerate((11, 12, 13, 14)):
            q = 256 * 8 + 32 * (2 * j) + 9 + j
            R.plant(q, [tile(4, 0) + 32 * i + j for i in range(p)], [0.5 + 0.01 * i for i in range(p)])
            R.plant(256 * 8 + 32 * (2 * j) + 40 + j, [], [])      # (keeps the neighbouring wave's rows Gaussian)
            last = tile(6, j)
            R.taken.discard(q)
            R.plant(q, [last + r for r in (0, 1, 2, 3, 8, 9)], falling(6, 0.9, 0.02))
        for j, p in enumerate((12, 13)):
            q = 256 * 1 + 32 * (4 + j) + 3
            own = [tile(1, i) + 16 + j for i in range(8)]
            far = [tile(9, i) + 16 + j for i in range(p - 8)]
            R.plant(q, own + far, [0.5 + 0.01 * i for i in range(p)])
            R.taken.discard(q)
            R.plant(q, [tile(9, 6 + j) + r for r in (4, 5, 6, 7, 12, 13)], falling(6, 0.9, 0.02))
    elif name == "crowded_lists":
        # 300 near-duplicates of one row, cosines 1 - 5e-6 .. 1 - 2e-4 with it and with each other: far more of them inside a
        # query's margin band (1e-3) than two 15-entry lists hold — tband, sink.put and the overflow lists
        R = Rows(4096, 512, 14)
        rows = [100 + 13 * i for i in range(300)]
        R.plant(61, rows, [1.0 / (1.0 + (0.003 + 0.017 * i / 299.0) ** 2) ** 0.5 for i in range(300)])
    elif name == "ragged_end":
        # 2048 + 37 rows: the last tile has 5 real rows, the last row block 37.  Hits in the last tile and in the last row
        # block's first tile for a query of row block 0 (second launch: row blocks 5 .. 8 behind it), of row block 1 and of the
        # last row block itself (first launch)
        R = Rows(2048 + 37, 512, 15)
        R.plant(17, [2080, 2081, 2082], falling(3))
        R.plant(2058, [2083, 2084], falling(2))
        R.plant(300, [2048, 2049, 2050, 2051, 2056], falling(5))
    elif name in ("lists_of_16", "lists_of_32"):
        # k = 16 / 32: 16- and 32-entry lists on the shared code, a full tile of hits (16 per lane) and 8 in one lane
        k = 16 if name == "lists_of_16" else 32
        R = Rows(2048, 512, 16 + k)
        R.plant(1000, [tile(5, 1) + r for r in range(32)], falling(32))
        R.plant(333, [tile(6, 4) + r for r in LOW[:8]], falling(8))
        R.plant(1700, [tile(2, 0) + 32 * i + 9 for i in range(14)] + [tile(4, 7) + r for r in (8, 9, 10, 11, 0, 1)], falling(20, 0.9, 0.015))
    elif name == "split_k":
        # d = 1024: the split-k pair kernel (the lower-half wave runs the list code)
        R = Rows(1024, 1024, 18)
        R.plant(700, [tile(1, 3) + r for r in range(32)], falling(32))
        R.plant(40, [tile(3, 5) + r for r in LOW[:3]], falling(3))
        R.plant(901, [tile(0, 2) + (7 * i + 3) % 32 for i in range(8)], falling(8))
    else:
        raise KeyError(name)
    X = R.done()
    ri, rv = oracle.simtopk(X.numpy(), metric="cosine", k=k, exclude_self=True)
    return X, k, ri, rv


def check(mmf, name, path, fallback_free=True):
    X, k, ri, rv = case(name)
    n = X.shape[0]
    sym, G, splits = {"symmetric": (1, 1, 0), "plain": (0, None, 0), "plain_one_range": (0, None, 1)}[path]
    with switches(sym, G):
        i, v, st = mmf.simtopk(X.cuda(), metric="cosine", k=k, precision="fast", col_splits=splits, return_stats=True, query_order="off")
        torch.cuda.synchronize()
    print(f"{name} / {path}: fallback rows {st['fallback_rows']}, scan grid {st['scan_grid']}, column splits {st['col_splits']}")
    assert st["precision_used"] == mmf._lib.PRECISIONS["fast"], st
    if sym:
        assert st["scan_grid"] == sym_grid(mmf, n, G), st
    elif splits:
        assert st["col_splits"] == 1, st
    assert np.array_equal(i.cpu().numpy(), ri), "ids differ from the oracle"
    assert np.array_equal(v.cpu().numpy(), rv), "scores differ from the oracle"
    if fallback_free:
        assert st["fallback_rows"] == 0, st
    return i, v, st


PATHS = ["symmetric", "plain", "plain_one_range"]


@pytest.mark.parametrize("path", PATHS)
def test_several_hits_of_one_lane_in_one_tile(mmf, path):
    X, k, ri, _ = case("several_hits_in_one_lane")
    # the plants are what the queries must find: the query with 3 planted rows has them on top, the others their best 5
    assert sorted(ri[256 * 8 + 5][:3].tolist()) == [tile(5, 0) + r for r in range(3)]
    assert sorted(ri[256 * 8 + 37 * 2 + 5].tolist()) == [tile(5, 4) + r for r in range(5)]
    check(mmf, "several_hits_in_one_lane", path)


@pytest.mark.parametrize("path", PATHS)
def test_one_hit_in_every_lane_in_different_rows(mmf, path):
    X, k, ri, _ = case("one_hit_per_lane")
    assert [int(ri[256 * 8 + 64 + i][0]) for i in range(32)] == [tile(6, 3) + (7 * i + 3) % 32 for i in range(32)]
    check(mmf, "one_hit_per_lane", path)


@pytest.mark.parametrize("path", PATHS)
def test_a_list_that_fills_in_the_middle_of_a_visit(mmf, path):
    X, k, ri, _ = case("list_fills_mid_visit")
    assert ri[256 * 8 + 9][:4].tolist() == [tile(6, 0) + r for r in range(4)]      # the late tile's hits are the best
    check(mmf, "list_fills_mid_visit", path)


@pytest.mark.parametrize("path", PATHS)
def test_crowded_lists_and_the_overflow_path(mmf, path):
    """Rows may overflow here (fallback rows are allowed); the result equals the exact path's."""
    i, v, st = check(mmf, "crowded_lists", path, fallback_free=False)
    X, k, _, _ = case("crowded_lists")
    with switches(0, None):
        ie, ve = mmf.simtopk(X.cuda(), metric="cosine", k=k, precision="exact", query_order="off")
    assert torch.equal(i, ie) and torch.equal(v, ve)


@pytest.mark.parametrize("path", PATHS)
def test_ragged_last_tile_and_last_row_block(mmf, path):
    X, k, ri, _ = case("ragged_end")
    assert sorted(ri[17][:3].tolist()) == [2080, 2081, 2082] and sorted(ri[2058][:2].tolist()) == [2083, 2084]
    i, v, st = check(mmf, "ragged_end", path)
    assert int(i.max()) < X.shape[0], "a padding row was reported"


@pytest.mark.parametrize("path", ["plain", "plain_one_range"])
@pytest.mark.parametrize("name", ["lists_of_16", "lists_of_32"])
def test_the_other_list_capacities(mmf, name, path):
    check(mmf, name, path)


@pytest.mark.parametrize("path", ["plain", "plain_one_range"])
def test_split_k_at_d_1024(mmf, path):
    check(mmf, "split_k", path)
