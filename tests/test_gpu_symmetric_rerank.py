"""The re-rank behind the symmetric 16-bit scan (DESIGN.md §4.3 "Lean gather"): the received entries as (id, key) pairs, every
count of a row in one memory round trip and every entry in a second, and the pruning threshold by rank counting when the union
holds at most 64 entries.  Every result is compared bit for bit, ids and scores, with the plain scan (MMF_SYMMETRIC=0), with the
serial gather and the round loop (MMF_SELECT_LEAN=0) and with precision="exact" on the same rows."""
import os
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 512


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available()
    return m


@contextmanager
def switches(**env):
    """Sets the given MMF_* switches (None: unset) for the calls inside; all of them are read per call."""
    keys = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G", "MMF_SELECT_LEAN")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        v = env.get(k)
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


def make(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, D), generator=g, device="cuda", dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def sym_grid(mmf, n, G):
    return 2 * mmf._lib.lib().mmf_debug_symmetric_schedule((n + 255) // 256, G, 0, None, 0)


_exact = {}


def exact(mmf, tag, X, k):
    """precision="exact" on the same rows, computed once per (data set, k)."""
    if (tag, k) not in _exact:
        i, v = mmf.simtopk(X, metric="cosine", k=k, precision="exact", query_order="off")
        _exact[(tag, k)] = (i, v)
    return _exact[(tag, k)]


def all_ways(mmf, tag, X, G, k, precision="fast"):
    """The lean re-rank behind the symmetric scan; asserts that the symmetric path ran and that its bits are those of the serial
    gather with the round loop, of the plain scan and of the exact path.  Returns (ids, scores, stats) of the lean call."""
    n = X.shape[0]
    kw = dict(metric="cosine", k=k, precision=precision, query_order="off", return_stats=True)
    with switches(MMF_SYMMETRIC=1, MMF_SYMMETRIC_G=G):
        i1, v1, s1 = mmf.simtopk(X, **kw)
    with switches(MMF_SYMMETRIC=1, MMF_SYMMETRIC_G=G, MMF_SELECT_LEAN=0):
        i2, v2, s2 = mmf.simtopk(X, **kw)
    with switches(MMF_SYMMETRIC=0):
        i0, v0, s0 = mmf.simtopk(X, **kw)
    assert s1["scan_grid"] == sym_grid(mmf, n, G) and s2["scan_grid"] == s1["scan_grid"], (s1, s2)
    if (n + 255) // 256 > 1:
        assert s0["scan_grid"] != s1["scan_grid"]
    assert torch.equal(i1, i2) and torch.equal(v1, v2), "MMF_SELECT_LEAN=0 gives other bits"
    assert torch.equal(i1, i0) and torch.equal(v1, v0), "MMF_SYMMETRIC=0 gives other bits"
    ie, ve = exact(mmf, tag, X, k)
    assert torch.equal(i1, ie) and torch.equal(v1, ve), "precision=exact gives other bits"
    return i1, v1, s1


_rows = {}


def gaussian(n):
    if n not in _rows:
        _rows[n] = make(n, 700 + n)
    return _rows[n]


# G = 2: 3072 rows are 12 row blocks in 6 super-blocks, 3072 + 300 rows are 14 row blocks (the last one ragged) in 7.  The unions of
# Gaussian rows (at most 60 list entries and a few received ones, 30-50 together) stay under 65: rank counting finds the threshold.
@pytest.mark.parametrize("k", [1, 5, 10])
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("n", [3072, 3072 + 300])
def test_gaussian_rows(mmf, n, precision, k):
    _, _, st = all_ways(mmf, ("gauss", n), gaussian(n), 2, k, precision)
    assert st["fallback_rows"] == 0


def test_equal_keys_meet_in_the_union(mmf):
    """Blocks of identical rows spread over different super-blocks (512 rows each): a copy finds some of the others through its own
    lists and receives the rest, all with the same key, and (key desc, position asc) decides which of them rank before the
    threshold entry.  Same ids as with the switch off (all_ways), and the ids the tie-break by id demands."""
    n = 3072
    X = make(n, 7).clone()
    a = [50, 51, 52, 700, 701, 1500, 2300, 2301, 3000]          # super-blocks 0, 1, 2, 4, 5
    b = [10, 600, 1200, 1800, 2400, 3071]                       # one copy in every super-block
    X[a] = X[a[0]].clone()
    X[b] = X[b[0]].clone()
    for k in (1, 5):
        i, _, st = all_ways(mmf, "ties", X, 2, k)
        assert i[a[0]].tolist() == a[1:1 + k] and i[a[-1]].tolist() == a[:k]
        assert i[b[0]].tolist() == b[1:1 + k] and i[b[2]].tolist() == (b[:2] + b[3:])[:k]


def test_a_union_above_64_takes_the_round_loop(mmf):
    """One row copied to every 40th row of 4096 (8 super-blocks of 512 rows, 12 or 13 copies in each): a copy finds the copies of its
    own and the antipodal super-block (about 25) and of three more (about 38) through its own lists, and receives those of the other
    three (about 38): a union of about 100 entries with equal keys — above the 64 that rank counting takes, far below the 512 received
    entries and the 60 + 192 list and overflow entries a row can hold.  The round loop finds the threshold, and no row is flagged."""
    n, G = 4096, 2
    X = make(n, 17).clone()
    X[::40] = X[0]
    i, _, st = all_ways(mmf, "union", X, G, 5)
    assert st["fallback_rows"] == 0
    assert i[0].tolist() == [40, 80, 120, 160, 200] and i[40].tolist() == [0, 80, 120, 160, 200]


@pytest.mark.parametrize("n,k", [(6, 5), (11, 10), (3, 2)])
def test_a_union_of_at_most_k_plus_self_entries(mmf, n, k):
    """A row cannot carry more than n <= k + self entries (its own column among them): nothing is pruned, neither way of finding the
    threshold runs.  One row block, which is its own super-block pair."""
    _, _, st = all_ways(mmf, ("tiny", n), make(n, 900 + n), 1, k)
    assert st["fallback_rows"] == 0


def test_two_super_blocks_of_a_few_rows(mmf):
    """256 + 5 rows with G = 1: one pair of super-blocks, the second one of five rows."""
    _, _, st = all_ways(mmf, "pair", make(261, 33), 1, 5)
    assert st["fallback_rows"] == 0


def test_a_full_received_list_still_takes_the_exact_rescan(mmf):
    """One row copied to every 10th row of 16384 (8 super-blocks): a copy receives 3/8 of the 1638 others, 614 entries — more than
    the 512 pairs its received list holds — while the waves' logs hold everything: the filing finds the lists full, flags the rows,
    and the exact rescan serves them."""
    n, G = 16384, 8
    X = make(n, 71).clone()
    X[::10] = X[0]
    i, _, st = all_ways(mmf, "full", X, G, 5)
    assert st["fallback_rows"] > 0
    assert i[0].tolist() == [10, 20, 30, 40, 50] and i[10].tolist() == [0, 20, 30, 40, 50]
