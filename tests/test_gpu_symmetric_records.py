"""The symmetric 16-bit scan's hit records (DESIGN.md §4.1 "Symmetric scan", *Kernel*): a lane with a hit appends one 64-byte record
per candidate block — header, the four thresholds it tested against, its eight values — and the filing kernel applies the per-value
test (value >= recorded threshold, both rows real) the scan kernel used to do.  Ids and scores bit for bit against the plain scan
(MMF_SYMMETRIC=0) and, for a sample of rows, against the oracle: ragged last row blocks (records carry padding candidates and
queries past n_rows), phase B and the antipodal range, lanes that write two records of several values in one tile, negative
scores in the last row block, both filings, both threshold images, and logs clamped to a few records (MMF_SYMMETRIC_LOG_CAP)."""
import functools
import json
import os
import re
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

KEYS = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G", "MMF_SYMMETRIC_LIVE", "MMF_SYMMETRIC_PRUNE", "MMF_SYMMETRIC_DEBUG", "MMF_SYMMETRIC_LOG_CAP",
        "MMF_SYMMETRIC_ANTIPODAL", "MMF_SYMMETRIC_PHASES")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "symmetric_records_counts.json")

# 2048 rows = 8 row blocks: G = 1 gives eight super-blocks of one row block (phase A, phase B and an antipodal range), G = 2 four;
# 2048 + 300: ten row blocks, the last one 44 real rows and 212 padding rows (its second tile is ragged: 12 real rows)
SHAPES = [(2048, 1), (2048, 2), (2348, 1), (2348, 2)]


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available()
    return m


@contextmanager
def switches(**kw):
    """MMF_SYMMETRIC_<KEY>=value for the calls inside (symmetric=1 -> MMF_SYMMETRIC=1, G=2 -> MMF_SYMMETRIC_G=2, ...); every
    other switch of the symmetric scan is unset."""
    names = {"symmetric": "MMF_SYMMETRIC", **{k[len("MMF_SYMMETRIC_"):].lower(): k for k in KEYS[1:]}}
    old = {k: os.environ.get(k) for k in KEYS}
    for k in KEYS:
        os.environ.pop(k, None)
    for k, v in kw.items():
        if v is not None:
            os.environ[names[k.lower()]] = str(v)
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


# ---- data ----------------------------------------------------------------------------------------------------------------------
# "dup": Gaussian rows with planted groups of six near-duplicates, one group per row block A: rows 5 and 21 of a wave's 32 queries
# in A (the two queries ONE lane holds values for) and rows 1, 2, 17, 18 of a tile in another row block B (the lane's row group in
# BOTH candidate blocks).  Whichever of A and B is the query side of the pair, some lane's eight values of a candidate block are
# group members, for both of its queries and in both candidate blocks: two records from one lane, several passing values in each.
# B = A + 1 + A mod (nb / 2) (cyclic) spreads the pairs over look-back distances 1 .. nb / 2: phase A, the wrap-around pairs of
# phase B, and the antipodal super-block.
def dup_groups(n):
    nb = (n + 255) // 256
    groups, used = [], set()
    for A in range(nb):
        B = (A + 1 + A % (nb // 2)) % nb
        rows = [A * 256 + 32 * (A % 8) + 5, A * 256 + 32 * (A % 8) + 21] + [B * 256 + 32 * ((3 * A + 3) % 8) + r for r in (1, 2, 17, 18)]
        if max(rows) >= n or used & set(rows):
            continue
        used |= set(rows)
        groups.append(rows)
    assert len(groups) >= nb - 2, groups
    return groups


# "opposed" (as in test_gpu_symmetric_lean.py): all rows around one unit vector v (cosines of 0.5 among them), three rows around -v
# in the LAST row block: beyond the other two, everything such a row finds scores about -0.5 — its 3rd to 5th best are negative, and
# the zero of a padding row (no bias rejects it) or of a query past n_rows would beat them.
def opposed_rows(n):
    return [n - 3, n - 20, n - 40]


@functools.lru_cache(maxsize=None)
def data(kind, n, metric):
    g = torch.Generator().manual_seed(4100 + n + (0 if kind == "dup" else 7))
    if kind == "dup":
        X = torch.randn((n, 512), generator=g)
        X = X / X.norm(dim=1, keepdim=True)
        for rows in dup_groups(n):
            base = X[rows[0]].clone()
            X[rows] = base[None, :] + 0.1 * torch.randn((len(rows), 512), generator=g) / 512 ** 0.5
        X = X / X.norm(dim=1, keepdim=True)
    else:
        v = torch.randn(512, generator=g)
        v = v / v.norm()
        noise = torch.randn((n, 512), generator=g) / 512 ** 0.5
        X = v[None, :] + noise
        rows = opposed_rows(n)
        X[rows] = -v[None, :] + noise[rows]
        X = X / X.norm(dim=1, keepdim=True)
    if metric == "dot":
        X = X * 0.3
    return X.contiguous()


def sample_rows(kind, n):
    """First rows of the 32-row slabs checked against the oracle: the planted rows' slabs, the first and the last rows."""
    planted = [r for grp in dup_groups(n) for r in grp] if kind == "dup" else opposed_rows(n)
    return sorted({0, n - 32} | {min(r // 32 * 32, n - 32) for r in planted})


@functools.lru_cache(maxsize=None)
def oracle_slabs(kind, n, metric):
    Xh = data(kind, n, metric).numpy()
    out = {}
    for lo in sample_rows(kind, n):
        out[lo] = oracle.simtopk(Xh[lo:lo + 32], Xh, metric=metric, k=5, exclude_self=True, row_offset=lo)
    if kind == "opposed":     # the case bites only if a score of 0 would enter the three rows' top 5
        assert opposed_rows(n)[0] // 256 == opposed_rows(n)[-1] // 256 == (n - 1) // 256
        for r in opposed_rows(n):
            slab = min(r // 32 * 32, n - 32)
            rv = out[slab][1][r - slab]
            assert (rv[:2] > 0).all() and (rv[2:] < 0).all(), rv
    else:                     # ... and a planted group is each member's top 5
        for grp in dup_groups(n):
            slab = min(grp[0] // 32 * 32, n - 32)
            assert sorted(out[slab][0][grp[0] - slab].tolist()) == sorted(grp[1:]), grp
    return out


def call(mmf, X, metric, precision):
    i, v, st = mmf.simtopk(X, metric=metric, k=5, exclude_self=True, precision=precision, return_stats=True, query_order="off")
    torch.cuda.synchronize()
    return i, v, st


@functools.lru_cache(maxsize=None)
def plain(kind, n, metric, precision):
    """The same call without the symmetric scan: computed once per data set and shared."""
    import multimodal_fusion_amd as m
    with switches(symmetric=0):
        return call(m, data(kind, n, metric).cuda(), metric, precision)


def records_call(mmf, kind, n, G, metric, precision, **sw):
    with switches(symmetric=1, G=G, **sw):
        res = call(mmf, data(kind, n, metric).cuda(), metric, precision)
    assert res[2]["scan_grid"] == sym_grid(mmf, n, G), res[2]
    return res


def check(mmf, kind, n, G, metric, precision, **sw):
    a = records_call(mmf, kind, n, G, metric, precision, **sw)
    b = plain(kind, n, metric, precision)
    assert a[2]["scan_grid"] != b[2]["scan_grid"] and a[2]["precision_used"] == b[2]["precision_used"]
    assert int(a[0].max()) < n, "a padding row was reported"
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "symmetric scan differs from the plain scan"
    ai, av = a[0].cpu().numpy(), a[1].cpu().numpy()
    for lo, (ri, rv) in oracle_slabs(kind, n, metric).items():
        assert np.array_equal(ai[lo:lo + 32], ri) and np.array_equal(av[lo:lo + 32], rv), lo
    return a


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("n,G", SHAPES)
@pytest.mark.parametrize("kind", ["dup", "opposed"])
def test_records_give_the_plain_scans_result(mmf, kind, n, G, metric, precision):
    a = check(mmf, kind, n, G, metric, precision)
    print(f"{kind} n {n} G {G} {metric} {precision}: fallback rows {a[2]['fallback_rows']}")
    if kind == "opposed":    # (the three rows were served by the 16-bit kernels, not by an exact rescan)
        assert a[2]["fallback_rows"] == 0


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("live", [0, None])
@pytest.mark.parametrize("prune", [0, 1])
@pytest.mark.parametrize("kind,metric", [("dup", "cosine"), ("opposed", "dot")])
def test_both_filings_and_both_threshold_images(mmf, kind, metric, prune, live, precision):
    check(mmf, kind, 2348, 1, metric, precision, prune=prune, live=live)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("antipodal,phases", [(1, 2), (0, 1)])
def test_antipodal_pairs_in_the_symmetric_launch_and_the_single_look_back(mmf, antipodal, phases, precision):
    """Eight super-blocks of one row block: the antipodal pairs as symmetric ones (the default only from G = 32 on), and the
    schedule without phases."""
    check(mmf, "dup", 2048, 1, "cosine", precision, antipodal=antipodal, phases=phases)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("prune", [0, 1])
@pytest.mark.parametrize("kind,n,G,metric,cap", [("dup", 2348, 1, "cosine", 3), ("dup", 2048, 2, "dot", 1), ("opposed", 2348, 2, "cosine", 2)])
def test_full_logs_send_their_rows_to_the_exact_rescan(mmf, kind, n, G, metric, cap, prune, precision):
    """Logs of a few records fill; a record that finds none flags its four candidate rows (the real ones), and those rows come out
    of the exact rescan: the results are still the plain scan's.  (How many rows are flagged varies with the live image.)"""
    a = check(mmf, kind, n, G, metric, precision, log_cap=cap, prune=prune)
    print(f"{kind} n {n} G {G} cap {cap}: fallback rows {a[2]['fallback_rows']}")
    assert a[2]["fallback_rows"] > 0


def debug_line(mmf, capfd, prune):
    capfd.readouterr()
    res = check(mmf, "dup", 2348, 1, "cosine", "fast", live=0, prune=prune, debug=1)
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("[mmf symmetric]")]
    assert len(lines) == 1, err
    print(lines[0])
    m = re.search(r"received entries (\d+) \([\d.]+ per row, largest (\d+) of \d+\), fullest wave log (\d+) of (\d+), "
                  r"logged entries (\d+) .*filing (\w+)\), records (\d+),", lines[0])
    assert m, lines[0]
    assert m.group(6) == ("pruned" if prune else "complete")
    received, largest, fullest, cap, logged, records = (int(m.group(i)) for i in (1, 2, 3, 4, 5, 7))
    return res, dict(received=received, largest=largest, fullest=fullest, cap=cap, logged=logged, records=records)


@pytest.mark.parametrize("prune", [0, 1])
def test_counters_against_the_entry_path(mmf, capfd, prune):
    """MMF_SYMMETRIC_DEBUG's counters under the frozen image (MMF_SYMMETRIC_LIVE=0), where they are deterministic.  The entries
    filed into the rows' received lists — their number and the largest list — are those of the entry path, the library built with
    -DMMF_SYM_RECORDS=0 (tests/golden/symmetric_records_counts.json: that build's debug line on these rows, recorded with
    scripts/symmetric_counts.py); a record holds at least one entry, and the complete filing files every entry."""
    with open(GOLDEN) as f:
        want = json.load(f)["pruned" if prune else "complete"]
    _, got = debug_line(mmf, capfd, prune)
    print(got, want)
    assert 0 < got["records"] <= got["logged"]
    assert got["fullest"] <= got["cap"]
    assert got["logged"] == want["logged"]
    assert got["received"] == want["received"] and got["largest"] == want["largest"]
    if not prune:
        assert got["received"] == got["logged"]
    else:
        assert got["received"] < got["logged"]
