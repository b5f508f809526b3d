"""The symmetric 16-bit scan's group test (DESIGN.md §4.1 "Symmetric scan", *Kernel*): behind a tile's chain the candidate side
costs one compare, the lane's largest value against the smallest threshold of the eight candidate rows its values belong to (the
group minima: a second live image behind the thresholds); the per-row test runs in the cold block behind it.  The group test may
only ever drop what the per-row test would drop: ids and scores bit for bit against the plain scan (MMF_SYMMETRIC=0) for f16 and
bf16 operands, the frozen and the live image, cosine and dot; the frozen image's counters against the entry path's golden
line; groups whose rows have very different thresholds; the padded last tile and logs clamped to a few records; the debug line's
"coarse visits" and "hit wave-tiles".

Counts: tests/golden/symmetric_records_counts.json is the line of the -DMMF_SYM_RECORDS=0 build, whose "records" are ENTRIES
(24 884); logged entries, received entries and the largest list are compared with it.  The number of 64-byte records on the same
rows is 23 572 (profiles/r10_symmetric_records.txt §1), and that is what the records are compared with."""
import functools
import json
import os
import re
import subprocess
import sys
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G", "MMF_SYMMETRIC_LIVE", "MMF_SYMMETRIC_PRUNE", "MMF_SYMMETRIC_DEBUG", "MMF_SYMMETRIC_LOG_CAP",
        "MMF_SYMMETRIC_ANTIPODAL", "MMF_SYMMETRIC_PHASES")
GOLDEN = os.path.join(HERE, "golden", "symmetric_records_counts.json")
RECORDS_R10 = 23572          # 64-byte records of the 'dup' rows under the frozen image (profiles/r10_symmetric_records.txt §1)
COARSE0 = os.path.join(ROOT, "multimodal-fusion_amd", "libmmf_hg_coarse0.so")    # scripts/ab_build.sh coarse0 -DMMF_SYM_COARSE=0

# 2348 rows: ten row blocks, the last one 44 real rows and 212 padding rows (its second tile is ragged: 12 real rows, and its row
# groups 2 and 3 hold no real row at all).  G = 1: ten super-blocks; G = 3: three super-blocks and one left-over row block.
N = 2348


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


# ---- data ----------------------------------------------------------------------------------------------------------------------
def dup_groups(n):
    """The planted groups of six near-duplicates of tests/test_gpu_symmetric_records.py (the golden counts are of these rows)."""
    nb = (n + 255) // 256
    groups, used = [], set()
    for A in range(nb):
        B = (A + 1 + A % (nb // 2)) % nb
        rows = [A * 256 + 32 * (A % 8) + 5, A * 256 + 32 * (A % 8) + 21] + [B * 256 + 32 * ((3 * A + 3) % 8) + r for r in (1, 2, 17, 18)]
        if max(rows) >= n or used & set(rows):
            continue
        used |= set(rows)
        groups.append(rows)
    return groups


# "mixed": unequal thresholds inside one row group.  All rows lie around one unit vector v (cosines of about 0.5 among them).  In
# the first tile of the first, a middle and the last row block, row group 0 (rows 0..3 and 16..19 of the tile) holds
#   * row 1: a row with five near-duplicates in the NEXT row block (cyclic) — its threshold is about 0.99;
#   * rows 2 and 17: rows around -2 v with a private component each (the six of them are spread like a simplex: cosines among them
#     about -0.03, with everything else about -0.25) — every cosine they see is negative, their thresholds are the lowest there are;
#   * the other five: ordinary rows, thresholds a little above 0.5.
# The group's minimum is a negative number that every value of the tile passes; the per-row test behind it has to tell a 0.5 that is
# nothing for rows 1 and 0 from the -0.2 that is a top-5 entry of row 2.
def mixed_plan(n):
    nb = (n + 255) // 256
    plan = []
    for i, A in enumerate((0, nb // 2, nb - 1)):
        r0 = A * 256
        B = (A + 1) % nb
        plan.append(dict(high=r0 + 1, dups=[B * 256 + 64 + 32 * i + r for r in (3, 9, 20, 21, 30)], low=[r0 + 2, r0 + 17]))
    return plan


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
    elif kind == "opposed":     # as in tests/test_gpu_symmetric_records.py: three rows around -v in the last row block
        v = torch.randn(512, generator=g)
        v = v / v.norm()
        noise = torch.randn((n, 512), generator=g) / 512 ** 0.5
        X = v[None, :] + noise
        rows = [n - 3, n - 20, n - 40]
        X[rows] = -v[None, :] + noise[rows]
        X = X / X.norm(dim=1, keepdim=True)
    else:
        v = torch.randn(512, generator=g)
        v = v / v.norm()
        noise = torch.randn((n, 512), generator=g) / 512 ** 0.5
        X = v[None, :] + noise
        plan = mixed_plan(n)
        low = [r for p in plan for r in p["low"]]
        Z = torch.randn((len(low), 512), generator=g)
        Z = Z - (Z @ v)[:, None] * v[None, :]
        Z = torch.linalg.qr(Z.T).Q.T                        # orthonormal rows, orthogonal to v ...
        Z = Z - Z.mean(dim=0, keepdim=True)                 # ... centred: the rows point away from each other, a simplex
        Z = 5.0 * Z / Z.norm(dim=1, keepdim=True)
        X[low] = -2.0 * v[None, :] + Z + noise[low]
        for p in plan:
            X[p["dups"]] = X[p["high"]][None, :] + 0.1 * torch.randn((5, 512), generator=g) / 512 ** 0.5
        X = X / X.norm(dim=1, keepdim=True)
    if metric == "dot":
        X = X * 0.3
    return X.contiguous()


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


def check(mmf, kind, n, G, metric, precision, **sw):
    with switches(symmetric=1, G=G, **sw):
        a = call(mmf, data(kind, n, metric).cuda(), metric, precision)
    b = plain(kind, n, metric, precision)
    assert a[2]["scan_grid"] != b[2]["scan_grid"] and a[2]["precision_used"] == b[2]["precision_used"]
    assert int(a[0].max()) < n, "a padding row was reported"
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "symmetric scan differs from the plain scan"
    return a


# ---- results -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("live", [0, None])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_group_test_gives_the_plain_scans_result(mmf, metric, live, precision):
    check(mmf, "dup", N, 1, metric, precision, live=live)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("live", [0, None])
def test_left_over_row_blocks_and_a_ragged_last_row_block(mmf, live, precision):
    check(mmf, "dup", N, 3, "cosine", precision, live=live)


def test_mixed_rows_are_what_they_are_meant_to_be():
    """(on the CPU, f32) row 1's best five are its near-duplicates; the rows around -v see nothing but negative cosines."""
    X = data("mixed", N, "cosine")
    for p in mixed_plan(N):
        s = X[[p["high"]] + p["low"]] @ X.T
        s[0, p["high"]] = s[1, p["low"][0]] = s[2, p["low"][1]] = -2.0
        top = s.topk(5, dim=1)
        assert sorted(top.indices[0].tolist()) == sorted(p["dups"]) and float(top.values[0].min()) > 0.95
        assert float(s[1:].max()) < 0.0, float(s[1:].max())
    assert mixed_plan(N)[-1]["high"] // 256 == (N - 1) // 256 and mixed_plan(N)[0]["high"] // 256 == 0


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("live", [0, None])
@pytest.mark.parametrize("G,metric", [(1, "cosine"), (1, "dot"), (3, "cosine")])
def test_unequal_thresholds_inside_one_group(mmf, G, metric, live, precision):
    a = check(mmf, "mixed", N, G, metric, precision, live=live)
    i = a[0].cpu()
    for p in mixed_plan(N):
        assert sorted(i[p["high"]].tolist()) == sorted(p["dups"])
    assert a[2]["fallback_rows"] == plain("mixed", N, metric, precision)[2]["fallback_rows"] == 0


# ---- padding and capacity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("live", [0, None])
@pytest.mark.parametrize("G", [1, 3])
def test_padded_last_tile(mmf, G, live, precision):
    """Rows around -v in the ragged last row block: a zero of a padding row would beat their negative scores, and a padding group
    that passed would offer them.  The rows are served by the 16-bit kernels, as before: no row goes to the exact rescan."""
    a = check(mmf, "opposed", N, G, "cosine", precision, live=live)
    assert a[2]["fallback_rows"] == 0


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("kind,G,metric,cap", [("dup", 1, "cosine", 3), ("mixed", 3, "dot", 2), ("opposed", 1, "cosine", 2)])
def test_full_logs_send_their_rows_to_the_exact_rescan(mmf, kind, G, metric, cap, precision):
    a = check(mmf, kind, N, G, metric, precision, log_cap=cap)
    print(f"{kind} G {G} cap {cap}: fallback rows {a[2]['fallback_rows']}")
    assert a[2]["fallback_rows"] > 0


# ---- counters ------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"received entries (\d+) \([\d.]+ per row, largest (\d+) of \d+\), fullest wave log (\d+) of (\d+), "
                  r"logged entries (\d+) .*filing (\w+)\), records (\d+),.* coarse visits (\d+), hit wave-tiles (\d+)")


def parse(err):
    lines = [l for l in err.splitlines() if l.startswith("[mmf symmetric]")]
    assert len(lines) == 1, err
    print(lines[0])
    m = LINE.search(lines[0])
    assert m, lines[0]
    names = ("received", "largest", "fullest", "cap", "logged", "filing", "records", "coarse", "hit_tiles")
    return {k: (v if k == "filing" else int(v)) for k, v in zip(names, m.groups())}


def debug_line(mmf, capfd, **sw):
    capfd.readouterr()
    res = check(mmf, "dup", N, 1, "cosine", "fast", debug=1, **sw)
    return res, parse(capfd.readouterr().err)


@pytest.mark.parametrize("prune", [0, 1])
def test_counts_under_the_frozen_image(mmf, capfd, prune):
    """The group test never hides a hit of the per-row test: with the frozen image the group minima are the exact minima of the
    thresholds the per-row test reads, and records, logged and filed entries are what they were."""
    with open(GOLDEN) as f:
        want = json.load(f)["pruned" if prune else "complete"]
    _, got = debug_line(mmf, capfd, live=0, prune=prune)
    print(got, want)
    assert got["filing"] == ("pruned" if prune else "complete")
    assert got["records"] == RECORDS_R10
    assert got["logged"] == want["logged"]
    assert got["received"] == want["received"] and got["largest"] == want["largest"]
    assert got["fullest"] <= got["cap"]
    assert got["hit_tiles"] <= got["coarse"] and 0 < got["hit_tiles"] <= got["records"]


@pytest.mark.parametrize("live", [0, None])
def test_coarse_visits_cover_the_wave_tiles_with_records(mmf, capfd, live):
    _, got = debug_line(mmf, capfd, live=live)
    assert got["coarse"] >= got["hit_tiles"] > 0
    assert got["records"] >= got["hit_tiles"]           # a wave-tile with a hit writes at least one record


def _child():
    """Run in a process of its own (the library is chosen when the package is first used): the debug line of the frozen image."""
    import multimodal_fusion_amd as m
    with switches(symmetric=1, G=1, live=0, debug=1):
        a = call(m, data("dup", N, "cosine").cuda(), "cosine", "fast")
    print("fallback_rows", a[2]["fallback_rows"])


def test_records_of_the_build_without_the_group_test(mmf, capfd):
    """The same call on a library built with -DMMF_SYM_COARSE=0 (scripts/ab_build.sh coarse0 -DMMF_SYM_COARSE=0), chosen with
    MMF_HG_LIBRARY: under the frozen image both builds write the same records and file the same entries."""
    if not os.path.exists(COARSE0):
        pytest.skip("no -DMMF_SYM_COARSE=0 build (scripts/ab_build.sh coarse0 -DMMF_SYM_COARSE=0)")
    a, got = debug_line(mmf, capfd, live=0)
    env = dict(os.environ, MMF_HG_LIBRARY=COARSE0, PYTHONPATH=os.pathsep.join([ROOT, HERE] + sys.path))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_symmetric_coarse as t; t._child()"], env=env, cwd=HERE,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ref = parse(r.stderr)
    assert ref["coarse"] == 0                          # that build has no group test
    for k in ("records", "logged", "received", "largest", "fullest", "hit_tiles"):
        assert got[k] == ref[k], (k, got, ref)
    assert f"fallback_rows {a[2]['fallback_rows']}" in r.stdout
