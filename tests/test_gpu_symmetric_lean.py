"""The symmetric 16-bit scan without the zero bias, with one early threshold fetch per iteration and with pruned filing of the
received entries (DESIGN.md §4.1 "Symmetric scan"): padding rows that no bias rejects any more, the candidate thresholds under
both images, and MMF_SYMMETRIC_PRUNE both ways — always ids and scores bit for bit against the plain scan (MMF_SYMMETRIC=0) and
against the oracle."""
import functools
import os
import re
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

KEYS = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G", "MMF_SYMMETRIC_LIVE", "MMF_SYMMETRIC_PRUNE", "MMF_SYMMETRIC_DEBUG")


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available()
    return m


@contextmanager
def switches(symmetric, G=None, live=None, prune=None, debug=None):
    old = {k: os.environ.get(k) for k in KEYS}
    for k, v in zip(KEYS, (symmetric, G, live, prune, debug)):
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


def gaussian(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, 512), generator=g, device="cuda", dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def run(mmf, X, sym, G=None, live=None, prune=None, debug=None, **kw):
    kw.setdefault("metric", "cosine")
    kw.setdefault("k", 5)
    with switches(sym, G, live, prune, debug):
        i, v, st = mmf.simtopk(X, return_stats=True, query_order="off", **kw)
        torch.cuda.synchronize()
    if sym:
        assert st["scan_grid"] == sym_grid(mmf, X.shape[0], G), st
    return i, v, st


def same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what


# ---- 1. padding rows without a bias ----------------------------------------------------------------------------------------
# All rows lie around one unit vector v (v plus unit-size noise: cosines of 0.5 among them), three rows around -v sit in the
# first, a middle and the last row block.  Beyond the other two of their group every real candidate of those three scores
# about -0.5, so a padding row of the ragged last row block that came through with G = 0 would enter their top 5.
PAD_SHAPES = [(300, 1), (1100, 1), (2300, 2)]     # no multiple of 32 or 256: the last tile and the last row block are ragged


def opposed_rows(n):
    return [7, (n // 512) * 256 + 131 if n > 512 else 150, n - 3]


@functools.lru_cache(maxsize=None)
def opposed_data(n, metric):
    g = torch.Generator().manual_seed(9000 + n)
    v = torch.randn(512, generator=g)
    v = v / v.norm()
    noise = torch.randn((n, 512), generator=g) / 512 ** 0.5
    X = v[None, :] + noise
    rows = opposed_rows(n)
    X[rows] = -v[None, :] + noise[rows]
    if metric == "cosine":
        X = X / X.norm(dim=1, keepdim=True)
    else:
        X = X * 0.3
    return X.contiguous()


@functools.lru_cache(maxsize=None)
def opposed_oracle(n, metric, exclude_self):
    X = opposed_data(n, metric).numpy()
    ri, rv = oracle.simtopk(X, metric=metric, k=5, exclude_self=exclude_self)
    # the test bites only if a score of 0 would enter the three rows' top 5: beyond the members of their own group (two others,
    # and the row itself when it is not excluded) everything they can find is negative
    first_other = 2 if exclude_self else 3
    rows = opposed_rows(n)
    assert (rv[rows][:, first_other:] < 0).all(), rv[rows]
    assert (rv[rows][:, :first_other] > 0).all(), rv[rows]
    assert len({r // 256 for r in rows}) == (3 if n > 512 else 2) and rows[-1] // 256 == (n - 1) // 256
    return ri, rv


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("n,G", PAD_SHAPES)
def test_padding_rows_are_rejected_without_a_bias(mmf, n, G, metric, exclude_self, precision):
    ri, rv = opposed_oracle(n, metric, exclude_self)
    X = opposed_data(n, metric).cuda()
    kw = dict(metric=metric, k=5, exclude_self=exclude_self, precision=precision)
    a = run(mmf, X, 1, G, **kw)
    b = run(mmf, X, 0, **kw)
    print(f"n {n} G {G} {metric} self excluded {exclude_self} {precision}: fallback rows {a[2]['fallback_rows']} / {b[2]['fallback_rows']}")
    assert a[2]["scan_grid"] != b[2]["scan_grid"] and a[2]["precision_used"] == b[2]["precision_used"]
    assert int(a[0].max()) < n, "a padding row was reported"
    same(a, b, "symmetric scan differs from the plain scan")
    assert np.array_equal(a[0].cpu().numpy(), ri) and np.array_equal(a[1].cpu().numpy(), rv)
    assert a[2]["fallback_rows"] == 0      # (the three rows were served by the 16-bit kernels, not by an exact rescan)


# ---- 2. the early threshold fetch --------------------------------------------------------------------------------------------
FETCH_SHAPES = [(2700, 2), (1900, 3)]       # several super-blocks, wrap-around ranges, left-over row blocks


@functools.lru_cache(maxsize=None)
def gaussian_case(n):
    X = gaussian(n, 1200 + n)
    ri, rv = oracle.simtopk(X.cpu().numpy(), metric="cosine", k=5, exclude_self=True)
    return X, ri, rv


@pytest.mark.parametrize("n,G", FETCH_SHAPES)
def test_one_early_threshold_fetch_per_iteration(mmf, n, G):
    X, ri, rv = gaussian_case(n)
    frozen = run(mmf, X, 1, G, live=0)
    live = run(mmf, X, 1, G, live=1)
    plain = run(mmf, X, 0)
    assert plain[2]["scan_grid"] != live[2]["scan_grid"]
    same(frozen, live, "frozen and live images differ")
    same(live, plain, "symmetric scan differs from the plain scan")
    assert np.array_equal(live[0].cpu().numpy(), ri) and np.array_equal(live[1].cpu().numpy(), rv)
    assert frozen[2]["fallback_rows"] == 0 and live[2]["fallback_rows"] == 0


# ---- 3. pruned filing --------------------------------------------------------------------------------------------------------
def filed_entries(mmf, capfd, X, G, prune):
    """Result of a symmetric call with MMF_SYMMETRIC_PRUNE=prune and the number of entries its filing kernel put into the rows'
    received lists (the library's MMF_SYMMETRIC_DEBUG line)."""
    capfd.readouterr()
    res = run(mmf, X, 1, G, prune=prune, debug=1)
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("[mmf symmetric]")]
    assert len(lines) == 1, err
    m = re.search(r"received entries (\d+) .*logged entries (\d+) .*filing (\w+)", lines[0])
    assert m, lines[0]
    assert m.group(3) == ("pruned" if prune else "complete")
    print(lines[0])
    return res, int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("n,G", FETCH_SHAPES)
def test_pruned_filing_gaussian(mmf, capfd, n, G):
    X, ri, rv = gaussian_case(n)
    full, filed_full, logged_full = filed_entries(mmf, capfd, X, G, 0)
    lean, filed_lean, logged_lean = filed_entries(mmf, capfd, X, G, 1)
    plain = run(mmf, X, 0)
    same(full, lean, "MMF_SYMMETRIC_PRUNE changes the result")
    same(lean, plain, "symmetric scan differs from the plain scan")
    assert np.array_equal(lean[0].cpu().numpy(), ri) and np.array_equal(lean[1].cpu().numpy(), rv)
    assert filed_full <= logged_full and filed_lean <= logged_lean
    # ns = nb / G super-blocks; the symmetric launch has pairs to serve in both directions only from three on ((ns - 1) / 2 > 0):
    # 1900 rows with G = 3 are two super-blocks of plain pairs, nothing is logged and nothing can be pruned
    ns = ((n + 255) // 256) // G
    if (ns - 1) // 2 > 0:
        assert 0 < filed_lean < filed_full, (filed_lean, filed_full)
    else:
        assert filed_lean == filed_full == logged_full == 0, (filed_lean, filed_full, logged_full)


def test_pruned_filing_with_full_received_lists(mmf, capfd):
    """The clustered rows of test_gpu_symmetric.py::test_a_full_received_list_takes_the_exact_rescan: one row copied to every 10th
    row of 16384.  The copies' entries all reach the final threshold, so pruning cannot empty their lists; whether a list still
    overflows or not, the rows come out the same."""
    n, G = 16384, 8
    X = gaussian(n, 71)
    X[::10] = X[0]
    full, filed_full, _ = filed_entries(mmf, capfd, X, G, 0)
    lean, filed_lean, _ = filed_entries(mmf, capfd, X, G, 1)
    plain = run(mmf, X, 0)
    same(full, lean, "MMF_SYMMETRIC_PRUNE changes the result")
    same(lean, plain, "symmetric scan differs from the plain scan")
    assert filed_lean <= filed_full, (filed_lean, filed_full)
    Xh = X.cpu().numpy()
    for lo in (0, 5000, n - 32):
        ri, rv = oracle.simtopk(Xh[lo:lo + 32], Xh, metric="cosine", k=5, exclude_self=True, row_offset=lo)
        assert np.array_equal(lean[0][lo:lo + 32].cpu().numpy(), ri) and np.array_equal(lean[1][lo:lo + 32].cpu().numpy(), rv), lo
    assert lean[0][0].tolist() == [10, 20, 30, 40, 50] and lean[0][10].tolist() == [0, 20, 30, 40, 50]
