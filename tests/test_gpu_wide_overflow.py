"""The wide 16-bit scan's row overflow lists (csrc/mmf_scan_b16w.hip): a crowded list hands what it cannot hold
to the row's 192 overflow slots and loses it only when they are full, so near-duplicate rows at 1024 < d <= 4096 stay on the
fast path.  Every case compares ids and value bits with precision="exact" and with the oracle (rbf values: 1e-5).

Bounds the cases rest on (the header of mmf_scan_b16w.hip): a column is offered to one list pair once and goes to a list, to the
sink, or below the pair's threshold; nothing is written to the sink twice.  So a row that is offered m columns puts at most m
entries into its sink, whatever the policy does with them:
  (a) m = 160 columns.  One column range: the two-stack form has no reservation waste, 160 <= 192 (the issue's tighter count,
      160 - 16 = 144, holds as well).  Two ranges: four lanes reserve in chunks of 8 and waste at most 7 slots each,
      160 + 28 = 188 <= 192.  Nothing can be refused, so no row may be flagged: a condition, not a measurement.
  (b) m = 400 columns, every one inside every row's band (tests/test_wide_overflow_cpu.py recomputes it): lists and sink hold at
      most 2 * splits * CAP + 192 <= 320 < 400 of them, a band column that is in neither has raised `lost` to its key (the
      header's contract), and the audit flags every row.
  (c) the parent's flagged counts on the `tight` rows, measured once with MMF_WIDE_SINK=0 (which (a) shows to be the parent's
      path) at commit 6af99c6; the new counts are printed, not fixed.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_wide_scan import LAM, PRECISION_USED, equal_to, planted, planted_rows   # noqa: E402

pytestmark = pytest.mark.gpu

OVERFLOW_SLOTS = 192
SINK_CHUNK = 8                       # SpillSink::kChunk: slots a lane reserves at a time in the counter form


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert m.wide_scan.OVERFLOW_SLOTS == OVERFLOW_SLOTS
    return m


# ---- data (tests/test_wide_overflow_cpu.py recomputes the bands these cases assume) ---------------------------------------------
@functools.lru_cache(maxsize=None)
def near_identical(m, d):
    """m rows within 1e-4 of row 500 of planted(d): every row has every column inside its margin band."""
    rng = np.random.default_rng(9)
    return planted(d)[500] + 1e-4 * torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def tight_rows():
    """The `tight` rows of test_gpu_wide_scan.test_exact_copies_tight_cluster_and_equal_images."""
    rng = np.random.default_rng(5)
    tight = planted(1536).clone()
    tight[100:200] = tight[100] + 1e-4 * torch.from_numpy(rng.standard_normal((100, 1536)).astype(np.float32))
    return tight


def copies_and_pairs():
    """The exact copies and the shared-image pairs of the same test (same generator, same draws)."""
    base = planted(1536)
    rng = np.random.default_rng(5)
    copies = torch.cat([base[:10].repeat(60, 1), base[600:]])
    rng.standard_normal((100, 1536))                                       # the draws `tight` takes first
    pairs = base.clone()
    cols = torch.from_numpy(rng.integers(0, 1536, size=(360, 8)))
    twin = pairs[0::2].clone()
    twin.scatter_(1, cols, torch.nextafter(twin.gather(1, cols), torch.full((360, 8), 2.0)))
    pairs[1::2] = twin
    return copies, pairs


@functools.lru_cache(maxsize=None)
def clustered_2048():
    """planted_rows(64, 32, 1536, seed=11) with each cluster's 32 rows replaced by its first row + 1e-4 noise."""
    X = torch.from_numpy(planted_rows(64, 32, 1536, seed=11))
    rng = np.random.default_rng(11)
    near = X.clone().reshape(64, 32, 1536)
    near = near[:, :1, :] + 1e-4 * torch.from_numpy(rng.standard_normal((64, 32, 1536)).astype(np.float32))
    return X, near.reshape(2048, 1536).contiguous()


def call(mmf, X, Y, precision, col_splits, **kw):
    got = mmf.simtopk(X, Y, precision=precision, col_splits=col_splits, return_stats=True, **kw)
    torch.cuda.synchronize()
    assert got[2]["precision_used"] == PRECISION_USED[precision] and got[2]["scan_grid"] > 0, got[2]
    return got


def checked(mmf, X, Y, precision, col_splits, what, **kw):
    """One fast call on the GPU copies of X / Y: bits of precision="exact" and of the oracle; returns (idx, val, stats)."""
    metric = kw.get("metric", "cosine")
    Xg, Yg = X.cuda(), None if Y is None else Y.cuda()
    got = call(mmf, Xg, Yg, precision, col_splits, **kw)
    exact = mmf.simtopk(Xg, Yg, precision="exact", **kw)
    torch.cuda.synchronize()
    st = got[2]
    print(f"{what} {precision} splits {col_splits} {kw}: fallback_rows {st['fallback_rows']} overflow_rows {st['overflow_rows']} "
          f"col_splits {st['col_splits']} candidates {st['candidates']}")
    equal_to(got, exact, metric, "exact")
    equal_to(got, oracle.simtopk(X, Y, **kw), metric, "oracle")
    return got


def same_bits(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- (a) everything a row can see fits: nothing may be flagged --------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("shape", ["self", "xy"])
def test_what_fits_the_overflow_slots_is_never_flagged(mmf, monkeypatch, shape, k, precision):
    m, d = 160, 1100
    assert m + 2 * 2 * (SINK_CHUNK - 1) <= OVERFLOW_SLOTS                  # the header's bound for two column ranges
    for dtype in (torch.float32, torch.float16):
        Y = near_identical(m, d).to(dtype)
        if shape == "self":
            X, Yarg, extra = Y, None, {}
        else:
            X = torch.cat([Y, planted(d)[:140].to(dtype)])
            Yarg, extra = Y, {"exclude_self": True, "row_offset": 1000, "col_offset": 1000}
        for metric in ("cosine", "neg_sq_l2"):
            for splits in (1, 2):
                kw = dict(metric=metric, lam=LAM, k=k, **extra)
                monkeypatch.delenv("MMF_WIDE_SINK", raising=False)
                got = checked(mmf, X, Yarg, precision, splits, f"(a) {shape} {dtype}", **kw)
                st = got[2]
                assert st["col_splits"] == splits
                assert st["fallback_rows"] == 0 and st["overflow_rows"] == 0, st
                monkeypatch.setenv("MMF_WIDE_SINK", "0")                   # the parent's path: same bits, never fewer flagged rows
                old = call(mmf, X.cuda(), None if Yarg is None else Yarg.cuda(), precision, splits, **kw)
                monkeypatch.delenv("MMF_WIDE_SINK")
                print(f"    MMF_WIDE_SINK=0: fallback_rows {old[2]['fallback_rows']}")
                same_bits(got, old)
                assert old[2]["fallback_rows"] >= st["fallback_rows"]


# ---- (b) what cannot fit must be flagged ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("splits", [1, 2])
def test_what_cannot_fit_is_flagged(mmf, monkeypatch, splits, k, precision):
    monkeypatch.delenv("MMF_WIDE_SINK", raising=False)
    m = 400
    assert m > 2 * splits * mmf.wide_scan.list_capacity(k, True) + OVERFLOW_SLOTS
    got = checked(mmf, near_identical(m, 1100), None, precision, splits, "(b)", metric="cosine", lam=LAM, k=k)
    assert got[2]["col_splits"] == splits and got[2]["fallback_rows"] == m, got[2]


# ---- (c) the cluster inside a larger scan ---------------------------------------------------------------------------------------------
# fallback_rows of the parent (commit 6af99c6: the MMF_WIDE_SINK=0 path of this build, one run on an MI355X), keyed by
# (metric, precision, k, col_splits): 104 in all sixteen calls — the 100 cluster rows and the four rows whose band is 101 .. 104
PARENT_FLAGGED = {(metric, precision, k, splits): 104
                  for metric in ("cosine", "rbf") for precision in ("fast", "fast_bf16") for k in (5, 15) for splits in (0, 1)}


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("metric", ["cosine", "rbf"])
def test_cluster_inside_a_larger_scan(mmf, monkeypatch, metric, k, precision):
    monkeypatch.delenv("MMF_WIDE_SINK", raising=False)
    for splits in (0, 1):
        got = checked(mmf, tight_rows(), None, precision, splits, "(c) tight", metric=metric, lam=LAM, k=k)
        parent = PARENT_FLAGGED[(metric, precision, k, splits)]
        print(f"    parent's fallback_rows {parent}, now {got[2]['fallback_rows']}")
        assert got[2]["fallback_rows"] <= parent
        assert parent == 0 or got[2]["fallback_rows"] < parent


# ---- (d) several tiles and row blocks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 15])
def test_several_tiles_and_row_blocks(mmf, monkeypatch, k, precision):
    plain, near = clustered_2048()
    for splits in (0, 1, 4):
        monkeypatch.delenv("MMF_WIDE_SINK", raising=False)
        checked(mmf, near, None, precision, splits, "(d) near", metric="cosine", lam=LAM, k=k)
        got = checked(mmf, plain, None, precision, splits, "(d) planted", metric="cosine", lam=LAM, k=k)
        assert got[2]["fallback_rows"] == 0, got[2]
        monkeypatch.setenv("MMF_WIDE_SINK", "0")                           # the band fits: the sink stays empty and costs no candidates
        old = call(mmf, plain.cuda(), None, precision, splits, metric="cosine", lam=LAM, k=k)
        monkeypatch.delenv("MMF_WIDE_SINK")
        same_bits(got, old)
        assert got[2]["candidates"] == old[2]["candidates"], (got[2], old[2])


# ---- (e) exact copies and shared 16-bit images: ties between sink and list entries resolve by id ---------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_exact_copies_and_equal_images_with_the_sink(mmf, monkeypatch, precision):
    monkeypatch.delenv("MMF_WIDE_SINK", raising=False)
    copies, pairs = copies_and_pairs()
    for name, X in (("copies", copies), ("pairs", pairs)):
        for k in (5, 15):
            for splits in (0, 1):
                checked(mmf, X, None, precision, splits, f"(e) {name}", metric="cosine", lam=LAM, k=k)
    checked(mmf, copies, None, precision, 1, "(e) copies", metric="rbf", lam=LAM, k=5)


# ---- (f) stream contract ---------------------------------------------------------------------------------------------------------------
def test_stream_contract_behind_a_closed_gate(mmf, monkeypatch):
    """tests/streamgate.py: one call of case (a) on a busy non-default stream, its inputs produced behind a closed gate."""
    import streamgate
    monkeypatch.delenv("MMF_WIDE_SINK", raising=False)

    def make_inputs(which):
        Y = near_identical(160, 1100)
        return [Y.clone() if which == "truth" else planted(1100)[:160].clone()]

    def entry(X):
        idx, val, st = mmf.simtopk(X, metric="cosine", k=5, precision="fast", col_splits=1, return_stats=True)
        assert st["precision_used"] == 2, st
        return idx, val

    def reference(X):
        idx, val = oracle.simtopk(X, metric="cosine", k=5)
        return [np.asarray(idx), np.asarray(val)]

    streamgate.run_gated(entry, make_inputs, reference, name="ops.simtopk wide scan with overflow lists")
