"""The segmented 16-bit top-k of the combined similarity K_h * K_g on the MI355X (mmf_simtopk_combined_fast_segmented, DESIGN.md
§4.18): every graph of a ragged batch from ONE launch of the combined-key 16-bit scan.

Every call made through check() is checked four ways: the indices are those of the numpy reference() of
tests/test_gpu_simtopk_combined.py with the batch's offsets; the values are BITWISE the entries ops.sim_dense_combined writes for
the row's segment and within 1e-5 of the oracle's; the whole result is BITWISE combined_topk.simtopk_combined(ptr=...)'s; and no
index leaves its row's segment (ptr[s] <= idx < ptr[s + 1] or idx == -1).  precision="fast" (f16 operands) and "fast_bf16" both
run unless a case says otherwise.

Data: tests/combined16_seg_restate.py batch(): per segment the 12 Gaussian centres + noise of combined16_restate.make_data with
seed + s; lambda_h = 0.5, lambda_g = 2e-7.  The margin band of a row inside its segment, with the batch's scale and maxima, is
restated there (bands_segmented); where a case relies on "no row is crowded" it asserts that from the restatement first, so the
exact rescan must stay idle and cannot hide a scan that loses candidates."""
import ctypes
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combined16_restate as cr        # noqa: E402
import combined16_seg_restate as sr    # noqa: E402
import streamgate as sg                # noqa: E402
from test_gpu_simtopk_combined import bits, offsets_of, reference   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
LH, LG = 0.5, 2e-7
PRECISIONS = ["fast", "fast_bf16"]
OPERAND = {"fast": "f16", "fast_bf16": "bf16"}
PREC_CODE = {"exact": 1, "fast": 2, "fast_bf16": 3}
ENTRY = "mmf_simtopk_combined_fast_segmented"

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "Segmented 16-bit top-k entries"
# (tests/test_simtopk_combined_fast_segmented_cpu.py keeps the two equal)
SYNC = {ENTRY: ("data-dependent", "the call")}

# the capacity condition's batches: (segment sizes, d, dp), seed CAP_SEED
CAPACITY_BATCHES = [([1, 2, 5, 127, 0, 128, 129, 257, 300, 40], 40, 2), ([300, 129, 64], 512, 2), ([129, 300], 1536, 2),
                    ([130, 7, 260], 130, 8), ([600, 300, 1100], 64, 3)]
CAP_SEED = 40

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def seg():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16_segmented")


def ct():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk")


def ct16():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16")


_REF = {}


def ref_of(key, F, P, ptr, k, lh=LH, lg=LG, exclude_self=True):
    """The numpy reference, computed once per case and shared by the precisions."""
    if key not in _REF:
        _REF[key] = reference(F, P, ptr, k, lh, lg, exclude_self)
    return _REF[key]


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def no_leak(idx, ptr):
    """ptr[s] <= idx < ptr[s + 1] or idx == -1, for every row of every segment."""
    idx = np.asarray(idx)
    for a, b in zip(ptr[:-1], ptr[1:]):
        blk = idx[a:b]
        if not np.all((blk == -1) | ((blk >= a) & (blk < b))):
            return False
    return True


def check(mmf, F, P, ptr, k, precision, lh=LH, lg=LG, exclude_self=True, how="ptr", ref=None, **kw):
    """One call against the reference, the dense entries, the exact entry and the segment bounds; (idx, val, stats) on the host."""
    n = F.shape[0]
    ptr = np.asarray(ptr, dtype=np.int64)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    s = {"ptr": T(ptr)} if how == "ptr" else {"batch": torch.repeat_interleave(torch.arange(len(ptr) - 1), T(ptr[1:] - ptr[:-1])).cuda()}
    gi, gv, st = seg().simtopk_combined_fast_segmented(Fd, Pd, lh, lg, k, exclude_self=exclude_self, precision=precision,
                                                       return_stats=True, **s, **kw)
    torch.cuda.synchronize()
    assert gi.shape == (n, k) and gi.dtype == torch.int64 and gv.dtype == torch.float32 and gi.is_cuda
    idx, val = gi.cpu().numpy(), gv.cpu().numpy()
    assert no_leak(idx, ptr), "an index outside its row's segment"
    ridx, rval = ref if ref is not None else reference(F, P, ptr, k, lh, lg, exclude_self)
    bad = np.nonzero((idx != ridx).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ from the reference, first {bad[0]}: got {idx[bad[0]]}, want {ridx[bad[0]]}"
    there = ridx >= 0
    assert np.all(np.isneginf(val[~there]))
    for a, b in zip(ptr[:-1], ptr[1:]):
        if not there[a:b].any():
            continue
        K = mmf.ops.sim_dense_combined(Fd[a:b], Pd[a:b], lh, lg).cpu().numpy()
        rows = np.broadcast_to(np.arange(b - a)[:, None], (b - a, k))[there[a:b]]
        want = K[rows, (ridx[a:b] - a)[there[a:b]]]
        assert np.array_equal(bits(val[a:b][there[a:b]]), bits(want)), f"segment [{a}, {b}): values differ from sim_dense_combined's bits"
    err = float(np.abs(val[there].astype(np.float64) - rval[there].astype(np.float64)).max()) if there.any() else 0.0
    print(f"max |val - oracle| = {err:.3e}, fallback_rows {st['fallback_rows']}, scan_grid {st['scan_grid']}, col_splits {st['col_splits']}")
    assert err <= TOL
    want = ct().simtopk_combined(Fd, Pd, lh, lg, k, exclude_self=exclude_self, ptr=T(ptr))
    assert same_bits((gi, gv), want), "the result differs from combined_topk.simtopk_combined(ptr=...)'s bits"
    return idx, val, st


# ---- 1. the capacity condition: the exact rescan must stay idle ------------------------------------------------------------
@pytest.mark.parametrize("sizes,d,dp", CAPACITY_BATCHES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_capacity_condition(mmf, sizes, d, dp, precision):
    """No row's restated band exceeds its list capacity (asserted here and, without a GPU, by
    tests/test_simtopk_combined_fast_segmented_cpu.py), so no row of a scanned segment may reach the exact pass — for every list
    capacity (k + self = 6, 11, 12, 20) and col_splits 1, 2, 4.  Segments with fewer than k admissible columns go to the exact
    pass by design; they are not counted as fallback.  The reference is checked at col_splits 1; the other counts give its bits."""
    F, P, ptr = sr.batch(sizes, d, dp, CAP_SEED)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    for kk in (6, 11, 12, 20):
        k = kk - 1
        _, _, cnt = sr.bands_segmented(F, P, ptr, LH, LG, kk, OPERAND[precision])
        cap = cr.capacity(kk)
        crowded = int((cnt > cap).sum())
        print(f"{sizes} d {d} dp {dp} {precision} k + self {kk}: largest band {int(cnt.max())} of {cap}, crowded rows {crowded}")
        assert crowded == 0
        ref = ref_of(("cap", tuple(sizes), d, dp, k), F, P, ptr, k)
        idx, val, st = check(mmf, F, P, ptr, k, precision, ref=ref, col_splits=1)
        assert st["fallback_rows"] == 0 and st["precision_used"] == PREC_CODE[precision] and st["col_splits"] == 1, st
        for cs in (2, 4):
            gi, gv, st = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, k, ptr=T(ptr), precision=precision, col_splits=cs,
                                                               return_stats=True)
            assert st["fallback_rows"] == 0, (kk, cs, st)
            assert np.array_equal(gi.cpu().numpy(), idx) and np.array_equal(bits(gv.cpu().numpy()), bits(val)), (kk, cs)


# ---- 2. the smallest shapes where it can go wrong ----------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_block_and_tile_boundaries(mmf, precision):
    """A segment of exactly one tile, one query past a row block, one column past two tiles — in one batch."""
    F, P, ptr = sr.batch([128, 129, 257], 40, 2, 1)
    _, _, st = check(mmf, F, P, ptr, 5, precision, ref=ref_of(("bound",), F, P, ptr, 5))
    assert st["scan_grid"] == 1 + 2 * 2 + 3 * 2 and st["precision_used"] == PREC_CODE[precision]      # one tile: one range; else two


@pytest.mark.parametrize("sizes", [[0, 130, 40], [130, 0, 40], [130, 40, 0], [0, 0, 130, 0]])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_empty_segments(mmf, sizes, precision):
    F, P, ptr = sr.batch(sizes, 40, 2, 2)
    check(mmf, F, P, ptr, 5, precision, ref=ref_of(("empty", tuple(sizes)), F, P, ptr, 5))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_batch_of_one_segment_is_the_one_graph_call(mmf, precision):
    F, P, ptr = sr.batch([300], 40, 2, 3)
    check(mmf, F, P, ptr, 5, precision, ref=ref_of(("one",), F, P, ptr, 5))
    Fd, Pd = T(F).cuda(), T(P).cuda()
    a = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=[0, 300], precision=precision)
    b = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision)
    assert same_bits(a, b)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_segments_of_one_row(mmf, precision):
    F, P, ptr = sr.batch([1, 1, 1, 1], 40, 2, 4)
    idx, val, _ = check(mmf, F, P, ptr, 5, precision)
    assert np.all(idx == -1) and np.all(np.isneginf(val))
    idx, val, _ = check(mmf, F, P, ptr, 5, precision, exclude_self=False)
    for i in range(4):
        assert list(idx[i]) == [i, -1, -1, -1, -1] and val[i, 0] == 1.0 and np.all(np.isneginf(val[i, 1:]))


@pytest.mark.parametrize("k", [5, 19])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_k_beyond_some_segments(mmf, k, precision):
    """k >= n_s in some segments (ranked exactly for what they have, then -1 / -inf) and not in others (scanned)."""
    sizes = [3, 140, 6, 1, 20, 260]
    F, P, ptr = sr.batch(sizes, 40, 2, 5)
    idx, _, st = check(mmf, F, P, ptr, k, precision, ref=ref_of(("kbeyond", k), F, P, ptr, k), col_splits=1)
    served = [n_s for n_s in sizes if n_s - 1 >= k]
    assert st["scan_grid"] == sum((n_s + 127) // 128 for n_s in served) and st["fallback_rows"] == 0
    for s, n_s in enumerate(sizes):
        blk = idx[ptr[s]:ptr[s + 1]]
        assert np.all(blk[:, :min(k, n_s - 1)] >= 0) and np.all(blk[:, min(k, n_s - 1):] == -1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_vector_instead_of_offsets(mmf, precision):
    F, P, ptr = sr.batch([130, 40, 129], 40, 2, 6)
    check(mmf, F, P, ptr, 5, precision, how="batch", ref=ref_of(("batchvec",), F, P, ptr, 5))


@pytest.mark.parametrize("dp", [1, 3, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_position_dims(mmf, dp, precision):
    """Every chain length of the epilogue: 2 (dp 1), 4 (dp 3), 8."""
    F, P, ptr = sr.batch([130, 40, 129], 40, dp, 7)
    check(mmf, F, P, ptr, 5, precision, ref=ref_of(("dp", dp), F, P, ptr, 5))


@pytest.mark.parametrize("term", ["features only", "positions only"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_zero_lambda_drops_its_term(mmf, term, precision):
    """Against an entry that is already pinned: the exact segmented RBF top-k of the one operand that is left.  lambda_h = 0
    makes a = 0, which meets the -inf bias of every segment's padding columns (127, 88 and 84 of them here)."""
    F, P, ptr = sr.batch([129, 40, 300], 40, 2, 8)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    if term == "features only":
        got = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, 0.0, 5, ptr=ptr, precision=precision)
        want = mmf.ops.simtopk_segmented(Fd, ptr=ptr, metric="rbf", lam=LH, k=5, precision="exact")
    else:
        got = seg().simtopk_combined_fast_segmented(Fd, Pd, 0.0, LG, 5, ptr=ptr, precision=precision)
        want = mmf.ops.simtopk_segmented(Pd, ptr=ptr, metric="rbf", lam=LG, k=5, precision="exact")
    torch.cuda.synchronize()
    assert same_bits(got, want) and no_leak(got[0].cpu().numpy(), ptr)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_all_zero_feature_row(mmf, precision):
    F, P, ptr = sr.batch([130, 40, 129], 40, 2, 9)
    F[7] = 0.0
    F[200] = 0.0
    check(mmf, F, P, ptr, 5, precision, ref=ref_of(("zero",), F, P, ptr, 5))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_planted_copies_across_a_segment_boundary(mmf, precision):
    """Rows 125 .. 129 of segment 0 and rows 0 .. 4 of segment 1 (global 130 .. 134) hold the same features and position: the best
    possible columns of each lie in the OTHER segment, next to the boundary.  A row's answer holds only ids of its own segment."""
    F, P, ptr = sr.batch([130, 140], 40, 2, 10)
    F[125:135] = F[125]
    P[125:135] = P[125]
    idx, val, _ = check(mmf, F, P, ptr, 5, precision, ref=ref_of(("plant",), F, P, ptr, 5))
    assert list(idx[125, :4]) == [126, 127, 128, 129] and list(idx[132, :4]) == [130, 131, 133, 134]
    assert np.all(val[125, :4] == 1.0) and np.all(val[132, :4] == 1.0) and val[125, 4] < 1.0


# ---- 3. no leak between segments: asserted by check() for every call above -------------------------------------------------
def test_the_leak_check_itself():
    ptr = np.array([0, 2, 2, 5])
    assert no_leak([[1, -1], [0, -1], [3, 4], [2, 4], [2, 3]], ptr)
    assert not no_leak([[1, -1], [2, -1], [3, 4], [2, 4], [2, 3]], ptr) and not no_leak([[1, -1], [0, -1], [3, 1], [2, 4], [2, 3]], ptr)


# ---- 4. column splits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_column_splits_give_identical_bits(mmf, precision):
    """[600, 129, 1100] = 5, 2 and 9 tiles: with 4 ranges the 129-row segment caps at 2, and the last range of the others is short."""
    sizes = [600, 129, 1100]
    F, P, ptr = sr.batch(sizes, 40, 2, 11)
    ref = ref_of(("splits",), F, P, ptr, 5)
    outs = [check(mmf, F, P, ptr, 5, precision, ref=ref, col_splits=c) for c in (1, 2, 4, 0)]
    assert [o[2]["col_splits"] for o in outs] == [1, 2, 4, 2]               # 0: 16 row blocks < 256, two ranges (DESIGN.md §4.18 "Decisions")
    blocks = [(n_s + 127) // 128 for n_s in sizes]
    for o, per_seg in zip(outs, ([1, 1, 1], [2, 2, 2], [4, 2, 4], [2, 2, 2])):
        assert o[2]["scan_grid"] == sum(b * r for b, r in zip(blocks, per_seg)), o[2]
    for idx, val, _ in outs[1:]:
        assert np.array_equal(idx, outs[0][0]) and np.array_equal(bits(val), bits(outs[0][1]))


# ---- 5. crowding and the per-segment slice rescan ------------------------------------------------------------------------
CROWD_SIZES, CROWD_SEED = [300, 1600, 129], 60
CROWD_ROWS = np.concatenate([np.arange(3, 43, 3), np.arange(130, 170, 3), np.arange(520, 559, 3)])[:40]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_crowded_rows_take_the_slice_rescan_of_their_segment(mmf, precision):
    """The 40 local rows of the one-graph crowded-rows test, planted identical inside segment 1 (three of its thirteen row blocks):
    each has 40 columns with the very same key, more than the 32 entries a row's two lists hold, so keys are dropped at the
    threshold and the audit flags the rows; their blocks are answered by slices of the exact pass against segment 1's columns.
    Segments 0 and 2 are untouched by it."""
    F, P, ptr = sr.batch(CROWD_SIZES, 40, 2, CROWD_SEED)
    F0, P0 = F.copy(), P.copy()
    rows = 300 + CROWD_ROWS
    assert len(rows) == 40 and len(set(CROWD_ROWS // 128)) == 3
    F[rows] = F[rows[0]]
    P[rows] = P[rows[0]]
    _, _, cnt = sr.bands_segmented(F, P, ptr, LH, LG, 6, OPERAND[precision])
    crowded = np.nonzero(cnt > 16)[0]
    assert (cnt[rows] >= 40).all() and crowded.size < 100 and np.all((crowded >= 300) & (crowded < 1900))
    Fd, Pd = T(F).cuda(), T(P).cuda()
    want = ct().simtopk_combined(Fd, Pd, LH, LG, 5, ptr=T(ptr))
    got = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision=precision, col_splits=1, return_stats=True)
    print(f"crowded rows {crowded.size}, fallback_rows {got[2]['fallback_rows']} (overflow {got[2]['overflow_rows']}, short {got[2]['short_rows']})")
    assert 1 <= got[2]["fallback_rows"] <= crowded.size          # only a row whose band exceeds its capacity may be flagged
    assert same_bits(got, want) and no_leak(got[0].cpu().numpy(), ptr)
    plain = seg().simtopk_combined_fast_segmented(T(F0).cuda(), T(P0).cuda(), LH, LG, 5, ptr=T(ptr), precision=precision, col_splits=1,
                                                  return_stats=True)
    assert plain[2]["fallback_rows"] == 0
    for a, b in ((0, 300), (1900, 2029)):
        assert same_bits((got[0][a:b], got[1][a:b]), (plain[0][a:b], plain[1][a:b]))
    check(mmf, F, P, ptr, 5, precision, ref=ref_of(("crowd",), F, P, ptr, 5), col_splits=1)


# ---- 6. MMF_DEBUG_FLAG_ROWS ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_batch():
    F, P, ptr = sr.batch([1200, 300, 129], 40, 2, 12)      # ten row blocks in segment 0: two flagged blocks are less than a quarter
    Fd, Pd = T(F).cuda(), T(P).cuda()
    return F, P, ptr, Fd, Pd, ct().simtopk_combined(Fd, Pd, LH, LG, 5, ptr=T(ptr))


@pytest.mark.parametrize("flag,blocks", [(130, "one whole block and one partial block of segment 0: one run"),
                                         (1200, "every row of segment 0: the whole segment is redone"),
                                         (1350, "segment 0 and half of segment 1's three blocks: both whole")])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_debug_flagged_rows(mmf, clean_batch, monkeypatch, precision, flag, blocks):
    F, P, ptr, Fd, Pd, want = clean_batch
    clean = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision=precision, return_stats=True)
    assert clean[2]["fallback_rows"] == 0 and same_bits(clean, want)
    monkeypatch.setenv("MMF_DEBUG_FLAG_ROWS", str(flag))
    got = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision=precision, return_stats=True)
    assert got[2]["fallback_rows"] == flag and got[2]["overflow_rows"] == flag, (blocks, got[2])
    assert same_bits(got, want), blocks


# ---- 7. worst-case rounding rows, the scale shared with a foreign segment ---------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_worst_case_rounding_rows(mmf, precision):
    """Two copies of tests/adversarial16.py's family (every component rounds the same way) with pixel positions as two segments,
    and a Gaussian segment whose rows take part in the scale and the maxima: the exact entry's bits."""
    import adversarial16 as adv
    fam = adv.self_family(OPERAND[precision], 128, 5)
    A = np.ascontiguousarray(fam.X)
    na = A.shape[0]
    rng = np.random.RandomState(7)
    side = 4 * int(np.ceil(np.sqrt(na)))
    cells = rng.choice(side * side, na, replace=False)
    PA = np.stack([(cells // side) * 224, (cells % side) * 224], axis=1).astype(np.float32)
    G, PG = cr.make_data(200, 128, 2, 70)
    G = (G * np.float32(3.0)).astype(np.float32)                 # the largest norm of the batch is the foreign segment's
    F = np.ascontiguousarray(np.concatenate([A, G, A]))
    P = np.ascontiguousarray(np.concatenate([PA, PG, PA]))
    ptr = offsets_of([na, 200, na])
    Fd, Pd = T(F).cuda(), T(P).cuda()
    want = ct().simtopk_combined(Fd, Pd, 1e-3, LG, 5, ptr=T(ptr))
    got = seg().simtopk_combined_fast_segmented(Fd, Pd, 1e-3, LG, 5, ptr=T(ptr), precision=precision, return_stats=True)
    print(f"fallback_rows {got[2]['fallback_rows']} of {F.shape[0]}")
    assert same_bits(got, want) and no_leak(got[0].cpu().numpy(), ptr)
    a, b = got[0][:na].cpu(), got[0][na + 200:].cpu() - (na + 200)
    assert torch.equal(a, b)                                    # the two copies answer alike, each in its own ids


# ---- 8. exact and auto ----------------------------------------------------------------------------------------------------
def auto_takes_the_scan(d, kk):
    """DESIGN.md §4.18 "Decisions": MMF_PREC_AUTO takes the 16-bit scan for 512 <= d <= 1536 with k + self <= 11 — the range in which
    the whole call beat combined_topk.simtopk_combined(ptr=...) by more than three of its spreads at every measured batch."""
    return 512 <= d <= 1536 and kk <= 11


def test_exact_and_auto(mmf, clean_batch):
    """precision="exact" is the exact pass for every segment; "auto" follows DESIGN.md §4.18's measured decision.  The same bits
    either way; precision_used says which ran."""
    F, P, ptr, Fd, Pd, want = clean_batch
    e = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision="exact", return_stats=True)
    a = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), return_stats=True)
    assert same_bits(e, want) and same_bits(a, want)
    assert e[2]["precision_used"] == 1 and e[2]["fallback_rows"] == 0
    assert a[2]["precision_used"] == (2 if auto_takes_the_scan(40, 6) else 1)
    F5, P5, p5 = sr.batch([300, 129, 64], 512, 2, CAP_SEED)
    F5d, P5d = T(F5).cuda(), T(P5).cuda()
    want5 = ct().simtopk_combined(F5d, P5d, LH, LG, 5, ptr=T(p5))
    a5 = seg().simtopk_combined_fast_segmented(F5d, P5d, LH, LG, 5, ptr=T(p5), return_stats=True)
    assert same_bits(a5, want5) and a5[2]["precision_used"] == (2 if auto_takes_the_scan(512, 6) else 1) and a5[2]["fallback_rows"] == 0
    a12 = seg().simtopk_combined_fast_segmented(F5d, P5d, LH, LG, 11, ptr=T(p5), return_stats=True)            # k + self = 12
    assert a12[2]["precision_used"] == (2 if auto_takes_the_scan(512, 12) else 1)
    assert same_bits(a12, ct().simtopk_combined(F5d, P5d, LH, LG, 11, ptr=T(p5)))


# ---- 9. repetition, CPU tensors, edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_calls_and_cpu_tensors(mmf, clean_batch, precision):
    F, P, ptr, Fd, Pd, want = clean_batch
    a = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision=precision)
    b = seg().simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision=precision)
    torch.cuda.synchronize()
    assert same_bits(a, b) and same_bits(a, want)
    hi, hv = seg().simtopk_combined_fast_segmented(T(F), T(P), LH, LG, 5, ptr=T(ptr), precision=precision)
    assert not hi.is_cuda and not hv.is_cuda and torch.equal(hi, a[0].cpu()) and torch.equal(hv.view(torch.int32), a[1].cpu().view(torch.int32))


def test_edge_builders(mmf):
    F, P, ptr = sr.batch([130, 3, 0, 1, 129], 40, 2, 14)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    ei, ew, eptr = seg().build_topk_weighted_hypergraph_fast_segmented(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision="fast")
    wi, ww, wptr = ct().build_topk_weighted_hypergraph(Fd, Pd, LH, LG, 5, ptr=T(ptr))
    assert ei.is_cuda and torch.equal(ei, wi) and torch.equal(ew.view(torch.int32), ww.view(torch.int32)) and torch.equal(eptr, wptr)
    assert eptr.tolist() == [0, 650, 656, 656, 656, 1301]
    ci, cw, cp = seg().build_topk_weighted_hypergraph_fast_segmented(T(F), T(P), LH, LG, 5, batch=torch.repeat_interleave(
        torch.arange(5), T(ptr[1:] - ptr[:-1])), precision="fast_bf16")
    assert not ci.is_cuda and torch.equal(ci, wi.cpu()) and torch.equal(cw, ww.cpu()) and cp.tolist() == eptr.tolist()
    got = seg().build_topk_hypergraph_data_fast(Fd, Pd, LH, LG, 5, ptr=T(ptr), precision="fast")
    want = ct().build_topk_hypergraph_data(Fd, Pd, LH, LG, 5, ptr=T(ptr))
    assert sorted(got) == sorted(want)
    for key in want:
        g, w = got[key], want[key]
        assert g.device == w.device and g.dtype == w.dtype and g.shape == w.shape, key
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w), key


# ---- 10. the entry behind a closed gate on a busy non-default stream --------------------------------------------------------
GATE_SIZES = [140, 3, 0, 157]


def gated_inputs(which):
    F, P, _ = sr.batch(GATE_SIZES, 40, 2, 20 if which == "truth" else 21)
    return [T(F), T(P)]


def gated_reference(F, P):
    ridx, rval = reference(F, P, offsets_of(GATE_SIZES), 5)
    return lambda got: sg.diff(got[0], ridx, "idx") + sg.diff(got[1], rval, "val", atol=TOL)


def _c_entry(F, P):
    import multimodal_fusion_amd as m
    o = m.ops
    n, k = F.shape[0], 5
    idx = torch.empty((n, k), dtype=torch.int64, device=F.device)
    val = torch.empty((n, k), dtype=torch.float32, device=F.device)
    ptr = T(offsets_of(GATE_SIZES))
    opts = m._lib.SimtopkOpts(m._lib.PRECISIONS["fast"], 0, 2, m._lib.QUERY_ORDERS["off"], None)
    rc = getattr(m._lib.lib(), ENTRY)(o._p(F), o._p(P), n, F.shape[1], P.shape[1], LH, LG, k, 1, o._hp(ptr), len(GATE_SIZES), o._p(idx),
                                      o._p(val), ctypes.byref(opts), None, F.device.index or 0, o._stream(F.device))
    m._lib.check(rc, ENTRY)
    return [idx, val]


def _wrapper(F, P):
    return list(seg().simtopk_combined_fast_segmented(F, P, LH, LG, 5, ptr=offsets_of(GATE_SIZES), precision="fast_bf16"))


def _wrapper_flagged(F, P):
    os.environ["MMF_DEBUG_FLAG_ROWS"] = "200"          # flagged rows in both scanned segments: the exact pass, behind the gate too
    try:
        return list(seg().simtopk_combined_fast_segmented(F, P, LH, LG, 5, ptr=offsets_of(GATE_SIZES), precision="fast"))
    finally:
        del os.environ["MMF_DEBUG_FLAG_ROWS"]


@pytest.mark.parametrize("name,entry", [("c_entry_simtopk_combined_fast_segmented", _c_entry), ("simtopk_combined_fast_segmented", _wrapper),
                                        ("simtopk_combined_fast_segmented_flagged", _wrapper_flagged)])
def test_entry_behind_a_closed_gate(mmf, name, entry):
    assert list(SYNC) == list(mmf._lib.EXPORTS_TOPK16_SEG)
    sg.run_gated(entry, gated_inputs, gated_reference, name=name, calls=2)


# ---- 11. refusals reach Python ---------------------------------------------------------------------------------------------
def test_refusals(mmf):
    F, P, ptr = sr.batch([130, 40, 130], 40, 2, 10)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    f = seg().simtopk_combined_fast_segmented
    with pytest.raises(RuntimeError, match=r"simtopk_combined_fast_segmented: k \+ self = 21 > 20"):
        f(Fd, Pd, LH, LG, 20, ptr=ptr, precision="fast")
    f(Fd, Pd, LH, LG, 20, ptr=ptr, exclude_self=False, precision="fast")             # k + self = 20: the limit itself is served
    with pytest.raises(RuntimeError, match=r"simtopk_combined_fast_segmented: dp = 9 > 8"):
        f(Fd, torch.zeros(300, 9, device="cuda"), LH, LG, 5, ptr=ptr, precision="fast")
    with pytest.raises(RuntimeError, match=r"simtopk_combined_fast_segmented: d = 4097 > 4096"):
        f(torch.zeros(4, 4097, device="cuda"), torch.zeros(4, 2, device="cuda"), LH, LG, 2, ptr=[0, 2, 4], precision="fast")
    with pytest.raises(ValueError, match="simtopk_combined_fast_segmented: lambda_g must be finite"):
        f(Fd, Pd, LH, float("nan"), 5, ptr=ptr)
    with pytest.raises(ValueError, match="simtopk_combined_fast_segmented: lambda_h must be finite"):
        f(Fd, Pd, -1.0, LG, 5, ptr=ptr)
    with pytest.raises(ValueError, match="simtopk_combined_fast_segmented: col_splits must be 0 or a power of two"):
        f(Fd, Pd, LH, LG, 5, ptr=ptr, col_splits=3)
    o = mmf.ops
    idx = torch.empty((300, 5), dtype=torch.int64, device="cuda")
    val = torch.empty((300, 5), dtype=torch.float32, device="cuda")
    fn = getattr(mmf._lib.lib(), ENTRY)
    bad = torch.tensor([0, 100, 299], dtype=torch.int64)
    opts = mmf._lib.SimtopkOpts(2, 0, 3, 0, None)
    for args, words in (((None, 0, None), "host offsets ptr_host"), ((o._hp(bad), 2, None), "ptr_host must end at 300"),
                        ((o._hp(T(ptr)), 3, ctypes.byref(opts)), "col_splits must be 0 or a power of two (got 3)")):
        rc = fn(o._p(Fd), o._p(Pd), 300, 40, 2, LH, LG, 5, 1, args[0], args[1], o._p(idx), o._p(val), args[2], None, 0, o._stream(Fd.device))
        msg = mmf._lib.lib().mmf_last_error().decode()
        assert rc == mmf._lib.MMF_E_INVALID and words in msg and "simtopk_combined_fast_segmented" in msg, (rc, msg)
    idx, val = f(Fd[:0], Pd[:0], LH, LG, 5, ptr=[0], precision="fast")
    assert idx.shape == (0, 5) and val.shape == (0, 5)
