"""The 16-bit top-k of the combined similarity K_h * K_g on the MI355X (mmf_simtopk_combined_fast).

Every case checks what tests/test_gpu_simtopk_combined.py checks for the exact entry (its check(), restated for this entry): the
indices are those of a numpy reference (canonical keys from oracle.sim_dense, one float32 add, np.lexsort by (-key, id)); the
values are BITWISE the entries ops.sim_dense_combined writes; and the values are within 1e-5 of the oracle's.  precision="fast"
(f16 operands) and "fast_bf16" both run unless a case says otherwise.

Data: 12 Gaussian centres + 0.05 noise, rows L2-normalised; positions are cells of a 24-cell grid x 224 up to 300 rows and
distinct cells of a grid of side 4 ceil(sqrt(n)) x 224 from 2048 rows on; lambda_h = 0.5, lambda_g = 2e-7
(tests/combined16_restate.py: make_data).  On this data no row's margin band exceeds its list capacity (the capacity condition
below asserts it from the numpy restatement of the kernel's margin), so the exact rescan must stay idle and cannot hide a scan
that loses candidates.

The margin, restated (mmf_scan_b16c.hip's header; tests/combined16_restate.py): A_ij = fl(fl(fmaf(a, G_ij, rc_i)) + eg_ij) with
a = 2 lambda_h / s^2, G_ij = cb_j + z_i . z_j and eg the canonical position exponent;
margin_i(t) = m0_i + 6.1 * 2^-24 |t|, m0_i = 2.002 (a (E1_i + E2_i) + 1.01 * 2^-24 (lambda_h n_i + 2 pb_i)) + 1e-30; band_i = the
columns with A_ij >= T_i - margin_i(T_i), T_i the (k + self)-th best A of the row; capacity 16 for k + self <= 11, 32 for 12..20."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combined16_restate as cr   # noqa: E402
import streamgate as sg           # noqa: E402
from test_gpu_simtopk_combined import bits, offsets_of, reference   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
LH, LG = 0.5, 2e-7
PRECISIONS = ["fast", "fast_bf16"]
OPERAND = {"fast": "f16", "fast_bf16": "bf16"}
PREC_CODE = {"exact": 1, "fast": 2, "fast_bf16": 3}

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "16-bit top-k entries"
# (tests/test_simtopk_combined_fast_cpu.py keeps the two equal)
SYNC_TOPK16 = {"mmf_simtopk_combined_fast": ("data-dependent", "no host arguments")}

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def ct16():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16")


def ct():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk")


_REF = {}


def data(n, d, dp=2, seed=0, plant=None):
    """make_data of the restatement, optionally with the planting of the exact entry's test: rows first .. first + 9 copy src's
    features, the first five of them its position too."""
    F, P = cr.make_data(n, d, dp, seed)
    if plant is not None:
        src, first = plant
        F[first:first + 10] = F[src]
        P[first:first + 5] = P[src]
    return F, P


def ref_of(key, F, P, k, lh=LH, lg=LG, exclude_self=True):
    """The numpy reference, computed once per case and shared by the precisions."""
    if key not in _REF:
        _REF[key] = reference(F, P, offsets_of([F.shape[0]]), k, lh, lg, exclude_self)
    return _REF[key]


def check(mmf, F, P, k, precision, lh=LH, lg=LG, exclude_self=True, ref=None, **kw):
    """One call against the reference; returns (idx, val, stats) on the host."""
    n = F.shape[0]
    Fd, Pd = T(F).cuda(), T(P).cuda()
    idx, val, st = ct16().simtopk_combined_fast(Fd, Pd, lh, lg, k, exclude_self=exclude_self, precision=precision, return_stats=True, **kw)
    torch.cuda.synchronize()
    assert idx.shape == (n, k) and idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    ridx, rval = ref if ref is not None else reference(F, P, offsets_of([n]), k, lh, lg, exclude_self)
    bad = np.nonzero((idx != ridx).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ from the reference, first {bad[0]}: got {idx[bad[0]]}, want {ridx[bad[0]]}"
    there = ridx >= 0
    assert np.all(np.isneginf(val[~there]))
    if there.any():
        K = mmf.ops.sim_dense_combined(Fd, Pd, lh, lg).cpu().numpy()
        rows = np.broadcast_to(np.arange(n)[:, None], (n, k))[there]
        assert np.array_equal(bits(val[there]), bits(K[rows, ridx[there]])), "values differ from sim_dense_combined's bits"
    err = float(np.abs(val[there].astype(np.float64) - rval[there].astype(np.float64)).max()) if there.any() else 0.0
    print(f"max |val - oracle| = {err:.3e}, fallback_rows {st['fallback_rows']}, candidates per row {st['candidates'] / max(n, 1):.1f}")
    assert err <= TOL
    return idx, val, st


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- 1. the capacity condition -----------------------------------------------------------------------------------------
CAPACITY_SHAPES = [(300, 40, 2), (257, 64, 3), (129, 130, 8), (300, 512, 2), (300, 1536, 2), (2048, 64, 2)]


def shape_seed(n, d):
    return n % 7 + d % 5


@pytest.mark.parametrize("n,d,dp", CAPACITY_SHAPES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_capacity_condition(mmf, n, d, dp, precision):
    """No row's restated band exceeds its list capacity, so no row may reach the exact pass — for every list capacity (k + self
    = 6, 11, 12, 20) and col_splits 1, 2, 4.  The reference is checked at col_splits 1; the other split counts must give its bits."""
    F, P = data(n, d, dp, shape_seed(n, d))
    Fd, Pd = T(F).cuda(), T(P).cuda()
    for kk in (6, 11, 12, 20):
        k = kk - 1
        _, _, cnt = cr.bands(F, P, LH, LG, kk, OPERAND[precision])
        cap = cr.capacity(kk)
        crowded = int((cnt > cap).sum())
        print(f"n {n} d {d} dp {dp} {precision} k + self {kk}: largest band {int(cnt.max())} of {cap}, crowded rows {crowded}")
        assert crowded == 0
        ref = ref_of(("cap", n, d, dp, k), F, P, k)
        idx, val, st = check(mmf, F, P, k, precision, ref=ref, col_splits=1)
        assert st["fallback_rows"] == 0 and st["precision_used"] == PREC_CODE[precision] and st["col_splits"] == 1
        for cs in (2, 4):
            gi, gv, st = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, k, precision=precision, col_splits=cs, return_stats=True)
            assert st["fallback_rows"] == 0, (kk, cs, st)
            assert np.array_equal(gi.cpu().numpy(), idx) and np.array_equal(bits(gv.cpu().numpy()), bits(val)), (kk, cs)


@pytest.fixture(scope="module")
def many_tiles():
    F, P = data(8192, 64, 2, shape_seed(8192, 64))
    Fd, Pd = T(F).cuda(), T(P).cuda()
    want = ct().simtopk_combined(Fd, Pd, LH, LG, 5)
    return F, P, Fd, Pd, want


@pytest.mark.parametrize("precision", PRECISIONS)
def test_many_tiles(mmf, many_tiles, precision):
    """N = 8192, d = 64, k = 5: 64 candidate tiles.  No crowded row in the restatement, none sent to the exact pass, and the bits
    of the exact entry (pinned against the oracle by its own test) — at the automatic split count and at 1, 2 and 4."""
    F, P, Fd, Pd, want = many_tiles
    _, _, cnt = cr.bands(F, P, LH, LG, 6, OPERAND[precision])
    crowded = int((cnt > 16).sum())
    print(f"n 8192 d 64 {precision} k + self 6: largest band {int(cnt.max())} of 16, crowded rows {crowded}")
    assert crowded == 0
    for cs in (0, 1, 2, 4):
        gi, gv, st = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision, col_splits=cs, return_stats=True)
        assert same_bits((gi, gv), want), cs
        assert st["fallback_rows"] == 0 and st["scan_grid"] == 64 * st["col_splits"], st


# ---- 2. the smallest shapes where it can go wrong ----------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_row(mmf, precision):
    F, P = data(1, 40, 2, 1)
    idx, val, _ = check(mmf, F, P, 5, precision)
    assert np.all(idx == -1) and np.all(np.isneginf(val))
    idx, val, _ = check(mmf, F, P, 5, precision, exclude_self=False)
    assert list(idx[0]) == [0, -1, -1, -1, -1] and np.all(np.isneginf(val[0, 1:])) and val[0, 0] == 1.0


@pytest.mark.parametrize("n,k", [(2, 1), (2, 5), (129, 5), (257, 5), (5, 19)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_small_graphs_and_k_beyond_n(mmf, n, k, precision):
    """Two rows; one query past a row block; one column past two tiles; k >= n (the row's columns first, then -1 / -inf)."""
    F, P = data(n, 40, 2, 2)
    idx, _, _ = check(mmf, F, P, k, precision, ref=ref_of(("small", n, k), F, P, k))
    if k >= n:
        assert np.all(idx[:, n - 1:] == -1) and np.all(idx[:, :n - 1] >= 0)


@pytest.mark.parametrize("d", [40, 130, 512, 1536])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_feature_dims(mmf, d, precision):
    """d below one staged chunk, one past two chunks' padding (130 -> 256), the exact entry's benchmark dim, and above 1024."""
    F, P = data(300, d, 2, 3, plant=(299, 100))
    check(mmf, F, P, 5, precision, ref=ref_of(("d", d), F, P, 5))


@pytest.mark.parametrize("dp", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_position_dims(mmf, dp, precision):
    """Every chain length of the epilogue: 2 (dp 1, 2), 4 (dp 3, 4), 8."""
    F, P = data(300, 40, dp, 4, plant=(299, 100))
    check(mmf, F, P, 5, precision, ref=ref_of(("dp", dp), F, P, 5))


@pytest.mark.parametrize("k", [1, 5, 10, 11, 19])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_list_capacities(mmf, k, precision):
    """k + self = 2, 6, 11 (16-entry lists, the last one their limit), 12 and 20 (32-entry lists and the entry's limit)."""
    F, P = data(300, 40, 2, 5, plant=(299, 100))
    _, _, st = check(mmf, F, P, k, precision, ref=ref_of(("k", k), F, P, k))
    assert st["precision_used"] == PREC_CODE[precision] and st["scan_grid"] >= 3 and st["col_splits"] >= 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_include_self_at_the_limit(mmf, precision):
    F, P = data(300, 40, 2, 7, plant=(299, 100))
    idx, _, _ = check(mmf, F, P, 20, precision, exclude_self=False, ref=ref_of(("self", 20), F, P, 20, exclude_self=False))
    for i in range(300):
        j = idx[i, 0]
        assert j == i or (j < i and np.array_equal(F[j], F[i]) and np.array_equal(P[j], P[i])), (i, j)


# ---- 3. forced column splits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_column_splits_give_identical_bits(mmf, precision):
    """600 rows = 5 row blocks and column tiles: 1, 2 and 4 ranges (the last of 4 is short), and the automatic count."""
    F, P = data(600, 40, 2, 6, plant=(599, 100))
    ref = ref_of(("splits",), F, P, 5)
    outs = [check(mmf, F, P, 5, precision, ref=ref, col_splits=c) for c in (1, 2, 4, 0)]
    assert [o[2]["col_splits"] for o in outs[:3]] == [1, 2, 4]
    for idx, val, _ in outs[1:]:
        assert np.array_equal(idx, outs[0][0]) and np.array_equal(bits(val), bits(outs[0][1]))


# ---- 4. zero lambdas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", ["features only", "positions only"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_zero_lambda_drops_its_term(mmf, term, precision):
    """Against entries that are already pinned: the exact RBF top-k of the one operand that is left.  lambda_h = 0 makes a = 0,
    which meets the -inf bias of the 84 padding columns of the third tile (n = 300)."""
    F, P = data(300, 40, 2, 8, plant=(299, 100))
    Fd, Pd = T(F).cuda(), T(P).cuda()
    if term == "features only":
        got = ct16().simtopk_combined_fast(Fd, Pd, LH, 0.0, 5, precision=precision)
        want = mmf.ops.simtopk(Fd, metric="rbf", lam=LH, k=5, precision="exact")
    else:
        got = ct16().simtopk_combined_fast(Fd, Pd, 0.0, LG, 5, precision=precision)
        want = mmf.ops.simtopk(Pd, metric="rbf", lam=LG, k=5, precision="exact")
    torch.cuda.synchronize()
    assert same_bits(got, want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_all_zero_feature_row(mmf, precision):
    F, P = data(300, 40, 2, 9)
    F[7] = 0.0
    F[150] = 0.0
    check(mmf, F, P, 5, precision, ref=ref_of(("zero",), F, P, 5))
    Z = np.zeros_like(F)
    check(mmf, Z, P, 5, precision, ref=ref_of(("allzero",), Z, P, 5))


# ---- 5. planted rows: the position alone, and for exact copies the id alone, decides -----------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_planted_rows(mmf, precision):
    F, P = data(300, 40, 2, 10, plant=(299, 100))
    idx, _, _ = check(mmf, F, P, 5, precision, ref=ref_of(("plant",), F, P, 5))
    assert list(idx[299, :5]) == [100, 101, 102, 103, 104] and list(idx[102, :4]) == [100, 101, 103, 104]


# ---- 6. crowding and the slice rescan ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_rows():
    F, P = data(1200, 40, 2, 12)                       # ten row blocks: two flagged blocks are less than a quarter
    Fd, Pd = T(F).cuda(), T(P).cuda()
    return F, P, Fd, Pd, ct().simtopk_combined(Fd, Pd, LH, LG, 5)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_crowded_rows_take_the_slice_rescan(mmf, precision):
    """40 rows with one feature row and one position, scattered over three of thirteen row blocks: each of them has 40 columns
    with the very same key, more than the 32 entries the two lists of one column range hold together, so keys are dropped at the
    threshold and the audit flags the rows; their three blocks are answered by slices of the exact pass."""
    F, P = data(1600, 40, 2, 13)
    rows = np.concatenate([np.arange(3, 43, 3), np.arange(130, 170, 3), np.arange(520, 559, 3)])[:40]
    assert len(rows) == 40 and len(set(rows // 128)) == 3
    F[rows] = F[rows[0]]
    P[rows] = P[rows[0]]
    _, _, cnt = cr.bands(F, P, LH, LG, 6, OPERAND[precision])
    crowded = int((cnt > 16).sum())
    assert (cnt[rows] >= 40).all() and crowded < 100
    Fd, Pd = T(F).cuda(), T(P).cuda()
    want = ct().simtopk_combined(Fd, Pd, LH, LG, 5)
    # one column range: a row's two lists see all 40 columns (with several ranges every range has lists of its own, and no
    # list of these rows fills up)
    got = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision, col_splits=1, return_stats=True)
    print(f"crowded rows {crowded}, fallback_rows {got[2]['fallback_rows']} (overflow {got[2]['overflow_rows']}, short {got[2]['short_rows']})")
    assert 1 <= got[2]["fallback_rows"] <= crowded          # only a row whose band exceeds its capacity may be flagged
    assert same_bits(got, want)
    auto = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision, return_stats=True)
    assert auto[2]["fallback_rows"] <= crowded and same_bits(auto, want)
    check(mmf, F, P, 5, precision, ref=ref_of(("crowd",), F, P, 5))


@pytest.mark.parametrize("flag,blocks", [(130, "one whole block and one partial block"), (1200, "every row: the whole exact pass")])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_debug_flagged_rows(mmf, clean_rows, monkeypatch, precision, flag, blocks):
    F, P, Fd, Pd, want = clean_rows
    clean = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision, return_stats=True)
    assert clean[2]["fallback_rows"] == 0 and same_bits(clean, want)
    monkeypatch.setenv("MMF_DEBUG_FLAG_ROWS", str(flag))
    got = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision, return_stats=True)
    assert got[2]["fallback_rows"] == flag and got[2]["overflow_rows"] == flag, (blocks, got[2])
    assert same_bits(got, want), blocks


# ---- 8. worst-case rounding data ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_worst_case_rounding_rows(mmf, precision):
    """The rows of tests/adversarial16.py (every component rounds the same way) with pixel positions added: the exact entry's bits."""
    import adversarial16 as adv
    fam = adv.self_family(OPERAND[precision], 128, 5)
    F = np.ascontiguousarray(fam.X)
    n = F.shape[0]
    rng = np.random.RandomState(7)
    side = 4 * int(np.ceil(np.sqrt(n)))
    cells = rng.choice(side * side, n, replace=False)
    P = np.stack([(cells // side) * 224, (cells % side) * 224], axis=1).astype(np.float32)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    want = ct().simtopk_combined(Fd, Pd, 1e-3, LG, 5)
    got = ct16().simtopk_combined_fast(Fd, Pd, 1e-3, LG, 5, precision=precision, return_stats=True)
    print(f"fallback_rows {got[2]['fallback_rows']} of {n}")
    assert same_bits(got, want)


# ---- 9. exact and auto ------------------------------------------------------------------------------------------------
def test_exact_and_auto(mmf, clean_rows):
    """precision="exact" is the exact entry; "auto" takes the 16-bit scan only in the measured range (DESIGN.md §4.17:
    512 <= d <= 1536, k + self <= 11) and the exact scan elsewhere.  The same bits either way; precision_used says which ran."""
    F, P, Fd, Pd, want = clean_rows
    e = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision="exact", return_stats=True)
    a = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, return_stats=True)
    assert same_bits(e, want) and same_bits(a, want)
    assert e[2]["precision_used"] == 1 and a[2]["precision_used"] == 1 and e[2]["fallback_rows"] == 0        # d = 40: exact
    F5, P5 = data(300, 512, 2, shape_seed(300, 512))
    F5d, P5d = T(F5).cuda(), T(P5).cuda()
    want5 = ct().simtopk_combined(F5d, P5d, LH, LG, 5)
    a5 = ct16().simtopk_combined_fast(F5d, P5d, LH, LG, 5, return_stats=True)
    assert same_bits(a5, want5) and a5[2]["precision_used"] == 2 and a5[2]["fallback_rows"] == 0
    a12 = ct16().simtopk_combined_fast(F5d, P5d, LH, LG, 11, return_stats=True)                              # k + self = 12
    assert a12[2]["precision_used"] == 1 and same_bits(a12, ct().simtopk_combined(F5d, P5d, LH, LG, 11))


# ---- 10. repetition, CPU tensors, edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_calls_and_cpu_tensors(mmf, clean_rows, precision):
    F, P, Fd, Pd, want = clean_rows
    a = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision)
    b = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=precision)
    torch.cuda.synchronize()
    assert same_bits(a, b) and same_bits(a, want)
    hi, hv = ct16().simtopk_combined_fast(T(F), T(P), LH, LG, 5, precision=precision)
    assert not hi.is_cuda and not hv.is_cuda and torch.equal(hi, a[0].cpu()) and torch.equal(hv.view(torch.int32), a[1].cpu().view(torch.int32))


def test_edge_builder(mmf, clean_rows):
    F, P, Fd, Pd, want = clean_rows
    ei, ew, eptr = ct16().build_topk_weighted_hypergraph_fast(Fd, Pd, LH, LG, 5, precision="fast")
    wi, ww, wptr = ct().build_topk_weighted_hypergraph(Fd, Pd, LH, LG, 5)
    assert ei.is_cuda and torch.equal(ei, wi) and torch.equal(ew.view(torch.int32), ww.view(torch.int32)) and torch.equal(eptr, wptr)
    assert eptr.tolist() == [0, 6000]
    ci, cw, cp = ct16().build_topk_weighted_hypergraph_fast(T(F), T(P), LH, LG, 5, precision="fast_bf16")
    assert not ci.is_cuda and torch.equal(ci, wi.cpu()) and torch.equal(cw, ww.cpu()) and cp.tolist() == [0, 6000]


# ---- 11. the entry behind a closed gate on a busy non-default stream -----------------------------------------------------
def gated_inputs(which):
    F, P = data(300, 40, 2, 20 if which == "truth" else 21, plant=(299, 100))
    return [T(F), T(P)]


def gated_reference(F, P):
    ridx, rval = reference(F, P, offsets_of([F.shape[0]]), 5)
    return lambda got: sg.diff(got[0], ridx, "idx") + sg.diff(got[1], rval, "val", atol=TOL)


def _c_entry(F, P):
    import multimodal_fusion_amd as m
    o = m.ops
    n, k = F.shape[0], 5
    idx = torch.empty((n, k), dtype=torch.int64, device=F.device)
    val = torch.empty((n, k), dtype=torch.float32, device=F.device)
    opts = m._lib.SimtopkOpts(m._lib.PRECISIONS["fast"], 0, 0, m._lib.QUERY_ORDERS["off"], None)
    import ctypes
    rc = m._lib.lib().mmf_simtopk_combined_fast(o._p(F), o._p(P), n, F.shape[1], P.shape[1], LH, LG, k, 1, None, 0, o._p(idx), o._p(val),
                                                ctypes.byref(opts), None, F.device.index or 0, o._stream(F.device))
    m._lib.check(rc, "mmf_simtopk_combined_fast")
    return [idx, val]


def _wrapper(F, P):
    return list(ct16().simtopk_combined_fast(F, P, LH, LG, 5, precision="fast_bf16"))


def _wrapper_flagged(F, P):
    os.environ["MMF_DEBUG_FLAG_ROWS"] = "130"          # the second synchronisation and the exact pass, behind the gate too
    try:
        return list(ct16().simtopk_combined_fast(F, P, LH, LG, 5, precision="fast"))
    finally:
        del os.environ["MMF_DEBUG_FLAG_ROWS"]


@pytest.mark.parametrize("name,entry", [("c_entry_simtopk_combined_fast", _c_entry), ("simtopk_combined_fast", _wrapper),
                                        ("simtopk_combined_fast_flagged", _wrapper_flagged)])
def test_entry_behind_a_closed_gate(mmf, name, entry):
    assert list(SYNC_TOPK16) == list(mmf._lib.EXPORTS_TOPK16)
    sg.run_gated(entry, gated_inputs, gated_reference, name=name, calls=2)


# ---- 12. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(mmf):
    F, P = data(300, 40, 2, 10)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    f = ct16().simtopk_combined_fast
    with pytest.raises(RuntimeError, match=r"simtopk_combined_fast: k \+ self = 21 > 20"):
        f(Fd, Pd, LH, LG, 20, precision="fast")
    f(Fd, Pd, LH, LG, 20, exclude_self=False, precision="fast")             # k + self = 20: the limit itself is served
    with pytest.raises(RuntimeError, match="dp = 9 > 8"):
        f(Fd, torch.zeros(300, 9, device="cuda"), LH, LG, 5, precision="fast")
    with pytest.raises(RuntimeError, match="d = 4097 > 4096"):
        f(torch.zeros(4, 4097, device="cuda"), torch.zeros(4, 2, device="cuda"), LH, LG, 2, precision="fast")
    with pytest.raises(ValueError, match="k must be >= 1"):
        f(Fd, Pd, LH, LG, 0)
    with pytest.raises(ValueError, match="lambda_g must be finite"):
        f(Fd, Pd, LH, float("nan"), 5)
    with pytest.raises(ValueError, match="lambda_h must be finite"):
        f(Fd, Pd, -1.0, LG, 5)
    with pytest.raises(ValueError, match="col_splits must be >= 0"):
        f(Fd, Pd, LH, LG, 5, col_splits=-1)
    with pytest.raises(ValueError, match="unknown precision"):
        f(Fd, Pd, LH, LG, 5, precision="f16")
    import ctypes
    o = mmf.ops
    idx = torch.empty((300, 5), dtype=torch.int64, device="cuda")
    val = torch.empty((300, 5), dtype=torch.float32, device="cuda")
    ptr = torch.tensor([0, 100, 300], dtype=torch.int64)
    rc = mmf._lib.lib().mmf_simtopk_combined_fast(o._p(Fd), o._p(Pd), 300, 40, 2, LH, LG, 5, 1, o._hp(ptr), 2, o._p(idx), o._p(val), None, None,
                                                  0, o._stream(Fd.device))
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and "stays on mmf_simtopk_combined" in mmf._lib.lib().mmf_last_error().decode()
    idx, val = f(Fd[:0], Pd[:0], LH, LG, 5, precision="fast")
    assert idx.shape == (0, 5) and val.shape == (0, 5)
    del ctypes
