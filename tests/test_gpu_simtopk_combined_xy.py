"""The top-k of the combined similarity K_h * K_g for two node sets on the MI355X (mmf_simtopk_combined_xy).

Every case checks what tests/test_gpu_simtopk_combined.py checks for the self entry, composed the same way from the oracle
(tests/combined_xy_restate.py: reference): the indices are those of key = lh * oracle.sim_dense(Fq, Fc, "neg_sq_l2") + lg * (the
same of the positions) in f32 under np.lexsort by (-key, id); the values are BITWISE the entries ops.sim_dense_combined writes
for the stacked set; and the values are within 1e-5 (TOL of tests/test_gpu_pipeline.py) of oracle.sim_dense_combined's.

The cases (tests/combined_xy_restate.py: CASES) are row ranges of combined16_restate.make_data(total, d, dp, total % 7 + d % 5),
lambda_h = 0.5, lambda_g = 2e-7, ids = row numbers of the data set:
  R1 390 x 40, dp 2: rows 0..129 against rows 130..389;  R2 400 x 64, dp 3: rows 100..299 against rows 50..349 (row_offset 100,
  col_offset 50: the identity hits mid-range), self excluded and not;  R3 258 x 130, dp 8: 129 against 129 (one row past a tile on
  both sides, d no multiple of 64);  R4 600 x 512: 300 against 300;  R5 700 x 96: the slice rows 175..349 against all 700;
  R6 300 x 1536: 150 against 150.
The capacity condition: the numpy restatement of the kernel's margin (bands_xy: image, scale, maxima and the largest position
chain over both sides, a query's band among the candidate columns) finds no crowded query on any of them — asserted here before
fallback_rows == 0 is — so a 16-bit path that flags everything cannot pass through the exact pass."""
import ctypes
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combined16_restate as cr   # noqa: E402
import combined_xy_restate as xr  # noqa: E402
import streamgate as sg           # noqa: E402
from test_gpu_simtopk_combined import bits   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
LH, LG = xr.LH, xr.LG
PRECISIONS = ["exact", "fast", "fast_bf16"]
OPERAND = {"fast": "f16", "fast_bf16": "bf16"}
PREC_CODE = {"exact": 1, "fast": 2, "fast_bf16": 3}

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "Two-set top-k entries"
# (tests/test_simtopk_combined_xy_cpu.py keeps the two equal)
SYNC = {"mmf_simtopk_combined_xy": ("data-dependent", "no host arguments")}

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def xy():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk_xy")


def ct():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk")


def ct16():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16")


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


_SHARED = {}


def shared(mmf, F, P, lh=LH, lg=LG, key=None):
    """Per data set, computed once and left unchanged: the device copies, the oracle's dense K and the library's."""
    key = key or (F.shape, P.shape, hash(F.tobytes()), hash(P.tobytes()), lh, lg)
    if key not in _SHARED:
        import oracle
        Fd, Pd = T(F).cuda(), T(P).cuda()
        _SHARED[key] = (Fd, Pd, oracle.sim_dense_combined(F, P, lh, lg), mmf.ops.sim_dense_combined(Fd, Pd, lh, lg).cpu().numpy())
    return _SHARED[key]


_REF = {}


def ref_of(key, F, P, q, c, k, lh, lg, exclude_self, K):
    if key not in _REF:
        _REF[key] = xr.reference(F, P, q, c, k, lh, lg, exclude_self, K)
    return _REF[key]


def sides(Fd, Pd, q, c, as_slice):
    """The four device arrays: views of the data set (the library sees a row slice when the queries lie inside the candidates)
    or arrays of their own."""
    (q0, q1), (c0, c1) = q, c
    if as_slice:
        return Fd[q0:q1], Pd[q0:q1], Fd[c0:c1], Pd[c0:c1]
    return Fd[q0:q1].clone(), Pd[q0:q1].clone(), Fd[c0:c1].clone(), Pd[c0:c1].clone()


def check(mmf, F, P, q, c, k, precision, lh=LH, lg=LG, exclude_self=False, as_slice=False, ref_key=None, **kw):
    """One call against the reference; returns (idx, val, stats) on the host."""
    Fd, Pd, K_oracle, K_dev = shared(mmf, F, P, lh, lg)
    nq = q[1] - q[0]
    Fq, Pq, Fc, Pc = sides(Fd, Pd, q, c, as_slice)
    idx, val, st = xy().simtopk_combined_xy(Fq, Pq, Fc, Pc, lh, lg, k, exclude_self=exclude_self, row_offset=q[0], col_offset=c[0],
                                            precision=precision, return_stats=True, **kw)
    torch.cuda.synchronize()
    assert idx.shape == (nq, k) and idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    key = ref_key or (F.shape, P.shape, hash(F.tobytes()), hash(P.tobytes()), q, c, k, lh, lg, exclude_self)
    ridx, rval = ref_of(key, F, P, q, c, k, lh, lg, exclude_self, K_oracle)
    bad = np.nonzero((idx != ridx).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} queries differ from the reference, first {bad[0]}: got {idx[bad[0]]}, want {ridx[bad[0]]}"
    there = ridx >= 0
    assert np.all(np.isneginf(val[~there]))
    if there.any():
        rows = np.broadcast_to(np.arange(q[0], q[1])[:, None], (nq, k))[there]
        assert np.array_equal(bits(val[there]), bits(K_dev[rows, ridx[there]])), "values differ from sim_dense_combined's bits"
    err = float(np.abs(val[there].astype(np.float64) - rval[there].astype(np.float64)).max()) if there.any() else 0.0
    print(f"max |val - oracle| = {err:.3e}, fallback_rows {st['fallback_rows']}, candidates per query {st['candidates'] / max(nq, 1):.1f}")
    assert err <= TOL
    return idx, val, st


# ---- 1. the capacity condition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", xr.CASES, ids=[c.name for c in xr.CASES])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_capacity_condition(mmf, case, precision):
    """k + self = 6, 11, 12, 20 at col_splits 1 against the reference, then 2 and 4 with its bits.  Under the 16-bit precisions
    the restated band of every query fits its lists, so none may reach the exact pass."""
    F, P = xr.case_data(case)
    Fd, Pd, _, _ = shared(mmf, F, P)
    selves = (True, False) if case.name == "R2" else (True,)
    for kk in (6, 11, 12, 20):
        if precision != "exact":
            _, _, cnt = xr.bands_xy(F, P, case.q, case.c, LH, LG, kk, OPERAND[precision])
            cap = cr.capacity(kk)
            crowded = int((cnt > cap).sum())
            print(f"{case.name} {precision} k + self {kk}: largest band {int(cnt.max())} of {cap}, crowded queries {crowded}")
            assert crowded == 0
        for ex in selves:
            k = kk - 1 if ex else kk
            idx, val, st = check(mmf, F, P, case.q, case.c, k, precision, exclude_self=ex, as_slice=case.slice,
                                 ref_key=("cap", case.name, k, ex), col_splits=1)
            assert st["precision_used"] == PREC_CODE[precision] and st["col_splits"] == 1, st
            if precision != "exact":
                assert st["fallback_rows"] == 0, (kk, st)
            Fq, Pq, Fc, Pc = sides(Fd, Pd, case.q, case.c, case.slice)
            for cs in (2, 4):
                gi, gv, st = xy().simtopk_combined_xy(Fq, Pq, Fc, Pc, LH, LG, k, exclude_self=ex, row_offset=case.q[0], col_offset=case.c[0],
                                                      precision=precision, col_splits=cs, return_stats=True)
                assert st["precision_used"] == PREC_CODE[precision] and (precision == "exact" or st["fallback_rows"] == 0), (kk, cs, st)
                assert np.array_equal(gi.cpu().numpy(), idx) and np.array_equal(bits(gv.cpu().numpy()), bits(val)), (kk, cs)


# ---- 2. slices equal the self call --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole():
    """n = 700, d = 96 (R5's data set) and the self entries' results on it."""
    F, P = xr.case_data(xr.CASES[4])
    Fd, Pd = T(F).cuda(), T(P).cuda()
    want = {"exact": ct().simtopk_combined(Fd, Pd, LH, LG, 5)}
    for p in ("fast", "fast_bf16"):
        want[p] = ct16().simtopk_combined_fast(Fd, Pd, LH, LG, 5, precision=p)
    return Fd, Pd, want


@pytest.mark.parametrize("precision", PRECISIONS)
def test_row_panels_are_the_self_call(mmf, whole, precision):
    """R5's rows and the shard_bounds panels for 1, 2, 3 and 4 shards: bitwise the rows of simtopk_combined under "exact" and of
    simtopk_combined_fast under the 16-bit precisions; the same through the sharded driver with one rank."""
    from multimodal_fusion_amd.distributed import shard_bounds, sharded_simtopk_combined
    Fd, Pd, want = whole
    wi, wv = want[precision]
    lo, hi = xr.CASES[4].q
    got = xy().simtopk_combined_rows(Fd, Pd, lo, hi, LH, LG, 5, precision=precision, return_stats=True)
    assert same_bits(got, (wi[lo:hi], wv[lo:hi])) and got[2]["precision_used"] == PREC_CODE[precision]
    off = xy().simtopk_combined_rows(Fd, Pd, lo, hi, LH, LG, 5, precision=precision, col_offset=1000)
    assert torch.equal(off[0], wi[lo:hi] + 1000) and torch.equal(off[1].view(torch.int32), wv[lo:hi].view(torch.int32))
    for shards in (1, 2, 3, 4):
        parts = [xy().simtopk_combined_rows(Fd, Pd, *shard_bounds(700, shards, r), LH, LG, 5, precision=precision) for r in range(shards)]
        assert same_bits((torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])), (wi, wv)), shards
    one = sharded_simtopk_combined(Fd, Pd, 700, lambda_h=LH, lambda_g=LG, k=5, precision=precision, return_stats=True)
    assert same_bits(one, (wi, wv)) and one[2]["precision_used"] == PREC_CODE[precision] and one[2]["driver"] == "simple"


# ---- 3. edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_query_few_candidates_and_none(mmf, precision):
    F, P = cr.make_data(300, 40, 2, 1)
    check(mmf, F, P, (7, 8), (100, 300), 5, precision)                                            # nq = 1
    idx, _, st = check(mmf, F, P, (0, 130), (200, 203), 5, precision)                             # nc = 3 < k = 5: padding
    assert np.all(idx[:, 3:] == -1) and np.all(idx[:, :3] >= 200) and st["precision_used"] == 1
    idx, _, _ = check(mmf, F, P, (0, 6), (2, 5), 5, precision, exclude_self=True)                 # ... and three of the queries are candidates
    assert [int((r >= 0).sum()) for r in idx] == [3, 3, 2, 2, 2, 3]
    idx, _, _ = check(mmf, F, P, (4, 6), (4, 5), 2, precision, exclude_self=True)                 # one candidate, and it is query 0 itself
    assert idx.tolist() == [[-1, -1], [4, -1]]
    Fd, Pd, _, _ = shared(mmf, F, P)
    gi, gv = xy().simtopk_combined_xy(Fd[:9], Pd[:9], Fd[:0], Pd[:0], LH, LG, 5, precision=precision)   # nc = 0
    assert gi.shape == (9, 5) and bool((gi == -1).all()) and bool(torch.isneginf(gv).all())
    gi, gv = xy().simtopk_combined_xy(Fd[:0], Pd[:0], Fd, Pd, LH, LG, 5, precision=precision)           # nq = 0
    assert gi.shape == (0, 5) and gv.shape == (0, 5)


@pytest.mark.parametrize("dp", [1, 2, 3, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_position_dims(mmf, dp, precision):
    F, P = cr.make_data(300, 40, dp, 4)
    check(mmf, F, P, (0, 140), (140, 300), 5, precision)


@pytest.mark.parametrize("d", [1, 63, 200])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_feature_dims(mmf, d, precision):
    F, P = cr.make_data(300, d, 2, 3)
    check(mmf, F, P, (0, 140), (140, 300), 5, precision)


def test_the_limits_of_k(mmf):
    """k + self = 44 under exact; 21 under auto (the exact scan runs) and under fast (refused); 45 refused."""
    F, P = cr.make_data(300, 40, 2, 5)
    _, _, st = check(mmf, F, P, (0, 140), (100, 300), 43, "exact", exclude_self=True)
    assert st["precision_used"] == 1
    check(mmf, F, P, (0, 140), (140, 300), 44, "exact")
    _, _, st = check(mmf, F, P, (0, 140), (100, 300), 20, "auto", exclude_self=True)
    assert st["precision_used"] == 1
    Fd, Pd, _, _ = shared(mmf, F, P)
    f = xy().simtopk_combined_xy
    for p in ("fast", "fast_bf16"):
        with pytest.raises(RuntimeError, match=r"simtopk_combined_xy: k \+ self = 21 > 20"):
            f(Fd[:140], Pd[:140], Fd, Pd, LH, LG, 20, exclude_self=True, precision=p)
        f(Fd[:140], Pd[:140], Fd, Pd, LH, LG, 20, precision=p)                                     # k + self = 20: served
    with pytest.raises(RuntimeError, match=r"k \+ self = 45 > 44"):
        f(Fd[:140], Pd[:140], Fd, Pd, LH, LG, 45)
    with pytest.raises(RuntimeError, match="d = 4097 > 4096"):
        f(torch.zeros(4, 4097, device="cuda"), torch.zeros(4, 2, device="cuda"), torch.zeros(30, 4097, device="cuda"),
          torch.zeros(30, 2, device="cuda"), LH, LG, 2, precision="fast")


def test_exact_and_auto(mmf, whole):
    """ "auto" takes the 16-bit scan only in the measured range (512 <= d <= 1536, k + self <= 11) and the exact scan
    elsewhere.  The same bits either way; precision_used says which ran."""
    Fd, Pd, want = whole                                                                      # d = 96: exact
    a = xy().simtopk_combined_rows(Fd, Pd, 100, 400, LH, LG, 5, return_stats=True)
    assert a[2]["precision_used"] == 1 and same_bits(a, (want["exact"][0][100:400], want["exact"][1][100:400]))
    F, P = xr.case_data(xr.CASES[3])                                                          # R4: d = 512
    Fs, Ps, _, _ = shared(mmf, F, P)
    s4 = sides(Fs, Ps, (0, 300), (300, 600), False)
    e = xy().simtopk_combined_xy(*s4, LH, LG, 5, col_offset=300, precision="exact", return_stats=True)
    a = xy().simtopk_combined_xy(*s4, LH, LG, 5, col_offset=300, return_stats=True)
    assert e[2]["precision_used"] == 1 and a[2]["precision_used"] == 2 and a[2]["fallback_rows"] == 0 and same_bits(a, e)
    a12 = xy().simtopk_combined_xy(*s4, LH, LG, 12, col_offset=300, return_stats=True)         # k + self = 12: 32-entry lists, not measured
    assert a12[2]["precision_used"] == 1
    few = xy().simtopk_combined_xy(s4[0], s4[1], s4[2][:4], s4[3][:4], LH, LG, 5, col_offset=300, return_stats=True)   # 4 candidates < k
    assert few[2]["precision_used"] == 1 and bool((few[0][:, 4] == -1).all())


@pytest.mark.parametrize("term", ["features only", "positions only"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_zero_lambda_drops_its_term(mmf, term, precision):
    """Bitwise the exact RBF top-k of the one operand that is left, with the same offsets."""
    F, P = cr.make_data(300, 40, 2, 8)
    Fd, Pd, _, _ = shared(mmf, F, P)
    Fq, Pq, Fc, Pc = sides(Fd, Pd, (60, 200), (0, 300), False)
    kw = dict(exclude_self=True, row_offset=60, col_offset=0)
    if term == "features only":
        got = xy().simtopk_combined_xy(Fq, Pq, Fc, Pc, LH, 0.0, 5, precision=precision, **kw)
        want = mmf.ops.simtopk(Fq, Fc, metric="rbf", lam=LH, k=5, precision="exact", **kw)
    else:
        got = xy().simtopk_combined_xy(Fq, Pq, Fc, Pc, 0.0, LG, 5, precision=precision, **kw)
        want = mmf.ops.simtopk(Pq, Pc, metric="rbf", lam=LG, k=5, precision="exact", **kw)
    torch.cuda.synchronize()
    assert same_bits(got, want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_planted_rows(mmf, precision):
    """The planting of the self entry's test: candidate rows 100..109 copy query row 299's features, 100..104 its position too —
    the position alone, and for exact copies the id alone, decides."""
    F, P = cr.make_data(300, 40, 2, 10)
    F[100:110] = F[299]
    P[100:105] = P[299]
    idx, _, _ = check(mmf, F, P, (170, 300), (0, 170), 5, precision)
    assert list(idx[129]) == [100, 101, 102, 103, 104]
    idx, _, _ = check(mmf, F, P, (90, 300), (0, 170), 5, precision, exclude_self=True)
    assert list(idx[209]) == [100, 101, 102, 103, 104] and list(idx[12, :4]) == [100, 101, 103, 104]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_calls_cpu_tensors_and_flagged_rows(mmf, monkeypatch, precision):
    F, P = cr.make_data(300, 40, 2, 12)
    Fd, Pd, _, _ = shared(mmf, F, P)
    Fq, Pq, Fc, Pc = sides(Fd, Pd, (0, 140), (100, 300), False)
    kw = dict(exclude_self=True, row_offset=0, col_offset=100, precision=precision)
    a = xy().simtopk_combined_xy(Fq, Pq, Fc, Pc, LH, LG, 5, return_stats=True, **kw)
    b = xy().simtopk_combined_xy(Fq, Pq, Fc, Pc, LH, LG, 5, **kw)
    torch.cuda.synchronize()
    assert same_bits(a, b)
    hi, hv = xy().simtopk_combined_xy(Fq.cpu(), Pq.cpu(), Fc.cpu(), Pc.cpu(), LH, LG, 5, **kw)
    assert not hi.is_cuda and not hv.is_cuda and same_bits((hi, hv), (a[0].cpu(), a[1].cpu()))
    for as_slice in (False, True):          # MMF_DEBUG_FLAG_ROWS: the first 40 queries go down the exact pass
        s4 = sides(Fd, Pd, (130, 270), (0, 300), as_slice)
        kw2 = dict(exclude_self=True, row_offset=130, col_offset=0, precision=precision, return_stats=True)
        clean = xy().simtopk_combined_xy(*s4, LH, LG, 5, **kw2)
        with monkeypatch.context() as mp:
            mp.setenv("MMF_DEBUG_FLAG_ROWS", "40")
            flagged = xy().simtopk_combined_xy(*s4, LH, LG, 5, **kw2)
        assert same_bits(flagged, clean), as_slice
        if precision != "exact":
            assert clean[2]["fallback_rows"] == 0 and flagged[2]["fallback_rows"] == 40, (clean[2], flagged[2])


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_flagged_block_of_a_long_panel(mmf, whole, monkeypatch, precision):
    """680 queries = six row blocks, the first 40 flagged: one block of six is less than a quarter, so only that block's 128
    queries go through the exact pass — as a slice starting at row 20 of the candidates, and as a set of their own."""
    Fd, Pd, want = whole
    wi, wv = want[precision]
    monkeypatch.setenv("MMF_DEBUG_FLAG_ROWS", "40")
    got = xy().simtopk_combined_rows(Fd, Pd, 20, 700, LH, LG, 5, precision=precision, return_stats=True)
    assert got[2]["fallback_rows"] == 40 and same_bits(got, (wi[20:], wv[20:])), got[2]
    two = xy().simtopk_combined_xy(Fd[20:].clone(), Pd[20:].clone(), Fd, Pd, LH, LG, 5, exclude_self=True, row_offset=20, precision=precision,
                                   return_stats=True)
    assert two[2]["fallback_rows"] == 40 and same_bits(two, (wi[20:], wv[20:])), two[2]


# ---- 4. the stream contract: the C entry and both wrappers behind a closed gate ------------------------------------------------
def gated_inputs(which):
    F, P = cr.make_data(300, 40, 2, 20 if which == "truth" else 21)
    return [T(F), T(P)]


def gated_reference(q, c, exclude_self):
    def ref(F, P):
        ridx, rval = xr.reference(F, P, q, c, 5, LH, LG, exclude_self)
        return lambda got: sg.diff(got[0], ridx, "idx") + sg.diff(got[1], rval, "val", atol=TOL)
    return ref


def _c_entry(F, P):
    import multimodal_fusion_amd as m
    o = m.ops
    Fq, Pq, Fc, Pc = F[:140].clone(), P[:140].clone(), F[140:], P[140:]
    idx = torch.empty((140, 5), dtype=torch.int64, device=F.device)
    val = torch.empty((140, 5), dtype=torch.float32, device=F.device)
    opts = m._lib.SimtopkOpts(m._lib.PRECISIONS["fast"], 0, 0, m._lib.QUERY_ORDERS["off"], None)
    rc = m._lib.lib().mmf_simtopk_combined_xy(o._p(Fq), o._p(Pq), 140, o._p(Fc), o._p(Pc), 160, F.shape[1], P.shape[1], LH, LG, 5, 0, 0, 140,
                                              o._p(idx), o._p(val), ctypes.byref(opts), None, F.device.index or 0, o._stream(F.device))
    m._lib.check(rc, "mmf_simtopk_combined_xy")
    return [idx, val]                  # the entry has synchronised the stream: the copies may go


def _wrapper_xy(F, P):
    return list(xy().simtopk_combined_xy(F[:140].clone(), P[:140].clone(), F[140:], P[140:], LH, LG, 5, row_offset=0, col_offset=140,
                                         precision="fast_bf16"))


def _wrapper_rows_flagged(F, P):
    os.environ["MMF_DEBUG_FLAG_ROWS"] = "40"          # the second synchronisation and the exact pass, behind the gate too
    try:
        return list(xy().simtopk_combined_rows(F, P, 130, 270, LH, LG, 5, precision="fast"))
    finally:
        del os.environ["MMF_DEBUG_FLAG_ROWS"]


def _wrapper_rows_exact(F, P):
    return list(xy().simtopk_combined_rows(F, P, 130, 270, LH, LG, 5, precision="exact"))


@pytest.mark.parametrize("name,entry,q,c,ex", [("c_entry_simtopk_combined_xy", _c_entry, (0, 140), (140, 300), False),
                                               ("simtopk_combined_xy", _wrapper_xy, (0, 140), (140, 300), False),
                                               ("simtopk_combined_rows_flagged", _wrapper_rows_flagged, (130, 270), (0, 300), True),
                                               ("simtopk_combined_rows_exact", _wrapper_rows_exact, (130, 270), (0, 300), True)])
def test_entry_behind_a_closed_gate(mmf, name, entry, q, c, ex):
    assert list(SYNC) == list(mmf._lib.EXPORTS_TOPK_XY)
    sg.run_gated(entry, gated_inputs, gated_reference(q, c, ex), name=name, calls=2)
