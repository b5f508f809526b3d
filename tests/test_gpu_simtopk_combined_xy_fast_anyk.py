"""The 16-bit combined top-k for two node sets and any k on the MI355X (mmf_simtopk_combined_xy_fast_anyk), f16 and
bf16 operands.

Every case checks the indices against tests/combined_xy_restate.py's reference (np.lexsort by (-key, id) over the admissible
candidates), the values BITWISE against the entries ops.sim_dense_combined writes for the stacked data set, and the whole result
bitwise against the exact two-set any-k call (combined_topk_anyk.simtopk_combined_xy_any_k); `info` must agree with the plan
(tests/test_gpu_simtopk_combined_fast_anyk.py: check_info).  The shapes are the smallest at which each mechanism can go wrong: a
partial query block against a partial candidate tile with k on both sides of every pass boundary, the identity mid-range, a row slice
as views and as clones, many k-chunks, calls that run out of candidates, ghosts under the ceiling, a tie group across the first
floor, operating settings that must not change a bit, the stream contract and the sharded driver.  The cases are
tests/combined_xy_restate.py's (R1, R2, R5, R6); the clean, ghost and tie inputs are tests/combined_xy_anyk_restate.py's, whose
numpy restatement tests/test_simtopk_combined_xy_fast_anyk_cpu.py runs."""
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combined16_anyk_restate as ar      # noqa: E402
import combined_xy_anyk_restate as xa     # noqa: E402
import combined_xy_restate as xr          # noqa: E402
import streamgate as sg                   # noqa: E402
from test_gpu_simtopk_combined import bits   # noqa: E402
from test_gpu_simtopk_combined_fast_anyk import check_info   # noqa: E402
from test_gpu_simtopk_combined_xy import same_bits, shared, sides   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ["fast", "fast_bf16"]
PREC_CODE = {"exact": 1, "fast": 2, "fast_bf16": 3}
LH, LG = xr.LH, xr.LG
ENTRY = "mmf_simtopk_combined_xy_fast_anyk"
R1, R2, R5, R6 = xr.CASES[0], xr.CASES[1], xr.CASES[4], xr.CASES[5]

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "16-bit two-set any-k entries"
# (tests/test_simtopk_combined_xy_fast_anyk_cpu.py keeps the two equal)
SYNC = {ENTRY: ("data-dependent", "no host arguments")}

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def xk():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16_xy_anyk")


def ak():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk_anyk")


_EXACT = {}


def exact_of(key, s4, k, lh, lg, exclude_self, q0, c0):
    """The exact two-set any-k call, once per (data, ranges, self) at its largest k: a smaller k is its first columns."""
    if key not in _EXACT:
        _EXACT[key] = ak().simtopk_combined_xy_any_k(*s4, lh, lg, k, exclude_self=exclude_self, row_offset=q0, col_offset=c0)
    return _EXACT[key]


_REF = {}


def full_check(mmf, F, P, q, c, k, precision, *, exclude_self=False, as_slice=False, lh=LH, lg=LG, k_ref=None, clean=False, plan=True, **kw):
    """One call against the reference, sim_dense_combined's bits and the exact two-set any-k call's bits; (idx, val, info, stats)."""
    Fd, Pd, K_oracle, K_dev = shared(mmf, F, P, lh, lg)
    nq, k_ref = q[1] - q[0], k_ref or k
    s4 = sides(Fd, Pd, q, c, as_slice)
    idx, val, st, info = xk().simtopk_combined_xy_fast_any_k(*s4, lh, lg, k, exclude_self=exclude_self, row_offset=q[0], col_offset=c[0],
                                                            precision=precision, return_stats=True, return_info=True, **kw)
    torch.cuda.synchronize()
    assert idx.shape == (nq, k) and idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
    key = (F.shape, hash(F.tobytes()), hash(P.tobytes()), q, c, k_ref, lh, lg, exclude_self)
    if key not in _REF:
        _REF[key] = xr.reference(F, P, q, c, k_ref, lh, lg, exclude_self, K_oracle)
    ridx, rval = _REF[key][0][:, :k], _REF[key][1][:, :k]
    hi, hv = idx.cpu().numpy(), val.cpu().numpy()
    bad = np.nonzero((hi != ridx).any(axis=1))[0]
    if bad.size:
        col = int(np.nonzero(hi[bad[0]] != ridx[bad[0]])[0][0])
        raise AssertionError(f"{bad.size} queries differ from the reference, first query {bad[0]} at column {col}: got "
                             f"{hi[bad[0], max(col - 2, 0):col + 3]}, want {ridx[bad[0], max(col - 2, 0):col + 3]}")
    there = ridx >= 0
    assert np.all(np.isneginf(hv[~there]))
    if there.any():
        rows = np.broadcast_to(np.arange(q[0], q[1])[:, None], (nq, k))[there]
        assert np.array_equal(bits(hv[there]), bits(K_dev[rows, ridx[there]])), "values differ from sim_dense_combined's bits"
    exact = exact_of(key + (as_slice,), s4, k_ref, lh, lg, exclude_self, q[0], c[0])
    assert same_bits((idx, val), (exact[0][:, :k].contiguous(), exact[1][:, :k].contiguous())), "differs from the exact two-set any-k call"
    if plan:
        check_info(info, k, exclude_self, nq, clean)
    return idx, val, info, st


# ---- 1. pass boundaries on the clean input: a partial query block against a partial candidate tile -----------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("k", [18, 19, 20, 21, 38, 39, 45, 64])
def test_pass_boundaries(mmf, k, exclude_self, precision):
    """R1.  No band under a ceiling outgrows the lists (asserted on the CPU): no query is flagged in the first pass, and a later pass
    rescans at most nq // 64 — the yield rule's own bound."""
    (F, P), q, c = xa.clean_case()
    _, _, info, st = full_check(mmf, F, P, q, c, k, precision, exclude_self=exclude_self, k_ref=64, clean=True)
    assert (info["passes"] == 1) == (k + exclude_self <= 20) and st["precision_used"] == PREC_CODE[precision]
    assert info["exact_rows"][0] == 0 and all(r <= (q[1] - q[0]) // 64 for r in info["exact_rows"][1:]), info


# ---- 2. identity mid-range, 3. the slice, 4. many k-chunks ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("exclude_self", [True, False])
def test_identity_mid_range(mmf, exclude_self, precision):
    """R2: rows 100..299 against rows 50..349 (row_offset 100, col_offset 50) — every query's own id lies among the candidates'."""
    F, P = xr.case_data(R2)
    idx, _, _, _ = full_check(mmf, F, P, R2.q, R2.c, 45, precision, exclude_self=exclude_self)
    own = (idx.cpu() == torch.arange(R2.q[0], R2.q[1])[:, None]).any(dim=1)
    assert bool(own.any()) != exclude_self and (exclude_self or bool(own.all()))     # the nearest candidate of a row is the row


@pytest.fixture(scope="module")
def whole_r5(mmf):
    F, P = xr.case_data(R5)
    Fd, Pd, _, _ = shared(mmf, F, P)
    ak16 = import_module("multimodal_fusion_amd.combined_topk16_anyk")
    return F, P, Fd, Pd, {p: ak16.simtopk_combined_fast_any_k(Fd, Pd, LH, LG, 45, precision=p) for p in PRECISIONS}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_slice_as_views_and_as_clones(mmf, whole_r5, precision):
    """R5: rows 175..349 against all 700 — both equal those rows of the self call on the whole set; the rows call hands the views."""
    F, P, Fd, Pd, want = whole_r5
    wi, wv = want[precision]
    lo, hi = R5.q
    for as_slice in (True, False):
        idx, val, _, _ = full_check(mmf, F, P, R5.q, R5.c, 45, precision, exclude_self=True, as_slice=as_slice)
        assert same_bits((idx, val), (wi[lo:hi], wv[lo:hi])), as_slice
    got = xk().simtopk_combined_rows_fast_any_k(Fd, Pd, lo, hi, LH, LG, 45, precision=precision, return_info=True)
    assert same_bits(got, (wi[lo:hi], wv[lo:hi])) and got[2]["passes"] >= 3
    off = xk().simtopk_combined_rows_fast_any_k(Fd, Pd, lo, hi, LH, LG, 45, precision=precision, col_offset=1000)
    assert torch.equal(off[0], wi[lo:hi] + 1000) and torch.equal(off[1].view(torch.int32), wv[lo:hi].view(torch.int32))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_many_k_chunks(mmf, precision):
    """R6: 150 x 150 at d = 1536 (24 k-chunks)."""
    F, P = xr.case_data(R6)
    full_check(mmf, F, P, R6.q, R6.c, 45, precision)


# ---- 5. one pass is the existing entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_pass_is_the_existing_entry_and_a_deeper_call_keeps_its_prefix(mmf, precision):
    (F, P), q, c = xa.clean_case()
    Fd, Pd, _, _ = shared(mmf, F, P)
    s4 = sides(Fd, Pd, q, c, False)
    old = import_module("multimodal_fusion_amd.combined_topk_xy").simtopk_combined_xy(*s4, LH, LG, 19, exclude_self=True, row_offset=q[0], col_offset=c[0],
                                                                                     precision=precision)
    kw = dict(exclude_self=True, row_offset=q[0], col_offset=c[0], precision=precision, return_info=True)
    idx, val, info = xk().simtopk_combined_xy_fast_any_k(*s4, LH, LG, 19, **kw)
    assert same_bits((idx, val), old) and info == {"passes": 1, "yield": [19], "ghost_max": [0], "exact_rows": [0]}
    deep = xk().simtopk_combined_xy_fast_any_k(*s4, LH, LG, 45, **kw)
    assert same_bits((deep[0][:, :19].contiguous(), deep[1][:, :19].contiguous()), old) and deep[2]["passes"] >= 3


# ---- 6. running out of candidates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_running_out_of_candidates(mmf, precision):
    (F, P), _, _ = xa.clean_case()
    # nc = 30 with k = 45: served exactly, -1 / -inf tail
    idx, val, info, st = full_check(mmf, F, P, (0, 130), (200, 230), 45, precision, plan=False)
    assert st["precision_used"] == 1 and info == {"passes": 1, "yield": [45], "ghost_max": [0], "exact_rows": [0]}
    assert bool((idx[:, :30] >= 200).all()) and bool((idx[:, 30:] == -1).all()) and bool(torch.isneginf(val[:, 30:]).all())
    # nc = 45 = k, self excluded, query ids 80 .. 169 straddle the candidate ids 100 .. 144: the queries inside end in one -1
    idx, _, info, st = full_check(mmf, F, P, (80, 170), (100, 145), 45, precision, exclude_self=True, plan=False)
    inside = (torch.arange(80, 170) >= 100) & (torch.arange(80, 170) < 145)
    assert st["precision_used"] == 1 and info["passes"] == 1
    assert torch.equal((idx[:, 44] == -1).cpu(), inside) and bool((idx[:, :44] >= 0).all())
    # nc = 50, k = 45: the later pass is deeper than what is left — short lists, the re-rank flags, the rescan answers
    idx, _, info, st = full_check(mmf, F, P, (80, 170), (100, 150), 45, precision, exclude_self=True)
    assert st["precision_used"] == PREC_CODE[precision] and info["passes"] >= 3 and bool((idx >= 0).all())
    assert info["exact_rows"][-1] == 90 or max(info["exact_rows"][1:]) > 0, info
    gi, gv, info = xk().simtopk_combined_xy_fast_any_k(*sides(*shared(mmf, F, P)[:2], (0, 9), (0, 0), False), LH, LG, 45, precision=precision,
                                                       return_info=True)                               # nc = 0
    assert gi.shape == (9, 45) and bool((gi == -1).all()) and bool(torch.isneginf(gv).all()) and info["passes"] == 1
    gi, gv = xk().simtopk_combined_xy_fast_any_k(*sides(*shared(mmf, F, P)[:2], (0, 0), (0, 390), False), LH, LG, 45, precision=precision)   # nq = 0
    assert gi.shape == (0, 45) and gv.shape == (0, 45)


# ---- 7. ghosts, 8. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ghosts_under_the_ceiling(mmf, precision):
    """Near-duplicate clusters with every position equal, the first 200 rows against all 600: the emitted rows of the cluster the
    floor lies in pass under the next ceiling (the restatement predicts it); the re-rank drops them as a prefix."""
    (F, P), q, c = xa.ghost_case()
    for as_slice in (True, False):
        _, _, info, _ = full_check(mmf, F, P, q, c, 45, precision, exclude_self=True, as_slice=as_slice, lh=ar.GHOST_LH, lg=ar.GHOST_LG)
        assert info["passes"] >= 3 and info["ghost_max"][1] >= 1, info


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("exclude_self", [True, False])
def test_ties_straddle_the_first_floor(mmf, exclude_self, precision):
    """30 identical candidates at one position are ranks 15 .. 44 of queries 0 .. 2: ids ascending across the pass boundary."""
    F, P = xa.tie_inputs()
    (_, _), q, c = xa.clean_case()
    idx, val, _, _ = full_check(mmf, F, P, q, c, 64, precision, exclude_self=exclude_self)
    idx = idx.cpu().numpy()
    for r in xa.TIE_QUERIES:
        assert sorted(idx[r, :15]) == list(xa.TIE_NEAR) and np.array_equal(idx[r, 15:45], xa.TIE_GROUP), r
        assert len(set(bits(val[r, 15:45].cpu().numpy()).tolist())) == 1


# ---- 9. operating settings must not change a bit --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def settings_case(mmf):
    (F, P), q, c = xa.clean_case()
    Fd, Pd, _, _ = shared(mmf, F, P)
    s4 = sides(Fd, Pd, q, c, False)
    return s4, q, c, ak().simtopk_combined_xy_any_k(*s4, LH, LG, 45, exclude_self=True, row_offset=q[0], col_offset=c[0])


def _call(s4, q, c, precision, **kw):
    out = xk().simtopk_combined_xy_fast_any_k(*s4, LH, LG, 45, exclude_self=True, row_offset=q[0], col_offset=c[0], precision=precision,
                                              return_stats=True, return_info=True, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forced_column_splits(mmf, settings_case, precision):
    s4, q, c, exact = settings_case
    for cs in (1, 2, 4):
        idx, val, st, _ = _call(s4, q, c, precision, col_splits=cs)
        assert st["col_splits"] == min(cs, 2) and st["precision_used"] == PREC_CODE[precision], st      # 260 candidates: three tiles
        assert same_bits((idx, val), exact), cs


@pytest.mark.parametrize("precision", PRECISIONS)
def test_short_div_changes_the_passes_not_the_bits(mmf, settings_case, precision, monkeypatch):
    s4, q, c, exact = settings_case
    seen = {}
    for div in ("1", "65536"):
        monkeypatch.setenv("MMF_ANYK_SHORT_DIV", div)
        idx, val, _, info = _call(s4, q, c, precision)
        assert same_bits((idx, val), exact), div
        check_info(info, 45, True, 130, clean=(div != "1"))
        seen[div] = info
    assert seen["65536"]["exact_rows"][1:] == [0] * (seen["65536"]["passes"] - 1)
    assert seen["1"]["passes"] <= seen["65536"]["passes"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_flagged_queries_take_the_gathered_rescan_in_every_pass(mmf, settings_case, precision, monkeypatch):
    s4, q, c, exact = settings_case
    monkeypatch.setenv("MMF_DEBUG_FLAG_ROWS", "37")
    idx, val, st, info = _call(s4, q, c, precision)
    assert same_bits((idx, val), exact)
    assert info["exact_rows"][0] == 37 and all(37 <= r <= 37 + 130 // 64 for r in info["exact_rows"][1:]), info
    assert st["fallback_rows"] == sum(info["exact_rows"])
    F, P = xr.case_data(R5)                     # ... and as a row slice that does not start at the candidates' first row
    Fd, Pd, _, _ = shared(mmf, F, P)
    got = xk().simtopk_combined_rows_fast_any_k(Fd, Pd, 175, 350, LH, LG, 45, precision=precision, return_info=True)
    monkeypatch.delenv("MMF_DEBUG_FLAG_ROWS")
    want = ak().simtopk_combined_rows_any_k(Fd, Pd, 175, 350, LH, LG, 45)
    assert same_bits(got, want) and all(r >= 37 for r in got[2]["exact_rows"]), got[2]


# ---- 10. refusals and routing with device tensors -----------------------------------------------------------------------------------------
def test_refusals_and_routing(mmf, settings_case):
    s4, q, c, exact = settings_case
    m = xk()
    wide = [torch.zeros(4, 4200, device="cuda"), torch.zeros(4, 2, device="cuda"), torch.zeros(60, 4200, device="cuda"), torch.zeros(60, 2, device="cuda")]
    with pytest.raises(RuntimeError, match=r"simtopk_combined_xy_fast_anyk: d = 4200 > 4096 is not supported \(MMF_PREC_EXACT takes any d\)"):
        m.simtopk_combined_xy_fast_any_k(*wide, LH, LG, 45, precision="fast")
    want = ak().simtopk_combined_xy_any_k(*wide, LH, LG, 45)
    for prec in ("exact", "auto"):                        # d = 4200: the exact call's bits through the entry ("exact") and the router
        assert same_bits(m.simtopk_combined_xy_any_k(*wide, LH, LG, 45, precision=prec), want), prec
    got = m.simtopk_combined_xy_fast_any_k(*wide, LH, LG, 45, precision="exact", return_info=True)
    assert same_bits(got, want) and got[2] == {"passes": 1, "yield": [45], "ghost_max": [0], "exact_rows": [0]}
    kw = dict(exclude_self=True, row_offset=q[0], col_offset=c[0])
    for prec in ("auto", "exact", "fast", "fast_bf16"):   # R1 is off the measured classes: "auto" is the exact call
        out = m.simtopk_combined_xy_any_k(*s4, LH, LG, 45, precision=prec, return_stats=True, **kw)
        assert same_bits(out, exact) and out[2]["precision_used"] == PREC_CODE[prec if prec != "auto" else "exact"], prec
    cpu = m.simtopk_combined_xy_any_k(*(t.cpu() for t in s4), LH, LG, 45, precision="fast", **kw)          # CPU tensors through the router
    assert not cpu[0].is_cuda and same_bits((cpu[0].cuda(), cpu[1].cuda()), exact)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.simtopk_combined_xy_fast_any_k(*(t.cpu() for t in s4), LH, LG, 45)
    F, P = xr.case_data(R5)
    Fd, Pd, _, _ = shared(mmf, F, P)
    want = ak().simtopk_combined_rows_any_k(Fd, Pd, 175, 350, LH, LG, 45)
    for prec in ("auto", "exact", "fast", "fast_bf16"):
        assert same_bits(m.simtopk_combined_rows_any_k(Fd, Pd, 175, 350, LH, LG, 45, precision=prec), want), prec


# ---- 11. stream contract ---------------------------------------------------------------------------------------------------------------------
def _gated_inputs(which):
    g = torch.Generator().manual_seed(61 if which == "truth" else 62)
    return [torch.randn(413, 40, generator=g) * 0.3, torch.rand(413, 2, generator=g) * 4.0]


def _gated_two_sets(precision):
    def entry(F, P):
        return list(xk().simtopk_combined_xy_fast_any_k(F[:150].clone(), P[:150].clone(), F[150:], P[150:], 0.7, 0.3, 45, row_offset=0, col_offset=150,
                                                        precision=precision))
    return entry


def _gated_rows_flagged(precision):
    def entry(F, P):
        os.environ["MMF_DEBUG_FLAG_ROWS"] = "40"          # the rescans' synchronisations and exact passes, behind the gate too
        try:
            return list(xk().simtopk_combined_rows_fast_any_k(F, P, 130, 300, 0.7, 0.3, 45, precision=precision))
        finally:
            del os.environ["MMF_DEBUG_FLAG_ROWS"]
    return entry


GATED = {"two sets": _gated_two_sets, "rows flagged": _gated_rows_flagged}


def test_the_sync_table_names_the_entry(mmf):
    assert set(SYNC) == set(mmf._lib.TOPK16_XY_ANYK_EXPORTS)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(GATED))
def test_stream_contract_behind_a_closed_gate(mmf, name, precision):
    """The call on a busy non-default stream, twice in a row, behind a producer that sits behind a closed gate: the bits of the
    same call on the idle default stream (tests/streamgate.py, the harness of tests/test_gpu_stream_contract.py)."""
    sg.run_gated(GATED[name](precision), _gated_inputs, None, name=f"{ENTRY} {name} {precision}", calls=2)


# ---- 12. the sharded driver --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sharded_driver_with_one_rank(mmf, precision):
    """World 1, no process group, n = 400 (R2's data set), k = 45: the rows call on everything, and the exact sharded call's bits."""
    from multimodal_fusion_amd.distributed import sharded_simtopk_combined_any_k, sharded_simtopk_combined_fast_any_k
    F, P = xr.case_data(R2)
    Fd, Pd, _, _ = shared(mmf, F, P)
    one = sharded_simtopk_combined_fast_any_k(Fd, Pd, 400, lambda_h=LH, lambda_g=LG, k=45, precision=precision, return_stats=True)
    rows = xk().simtopk_combined_rows_fast_any_k(Fd, Pd, 0, 400, LH, LG, 45, precision=precision)
    want = sharded_simtopk_combined_any_k(Fd, Pd, 400, lambda_h=LH, lambda_g=LG, k=45)
    assert same_bits(one, rows) and same_bits(one, want)
    assert one[2]["driver"] == "simple" and one[2]["precision_used"] == PREC_CODE[precision]


def test_sharded_driver_two_ranks_uneven_shards():
    """One torch.distributed.run child, 2 ranks over gloo on one GPU, n = 401: each rank's rows equal the unsharded exact call
    (scripts/shard_combined_fast_any_k.py; launched as tests/test_gpu_distributed.py's _torchrun does, with its own time limit)."""
    from test_gpu_distributed import _free_port
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(ROOT, "scripts", "shard_combined_fast_any_k.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    tail = out.stdout[-3000:] + "\n---- stderr ----\n" + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert "SHARDED FAST ANY-K OK" in out.stdout and "MISMATCH" not in out.stdout and out.stdout.count(": OK") == 4, tail
