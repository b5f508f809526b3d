"""The 16-bit combined top-k for any k on the MI355X (mmf_simtopk_combined_fast_anyk), f16 and bf16 operands.

Every case checks the indices against the numpy reference of tests/test_gpu_simtopk_combined.py (np.lexsort by (-key, id)), the
values BITWISE against the entries ops.sim_dense_combined writes, and the whole result bitwise against the exact any-k call
(combined_topk_anyk.simtopk_combined_any_k).  The shapes are the smallest at which each mechanism can go wrong: three row blocks
with a partial last one, many k-chunks, k on both sides of every pass boundary with and without self, ghosts under the ceiling,
tie groups that straddle the first floor, rows and segments that run out of columns, a ragged batch with unserved segments, and
operating settings (column ranges, MMF_ANYK_SHORT_DIV, flagged rows) that must not change a bit.  The "clean" and the "ghost"
inputs are tests/combined16_anyk_restate.py's, whose numpy restatement tests/test_simtopk_combined_fast_anyk_cpu.py runs."""
import ctypes
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combined16_anyk_restate as ar   # noqa: E402
from test_gpu_simtopk_combined import make_data, offsets_of, reference   # noqa: E402
from test_gpu_simtopk_combined_anyk import same_bits, verify   # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ["fast", "fast_bf16"]
LH, LG = ar.LH, ar.LG
RAGGED_PTR = [0, 0, 1, 38, 166, 295, 700]
ENTRY = "mmf_simtopk_combined_fast_anyk"

# entry -> (host synchronisations, how long *_host arguments must stay valid): INTEGRATION.md "16-bit combined any-k entries"
SYNC = {ENTRY: ("data-dependent", "the call")}

T = torch.from_numpy


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def ak16():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16_anyk")


def ak():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk_anyk")


def call(Fd, Pd, k, precision, lh=LH, lg=LG, **kw):
    out = ak16().simtopk_combined_fast_any_k(Fd, Pd, lh, lg, k, precision=precision, return_info=True, **kw)
    torch.cuda.synchronize()
    return out


def check_info(info, k, exclude_self, n_served, clean=False):
    plan = ar.plan(k, exclude_self)
    print(f"k = {k} self = {exclude_self}: {info}")
    assert info["passes"] == len(info["yield"]) and sum(info["yield"]) == k
    if max(info["yield"]) <= 20 - exclude_self:      # (a pass the exact scan finished emits all that is left)
        assert info["passes"] >= plan[2]
    assert info["yield"][0] == plan[1] and info["ghost_max"][0] == 0
    assert all(1 <= y <= 20 - exclude_self for y in info["yield"][1:-1])
    if clean:        # no band under a ceiling outgrows the lists (asserted on the CPU): no row is flagged, at most n / 64 fall short
        assert info["exact_rows"][0] == 0 and all(r <= n_served // 64 for r in info["exact_rows"][1:]), info


def full_check(mmf, F, P, k, precision, *, ptr=None, exclude_self=True, lh=LH, lg=LG, ref=None, exact=None, clean=False, **kw):
    """One call against the numpy reference, sim_dense_combined's bits and the exact any-k call's bits; returns (idx, val, info)."""
    Fd, Pd = T(F).cuda(), T(P).cuda()
    p = offsets_of([F.shape[0]]) if ptr is None else np.asarray(ptr, np.int64)
    seg = {} if ptr is None else {"ptr": T(p)}
    idx, val, info = call(Fd, Pd, k, precision, lh, lg, exclude_self=exclude_self, **seg, **kw)
    assert idx.shape == (F.shape[0], k) and idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
    verify(mmf, Fd, Pd, p, k, idx.cpu().numpy(), val.cpu().numpy(), ref if ref is not None else reference(F, P, p, k, lh, lg, exclude_self), lh, lg)
    if exact is None:
        exact = ak().simtopk_combined_any_k(Fd, Pd, lh, lg, k, exclude_self=exclude_self, **seg)
    assert same_bits((idx, val), (exact[0][:, :k].contiguous(), exact[1][:, :k].contiguous())), "differs from the exact any-k call"
    sizes = np.diff(p)
    check_info(info, k, exclude_self, int(sizes[sizes - exclude_self >= k].sum()), clean)
    return idx, val, info


# ---- 1. pass boundaries on the clean three-row-block graph -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph(mmf):
    """n = 300, d = 40, dp = 2: the reference and the exact any-k call at k = 64, per self mode — those of a smaller k are their
    first columns (one total order)."""
    F, P = ar.clean_inputs("n300")
    p = offsets_of([300])
    Fd, Pd = T(F).cuda(), T(P).cuda()
    return F, P, {s: (reference(F, P, p, 64, exclude_self=s), ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 64, exclude_self=s)) for s in (True, False)}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("k", [18, 19, 20, 21, 38, 39, 45, 64])
def test_pass_boundaries(mmf, graph, k, exclude_self, precision):
    F, P, refs = graph
    (ridx, rval), exact = refs[exclude_self]
    _, _, info = full_check(mmf, F, P, k, precision, exclude_self=exclude_self, ref=(ridx[:, :k], rval[:, :k]), exact=exact, clean=True)
    assert (info["passes"] == 1) == (k + exclude_self <= 20)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["n700", "n260"])
def test_basic_shapes(mmf, name, precision):
    """n = 700, d = 130, dp = 3 (six row blocks, an odd feature dim, no 16-byte rows) and n = 260, d = 1536 (24 k-chunks)."""
    F, P = ar.clean_inputs(name)
    full_check(mmf, F, P, 45, precision, clean=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_pass_is_the_existing_entry_and_a_deeper_call_keeps_its_prefix(mmf, graph, precision):
    F, P, _ = graph
    Fd, Pd = T(F).cuda(), T(P).cuda()
    old = import_module("multimodal_fusion_amd.combined_topk16").simtopk_combined_fast(Fd, Pd, LH, LG, 19, precision=precision)
    idx, val, info = call(Fd, Pd, 19, precision)
    assert same_bits((idx, val), old) and info == {"passes": 1, "yield": [19], "ghost_max": [0], "exact_rows": [0]}
    deep = call(Fd, Pd, 45, precision)
    assert same_bits((deep[0][:, :19].contiguous(), deep[1][:, :19].contiguous()), old)
    p = T(offsets_of([120, 180]))
    old = import_module("multimodal_fusion_amd.combined_topk16_segmented").simtopk_combined_fast_segmented(Fd, Pd, LH, LG, 19, ptr=p, precision=precision)
    idx, val, info = call(Fd, Pd, 19, precision, ptr=p)
    assert same_bits((idx, val), old) and info["passes"] == 1


# ---- 2. ghosts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ghosts_under_the_ceiling(mmf, precision):
    """Near-duplicate clusters with every position equal: the emitted rows of the cluster the floor lies in pass under the next
    ceiling (the restatement predicts it); the re-rank drops them as a prefix and the bits stay the exact call's."""
    F, P = ar.ghost_inputs()
    _, _, info = full_check(mmf, F, P, 45, precision, lh=ar.GHOST_LH, lg=ar.GHOST_LG)
    assert info["passes"] >= 3 and info["ghost_max"][1] >= 1, info


# ---- 3. ties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_copies_straddle_the_first_floor(mmf, precision):
    """Row 50 and its 30 exact copies (rows 100 .. 129, features and position) tie at every key: for each of them the tie group
    fills entries 0 .. 29 across the first floor at entry 18, ranked by id alone; a copy with a high id has its self entry BEHIND
    the first floor, where only the identity test drops it."""
    F, P = make_data(300, 40, 2, seed=4)
    F[100:130] = F[50]
    P[100:130] = P[50]
    idx, _, _ = full_check(mmf, F, P, 45, precision)
    idx = idx.cpu().numpy()
    group = np.r_[50, 100:130]
    for r in (50, 100, 115, 129):
        assert np.array_equal(idx[r, :30], group[group != r]), r


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("lh,lg", [(0.0, 2e-7), (0.0, 0.0)])
def test_equal_keys(mmf, lh, lg, precision):
    """lambda_h = 0: equal keys from grid positions; both zero: every key equal, the result is the first k ids without self."""
    F, P = make_data(300, 40, 2, seed=5)
    idx, val, _ = full_check(mmf, F, P, 45, precision, lh=lh, lg=lg)
    if lg == 0.0:
        want = np.stack([np.delete(np.arange(46), r)[:45] if r < 46 else np.arange(45) for r in range(300)])
        assert np.array_equal(idx.cpu().numpy(), want) and bool((val == 1.0).all())


# ---- 4. degenerate and edge inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_k_beyond_the_rows_fills_sentinel_filled_outputs(mmf, precision):
    F, P = make_data(50, 40, 2, seed=6)
    Fd, Pd = T(F).cuda(), T(P).cuda()
    n, k = 50, 64
    idx = torch.full((n, k), 7777777, dtype=torch.int64, device="cuda")
    val = torch.full((n, k), 123.0, dtype=torch.float32, device="cuda")
    opts = mmf._lib.SimtopkOpts(mmf._lib.PRECISIONS[precision], 0, 0, mmf._lib.QUERY_ORDERS["off"], None)
    info = mmf._lib.FastAnykInfo()
    rc = mmf._lib.lib().mmf_simtopk_combined_fast_anyk(mmf.ops._p(Fd), mmf.ops._p(Pd), n, 40, 2, LH, LG, k, 1, None, 0, mmf.ops._p(idx), mmf.ops._p(val),
                                                       ctypes.byref(opts), None, 0, mmf.ops._stream(Fd.device), ctypes.byref(info))
    mmf._lib.check(rc, ENTRY)
    torch.cuda.synchronize()
    ridx, _ = reference(F, P, offsets_of([50]), k)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert not (idx == 7777777).any() and not (val == 123.0).any() and np.array_equal(idx, ridx)
    assert (idx[:, :49] >= 0).all() and (idx[:, 49:] == -1).all() and np.isneginf(val[:, 49:]).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_all_zero_row_and_lambda_h_zero(mmf, precision):
    F, P = ar.clean_inputs("n300")
    F = F.copy()
    F[17] = 0.0
    full_check(mmf, F, P, 45, precision)
    full_check(mmf, F, P, 21, precision, lh=0.0, lg=3e-6)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("dp", [1, 8])
def test_position_dims(mmf, dp, precision):
    rng = np.random.RandomState(7300 + dp)
    F = (rng.randn(300, 40) * np.sqrt(8.0 / 40)).astype(np.float32)
    P = (rng.randint(0, 48, (300, dp)) * 224).astype(np.float32)
    full_check(mmf, F, P, 45, precision)


# ---- 5. ragged batches ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_case():
    F, P = ar.clean_inputs("n700")
    p = np.asarray(RAGGED_PTR, np.int64)
    return F, P, p, reference(F, P, p, 32)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("how", ["ptr", "batch"])
def test_ragged_batch(mmf, ragged_case, how, precision):
    """An empty segment, a one-row segment, a segment of 37 rows (served, and out of columns inside the second pass: its rows take
    the rescan), and segments of 128, 129 and 405 rows in one call; equal to a loop of one-graph calls."""
    F, P, p, ref = ragged_case
    Fd, Pd = T(F).cuda(), T(P).cuda()
    if how == "ptr":
        idx, val, info = full_check(mmf, F, P, 32, precision, ptr=p, ref=ref)
        assert info["passes"] == 2 and 30 <= info["exact_rows"][1] <= 37 + 699 // 64, info
    else:                                    # a batch vector cannot describe the empty segment: the same rows without it
        batch = torch.repeat_interleave(torch.arange(len(p) - 2), T(np.diff(p)[1:])).cuda()
        idx, val, info = call(Fd, Pd, 32, precision, batch=batch)
        verify(mmf, Fd, Pd, p, 32, idx.cpu().numpy(), val.cpu().numpy(), ref)
    for a, b in zip(p[:-1], p[1:]):
        if b > a:
            gi, gv, _ = call(Fd[a:b].contiguous(), Pd[a:b].contiguous(), 32, precision)
            gi = torch.where(gi >= 0, gi + int(a), gi)
            assert same_bits((gi, gv), (idx[a:b], val[a:b])), (a, b)


# ---- 6. operating settings must not change a bit ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def settings_case(mmf):
    F, P = ar.clean_inputs("n700")
    Fd, Pd = T(F).cuda(), T(P).cuda()
    return F, P, Fd, Pd, ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 64), ak().simtopk_combined_any_k(Fd, Pd, LH, LG, 32, ptr=T(np.asarray(RAGGED_PTR)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forced_column_splits(mmf, settings_case, precision):
    _, _, Fd, Pd, exact, exact_seg = settings_case
    for cs in (1, 2, 4):
        idx, val, st, info = ak16().simtopk_combined_fast_any_k(Fd, Pd, LH, LG, 64, precision=precision, col_splits=cs, return_stats=True, return_info=True)
        assert st["col_splits"] == cs and st["precision_used"] == mmf._lib.PRECISIONS[precision], st
        assert same_bits((idx, val), exact), cs
        idx, val, st = ak16().simtopk_combined_fast_any_k(Fd, Pd, LH, LG, 32, precision=precision, col_splits=cs, ptr=T(np.asarray(RAGGED_PTR)), return_stats=True)
        assert st["col_splits"] == min(cs, 4) and same_bits((idx, val), exact_seg), cs


@pytest.mark.parametrize("precision", PRECISIONS)
def test_short_div_changes_the_passes_not_the_bits(mmf, settings_case, precision, monkeypatch):
    """1: every unflagged row may fall short, so the best row sets the yield and the rest take the gathered rescan; 65536: none may
    at this n, so the worst row sets it and no unflagged row is rescanned."""
    _, _, Fd, Pd, exact, _ = settings_case
    seen = {}
    for div in ("1", "64", "65536"):
        monkeypatch.setenv("MMF_ANYK_SHORT_DIV", div)
        idx, val, info = call(Fd, Pd, 64, precision)
        assert same_bits((idx, val), exact), div
        check_info(info, 64, True, 700, clean=(div != "1"))
        seen[div] = info
    assert seen["65536"]["exact_rows"][1:] == [0] * (seen["65536"]["passes"] - 1)
    assert max(seen["1"]["exact_rows"][1:]) > 700 // 64 and seen["1"]["passes"] <= seen["64"]["passes"] <= seen["65536"]["passes"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_flagged_rows_take_the_gathered_rescan_in_every_pass(mmf, settings_case, precision, monkeypatch):
    _, _, Fd, Pd, exact, exact_seg = settings_case
    monkeypatch.setenv("MMF_DEBUG_FLAG_ROWS", "37")
    idx, val, info = call(Fd, Pd, 64, precision)
    assert same_bits((idx, val), exact)
    assert info["exact_rows"][0] == 37 and all(37 <= r <= 37 + 700 // 64 for r in info["exact_rows"][1:]), info
    idx, val, info = call(Fd, Pd, 32, precision, ptr=T(np.asarray(RAGGED_PTR)))
    assert same_bits((idx, val), exact_seg)
    assert info["exact_rows"][0] == 36 and info["exact_rows"][1] >= 36, info      # row 0 is a one-row segment: never served


# ---- 7. call mechanics -------------------------------------------------------------------------------------------------------------------
def test_exact_precision_the_router_and_two_calls_in_a_row(mmf, settings_case):
    F, P, Fd, Pd, exact, exact_seg = settings_case
    m = ak16()
    idx, val, info = call(Fd, Pd, 64, "exact")
    assert same_bits((idx, val), exact) and info["passes"] == 1 and info["yield"] == [64]
    idx, val, info = call(Fd, Pd, 32, "exact", ptr=T(np.asarray(RAGGED_PTR)))
    assert same_bits((idx, val), exact_seg) and info["passes"] == 1
    for prec in ("auto", "exact", "fast", "fast_bf16"):
        assert same_bits(m.simtopk_combined_any_k(Fd, Pd, LH, LG, 64, precision=prec), exact), prec
        assert same_bits(m.simtopk_combined_any_k(Fd, Pd, LH, LG, 32, precision=prec, ptr=T(np.asarray(RAGGED_PTR))), exact_seg), prec
    out = m.simtopk_combined_any_k(T(F), T(P), LH, LG, 64, precision="fast")                 # CPU tensors through the router
    assert not out[0].is_cuda and same_bits((out[0].cuda(), out[1].cuda()), exact)
    a, b = call(Fd, Pd, 64, "fast"), call(Fd, Pd, 45, "fast")                                  # a smaller call on the dirtied workspace
    assert same_bits(a[:2], exact) and same_bits(b[:2], (exact[0][:, :45].contiguous(), exact[1][:, :45].contiguous()))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.simtopk_combined_fast_any_k(T(F), T(P), LH, LG, 64)
    ei, ew, eptr = m.build_topk_weighted_hypergraph_fast_any_k(Fd, Pd, LH, LG, 32, ptr=T(np.asarray(RAGGED_PTR)), precision="fast")
    want = ak().build_topk_weighted_hypergraph_any_k(Fd, Pd, LH, LG, 32, ptr=T(np.asarray(RAGGED_PTR)))
    assert torch.equal(ei, want[0]) and torch.equal(ew, want[1]) and torch.equal(eptr, want[2])
    data = m.build_topk_hypergraph_data_fast_any_k(Fd, Pd, LH, LG, 32, ptr=T(np.asarray(RAGGED_PTR)), precision="fast")
    assert torch.equal(data["edge_index"], ei) and data["pooled_feature"].shape == (6, 130)


# ---- 8. stream contract ----------------------------------------------------------------------------------------------------------------
def _gated_inputs(n, seeds):
    def make_inputs(which):
        g = torch.Generator().manual_seed(seeds[0] if which == "truth" else seeds[1])
        return [torch.randn(n, 40, generator=g) * 0.3, torch.rand(n, 2, generator=g) * 4.0]
    return make_inputs


def _gated_one_graph(precision):
    def entry(F, P):
        return ak16().simtopk_combined_fast_any_k(F, P, 0.7, 0.3, 45, precision=precision)          # three passes
    return entry, _gated_inputs(413, (51, 52))


def _gated_batch(precision):
    xp = torch.tensor(offsets_of([3, 150, 0, 260]))

    def entry(F, P):
        return ak16().simtopk_combined_fast_any_k(F, P, 0.7, 0.3, 32, ptr=xp, precision=precision)  # one segment on the launch loop
    return entry, _gated_inputs(413, (53, 54))


GATED = {"one graph": _gated_one_graph, "batch": _gated_batch}


def test_the_sync_table_names_the_entry(mmf):
    assert set(SYNC) == {e for e in mmf._lib.TOPK16_ANYK_EXPORTS if "plan" not in e}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(GATED))
def test_stream_contract_behind_a_closed_gate(mmf, name, precision):
    """The call on a busy non-default stream, twice in a row, behind a producer that sits behind a closed gate: the bits of the
    same call on the idle default stream (tests/streamgate.py, the harness of tests/test_gpu_stream_contract.py)."""
    import streamgate
    entry, make_inputs = GATED[name](precision)
    streamgate.run_gated(entry, make_inputs, None, name=f"{ENTRY} {name} {precision}", calls=2)
