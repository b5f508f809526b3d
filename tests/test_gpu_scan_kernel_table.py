"""Every row of the 16-bit scan's instantiation table (padded dim x list capacity x operand type), through the plain and
the segmented launcher.  A wrong row or a swapped side only makes the call slower — the audit flags the rows and the exact
rescan repairs them — so beside the bits (indices and scores against the CPU oracle) each case pins how many rows took that
detour.  neg_sq_l2: its per-candidate bias makes a misplaced bias vector visible too."""
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DIMS = [100, 200, 500, 1000]          # pad to 128 / 256 / 512 / 1024
KS = [5, 15, 30]                      # k + self = 6 / 16 / 31: 15-, 16- and 32-entry lists
ROWS = [(d, k) for d in DIMS for k in KS if (d, k) != (1000, 30)]
PRECISION_USED = {"fast": 2, "fast_bf16": 3}
METRIC = "neg_sq_l2"
N_SELF, N_RECT, M_RECT = 300, 140, 300
SEGMENTS = [70, 300, 45]              # 45 - 1 admissible columns still cover k = 30: no segment goes to the exact pass

# (fallback_rows, overflow_rows) of commit 688316b (the parent of the change that introduced this file) for every case: this
# file run unchanged on that build gave 0 / 0 throughout.  A case that ever measures above zero there gets its entry here.
PARENT_FLAGGED = {}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


@functools.lru_cache(maxsize=None)
def rows(n, d, seed):
    return np.random.RandomState(seed).randn(n, d).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(kind, d, k):
    """The oracle's (idx, val) of a case, computed once and shared by both operand types."""
    if kind == "self":
        X = rows(N_SELF, d, d)
        return oracle.simtopk(X, X, metric=METRIC, k=k, exclude_self=True)
    if kind == "rect":
        return oracle.simtopk(rows(N_RECT, d, d + 1), rows(M_RECT, d, d + 2), metric=METRIC, k=k, exclude_self=True)
    X = rows(sum(SEGMENTS), d, d + 3)
    xp = np.concatenate([[0], np.cumsum(SEGMENTS)])
    parts = [oracle.simtopk(X[a:b], X[a:b], metric=METRIC, k=k, exclude_self=True, row_offset=int(a), col_offset=int(a))
             for a, b in zip(xp[:-1], xp[1:])]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def check(kind, d, k, precision, got):
    idx, val, st = got
    print(f"{kind} d={d} k={k} {precision}: precision_used {st['precision_used']} scan_grid {st['scan_grid']} "
          f"fallback_rows {st['fallback_rows']} overflow_rows {st['overflow_rows']}")
    ridx, rval = reference(kind, d, k)
    assert np.array_equal(idx.cpu().numpy(), ridx), "indices differ from the oracle"
    assert np.array_equal(val.cpu().numpy().view(np.int32), rval.view(np.int32)), "scores differ from the oracle"
    assert st["precision_used"] == PRECISION_USED[precision] and st["scan_grid"] > 0
    fb, ov = PARENT_FLAGGED.get((kind, d, k, precision), (0, 0))
    assert st["fallback_rows"] <= fb and st["overflow_rows"] <= ov


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("d,k", ROWS)
def test_plain_self(mmf, d, k, precision):
    """X against itself: one full row block and a partial one (three row blocks of 128 queries at d = 1000)."""
    X = torch.from_numpy(rows(N_SELF, d, d)).cuda()
    check("self", d, k, precision, mmf.simtopk(X, metric=METRIC, k=k, exclude_self=True, precision=precision, return_stats=True))


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("d,k", ROWS)
def test_plain_rectangular(mmf, d, k, precision):
    """Separate buffers of 140 and 300 rows: the two sides differ in every pointer and length."""
    X = torch.from_numpy(rows(N_RECT, d, d + 1)).cuda()
    Y = torch.from_numpy(rows(M_RECT, d, d + 2)).cuda()
    check("rect", d, k, precision, mmf.simtopk(X, Y, metric=METRIC, k=k, exclude_self=True, precision=precision, return_stats=True))


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("d,k", ROWS)
def test_segmented_self(mmf, d, k, precision):
    X = torch.from_numpy(rows(sum(SEGMENTS), d, d + 3)).cuda()
    xp = [0] + [int(v) for v in np.cumsum(SEGMENTS)]
    check("seg", d, k, precision, mmf.simtopk_segmented(X, ptr=xp, metric=METRIC, k=k, precision=precision, return_stats=True))


def test_no_32_entry_lists_at_padded_dim_1024(mmf):
    assert not mmf.ops.fast_scan_supported(1000, 30, True)
    assert all(mmf.ops.fast_scan_supported(d, k, True) for d, k in ROWS)
