"""Segmented simtopk (mmf_simtopk_segmented): per-segment k-NN over a ragged batch in one call.  Every result is checked
against one simtopk call per segment (indices equal, values bitwise), a subset against the CPU oracle."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def dup_rows(n, d, seed, clusters=None, noise=0.02, scale=1.0):
    rng = np.random.RandomState(seed)
    c = rng.randn(clusters or max(3, n // 40), d).astype(np.float32)
    return ((c[rng.randint(0, len(c), n)] + noise * rng.randn(n, d).astype(np.float32)) * scale).astype(np.float32)


def offsets(sizes):
    return [0] + list(np.cumsum(sizes).astype(np.int64))


def per_segment(mmf, X, Y, xp, yp, k, exclude_self, **kw):
    """The loop the segmented call replaces: one simtopk per segment, short segments padded with -1 / -inf."""
    n = X.shape[0]
    idx = torch.full((n, k), -1, dtype=torch.int64, device=X.device)
    val = torch.full((n, k), float("-inf"), dtype=torch.float32, device=X.device)
    Yf = X if Y is None else Y
    for s in range(len(xp) - 1):
        a, b, c, e = xp[s], xp[s + 1], yp[s], yp[s + 1]
        if b == a:
            continue
        overlap = exclude_self and a < e and b > c
        ks = min(k, (e - c) - (1 if overlap else 0))
        if ks <= 0:
            continue
        i, v = mmf.simtopk(X[a:b], Yf[c:e], row_offset=a, col_offset=c, exclude_self=exclude_self, k=ks, **kw)
        idx[a:b, :ks] = i
        val[a:b, :ks] = v
    return idx, val


def assert_same(got, ref):
    assert torch.equal(got[0], ref[0]), "indices differ"
    assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), "values differ"


RAGGED = [33, 0, 1, 257, 5, 6, 128, 31, 4096, 129, 32, 255, 127, 256, 0, 1]


@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("precision", ["auto", "exact"])
def test_self_same_bits_as_the_loop(mmf, metric, dtype, precision):
    sizes = RAGGED if precision == "auto" else [s for s in RAGGED if s != 4096] + [700]
    xp = offsets(sizes)
    X = torch.from_numpy(dup_rows(xp[-1], 64, 7, scale=0.1 if metric == "rbf" else 1.0)).to(dtype).cuda()
    kw = dict(metric=metric, lam=0.5, k=5)
    got = mmf.simtopk_segmented(X, ptr=xp, precision=precision, return_stats=True, **kw)
    assert got[2]["near_rows"] == -1                                   # the query order is never probed here
    assert_same(got[:2], per_segment(mmf, X, None, xp, xp, exclude_self=True, **kw))


@pytest.mark.parametrize("metric", ["cosine", "dot", "neg_sq_l2", "rbf"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("precision", ["auto", "exact"])
def test_cross_same_bits_as_the_loop(mmf, metric, dtype, precision):
    xs = [40, 0, 129, 5, 257, 1, 300, 32]
    ys = [300, 7, 33, 0, 128, 256, 4, 1000]
    xp, yp = offsets(xs), offsets(ys)
    sc = 0.1 if metric == "rbf" else 1.0
    X = torch.from_numpy(dup_rows(xp[-1], 100, 1, scale=sc)).to(dtype).cuda()
    Y = torch.from_numpy(dup_rows(yp[-1], 100, 2, scale=sc)).to(dtype).cuda()
    kw = dict(metric=metric, lam=0.5, k=5)
    got = mmf.simtopk_segmented(X, Y, ptr=xp, y_ptr=yp, precision=precision, **kw)
    assert_same(got, per_segment(mmf, X, Y, xp, yp, exclude_self=False, **kw))


@pytest.mark.parametrize("d,k,precision", [(200, 5, "auto"), (64, 25, "fast"), (200, 25, "auto"), (300, 9, "fast_bf16"),
                                             (96, 30, "fast_bf16"), (1000, 12, "fast"), (200, 14, "fast")])
@pytest.mark.parametrize("metric", ["cosine", "neg_sq_l2"])
def test_scan_shapes_same_bits_as_the_loop(mmf, d, k, precision, metric):
    """The other instantiations of the segmented 16-bit scan: padded dim 256 / 512 / 1024, 16- and 32-entry lists
    (k + self in 12..20 and 21..44), bf16 operands."""
    xp = offsets([40, 300, 0, 257, 26, 1100, 31, 129])
    X = torch.from_numpy(dup_rows(xp[-1], d, d + k)).cuda()
    kw = dict(metric=metric, k=k)
    got = mmf.simtopk_segmented(X, ptr=xp, precision=precision, return_stats=True, **kw)
    assert got[2]["precision_used"] == (3 if precision == "fast_bf16" else 2) and got[2]["scan_grid"] > 0
    assert_same(got[:2], per_segment(mmf, X, None, xp, xp, exclude_self=True, **kw))


def test_many_flagged_rows_in_batches(mmf):
    """More flagged rows than one gathered batch of the exact pass holds (4096): pieces and batches."""
    rng = np.random.RandomState(13)
    xp = offsets([300, 9000, 50])
    base = rng.randn(3, 48).astype(np.float32)
    X = torch.from_numpy(base[rng.randint(0, 3, xp[-1])]).cuda()
    idx, val, st = mmf.simtopk_segmented(X, ptr=xp, k=5, precision="fast", return_stats=True)
    assert st["fallback_rows"] > 4096
    assert_same((idx, val), per_segment(mmf, X, None, xp, xp, k=5, exclude_self=True))


@pytest.mark.parametrize("metric", ["cosine", "neg_sq_l2", "rbf"])
def test_against_the_oracle(mmf, metric):
    sizes = [300, 17, 0, 129, 6, 513]
    xp = offsets(sizes)
    X = dup_rows(xp[-1], 48, 3, scale=0.1 if metric == "rbf" else 1.0)
    idx, val = mmf.simtopk_segmented(torch.from_numpy(X).cuda(), ptr=xp, metric=metric, lam=0.5, k=5)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for s in range(len(sizes)):
        a, b = xp[s], xp[s + 1]
        if b - a < 6:
            continue
        ridx, rval = oracle.simtopk(X[a:b], X[a:b], metric=metric, lam=0.5, k=5, exclude_self=True, row_offset=a, col_offset=a)
        assert np.array_equal(idx[a:b], ridx)
        if metric == "rbf":
            np.testing.assert_allclose(val[a:b], rval, rtol=0, atol=TOL)
        else:
            assert np.array_equal(val[a:b], rval)


def test_no_neighbour_crosses_a_segment(mmf):
    """Each row has an exact duplicate in the next segment and its cluster straddles the boundary: any masking error would
    rank those columns first."""
    rng = np.random.RandomState(5)
    sizes = [200, 37, 256, 300, 33, 129]
    xp = offsets(sizes)
    base = rng.randn(8, 96).astype(np.float32)
    X = base[rng.randint(0, 8, xp[-1])] + 0.01 * rng.randn(xp[-1], 96).astype(np.float32)
    for s in range(len(sizes) - 1):             # row i of segment s reappears in segment s + 1
        a, b, c = xp[s], xp[s + 1], xp[s + 2]
        t = min(b - a, c - b)
        X[b:b + t] = X[a:a + t]
    Xt = torch.from_numpy(X).cuda()
    for precision in ["auto", "exact"]:
        idx, val = mmf.simtopk_segmented(Xt, ptr=xp, k=5, precision=precision)
        idx = idx.cpu().numpy()
        for s in range(len(sizes)):
            a, b = xp[s], xp[s + 1]
            blk = idx[a:b]
            assert ((blk >= a) & (blk < b)).all(), f"segment {s} leaked ({precision})"
            assert not (blk == np.arange(a, b)[:, None]).any()


def test_short_segments(mmf):
    sizes = [3, 1, 6, 2, 0, 10]
    xp = offsets(sizes)
    X = torch.from_numpy(dup_rows(xp[-1], 40, 9)).cuda()
    idx, val = mmf.simtopk_segmented(X, ptr=xp, k=5)
    ref = per_segment(mmf, X, None, xp, xp, k=5, exclude_self=True)
    assert_same((idx, val), ref)
    idx, val = idx.cpu(), val.cpu()
    assert (idx[0:3, 2:] == -1).all() and torch.isinf(val[0:3, 2:]).all()      # 3 rows: 2 neighbours each
    assert (idx[3, :] == -1).all()                                              # alone in its segment
    assert (idx[4:10, :5] >= 4).all() and (idx[4:10, :5] < 10).all()            # 6 rows: exactly k = 5


def test_fallback_inside_segments(mmf):
    """Exact duplicates in large numbers: the 16-bit lists overflow and rows are rescanned exactly, segment by segment."""
    rng = np.random.RandomState(11)
    sizes = [1500, 700, 2100]
    xp = offsets(sizes)
    base = rng.randn(4, 64).astype(np.float32)
    X = torch.from_numpy(base[rng.randint(0, 4, xp[-1])]).cuda()
    idx, val, st = mmf.simtopk_segmented(X, ptr=xp, k=5, precision="fast", return_stats=True)
    assert st["fallback_rows"] > 0 or st["overflow_rows"] > 0
    assert_same((idx, val), per_segment(mmf, X, None, xp, xp, k=5, exclude_self=True))
    for s in range(len(sizes)):
        a, b = xp[s], xp[s + 1]
        blk = idx[a:b].cpu()
        assert ((blk >= a) & (blk < b)).all()


@pytest.mark.parametrize("d,k", [(512, 5), (512, 16), (1024, 5)])
def test_whole_result_at_scale(mmf, d, k):
    xp = offsets([4096] * 64)
    X = torch.randn(xp[-1], d, device="cuda")
    idx, val, st = mmf.simtopk_segmented(X, ptr=xp, k=k, return_stats=True)
    assert st["precision_used"] == 2 and st["scan_grid"] > 0
    assert_same((idx, val), per_segment(mmf, X, None, xp, xp, k=k, exclude_self=True))


def test_arguments(mmf):
    X = torch.randn(300, 32, device="cuda")
    xp = [0, 100, 180, 300]
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor([100, 80, 120])).cuda()
    a = mmf.simtopk_segmented(X, ptr=xp, k=4)
    b = mmf.simtopk_segmented(X, batch=batch, k=4)
    assert_same(a, b)
    with pytest.raises(ValueError):
        mmf.simtopk_segmented(X, batch=batch.flip(0), k=4)
    with pytest.raises(ValueError):
        mmf.simtopk_segmented(X, ptr=[0, 100, 299], k=4)
    with pytest.raises(ValueError):
        mmf.simtopk_segmented(X, X[:200], ptr=xp, y_ptr=[0, 200], k=4)
    with pytest.raises(ValueError):
        mmf.simtopk_segmented(X, ptr=xp, k=0)
    with pytest.raises(RuntimeError):
        mmf.simtopk_segmented(X, ptr=xp, k=44)          # k + self = 45
