"""The wide 16-bit scan (csrc/mmf_scan_b16w.hip): ops.simtopk(..., precision="fast" | "fast_bf16") for feature
dims 1025 .. 4096 with k + self <= 20.

Data: planted clusters — 30 clusters of 24 rows, row = a * centre + sqrt(1 - a^2) * unit noise with a graded 0.95 .. 0.60 inside
a cluster, normalised.  (Gaussian rows are the wrong input here: at d = 4096 their cosines crowd so much that most rows have more
columns inside the bf16 margin band than a list holds.)  The band of a row — the columns whose 16-bit value G lies within the
row's margin of its (k + self)-th best G — is recomputed here from a small restatement of the operand image and of the margin
formula in the header of mmf_scan_b16w.hip (G in float64), for every metric.

  1. capacity condition: fallback_rows <= (rows whose band exceeds wide_scan.list_capacity), so the exact rescan cannot hide a
     scan that flags everything; ids equal and values bitwise equal to precision="exact" and to the oracle (rbf values: 1e-5);
  2. the shapes where the kernel can go wrong; 3. near ties and crowding (fallback_rows reported, not capped);
  4. many tiles; 5. precision="auto".
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import scan16_restate as R

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PRECISION_USED = {"fast": 2, "fast_bf16": 3}
LAM = 0.5


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def planted_rows(n_clusters, per, d, seed):
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)   # noqa: E731
    centres = unit(rng.standard_normal((n_clusters, 1, d)))
    noise = unit(rng.standard_normal((n_clusters, per, d)))
    a = np.linspace(0.95, 0.60, per)[None, :, None]
    return unit(a * centres + np.sqrt(1.0 - a * a) * noise).reshape(n_clusters * per, d).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted(d, dtype="f32", n_clusters=30, per=24):
    """The rows as a CPU tensor of `dtype` (16-bit rows: the f32 rows rounded once; everything downstream sees those)."""
    return torch.from_numpy(planted_rows(n_clusters, per, d, seed=1000 + d)).to(TORCH_DT[dtype])


@functools.lru_cache(maxsize=None)
def reference(d, dtype, metric, k):
    X = planted(d, dtype)
    return oracle.simtopk(X, metric=metric, lam=LAM, k=k)


# ---- restatement: operand image, margin (header of mmf_scan_b16w.hip), band ----------------------------------------------
def band_sizes(X, metric, operand, kk):
    """Per row: the number of columns j with G_ij >= (kk-th best G_i.) - margin_i, all columns counted (self included)."""
    f = np.float32
    X = np.ascontiguousarray(X.float().numpy(), f)
    d = X.shape[1]
    dp = (d + 127) // 128 * 128
    scal = R.row_scalars(X, metric)
    scale = R.common_scale(float(R.sq_norms(X).max()), metric)
    u = ((X / scal[:, None]).astype(f) if metric == R.COSINE else X) * scale
    u = u.astype(f)
    z = u.astype(np.float16).astype(f) if operand == "f16" else R.bf16_to_f32(R.round_bf16(u))
    z64, u64 = z.astype(np.float64), u.astype(np.float64)
    norm = lambda v: np.sqrt((v * v).sum(axis=1).astype(f)) * R.UP   # noqa: E731
    zn, rn, un = norm(z64), norm((z - u).astype(np.float64)), norm(u64)
    cb = (f(-0.5) * scal * scale * scale).astype(f) if metric in (R.NEG_SQ_L2, R.RBF) else np.zeros(X.shape[0], f)
    ZB, RB, UB, CB = zn.max(), rn.max(), un.max(), np.abs(cb).max()
    g_acc, g_chain = f(dp + 8) * R.EPS24, f(d + 2) * R.EPS24
    e1 = rn * ZB + un * RB + g_acc * (zn * ZB + CB)
    if metric == R.DOT:
        e2 = g_chain * un * UB
    elif metric == R.COSINE:
        e2 = (g_chain + f(4.7683716e-7)) * un * UB * f(1.01)
    else:
        e2 = g_chain * un * UB + f(2.3841858e-7) * (un * un + UB * UB)
    margin = (f(2.0) * (e1 + e2) * f(1.001) + f(1e-30)).astype(np.float64)
    G = cb.astype(np.float64)[None, :] + z64 @ z64.T
    t = -np.partition(-G, kk - 1, axis=1)[:, kk - 1]
    return (G >= (t - margin)[:, None]).sum(axis=1)


def equal_to(got, ref, metric, what):
    idx, val = got[0].cpu().numpy(), got[1].cpu().numpy()
    ridx, rval = ref
    ridx, rval = (ridx.cpu().numpy(), rval.cpu().numpy()) if torch.is_tensor(ridx) else (ridx, rval)
    bad = np.flatnonzero((idx != ridx).any(axis=1))
    assert bad.size == 0, f"{what}: indices differ in rows {bad[:8].tolist()}"
    if metric == "rbf" and what == "oracle":
        assert np.allclose(val, rval, rtol=0, atol=1e-5), f"{what}: scores differ"
    else:
        assert np.array_equal(val.view(np.int32), rval.view(np.int32)), f"{what}: scores differ"


def run_case(mmf, d, dtype, metric, k, precision):
    X = planted(d, dtype).cuda()
    got = mmf.simtopk(X, metric=metric, lam=LAM, k=k, precision=precision, return_stats=True)
    exact = mmf.simtopk(X, metric=metric, lam=LAM, k=k, precision="exact")
    torch.cuda.synchronize()
    st = got[2]
    operand = "f16" if precision == "fast" else "bf16"
    band = band_sizes(planted(d, dtype), metric, operand, k + 1)
    cap = mmf.wide_scan.list_capacity(k, True)
    crowded = int((band > cap).sum())
    print(f"d {d} {dtype} {metric} k {k} {precision}: largest band {int(band.max())} of capacity {cap}, rows beyond it {crowded}, "
          f"fallback_rows {st['fallback_rows']} col_splits {st['col_splits']} scan_grid {st['scan_grid']} candidates {st['candidates']}")
    assert st["precision_used"] == PRECISION_USED[precision] and st["scan_grid"] > 0
    assert st["fallback_rows"] <= crowded
    equal_to(got, exact, metric, "exact")
    equal_to(got, reference(d, dtype, metric, k), metric, "oracle")


# ---- 1. capacity condition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 19])
@pytest.mark.parametrize("d", [1100, 1536, 2560, 4096])
def test_capacity_condition_cosine(mmf, d, k, precision):
    run_case(mmf, d, "f32", "cosine", k, precision)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("k", [5, 19])
@pytest.mark.parametrize("metric", ["dot", "neg_sq_l2", "rbf"])
def test_capacity_condition_other_metrics(mmf, metric, k, precision):
    run_case(mmf, 1536, "f32", metric, k, precision)


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
@pytest.mark.parametrize("dtype,d,metric,k", [("f16", 1100, "cosine", 5), ("bf16", 2560, "cosine", 19), ("f16", 1536, "rbf", 19),
                                              ("bf16", 1536, "neg_sq_l2", 5)])
def test_capacity_condition_16_bit_rows(mmf, dtype, d, metric, k, precision):
    run_case(mmf, d, dtype, metric, k, precision)


# ---- 2. shapes -----------------------------------------------------------------------------------------------------------
def against_oracle(mmf, X, Y, precision="fast", col_splits=0, **kw):
    got = mmf.simtopk(X.cuda(), None if Y is None else Y.cuda(), precision=precision, col_splits=col_splits, return_stats=True, **kw)
    torch.cuda.synchronize()
    st = got[2]
    print(f"n {X.shape[0]} m {(X if Y is None else Y).shape[0]} d {X.shape[1]} {kw}: fallback_rows {st['fallback_rows']} "
          f"col_splits {st['col_splits']} scan_grid {st['scan_grid']}")
    assert st["precision_used"] == PRECISION_USED[precision] and st["scan_grid"] > 0
    equal_to(got, oracle.simtopk(X, Y, **kw), kw.get("metric", "cosine"), "oracle")
    return got


@pytest.mark.parametrize("precision", ["fast", "fast_bf16"])
def test_one_query(mmf, precision):
    X = planted(1100)
    against_oracle(mmf, X[5:6].clone(), X, precision, metric="cosine", k=5, exclude_self=False)
    against_oracle(mmf, X[5:6].clone(), X, precision, metric="neg_sq_l2", k=5, exclude_self=True, row_offset=5)


@pytest.mark.parametrize("m", [6, 127, 128, 129])
def test_few_columns(mmf, m):
    X = planted(1100)[:m].clone()
    against_oracle(mmf, X, None, metric="cosine", k=5)                      # m = 6: k + 1 columns, every other row is a neighbour
    against_oracle(mmf, planted(1100)[200:329].clone(), X, metric="dot", k=min(5, m), exclude_self=False)


def test_129_queries_and_one_k_beyond_a_chunk(mmf):
    X = planted_rows(30, 24, 1025, seed=7)                                   # d = 1025: one real k in the last chunk's padding
    X = torch.from_numpy(X)
    against_oracle(mmf, X[:129].clone(), None, metric="cosine", k=5)
    for precision in ("fast", "fast_bf16"):
        against_oracle(mmf, X, None, precision, metric="cosine", k=5)
        against_oracle(mmf, X, None, precision, metric="rbf", lam=LAM, k=5)
    Xs = X.clone()
    Xs[:, 1024] *= 40.0                                                      # the last k carries most of every row: dropping it shows
    against_oracle(mmf, Xs, None, metric="neg_sq_l2", k=5)


@pytest.mark.parametrize("k", [1, 19])
def test_smallest_and_largest_k(mmf, k):
    for precision in ("fast", "fast_bf16"):
        against_oracle(mmf, planted(1536), None, precision, metric="cosine", k=k)


def test_separate_candidates_offsets_and_self_by_identity(mmf):
    Y = planted(1536)
    Xc = Y[100:229].clone()
    for metric in ("cosine", "neg_sq_l2"):
        a = against_oracle(mmf, Xc, Y, metric=metric, k=5, exclude_self=True, row_offset=1100, col_offset=1000)   # self: column 100 + i
        b = against_oracle(mmf, Xc, Y, metric=metric, k=5, exclude_self=True, row_offset=0, col_offset=5000)      # no id matches
        assert (a[0].cpu() - 1000 == torch.arange(100, 229)[:, None]).sum() == 0
        assert (b[0].cpu()[:, 0] - 5000 == torch.arange(100, 229)).all()      # nothing excluded: every row finds itself first
    # the queries as a row slice of the candidates (one operand image serves both sides)
    Yg = Y.cuda()
    got = mmf.simtopk(Yg[128:257], Yg, metric="cosine", k=5, exclude_self=True, row_offset=128, precision="fast", return_stats=True)
    torch.cuda.synchronize()
    assert got[2]["precision_used"] == 2
    equal_to(got, oracle.simtopk(Y[128:257], Y, metric="cosine", k=5, exclude_self=True, row_offset=128), "cosine", "oracle")


@pytest.mark.parametrize("k", [5, 19])
def test_column_splits_give_the_same_bits(mmf, k):
    X = planted(1536).cuda()
    ref = reference(1536, "f32", "cosine", k)
    for precision in ("fast", "fast_bf16"):
        for splits in (1, 2, 8):
            got = mmf.simtopk(X, metric="cosine", lam=LAM, k=k, precision=precision, col_splits=splits, return_stats=True)
            torch.cuda.synchronize()
            print(f"k {k} {precision} col_splits {splits}: used {got[2]['col_splits']} fallback_rows {got[2]['fallback_rows']}")
            assert got[2]["col_splits"] == min(splits, 4)       # 720 columns are six tiles of 128: at most four ranges
            assert got[2]["fallback_rows"] == 0                  # the bands fit (test 1) whatever the split
            equal_to(got, ref, "cosine", "oracle")


# ---- 3. near ties and crowding -------------------------------------------------------------------------------------------
def test_exact_copies_tight_cluster_and_equal_images(mmf):
    base = planted(1536)
    rng = np.random.default_rng(5)
    copies = torch.cat([base[:10].repeat(60, 1), base[600:]])                # 60 exact copies of 10 rows
    tight = base.clone()
    tight[100:200] = tight[100] + 1e-4 * torch.from_numpy(rng.standard_normal((100, 1536)).astype(np.float32))
    pairs = base.clone()                                                       # rows 2 i + 1: row 2 i with eight elements one f32 ulp up
    cols = torch.from_numpy(rng.integers(0, 1536, size=(360, 8)))
    twin = pairs[0::2].clone()
    twin.scatter_(1, cols, torch.nextafter(twin.gather(1, cols), torch.full((360, 8), 2.0)))
    pairs[1::2] = twin
    z = lambda x: (x / x.norm(dim=1, keepdim=True) * 256).to(torch.float16)   # noqa: E731
    same = (z(pairs[0::2]) == z(pairs[1::2])).all(dim=1) & (pairs[0::2] != pairs[1::2]).any(dim=1)
    assert same.sum() > 180, "the pairs are meant to share their 16-bit image"
    for name, X in (("copies", copies), ("tight", tight), ("pairs", pairs)):
        for precision in ("fast", "fast_bf16"):
            for k in (5, 19):
                print(name, end=" ")
                against_oracle(mmf, X, None, precision, metric="cosine", k=k)
                against_oracle(mmf, X, None, precision, 1, metric="cosine", k=k)      # one column range: the fullest lists
        against_oracle(mmf, X, None, metric="rbf", lam=LAM, k=5)


# ---- 4. many tiles ---------------------------------------------------------------------------------------------------------
def test_many_tiles(mmf):
    X = torch.from_numpy(planted_rows(256, 32, 1536, seed=11)).cuda()          # N = 8192: 64 row blocks x 64 column tiles
    exact = mmf.simtopk(X, metric="cosine", k=5, precision="exact")
    for precision in ("fast", "fast_bf16"):
        got = mmf.simtopk(X, metric="cosine", k=5, precision=precision, return_stats=True)
        torch.cuda.synchronize()
        print(f"N 8192 {precision}: fallback_rows {got[2]['fallback_rows']} col_splits {got[2]['col_splits']} candidates {got[2]['candidates']}")
        assert got[2]["precision_used"] == PRECISION_USED[precision]
        equal_to(got, exact, "cosine", "exact")


# ---- 5. auto ---------------------------------------------------------------------------------------------------------------
def test_auto_gives_the_exact_bits(mmf):
    X = planted(1536).cuda()
    got = mmf.simtopk(X, metric="cosine", k=5, precision="auto", return_stats=True)
    exact = mmf.simtopk(X, metric="cosine", k=5, precision="exact")
    torch.cuda.synchronize()
    assert got[2]["precision_used"] in (1, 2)
    equal_to(got, exact, "cosine", "exact")


# ---- what stays refused ------------------------------------------------------------------------------------------------------
def test_refusals_keep_their_text(mmf):
    X = planted(1536).cuda()
    with pytest.raises(RuntimeError, match="does not support"):
        mmf.simtopk(X, metric="cosine", k=20, precision="fast")                # k + self = 21
    with pytest.raises(RuntimeError, match="does not support"):
        mmf.simtopk(torch.zeros(64, 4097).cuda(), metric="dot", k=5, precision="fast_bf16")
    with pytest.raises(RuntimeError, match="does not support"):               # the segmented entry has no wide scan
        mmf.simtopk_segmented(X, ptr=[0, 360, 720], metric="cosine", k=5, precision="fast")
    assert mmf.wide_scan.wide_scan_supported(1536, 19) and not mmf.ops.fast_scan_supported(1536, 5)
