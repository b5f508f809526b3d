"""Segmented device KMeans (mmf_kmeans_fit_segmented) against a loop of the plain entry on each segment's slice, which
test_gpu_kmeans.py pins to scikit-learn and to oracle/kmeans_restate.py: labels, centres, seeds and every info field but the
lockstep iteration count must be equal bit for bit."""
import sys
import warnings
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


def _km():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.kmeans")


def _data(kind, n, d, rng):
    """The generators of test_gpu_kmeans.py::_data."""
    if kind == "gauss":
        return rng.standard_normal((n, d)).astype(np.float32)
    if kind == "blobs":
        c = rng.standard_normal((max(2, n // 40), d)).astype(np.float32) * 2
        return (c[rng.integers(0, len(c), n)] + rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    if kind == "unit":
        x = rng.standard_normal((n, d)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    if kind == "lattice":                        # 20 x 2, duplicate rows: empty clusters, relocation (test_gpu_kmeans.py, seed 27)
        r = np.random.default_rng(27)
        r.choice([20, 30, 50]); r.choice([6, 8, 12])
        x = r.integers(0, 4, (20, 2)).astype(np.float32) + r.standard_normal((20, 2)).astype(np.float32) * float(r.choice([0, 0.01, 0.3]))
        return x
    a = rng.standard_normal((n, 16)).astype(np.float32)
    b = rng.standard_normal((d, 16)).astype(np.float32)
    return np.exp(-0.05 * ((a[:, None, :] - b[None]) ** 2).sum(-1)).astype(np.float32)


def _batch(parts, d, seed):
    rng = np.random.default_rng(seed)
    X = np.concatenate([_data(kind, n, d, rng) for kind, n in parts], 0)
    ptr = np.concatenate([[0], np.cumsum([n for _, n in parts])]).astype(np.int64)
    assert ptr[-1] == len(X)
    return X, ptr


def _compare_with_loop(X, ptr, k):
    """One segmented call against kmeans_fit on every slice; returns the segmented info."""
    import multimodal_fusion_amd as mmf
    km = _km()
    Xg = torch.from_numpy(X).cuda()
    sizes = np.diff(ptr).tolist()
    first, u = km.segment_streams(42, 10, k, sizes)
    labels, centres, info, seeds = mmf.ops.kmeans_fit_segmented(Xg, ptr, k, first, u, return_seeds=True)
    assert labels.shape == (len(X),) and centres.shape == (len(sizes), k, X.shape[1]) and seeds.shape == (len(sizes), 10, k)
    lab, cen, sd = labels.cpu().numpy(), centres.cpu().numpy(), seeds.cpu().numpy()
    for s in range(len(sizes)):
        a, b = int(ptr[s]), int(ptr[s + 1])
        f1, u1 = km.sklearn_stream(42, 10, k, b - a)
        l1, c1, i1, s1 = mmf.ops.kmeans_fit(Xg[a:b], k, f1, u1, return_seeds=True)
        assert np.array_equal(lab[a:b], l1.cpu().numpy()), f"segment {s} ({b - a} rows): labels differ"
        assert np.array_equal(cen[s].view(np.uint32), c1.cpu().numpy().view(np.uint32)), f"segment {s}: centres differ"
        assert np.array_equal(sd[s] - a, s1.cpu().numpy()), f"segment {s}: seeds differ"
        got = dict(info[s])
        ref = dict(i1)
        got.pop("lockstep_iterations"), ref.pop("lockstep_iterations")
        assert got == ref, f"segment {s}: info differs: {got} vs {ref}"
    return info


def test_mixed_generators_and_exact_k_rows():
    X, ptr = _batch([("gauss", 300), ("blobs", 500), ("unit", 64), ("sim", 200), ("gauss", 6), ("blobs", 41)], 48, 1)
    _compare_with_loop(X, ptr, 6)


def test_one_cluster_and_one_row_segments():
    X, ptr = _batch([("gauss", 1), ("gauss", 1), ("blobs", 5), ("unit", 1), ("sim", 40)], 7, 2)
    _compare_with_loop(X, ptr, 1)


def test_relocating_segment_among_others():
    """The lattice segment relocates empty clusters (seed 27 of test_gpu_kmeans.py's relocation test)."""
    X, ptr = _batch([("blobs", 100), ("lattice", 20), ("gauss", 37), ("lattice", 20), ("unit", 64)], 2, 3)
    info = _compare_with_loop(X, ptr, 12)
    import oracle.kmeans_restate as kr
    lat = X[100:120]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from sklearn.cluster import KMeans
        ref = KMeans(n_clusters=12, random_state=42, n_init=10).fit_predict(lat)
    labels, _, _ = _km().kmeans_fit_predict_segmented(torch.from_numpy(X).cuda(), 12, ptr=ptr)
    assert np.array_equal(labels[100:120].cpu().numpy(), ref)
    assert np.array_equal(labels[100:120].cpu().numpy(), kr.kmeans_fit_predict(lat, 12))
    assert len(info) == 5


def test_large_segment_with_64_point_seeding_tiles_next_to_small_ones():
    """33000 rows: 516 tiles of 64 points, so the plain fit seeds on 64-point tiles; the small segments on 32-point ones."""
    X, ptr = _batch([("blobs", 150), ("gauss", 33000), ("unit", 90), ("sim", 700)], 40, 4)
    _compare_with_loop(X, ptr, 9)


@pytest.mark.parametrize("d", [1, 33])
def test_feature_dims_not_a_multiple_of_32(d):
    X, ptr = _batch([("gauss", 300), ("blobs", 120), ("gauss", 40), ("unit", 65)], d, 5 + d)
    _compare_with_loop(X, ptr, 4)


def test_several_groups():
    """40 segments with k = 50: sum of n_init * k = 20000 > 16384, so two lockstep groups."""
    rng = np.random.default_rng(6)
    parts = [(("gauss", "blobs", "unit", "sim")[i % 4], int(rng.integers(50, 130))) for i in range(40)]
    X, ptr = _batch(parts, 16, 6)
    info = _compare_with_loop(X, ptr, 50)
    lock = [i["lockstep_iterations"] for i in info]
    assert len(set(lock[:32])) == 1 and len(set(lock[32:])) == 1      # 32 segments of 500 clusters, then 8


def test_golden_g9_among_smaller_segments():
    """g9 'clustered' (16384 x 512, k = 100) between two smaller segments: scikit-learn's labels of golden G9; the small
    segments give the labels of scikit-learn run here."""
    sys.path.insert(0, GOLDEN)
    from make_g9_kmeans import g9_data
    from sklearn.cluster import KMeans
    g = load_golden("g9_kmeans_scale.npz")
    big = g9_data("clustered")
    rng = np.random.default_rng(9)
    small = [_data("blobs", 700, 512, rng), _data("unit", 300, 512, rng)]
    X = np.concatenate([small[0], big, small[1]], 0)
    ptr = np.array([0, 700, 700 + 16384, len(X)], dtype=np.int64)
    labels, centres, inertia = _km().kmeans_fit_predict_segmented(torch.from_numpy(X).cuda(), 100, ptr=ptr)
    lab = labels.cpu().numpy()
    assert np.array_equal(lab[700:700 + 16384], g["clustered_sklearn_labels"])
    for s, x in ((0, small[0]), (2, small[1])):
        ref = KMeans(n_clusters=100, random_state=42, n_init=10).fit(x)
        assert np.array_equal(lab[ptr[s]:ptr[s + 1]], ref.labels_), f"segment {s}"
    assert centres.shape == (3, 100, 512) and inertia.shape == (3,)


def test_errors():
    km = _km()
    X = torch.randn(100, 8).cuda()
    with pytest.raises(ValueError, match=r"segment 1: n_samples=5 should be >= n_clusters=6"):
        km.kmeans_fit_predict_segmented(X, 6, ptr=[0, 50, 55, 100])
    with pytest.raises(RuntimeError, match="16384"):               # n_init * k = 20000 in one segment
        km.kmeans_fit_predict_segmented(torch.randn(4100, 4).cuda(), 2000, ptr=[0, 2050, 4100])
    with pytest.raises(RuntimeError):
        km.kmeans_fit_predict_segmented(X.cpu(), 3, ptr=[0, 50, 100])
