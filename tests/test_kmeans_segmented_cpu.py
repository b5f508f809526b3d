"""Segmented KMeans without a GPU: the header declares the entry, the library exports it, bad segments are rejected on the
host before the device is touched, and the random stream is drawn once with per-segment first centres."""
import ctypes
import os
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _km():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.kmeans")


def test_header_declares_the_entry():
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        h = f.read()
    assert "int mmf_kmeans_fit_segmented(" in h
    assert "#define MMF_ABI_VERSION 3" in h


def test_library_exports_the_entry():
    import multimodal_fusion_amd as mmf
    assert "mmf_kmeans_fit_segmented" in mmf._lib.EXPORTS
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert hasattr(L, "mmf_kmeans_fit_segmented")
    assert callable(mmf.ops.kmeans_fit_segmented)


@pytest.mark.parametrize("kw,match", [
    (dict(batch=torch.tensor([0, 0, 0, 1, 1, 1, 0, 1, 1, 1])), "sorted"),                  # unsorted
    (dict(batch=torch.tensor([-1, -1, -1, 0, 0, 0, 0, 0, 0, 0])), "non-negative"),         # negative
    (dict(batch=torch.zeros(9, dtype=torch.long)), "one segment id per row"),             # wrong length
    (dict(ptr=[0, 5, 9]), "end at 10"),                                                   # not ending at n
    (dict(ptr=[0, 6, 4, 10]), "segment 1: ptr decreases"),                                # decreasing
    (dict(ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long)), "exactly one"),          # both
    (dict(), "exactly one"),                                                              # neither
    (dict(ptr=[0, 5, 5, 10]), r"segment 1: n_samples=0 should be >= n_clusters=3"),        # empty segment
    (dict(ptr=[0, 2, 10]), r"segment 0: n_samples=2 should be >= n_clusters=3"),           # shorter than k
    (dict(batch=torch.tensor([0, 0, 0, 0, 0, 0, 0, 0, 2, 2])), r"segment 1: n_samples=0"),  # an id with no rows
])
def test_bad_segments_are_rejected_on_the_host(kw, match):
    X = torch.randn(10, 8)                       # a CPU tensor: the segment checks come before the device check
    with pytest.raises(ValueError, match=match):
        _km().kmeans_fit_predict_segmented(X, 3, **kw)


def test_valid_segments_on_a_cpu_tensor_need_the_device():
    with pytest.raises(RuntimeError):
        _km().kmeans_fit_predict_segmented(torch.randn(10, 8), 3, ptr=[0, 4, 10])


def test_segmented_labels_check_the_sizes_before_the_device(monkeypatch):
    """The one backend dispatch of the cohort steps: with the default 'device' backend and no GPU, a short segment is the
    ValueError scikit-learn would raise, and only sizes that pass reach the device check."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    km, X = _km(), torch.randn(10, 8)
    with pytest.raises(ValueError, match=r"segment 1: n_samples=2 should be >= n_clusters=3\."):
        km.segmented_labels(X, torch.tensor([0, 8, 10]), 3)
    with pytest.raises(ValueError, match=r"segment 0: n_samples=4 should be >= n_clusters=0\."):
        km.segmented_labels(X, [0, 4, 10], 0)
    for p in (torch.tensor([0, 4, 10]), [0, 4, 10]):
        with pytest.raises(RuntimeError, match="ROCm"):
            km.segmented_labels(X, p, 3)


@pytest.mark.parametrize("k", [1, 3, 10, 100])
def test_stream_is_drawn_once_with_per_segment_first_centres(k):
    km = _km()
    sizes = [k, 7 * k + 3, 16384, 1000, k + 1]
    first, u = km.segment_streams(42, 10, k, sizes)
    assert first.shape == (len(sizes), 10) and first.dtype == np.int64
    for s, n_s in enumerate(sizes):
        f1, u1 = km.sklearn_stream(42, 10, k, n_s)
        assert np.array_equal(first[s], f1), s
        assert np.array_equal(u, u1), s
