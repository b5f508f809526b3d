"""Segmented weighted hypergraph without a GPU: the header declares the four entries, the library and the binding export
them, and the batched builders reject bad segments and a missing ratio on the host, before the device check."""
import ctypes
import os
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_sim_dense_combined_segmented", "mmf_offdiag_lower_median_segmented", "mmf_threshold_edges_segmented_count",
           "mmf_threshold_edges_segmented_fill"]


def _wh():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.weighted_hypergraph")


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        h = f.read()
    for name in ENTRIES:
        assert f"int {name}(" in h, name
    assert "#define MMF_ABI_VERSION 3" in h


def test_library_exports_the_entries():
    import multimodal_fusion_amd as mmf
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    for name in ENTRIES:
        assert name in mmf._lib.EXPORTS, name
        assert hasattr(L, name), name
    assert "sim_dense_combined_segmented" in mmf.__all__
    for fn in ("sim_dense_combined_segmented", "offdiag_lower_median_segmented", "threshold_edges_segmented"):
        assert callable(getattr(mmf.ops, fn)), fn


def test_mirror_package_is_unchanged():
    import multimodal_fusion_amd  # noqa: F401
    bh = import_module("multimodal_fusion_amd.build_hypergraph")
    assert "build_weighted_hypergraph_segmented" not in bh.__all__
    assert len(bh.__all__) == 17


@pytest.mark.parametrize("kw,match", [
    (dict(ptr=[0, 5, 9]), "end at 10"),                                                    # not ending at N
    (dict(ptr=[1, 5, 10]), "start at 0"),                                                  # not starting at 0
    (dict(ptr=[0, 6, 4, 10]), "segment 1: ptr decreases"),                                 # decreasing
    (dict(batch=torch.tensor([0, 0, 0, 1, 1, 1, 0, 1, 1, 1])), "sorted"),                  # unsorted
    (dict(batch=torch.tensor([-1, -1, 0, 0, 0, 0, 0, 0, 0, 0])), "non-negative"),          # negative
    (dict(batch=torch.zeros(9, dtype=torch.long)), "one segment id per row"),             # wrong length
    (dict(ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long)), "exactly one"),          # both
    (dict(), "exactly one"),                                                              # neither
    (dict(ptr=[0, 4, 5, 10]), r"segment 1: Number of nodes must be greater than 1, got N=1"),   # a one-row segment
    (dict(ptr=[0, 5, 5, 10]), r"segment 1: .*got N=0"),                                   # an empty segment
    (dict(batch=torch.tensor([0, 0, 0, 0, 0, 2, 2, 2, 2, 2])), r"segment 1: .*got N=0"),  # an id with no rows
])
@pytest.mark.parametrize("fn", ["build_weighted_hypergraph_segmented", "build_hypergraph_data_segmented"])
def test_bad_segments_are_rejected_on_the_host(fn, kw, match):
    F, P = torch.randn(10, 8), torch.rand(10, 2)           # CPU tensors: the checks come before the device check
    with pytest.raises(ValueError, match=match):
        getattr(_wh(), fn)(F, P, 1.0, 1.0, 0.5, **kw)


@pytest.mark.parametrize("fn", ["build_weighted_hypergraph_segmented", "build_hypergraph_data_segmented"])
def test_missing_ratio_is_a_type_error(fn):
    with pytest.raises(TypeError):
        getattr(_wh(), fn)(torch.randn(10, 8), torch.rand(10, 2), ptr=[0, 4, 10])
    with pytest.raises(ValueError):                        # as in the plain mirror, a short graph is reported first
        getattr(_wh(), fn)(torch.randn(10, 8), torch.rand(10, 2), ptr=[0, 1, 10])


def test_positions_must_match_the_rows():
    with pytest.raises(ValueError, match="share N"):
        _wh().build_weighted_hypergraph_segmented(torch.randn(10, 8), torch.rand(9, 2), 1.0, 1.0, 0.5, ptr=[0, 4, 10])


def test_ops_reject_bad_blocks_on_the_host():
    import multimodal_fusion_amd as mmf
    with pytest.raises(ValueError):
        mmf.ops.sim_dense_combined_segmented(torch.randn(10, 8), torch.rand(10, 2), ptr=[0, 4, 9])
    with pytest.raises(ValueError):
        mmf.ops.offdiag_lower_median_segmented(torch.randn(16), ptr=[0, 4, 3])


def test_groups_respect_the_budget():
    g = _wh()._groups([2, 3, 100, 5, 5, 4], 4 * 200)
    assert g == [(0, 2, False), (2, 3, True), (3, 6, False)]
    assert _wh()._groups([10, 10, 10], 4 * 200) == [(0, 2, False), (2, 3, False)]


def test_thresholds_are_f32_ceil():
    from multimodal_fusion_amd.build_hypergraph._common import f32_ceil
    x = np.array([0.1, 1 / 3, 0.0, -0.0, 1e39, -1e39, np.inf, -np.inf, np.nan, 0.7 * 0.5, 3.4028235677973366e38, 1e-46])
    got = _wh().f32_ceil_array(x)
    assert got.dtype == np.float32
    for v, t in zip(x, got):
        ref = f32_ceil(float(v))
        assert (np.isnan(ref) and np.isnan(t)) or (np.float32(ref).view(np.int32) == t.view(np.int32)), (v, t, ref)
