"""Segmented simtopk without a GPU: the library exports the entry, the header declares it, and the Python front end rejects
bad segment offsets before it touches a device."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry():
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        h = f.read()
    assert "int mmf_simtopk_segmented(" in h
    assert "#define MMF_ABI_VERSION 3" in h


def test_library_exports_the_entry():
    import multimodal_fusion_amd as mmf
    assert "mmf_simtopk_segmented" in mmf._lib.EXPORTS
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert hasattr(L, "mmf_simtopk_segmented")
    assert "simtopk_segmented" in mmf.__all__


@pytest.mark.parametrize("kw", [dict(ptr=[0, 5, 9]), dict(ptr=[1, 5, 10]), dict(ptr=[0, 6, 5, 10]),
                                dict(batch=torch.tensor([0, 0, 1, 0, 1, 1, 1, 1, 1, 1])),
                                dict(batch=torch.tensor([-1, 0, 0, 0, 0, 0, 0, 0, 0, 0])), dict(batch=torch.zeros(9, dtype=torch.long)),
                                dict(), dict(ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long)), dict(ptr=[0, 10], k=0),
                                dict(ptr=[0, 10], y_ptr=[0, 10])])
def test_bad_arguments_are_rejected_on_the_host(kw):
    import multimodal_fusion_amd as mmf
    X = torch.randn(10, 8)                       # a CPU tensor: validation must fail before the device check
    with pytest.raises(ValueError):
        mmf.simtopk_segmented(X, **kw)


def test_mismatched_segment_counts():
    import multimodal_fusion_amd as mmf
    with pytest.raises(ValueError):
        mmf.simtopk_segmented(torch.randn(10, 8), torch.randn(6, 8), ptr=[0, 4, 10], y_ptr=[0, 6])
