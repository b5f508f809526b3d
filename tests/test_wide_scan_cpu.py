"""The wide 16-bit scan without a GPU (include/mmf_hg_wide.h): the two host-only queries say what
ops.simtopk(..., precision="fast" | "fast_bf16") covers above a feature dim of 1024, the list capacities are those the
"band <= capacity => never flagged" contract is stated for, the binding registers them in a list of their own, and the
queries of the register-resident scan (the phase API that distributed.py probes) still answer for d <= 1024 only."""
import ctypes
import os
import re
from importlib import import_module

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_wide_scan_supported", "mmf_wide_scan_list_capacity"]


def _ws():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.wide_scan")


@pytest.mark.parametrize("d,want", [(1024, False), (1025, True), (4096, True), (4097, False)])
def test_supported_dims_at_k_plus_self_20_and_21(d, want):
    ws = _ws()
    assert ws.wide_scan_supported(d, 19, True) is want          # k + self = 20
    assert ws.wide_scan_supported(d, 20, False) is want
    assert ws.wide_scan_supported(d, 20, True) is False          # k + self = 21
    assert ws.wide_scan_supported(d, 21, False) is False
    assert ws.wide_scan_supported(d, 0, True) is False


def test_list_capacities():
    ws = _ws()
    assert ws.list_capacity(10, True) >= 16 and ws.list_capacity(11, False) >= 16         # k + self = 11
    assert ws.list_capacity(11, True) >= 32 and ws.list_capacity(12, False) >= 32         # k + self = 12
    assert ws.list_capacity(19, True) >= 32 and ws.list_capacity(20, False) >= 32         # k + self = 20
    assert ws.list_capacity(20, True) == 0 and ws.list_capacity(0, False) == 0            # outside the scan
    for kk in range(1, 21):                                                               # never smaller for a larger k
        assert ws.list_capacity(kk, False) >= ws.list_capacity(max(kk - 1, 1), False) >= 16


def test_register_resident_scan_queries_are_unchanged():
    import multimodal_fusion_amd as mmf
    assert mmf.ops.padded_dim(1536) == 0 and mmf.ops.padded_dim(1025) == 0 and mmf.ops.padded_dim(1024) == 1024
    assert mmf._lib.lib().mmf_fast_scan_supported(1536, 5, 1) == 0
    assert mmf.ops.fast_scan_supported(1536, 5, True) is False and mmf.ops.fast_scan_supported(1024, 5, True) is True


def test_header_library_and_binding():
    import multimodal_fusion_amd as mmf
    with open(os.path.join(ROOT, "include", "mmf_hg_wide.h")) as f:
        h = f.read()
    declared = set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S)))
    assert declared == set(ENTRIES)
    assert '#include "mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    L = ctypes.CDLL(mmf._lib.SO_PATH)
    assert list(mmf._lib.EXPORTS_WIDE) == ENTRIES and all(hasattr(L, e) for e in ENTRIES)
    others = (set(mmf._lib.EXPORTS) | set(mmf._lib.EXPORTS_COHORT) | set(mmf._lib.EXPORTS_POOL) | set(mmf._lib.EXPORTS_STREAM)
              | set(mmf._lib.EXPORTS_TOPK))
    assert not set(ENTRIES) & others
    lib = mmf._lib.lib()
    assert tuple(lib.mmf_wide_scan_supported.argtypes) == (ctypes.c_int64, ctypes.c_int, ctypes.c_int)
    assert tuple(lib.mmf_wide_scan_list_capacity.argtypes) == (ctypes.c_int, ctypes.c_int)
    assert lib.mmf_wide_scan_supported.restype is ctypes.c_int and mmf._lib.ABI_VERSION == 3 and lib.mmf_version() == 3


def test_module_is_exported_and_the_build_lists_the_kernel():
    import importlib.util
    import multimodal_fusion_amd as mmf
    ws = _ws()
    assert "wide_scan" in mmf.__all__ and mmf.wide_scan is ws
    for name in ("wide_scan_supported", "list_capacity"):
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(ws, name)
        assert not hasattr(mmf.ops, name)
    spec = importlib.util.spec_from_file_location("mmf_build_lists_wide", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mmf_scan_b16w.hip" in b.SOURCES and any(h.endswith(os.path.join("include", "mmf_hg_wide.h")) for h in b.HEADERS)
    assert b.EXTRA_FLAGS["mmf_scan_b16w.hip"] == ["-fno-honor-nans"]
