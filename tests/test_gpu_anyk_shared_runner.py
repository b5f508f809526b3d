"""The narrow and the wide any-k entries share one runner each (segmented_anyk_run, cross_anyk_run in mmf_api.hip: `wide = d > 1024`
chooses the sizes, the id scratch and the launches), so both carve the same cached workspace of their device and stream.  Here they
run one after the other on ONE stream — segmented narrow, wide, narrow again, then cross-segment narrow, wide, narrow again — so
that each call finds the workspace as the other path sized and left it.

The reference is always the exact entry on the same inputs (``segmented_exact.simtopk_segmented_exact``, and the cross-segment
router with precision="exact"), compared bit for bit, ids and values; a repeated narrow call also reports the passes, yields and
rescanned rows of its first run.  The shapes are the smallest that take two passes on both paths: a pass is 44 entries deep at
d <= 512 and 20 above it (k = 50 at d = 64, k = 30 at d = 1100)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg  # noqa: E402
from test_gpu_segmented import assert_same  # noqa: E402
from test_segmented_anyk_cpu import offsets  # noqa: E402

pytestmark = pytest.mark.gpu

DN, KN = 64, 50                        # narrow
DW, KW = 1100, 30                      # wide
SEG_SIZES = [0, 25, 280, 295]          # empty; short of k admissible columns on both paths (the -1 / -inf fill); two served
CROSS_SIZES = [170, 130, 90, 210]      # every segment has at least k columns outside itself


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def rows(seed, n, d):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, d).astype(np.float32)).cuda()


def record(info):
    return info["passes"], info["yield"], info["exact_rows"]


def check_info(info, k):
    assert info["passes"] >= 2 and sum(info["yield"]) == k and all(y >= 1 for y in info["yield"]), info


@pytest.mark.parametrize("exclude_self", [True, False])
def test_narrow_wide_narrow_on_one_stream(mmf, exclude_self):
    ptr, cptr = offsets(SEG_SIZES), offsets(CROSS_SIZES)
    Xn, Xw = rows(41, sum(SEG_SIZES), DN), rows(43, sum(SEG_SIZES), DW)
    Cn, Cw = rows(47, sum(CROSS_SIZES), DN), rows(53, sum(CROSS_SIZES), DW)
    seg_n = dict(ptr=ptr, metric="cosine", k=KN, exclude_self=exclude_self)
    seg_w = dict(ptr=ptr, metric="cosine", k=KW, exclude_self=exclude_self)
    cross_n = dict(ptr=cptr, metric="cosine", k=KN)
    cross_w = dict(ptr=cptr, metric="cosine", k=KW)
    seg_exact, cross_router = mmf.segmented_exact.simtopk_segmented_exact, mmf.cross_segments_wide_anyk.simtopk_cross_segments
    refs = [seg_exact(Xn, **seg_n), seg_exact(Xw, **seg_w), cross_router(Cn, precision="exact", **cross_n),
            cross_router(Cw, precision="exact", **cross_w)]
    calls = [(lambda: mmf.simtopk_segmented_fast_any_k(Xn, return_info=True, **seg_n), 0, KN),
             (lambda: mmf.simtopk_segmented_wide_any_k(Xw, return_info=True, **seg_w), 1, KW),
             (lambda: mmf.simtopk_segmented_fast_any_k(Xn, return_info=True, **seg_n), 0, KN),
             (lambda: mmf.simtopk_cross_segments_fast_any_k(Cn, return_info=True, **cross_n), 2, KN),
             (lambda: mmf.simtopk_cross_segments_wide_any_k(Cw, return_info=True, **cross_w), 3, KW),
             (lambda: mmf.simtopk_cross_segments_fast_any_k(Cn, return_info=True, **cross_n), 2, KN)]
    stream, _ = sg.streams()       # the process's side stream: a stream of its own would take a hardware queue from the gate tests
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = [fn() for fn, _, _ in calls]
    stream.synchronize()
    for step, ((idx, val, info), (_, ref, k)) in enumerate(zip(got, calls)):
        print(f"call {step + 1}: {info}")
        assert_same((idx, val), refs[ref])
        check_info(info, k)
    assert record(got[0][2]) == record(got[2][2]), (got[0][2], got[2][2])
    assert record(got[3][2]) == record(got[5][2]), (got[3][2], got[5][2])
    # the short segment of the segmented cohort: its admissible columns, then the fill
    lo, hi, adm = int(ptr[1]), int(ptr[2]), SEG_SIZES[1] - (1 if exclude_self else 0)
    for idx in (got[0][0], got[1][0]):
        assert bool((idx[lo:hi, :adm] >= 0).all()) and bool((idx[lo:hi, adm:] == -1).all())
