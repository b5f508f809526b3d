"""The wide scan's overflow lists, what can be checked without a GPU: the Python mirror of the slot count, the
per-call switch, the documents, and the band conditions that tests/test_gpu_wide_overflow.py assumes of its inputs — recomputed
with the restatement of tests/test_gpu_wide_scan.py.  If an input changes, the last tests say which GPU assertion lost its footing.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal-fusion_amd", "csrc")

METRICS = ("dot", "cosine", "neg_sq_l2", "rbf")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_overflow_slots_mirror_the_library():
    import multimodal_fusion_amd as mmf
    api = _read(CSRC, "mmf_api.hip")
    m = re.findall(r"static constexpr int kSpillCap = (\d+);", api)
    assert len(m) == 1
    assert mmf.wide_scan.OVERFLOW_SLOTS == 192 == int(m[0])
    assert "OVERFLOW_SLOTS" in mmf.wide_scan.__doc__ and "MMF_WIDE_SINK" in mmf.wide_scan.__doc__


def test_the_switch_is_read_per_call():
    api = _read(CSRC, "mmf_api.hip")
    uses = [ln for ln in api.splitlines() if 'getenv("MMF_WIDE_SINK")' in ln]
    assert len(uses) == 1 and "static" not in uses[0], uses
    body = api.split("static bool wide_sink_mode() {", 1)[1].split("\n}\n", 1)[0]
    assert 'getenv("MMF_WIDE_SINK")' in body and "static" not in body
    run = api.split("int run(const Request& r, const FastOperands& fo_in, void* select_wait_event) {", 1)[1]
    assert "wide_sink_mode()" in run.split("launch_scan_b16_audit", 1)[0]          # asked where the launch is made
    # the segmented launcher passes no sink, the plain one takes it from the lists
    scan = _read(CSRC, "mmf_scan_b16w.hip")
    seg = scan.split("int launch_scan_b16w_seg(", 1)[1]
    assert "spill" not in seg
    plain = scan.split("int launch_scan_b16w(", 1)[1].split("int launch_scan_b16w_seg(", 1)[0]
    for word in ("L.spill_cnt", "L.spill_ids", "L.spill_cap", "L.spill_stacks", "launch_b16w_t<W_CAP_SMALL, false, true>"):
        assert word in plain, word


def test_documents_name_the_feature_the_switch_and_the_timing_file():
    design = _read(ROOT, "DESIGN.md")
    sec = design.split("### 4.21", 1)[1]
    for words in ("overflow", "MMF_WIDE_SINK", "profiles/wide_overflow_timing.txt", "SpillSink", "tband", "Resources", "Measurements"):
        assert words in sec, words
    cut = design.split("### 4.15", 1)[1].split("### 4.16", 1)[0]
    assert "No overflow lists" not in cut
    readme = _read(ROOT, "README.md")
    for words in ("MMF_WIDE_SINK", "profiles/wide_overflow_timing.txt", "4096"):
        assert words in readme, words
    assert "wide_overflow_timing.py" in _read(ROOT, "scripts", "README.md")
    assert os.path.exists(os.path.join(ROOT, "scripts", "wide_overflow_timing.py"))


# ---- the band conditions of the GPU cases ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1100, 1536])
def test_near_identical_rows_have_every_column_in_their_band(d):
    """Cases (a) and (b): 160 / 400 rows within 1e-4 of one row — every row's band is all the columns."""
    from oracle import scan16_restate as R
    from test_gpu_wide_overflow import near_identical
    from test_gpu_wide_scan import band_sizes
    codes = {"dot": R.DOT, "cosine": R.COSINE, "neg_sq_l2": R.NEG_SQ_L2, "rbf": R.RBF}
    for m in (160, 400):
        X = near_identical(m, d)
        for metric in METRICS:
            for operand in ("f16", "bf16"):
                for kk in (6, 16):
                    band = band_sizes(X, codes[metric], operand, kk)
                    assert (band == m).all(), (m, d, metric, operand, kk, int(band.min()))


def test_near_identical_f16_rows_have_every_column_in_their_band():
    """Case (a) also runs on f16 input rows (the f32 rows rounded once)."""
    import torch
    from oracle import scan16_restate as R
    from test_gpu_wide_overflow import near_identical
    from test_gpu_wide_scan import band_sizes
    X = near_identical(160, 1100).to(torch.float16)
    for metric in (R.COSINE, R.NEG_SQ_L2):
        for operand in ("f16", "bf16"):
            for kk in (6, 16):
                assert (band_sizes(X, metric, operand, kk) == 160).all(), (metric, operand, kk)


def test_tight_rows_fit_lists_and_overflow_slots():
    """Case (c): the cluster rows have band 100, every other row at most 104 — inside one list pair + the overflow slots."""
    from oracle import scan16_restate as R
    from test_gpu_wide_overflow import OVERFLOW_SLOTS, tight_rows
    from test_gpu_wide_scan import band_sizes
    X = tight_rows()
    for metric in (R.DOT, R.COSINE, R.NEG_SQ_L2, R.RBF):
        for operand in ("f16", "bf16"):
            for kk in (6, 16):
                band = band_sizes(X, metric, operand, kk)
                assert (band[100:200] == 100).all(), (metric, operand, kk, int(band[100:200].min()), int(band[100:200].max()))
                assert band.max() <= 104 <= OVERFLOW_SLOTS, (metric, operand, kk, int(band.max()))


def test_pigeonhole_of_case_b():
    import multimodal_fusion_amd as mmf
    for k, cap in ((5, 16), (15, 32)):
        assert mmf.wide_scan.list_capacity(k, True) == cap
        for splits in (1, 2):
            assert 400 > 2 * splits * cap + mmf.wide_scan.OVERFLOW_SLOTS
