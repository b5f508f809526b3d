"""The 16-bit top-k of the combined similarity without a GPU (mmf_simtopk_combined_fast, include/mmf_hg_topk16.h, DESIGN.md
§4.17): the header declares exactly the one entry, the library exports it and the binding registers it in a list of its own,
the entry runs its host checks before any device call and names the argument, the Python wrapper raises its argument errors on
the host, the static stream scan reads the new kernel file and driver, the documents name the feature, and the margin of
mmf_scan_b16c.hip — restated in tests/combined16_restate.py — holds on the worst-case rounding rows of tests/adversarial16.py."""
import ctypes
import inspect
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mmf_simtopk_combined_fast"]
OTHER_HEADERS = ["mmf_hg.h", "mmf_hg_pool.h", "mmf_hg_stream.h", "mmf_hg_topk.h", "mmf_hg_wide.h", "mmf_hg_wide_seg.h"]


def _ct16():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk16")


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding ----------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_and_no_other_header_does():
    assert _declared("mmf_hg_topk16.h") == set(ENTRIES)
    assert sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h")) == sorted(OTHER_HEADERS + ["mmf_hg_topk16.h"])
    for h in OTHER_HEADERS:
        assert not _declared(h) & set(ENTRIES), h
    with open(os.path.join(ROOT, "include", "mmf_hg_topk16.h")) as f:
        h = f.read()
    assert '#include "mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    for words in ("key_ij = eh + eg", "val_ij = expf(eh) * expf(eg)", "column id ascending", "id -1 and value -inf", "bit for bit",
                  "k + self <= 20", "1 <= d <= 4096", "dp <= 8", "MMF_PREC_FAST_BF16", "Host-synchronous"):
        assert words in h, words
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()                  # additions only


def test_library_and_binding_export_the_entry_from_a_list_of_its_own():
    import multimodal_fusion_amd as mmf
    lb = mmf._lib
    L = ctypes.CDLL(lb.SO_PATH)
    assert list(lb.EXPORTS_TOPK16) == ENTRIES and hasattr(L, ENTRIES[0])
    others = (set(lb.EXPORTS) | set(lb.EXPORTS_COHORT) | set(lb.EXPORTS_POOL) | set(lb.EXPORTS_STREAM) | set(lb.EXPORTS_TOPK)
              | set(lb.EXPORTS_WIDE) | set(lb.EXPORTS_WIDE_SEG))
    assert not set(ENTRIES) & others
    fn = lb.lib().mmf_simtopk_combined_fast
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17 and tuple(fn.argtypes[-2:]) == (ctypes.c_int, ctypes.c_void_p)
    assert list(fn.argtypes) == list(lb.lib().mmf_simtopk_combined.argtypes)       # the two can be swapped
    assert lb.ABI_VERSION == 3 and lb.lib().mmf_version() == 3


def test_build_lists_the_new_source_and_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_topk16", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mmf_scan_b16c.hip" in b.SOURCES and any(h.endswith(os.path.join("include", "mmf_hg_topk16.h")) for h in b.HEADERS)
    assert "mmf_scan_b16c.hip" not in b.EXTRA_FLAGS                     # a = 0 meets -inf in this kernel: NaNs are honoured


def test_module_and_functions_are_exported():
    import multimodal_fusion_amd as mmf
    m = _ct16()
    assert "combined_topk16" in mmf.__all__ and mmf.combined_topk16 is m
    names = {"simtopk_combined_fast", "build_topk_weighted_hypergraph_fast"}
    for name in names:
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
        assert not hasattr(mmf.ops, name) and not hasattr(mmf.combined_topk, name)
    public = {n for n, fn in inspect.getmembers(m, inspect.isfunction) if fn.__module__ == m.__name__ and not n.startswith("_")}
    assert public == names
    sig = inspect.signature(m.simtopk_combined_fast)
    assert list(sig.parameters) == ["features", "positions", "lambda_h", "lambda_g", "k", "exclude_self", "precision", "col_splits",
                                    "return_stats", "profile"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [1.0, 1.0, 5, True, "auto", 0, False, False]
    sig = inspect.signature(m.build_topk_weighted_hypergraph_fast)
    assert list(sig.parameters) == ["features", "positions", "lambda_h", "lambda_g", "k", "device", "precision"]
    assert sig.parameters["precision"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["precision"].default == "auto"


# ---- the entry's host checks, with host buffers standing in for device pointers ------------------------------------------
def _call(**kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(F=b, P=b, n=4, d=4, dp=2, lh=1.0, lg=1.0, k=2, self=1, ptr=None, S=0, idx=b, val=b, opts=(2, 0, 0, 0, None), device=63)
    a.update(kw)
    ptr = a["ptr"]
    if ptr is not None:
        ptr = ctypes.cast((ctypes.c_int64 * len(ptr))(*ptr), ctypes.c_void_p)
    opts = a["opts"]
    if opts is not None:
        opts = ctypes.byref(mmf._lib.SimtopkOpts(*opts))
    rc = L.mmf_simtopk_combined_fast(a["F"], a["P"], a["n"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], ptr, a["S"], a["idx"],
                                     a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


INVALID = [
    (dict(F=None), "F is NULL"),
    (dict(P=None), "P is NULL"),
    (dict(idx=None), "out_idx is NULL"),
    (dict(val=None), "out_val is NULL"),
    (dict(n=-1), "n must be >= 0"),
    (dict(d=0), "d must be at least 1"),
    (dict(dp=0), "dp must be at least 1"),
    (dict(k=0), "k must be at least 1"),
    (dict(lh=-0.5), "lambda_h must be finite and >= 0"),
    (dict(lh=float("inf")), "lambda_h must be finite and >= 0"),
    (dict(lg=-1.0), "lambda_g must be finite and >= 0"),
    (dict(lg=float("nan")), "lambda_g must be finite and >= 0"),
    (dict(opts=(7, 0, 0, 0, None)), "precision 7"),
    (dict(opts=(2, 0, -1, 0, None)), "col_splits must be >= 0"),
]
UNSUPPORTED = [
    (dict(ptr=[0, 4], S=1), "stays on mmf_simtopk_combined"),
    (dict(ptr=[0, 2, 4], S=2), "stays on mmf_simtopk_combined"),
    (dict(ptr=None, S=2), "stays on mmf_simtopk_combined"),
    (dict(dp=9), "dp = 9 > 8"),
    (dict(k=20), "k + self = 21 > 20"),
    (dict(k=21, self=0), "k + self = 21 > 20"),
    (dict(d=4097), "d = 4097 > 4096"),
    (dict(n=1 << 31), "n must be < 2^31"),
]


@pytest.mark.parametrize("kw,words", INVALID)
def test_entry_refuses_bad_arguments_before_any_device_call(kw, words):
    """A device id that does not exist: an argument error must win over the device's."""
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and "simtopk_combined_fast" in msg, (rc, msg)


@pytest.mark.parametrize("kw,words", UNSUPPORTED)
def test_entry_refuses_what_it_does_not_support_before_any_device_call(kw, words):
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and words in msg and "simtopk_combined_fast" in msg, (rc, msg)


def test_entry_refuses_a_negative_device_first():
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(k=0), dict(F=None), dict(dp=9), dict(ptr=[0, 4], S=1), dict(d=4097)):
        rc, msg = _call(device=-1, **kw)
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and "no CPU path" in msg and "simtopk_combined_fast" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_rows_are_a_no_op():
    """Every precision, zero lambdas, the limits themselves: the call gets as far as the device (which is not there).  n == 0
    returns before it."""
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(opts=None), dict(opts=(0, 0, 0, 0, None)), dict(opts=(1, 0, 0, 0, None)), dict(opts=(3, 1, 4, 0, None)),
               dict(lh=0.0, lg=0.0), dict(k=19), dict(k=20, self=0), dict(dp=8), dict(d=4096), dict(n=1)):
        rc, msg = _call(**kw)
        assert rc == mmf._lib.MMF_E_HIP, (kw, rc, msg)
    assert _call(n=0)[0] == mmf._lib.MMF_OK and _call(n=0, F=None, P=None, idx=None, val=None)[0] == mmf._lib.MMF_OK


def test_the_exact_entry_still_refuses_the_fast_precisions():
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    b = ctypes.cast((ctypes.c_int64 * 64)(), ctypes.c_void_p)
    opts = mmf._lib.SimtopkOpts(2, 0, 0, 0, None)
    rc = L.mmf_simtopk_combined(b, b, 4, 4, 2, 1.0, 1.0, 2, 1, None, 0, b, b, ctypes.byref(opts), None, 63, None)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and "precision 2" in L.mmf_last_error().decode()


# ---- the wrapper's argument errors, on the host ---------------------------------------------------------------------
def test_wrapper_rejects_bad_input_before_any_library_call(monkeypatch):
    import multimodal_fusion_amd as mmf
    m = _ct16()

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    for f in (m.simtopk_combined_fast, m.build_topk_weighted_hypergraph_fast):
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:9])
        with pytest.raises(ValueError, match="must share N"):
            f(F, P[:, 0])
        with pytest.raises(ValueError, match=r"k must be >= 1 \(got 0\)"):
            f(F, P, k=0)
        with pytest.raises(ValueError, match="unknown precision 'half'"):
            f(F, P, precision="half")


def test_without_a_gpu_the_wrapper_raises(monkeypatch):
    m = _ct16()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    for f in (m.simtopk_combined_fast, m.build_topk_weighted_hypergraph_fast):
        with pytest.raises(RuntimeError, match="ROCm"):
            f(F, P)


# ---- static stream scan ------------------------------------------------------------------------------------------------
def test_new_kernels_are_launched_on_the_callers_stream_and_nothing_blocks():
    from test_stream_arguments_cpu import BLOCKING, enclosing, is_null, sources, stream_uses
    uses = [u for u in stream_uses() if u[0] == "mmf_scan_b16c.hip"]
    launched = " ".join(a[0] for _, _, what, _, a in uses if what == "hipLaunchKernelGGL")
    assert "kern" in launched and "comb_seed_union_kernel" in launched
    assert len(uses) >= 2 and not [u for u in uses if is_null(u[3])]
    text = dict(sources())["mmf_scan_b16c.hip"]
    for inst in ("scan_b16c_kernel<true, CAP>", "scan_b16c_kernel<false, CAP>", "launch_b16c_t<C_CAP_SMALL>", "launch_b16c_t<C_CAP_BIG>"):
        assert inst in text, inst
    assert not [m for m in BLOCKING.finditer(text) if not m.group(1).endswith("Async")]
    # the driver: every runtime call of run_simtopk_combined_fast is asynchronous and names the call's stream
    api = dict(sources())["mmf_api.hip"]
    body = api.split("int run_simtopk_combined_fast(", 1)[1].split("\n}\n", 1)[0]
    assert not [m for m in BLOCKING.finditer(body) if not m.group(1).endswith("Async")]
    assert body.count("hipStreamSynchronize(s)") == 1 and "launch_scan_b16c(" in body and "launch_rerank_combined(" in body
    assert "launch_scan_b16_audit(" in body and "MMF_DEBUG_FLAG_ROWS" in open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")).read().split("int run_simtopk_combined_fast(", 1)[1].split("\n}\n", 1)[0]
    mine = [u for u in stream_uses() if u[0] == "mmf_api.hip" and enclosing(api, _offset(api, u[1])) == "run_simtopk_combined_fast"]
    assert len(mine) >= 6 and all(u[3] == "s" for u in mine), mine


def _offset(text, line):
    return sum(len(x) + 1 for x in text.split("\n")[:line - 1])


def test_the_pinned_files_are_not_edited():
    """The new scan copies the wide kernel's structure: the files it was copied from do not name it."""
    csrc = os.path.join(ROOT, "multimodal-fusion_amd", "csrc")
    for name in ("mmf_scan_b16w.hip", "mmf_scan_bf16.hip", "mmf_scan_f32.hip", "mmf_select.hip", "mmf_topk.hip", "mmf_prep.hip"):
        with open(os.path.join(csrc, name)) as f:
            src = f.read()
        assert "b16c" not in src and "combined_fast" not in src, name


# ---- documents -------------------------------------------------------------------------------------------------------
def _topk16_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*16-bit top-k entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_table_equals_the_gpu_tests_table():
    from test_gpu_simtopk_combined_fast import SYNC_TOPK16
    import multimodal_fusion_amd as mmf
    rows = _topk16_table()
    assert rows == SYNC_TOPK16 == {"mmf_simtopk_combined_fast": ("data-dependent", "no host arguments")}, (rows, SYNC_TOPK16)
    assert set(rows) == set(mmf._lib.EXPORTS_TOPK16)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert text.index("Top-k entries") < text.index("16-bit top-k entries")        # a section of its own, after the exact entry's
    from test_simtopk_combined_cpu import _topk_table
    assert set(_topk_table()) == {"mmf_simtopk_combined"}


def test_design_readme_and_scripts_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design.split("4.17", 1)[1]
    for words in ("Contract", "margin_i(t)", "pos_exponent", "Resources", "ScratchSize", "Measurements", "MMF_PREC_AUTO", "Cut"):
        assert words in sec, words
    assert "simtopk_combined_fast" in design.split("## 4", 1)[0]          # §1's table has the row
    assert "§4.17" in design.split("4.14", 1)[1].split("4.15", 1)[0]      # §4.14's Cut points here
    with open(os.path.join(ROOT, "README.md")) as f:
        r = f.read()
    assert "simtopk_combined_fast" in r and "build_topk_weighted_hypergraph_fast" in r
    assert os.path.exists(os.path.join(ROOT, "scripts", "simtopk_combined_fast_timing.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "simtopk_combined_fast_timing.txt"))


# ---- the margin, restated, on worst-case rounding rows -------------------------------------------------------------------
def _restated_source_constants():
    with open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_scan_b16c.hip")) as f:
        return f.read()


def test_the_restatement_uses_the_kernels_constants():
    src = _restated_source_constants()
    for words in ("C_M1 = 6.1f * C_U", "2.002f * (ae + 1.01f * C_U * (__builtin_fabsf(rc) + 2.0f * pb)) + 1e-30f",
                  "(float)(2 * a.dpp + 4) * C_U * 1.01f", "const float pb = ae * 1.01f + egb;"):
        assert words in src, words
    import combined16_restate as cr
    assert cr.M1 == np.float32(6.1) * np.float32(5.9604645e-8) and cr.capacity(11) == 16 and cr.capacity(12) == 32 and cr.capacity(20) == 32


@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 500])
def test_margin_holds_on_worst_case_rounding_rows(operand, d):
    """Rows whose every component rounds the same way (tests/adversarial16.py: the error of z_i . z_j comes close to the
    Cauchy-Schwarz bound, with opposite signs for the A and the B columns), with pixel positions added.  For every row the
    canonical top-(k + self) — ranked by fl(eh + eg), then id, the row itself included — lies inside the restated band
    A_ij >= T_i - margin_i(T_i); and the approximate keys of the family's rows really are off by a good part of the margin, so the
    check is not vacuous."""
    import adversarial16 as adv
    import combined16_restate as cr
    fam = adv.self_family(operand, d, 5)
    F = fam.X
    n = F.shape[0]
    rng = np.random.RandomState(7)
    side = 4 * int(np.ceil(np.sqrt(n)))
    cells = rng.choice(side * side, n, replace=False)
    P = np.stack([(cells // side) * 224, (cells % side) * 224], axis=1).astype(np.float32)
    lh, lg = 1e-3, 2e-7
    key = cr.canonical_keys(F, P, lh, lg)
    img = cr.image(F, operand)
    A = cr.approx_keys(img, P, lh, lg)
    for kk in (6, 11, 12, 20):
        T, mg, cnt = cr.bands(F, P, lh, lg, kk, operand)
        order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), -key), axis=1)[:, :kk]
        Atop = np.take_along_axis(A, order, axis=1)
        slack = (Atop - (T - mg)[:, None]).min(axis=1)
        assert (slack >= 0).all(), (kk, int((slack < 0).sum()), float(slack.min()))
        assert (cnt >= kk).all()
    # |A - key| <= err_i(A) = margin_i(A) / 2 (less the 1.001 slack) for EVERY pair, and on the family's pairs it comes close
    err = np.abs(A.astype(np.float64) - key.astype(np.float64))
    m0 = cr.m0_of(img, rs_pn(P), 2, lh, lg).astype(np.float64)
    bound = m0[:, None] / 2 + 3.05 * 2.0 ** -24 * np.abs(A.astype(np.float64))
    assert (err <= bound).all(), float((err / bound).max())
    fam_cols = np.concatenate([fam.a_cols, fam.b_cols])
    sharp = float((err / bound)[np.ix_(fam.q_rows, fam_cols)].max())
    print(f"{operand} d={d}: largest |A - key| / err_i(A) over the family's pairs = {sharp:.3f}")
    # tests/adversarial16.py certifies 0.85 of the dot margin for this family; the L2 bias, the f32 terms and the position term add
    # to the bound here without adding to the family's error, so half of it is asked: Gaussian rows stay below a tenth
    assert sharp > 0.5


def rs_pn(P):
    from oracle import scan16_restate as rs
    return rs.sq_norms(np.ascontiguousarray(P, np.float32))
