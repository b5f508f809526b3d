"""The two-set top-k of the combined similarity without a GPU (mmf_simtopk_combined_xy, include/ext/mmf_hg_topk_xy.h, DESIGN.md
§4.19): the header declares exactly the one entry, the library exports it and the binding registers it in a list of its own, the
entry runs its host checks before any device call, in the documented order, and names the argument, the Python layer raises its
argument errors on the host, the new launcher and driver name the caller's stream, the documents name the feature, the sharded
driver equals the unsharded composition over gloo (the oracle standing in for the device op), and on every case of the GPU
capacity test no query's restated band (tests/combined_xy_restate.py) exceeds its list capacity."""
import ctypes
import inspect
import os
import re
import socket
import sys
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mmf_simtopk_combined_xy"
HEADER = os.path.join(ROOT, "include", "ext", "mmf_hg_topk_xy.h")


def _mod():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.combined_topk_xy")


def _declared(path):
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(mmf_[a-z_0-9]+)\s*\(", src))


# ---- header, library, binding ----------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_and_no_other_header_does():
    assert _declared(HEADER) == {ENTRY}
    inc = os.path.join(ROOT, "include")
    for folder in (inc, os.path.join(inc, "ext")):
        for h in os.listdir(folder):
            if h.endswith(".h") and os.path.join(folder, h) != HEADER:
                assert ENTRY not in _declared(os.path.join(folder, h)), h
    with open(HEADER) as f:
        h = f.read()
    assert '#include "../mmf_hg.h"' in h and "MMF_ABI_VERSION" not in h.replace("ABI version 3", "")      # no version of its own
    for words in ("bit for bit", "k + self <= 44", "k + self <= 20 and 1 <= d <= 4096", "dp <= 8", "MMF_PREC_FAST_BF16", "Host-synchronous",
                  "identity of ids, not of storage", "id -1 and value -inf", "Row slice", "MMF_PREC_AUTO = the f16 scan in the range DESIGN.md §4.19 measured",
                  "nc == 0 with nq > 0 fills"):
        assert words in h, words
    with open(os.path.join(inc, "mmf_hg.h")) as f:
        assert "#define MMF_ABI_VERSION 3" in f.read()                  # additions only


def test_library_and_binding_export_the_entry_from_a_list_of_its_own():
    import multimodal_fusion_amd as mmf
    lb = mmf._lib
    L = ctypes.CDLL(lb.SO_PATH)
    assert lb.EXPORTS_TOPK_XY == [ENTRY] and hasattr(L, ENTRY)
    others = (set(lb.EXPORTS) | set(lb.EXPORTS_COHORT) | set(lb.EXPORTS_POOL) | set(lb.EXPORTS_STREAM) | set(lb.EXPORTS_TOPK)
              | set(lb.EXPORTS_WIDE) | set(lb.EXPORTS_WIDE_SEG) | set(lb.EXPORTS_TOPK16) | set(lb.EXPORTS_TOPK16_SEG))
    assert ENTRY not in others
    fn = getattr(lb.lib(), ENTRY)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 20
    assert lb.ABI_VERSION == 3 and lb.lib().mmf_version() == 3


def test_build_lists_the_new_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmf_build_lists_topk_xy", os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith(os.path.join("include", "ext", "mmf_hg_topk_xy.h")) for h in b.HEADERS)
    assert all(os.path.exists(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", s)) for s in b.SOURCES)


def test_module_and_functions_are_exported():
    import multimodal_fusion_amd as mmf
    m = _mod()
    assert "combined_topk_xy" in mmf.__all__ and mmf.combined_topk_xy is m
    names = {"simtopk_combined_xy", "simtopk_combined_rows"}
    for name in names:
        assert name in mmf.__all__ and getattr(mmf, name) is getattr(m, name), name
        assert not hasattr(mmf.ops, name) and not hasattr(mmf.combined_topk, name) and not hasattr(mmf.combined_topk16, name)
    public = {n for n, fn in inspect.getmembers(m, inspect.isfunction) if fn.__module__ == m.__name__ and not n.startswith("_")}
    assert public == names
    sig = inspect.signature(m.simtopk_combined_xy)
    assert list(sig.parameters) == ["q_features", "q_positions", "c_features", "c_positions", "lambda_h", "lambda_g", "k", "exclude_self",
                                    "row_offset", "col_offset", "precision", "col_splits", "return_stats", "profile"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[7:])
    assert [sig.parameters[n].default for n in list(sig.parameters)[4:]] == [1.0, 1.0, 5, False, 0, 0, "auto", 0, False, False]
    sig = inspect.signature(m.simtopk_combined_rows)
    assert list(sig.parameters)[:8] == ["features", "positions", "lo", "hi", "lambda_h", "lambda_g", "k", "exclude_self"]
    assert sig.parameters["exclude_self"].default is True and sig.parameters["exclude_self"].kind is inspect.Parameter.KEYWORD_ONLY
    d = import_module("multimodal_fusion_amd.distributed")
    sig = inspect.signature(d.sharded_simtopk_combined)
    assert list(sig.parameters) == ["f_local", "p_local", "n_total", "lambda_h", "lambda_g", "k", "exclude_self", "precision", "group",
                                    "gather_output", "op", "return_stats"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[3:]] == [1.0, 1.0, 5, True, "auto", None, False, None, False]


# ---- the entry's host checks, with host buffers standing in for device pointers ------------------------------------------
def _call(**kw):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(Fq=b, Pq=b, nq=4, Fc=b, Pc=b, nc=6, d=4, dp=2, lh=1.0, lg=1.0, k=2, self=1, ro=0, co=0, idx=b, val=b, opts=(2, 0, 0, 0, None),
             device=0)
    a.update(kw)
    opts = a["opts"]
    if opts is not None:
        opts = ctypes.byref(mmf._lib.SimtopkOpts(*opts))
    rc = getattr(L, ENTRY)(a["Fq"], a["Pq"], a["nq"], a["Fc"], a["Pc"], a["nc"], a["d"], a["dp"], a["lh"], a["lg"], a["k"], a["self"], a["ro"],
                           a["co"], a["idx"], a["val"], opts, None, a["device"], None)
    return rc, L.mmf_last_error().decode()


INVALID = [
    (dict(nq=-1), "nq must be >= 0"),
    (dict(nc=-1), "nc must be >= 0"),
    (dict(d=0), "d must be at least 1"),
    (dict(dp=0), "dp must be at least 1"),
    (dict(k=0), "k must be at least 1"),
    (dict(ro=-1), "row_offset must be >= 0"),
    (dict(co=-5), "col_offset must be >= 0"),
    (dict(lh=-0.5), "lambda_h must be finite and >= 0"),
    (dict(lh=float("inf")), "lambda_h must be finite and >= 0"),
    (dict(lg=-1.0), "lambda_g must be finite and >= 0"),
    (dict(lg=float("nan")), "lambda_g must be finite and >= 0"),
    (dict(Fq=None), "Fq is NULL"),
    (dict(Pq=None), "Pq is NULL"),
    (dict(Fc=None), "Fc is NULL"),
    (dict(Pc=None), "Pc is NULL"),
    (dict(idx=None), "out_idx is NULL"),
    (dict(val=None), "out_val is NULL"),
    (dict(opts=(7, 0, 0, 0, None)), "precision 7"),
    (dict(opts=(2, 0, -1, 0, None)), "col_splits must be >= 0 (got -1)"),
]
UNSUPPORTED = [
    (dict(dp=9), "dp = 9 > 8"),
    (dict(k=44, opts=(1, 0, 0, 0, None)), "k + self = 45 > 44"),
    (dict(k=45, self=0, opts=None), "k + self = 45 > 44"),
    (dict(k=20), "k + self = 21 > 20"),
    (dict(k=21, self=0, opts=(3, 0, 0, 0, None)), "k + self = 21 > 20"),
    (dict(d=4097), "d = 4097 > 4096"),
    (dict(d=4097, opts=(3, 0, 0, 0, None)), "d = 4097 > 4096"),
    (dict(nq=1 << 31), "row_offset + nq must be < 2^31"),
    (dict(ro=(1 << 31) - 4), "row_offset + nq must be < 2^31"),
    (dict(nc=1 << 31), "col_offset + nc must be < 2^31"),
    (dict(co=(1 << 31) - 6), "col_offset + nc must be < 2^31"),
]


@pytest.mark.parametrize("kw,words", INVALID)
def test_entry_refuses_bad_arguments_before_any_device_call(kw, words):
    """device_id = 0 on a machine without a GPU (and host buffers for device pointers on one with): the argument error wins."""
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_INVALID and words in msg and "simtopk_combined_xy" in msg, (rc, msg)


@pytest.mark.parametrize("kw,words", UNSUPPORTED)
def test_entry_refuses_what_it_does_not_support_before_any_device_call(kw, words):
    import multimodal_fusion_amd as mmf
    rc, msg = _call(**kw)
    assert rc == mmf._lib.MMF_E_UNSUPPORTED and words in msg and "simtopk_combined_xy" in msg, (rc, msg)


def test_the_order_of_the_checks():
    """The device first, then every MMF_E_INVALID (shapes, offsets, lambdas, pointers, precision, col_splits — in that order),
    then every MMF_E_UNSUPPORTED (dp, k + self > 44, the 16-bit limits, the id ranges)."""
    import multimodal_fusion_amd as mmf
    inv, uns = mmf._lib.MMF_E_INVALID, mmf._lib.MMF_E_UNSUPPORTED
    chain = [(dict(nq=-1), "nq must"), (dict(nc=-1), "nc must"), (dict(d=0), "d must"), (dict(dp=0), "dp must"), (dict(k=0), "k must"),
             (dict(ro=-1), "row_offset must"), (dict(co=-1), "col_offset must"), (dict(lh=-1.0), "lambda_h"), (dict(lg=-1.0), "lambda_g"),
             (dict(Fq=None), "Fq is NULL"), (dict(Pq=None), "Pq is NULL"), (dict(Fc=None), "Fc is NULL"), (dict(Pc=None), "Pc is NULL"),
             (dict(idx=None), "out_idx"), (dict(val=None), "out_val"), (dict(opts=(7, 0, -1, 0, None)), "precision 7"),
             (dict(opts=(2, 0, -1, 0, None)), "col_splits"), (dict(dp=9), "dp = 9 > 8"), (dict(k=44), "k + self = 45 > 44"),
             (dict(d=4097), "d = 4097 > 4096"), (dict(ro=1 << 31), "row_offset + nq"), (dict(co=1 << 31), "col_offset + nc")]
    for i, (_, words) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):           # this mistake and every later one at once: this one is reported
            kw.update(later)
        rc, msg = _call(**kw)
        assert words in msg and rc == (inv if i < 17 else uns), (i, words, rc, msg)
    rc, msg = _call(k=20, d=4097)                      # under FAST: k + self before d
    assert rc == uns and "k + self = 21 > 20" in msg
    assert _call(k=20, d=4097, opts=(1, 0, 0, 0, None), device=63)[0] == mmf._lib.MMF_E_HIP        # the exact scan takes both


def test_entry_refuses_a_negative_device_first():
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(k=0), dict(Fq=None), dict(dp=9), dict(nq=-1), dict(d=4097)):
        rc, msg = _call(device=-1, **kw)
        assert rc == mmf._lib.MMF_E_UNSUPPORTED and "no CPU path" in msg and "simtopk_combined_xy" in msg, (rc, msg)


def test_valid_arguments_reach_the_device_and_no_queries_are_a_no_op():
    """Every precision, zero lambdas, the limits themselves, offsets, no candidates: the call gets as far as the device — one
    that does not exist, so that host buffers are never read as device memory.  nq == 0 returns before it."""
    import multimodal_fusion_amd as mmf
    for kw in (dict(), dict(opts=None), dict(opts=(0, 0, 0, 0, None)), dict(opts=(1, 0, 0, 0, None)), dict(opts=(3, 1, 4, 0, None)),
               dict(lh=0.0, lg=0.0), dict(k=19), dict(k=20, self=0), dict(k=43, opts=(1, 0, 0, 0, None)), dict(k=21, self=0, opts=None),
               dict(dp=8), dict(d=4096), dict(d=5000, opts=(1, 0, 0, 0, None)), dict(ro=100, co=(1 << 31) - 7), dict(nc=0, Fc=None, Pc=None)):
        rc, msg = _call(device=63, **kw)
        assert rc == mmf._lib.MMF_E_HIP, (kw, rc, msg)
    assert _call(nq=0)[0] == mmf._lib.MMF_OK
    assert _call(nq=0, Fq=None, Pq=None, Fc=None, Pc=None, idx=None, val=None)[0] == mmf._lib.MMF_OK


# ---- the Python layer's argument errors, on the host ------------------------------------------------------------------
def test_wrapper_rejects_bad_input_before_any_library_call(monkeypatch):
    import multimodal_fusion_amd as mmf
    m = _mod()

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mmf._lib, "lib", no_library)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    G, Q = torch.randn(6, 8), torch.zeros(6, 2)
    f = m.simtopk_combined_xy
    with pytest.raises(ValueError, match="must share Nq"):
        f(G, Q[:5], F, P)
    with pytest.raises(ValueError, match="must share Nc"):
        f(G, Q, F, P[:9])
    with pytest.raises(ValueError, match="must share Nq"):
        f(G, Q[:, 0], F, P)
    with pytest.raises(ValueError, match="must share D and dp"):
        f(G[:, :7], Q, F, P)
    with pytest.raises(ValueError, match="must share D and dp"):
        f(G, torch.zeros(6, 3), F, P)
    with pytest.raises(ValueError, match=r"k must be >= 1 \(got 0\)"):
        f(G, Q, F, P, k=0)
    with pytest.raises(ValueError, match="unknown precision 'half'"):
        f(G, Q, F, P, precision="half")
    with pytest.raises(ValueError, match="col_splits must be >= 0"):
        f(G, Q, F, P, col_splits=-1)
    with pytest.raises(ValueError, match="row_offset and col_offset must be >= 0"):
        f(G, Q, F, P, row_offset=-1)
    r = m.simtopk_combined_rows
    with pytest.raises(ValueError, match="must share N"):
        r(F, P[:9], 0, 4)
    for lo, hi in ((-1, 4), (5, 4), (0, 11)):
        with pytest.raises(ValueError, match="are no range of the 10 rows"):
            r(F, P, lo, hi)
    with pytest.raises(ValueError, match="simtopk_combined_rows: unknown precision"):
        r(F, P, 0, 4, precision="f16")


def test_without_a_gpu_the_wrappers_raise(monkeypatch):
    m = _mod()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    F, P = torch.randn(10, 8), torch.zeros(10, 2)
    with pytest.raises(RuntimeError, match="ROCm"):
        m.simtopk_combined_xy(F[:4], P[:4], F, P)
    with pytest.raises(RuntimeError, match="ROCm"):
        m.simtopk_combined_rows(F, P, 2, 6)


# ---- static stream scan ------------------------------------------------------------------------------------------------
def _body(text, name):
    return text.split("int " + name + "(", 1)[1].split("\n}\n", 1)[0]


def _offset(text, line):
    return sum(len(x) + 1 for x in text.split("\n")[:line - 1])


def test_launcher_and_driver_name_the_callers_stream_and_nothing_blocks():
    from test_stream_arguments_cpu import BLOCKING, BLOCKING_ALLOWED, enclosing, is_null, sources, stream_uses
    src = dict(sources())
    text, api = src["mmf_scan_b16c.hip"], src["mmf_api.hip"]
    # the launcher: the scan through launch_b16c_t's SEG instantiations, the seed union, both on the stream it was given
    mine = [u for u in stream_uses() if u[0] == "mmf_scan_b16c.hip" and enclosing(text, _offset(text, u[1])) == "launch_scan_b16c_xy"]
    assert [a[0] for _, _, what, _, a in mine if what == "hipLaunchKernelGGL"] == ["comb_seed_union_kernel"]
    assert all(u[3] == "s" for u in mine)
    launcher = _body(text, "launch_scan_b16c_xy")
    assert "launch_b16c_t<C_CAP_SMALL, true>(a, p.f16, grid, s)" in launcher and "launch_b16c_t<C_CAP_BIG, true>(a, p.f16, grid, s)" in launcher
    assert "template <bool F16, int CAP, bool SEG = false>" in text          # no new kernel parameter
    # the driver: every runtime call asynchronous and on the call's stream; the 16-bit path's one explicit synchronisation is taken
    # only when more than 1024 rows were flagged (its clean path's one synchronisation is FlagBlock::read's)
    for fn in ("xy_fast", "run_simtopk_combined_xy", "xy_fill_none"):
        body = api.split(" " + fn + "(", 1)[1].split("\n}\n", 1)[0]
        assert not [m for m in BLOCKING.finditer(body) if not m.group(1).endswith("Async")], fn
        assert "hipDeviceSynchronize" not in body
        mine = [u for u in stream_uses() if u[0] == "mmf_api.hip" and enclosing(api, _offset(api, u[1])) == fn]
        assert mine and all(u[3] == "s" for u in mine) and not [u for u in mine if is_null(u[3])], (fn, mine)
    fast = api.split(" xy_fast(", 1)[1].split("\n}\n", 1)[0]
    assert fast.count("hipStreamSynchronize(s)") == 1 and fast.index("if (h_fail > peek)") < fast.index("hipStreamSynchronize(s)")
    assert fast.count("flags.read(") == 1 and fast.count("launch_scan_b16c_xy(") == 1 and "launch_rerank_combined(" in fast
    assert "launch_scan_b16_audit(" in fast and "upload_table(s," in fast
    assert "hipStreamSynchronize" not in api.split("int run_simtopk_combined_xy(", 1)[1].split("\n}\n", 1)[0]
    raw = open(os.path.join(ROOT, "multimodal-fusion_amd", "csrc", "mmf_api.hip")).read()
    assert "MMF_DEBUG_FLAG_ROWS" in raw.split(" xy_fast(", 1)[1].split("\n}\n", 1)[0]
    assert not [k for k in BLOCKING_ALLOWED if "xy" in k[1]]          # the allow-list was not extended


# ---- documents -------------------------------------------------------------------------------------------------------
def _xy_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Two-set top-k entries$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_table_equals_the_gpu_tests_table():
    from test_gpu_simtopk_combined_xy import SYNC
    import multimodal_fusion_amd as mmf
    rows = _xy_table()
    assert rows == SYNC == {ENTRY: ("data-dependent", "no host arguments")}, (rows, SYNC)
    assert set(rows) == set(mmf._lib.EXPORTS_TOPK_XY)


def test_design_readme_and_scripts_name_the_feature():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design.split("## 4.19", 1)[1]
    for words in ("Contract", "Row slice", "union", "superset", "Table", "CSEG_IDOFF", "MMF_PREC_AUTO", "Cut", "sharded_simtopk_combined"):
        assert words in sec, words
    assert "§4.19" in design.split("## 4.18", 1)[1].split("## 4.19", 1)[0]          # §4.18's Cut points here
    with open(os.path.join(ROOT, "README.md")) as f:
        r = f.read()
    assert "simtopk_combined_xy" in r and "sharded_simtopk_combined" in r
    assert os.path.exists(os.path.join(ROOT, "scripts", "simtopk_combined_xy_timing.py"))
    with open(os.path.join(ROOT, "profiles", "simtopk_combined_xy_timing.txt")) as f:
        prof = f.read()
    assert "against all N" in prof and "distinct candidates" in prof and "the exact arm's spread" in prof


# ---- the sharded driver over gloo, the oracle standing in for the device op ------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, d, k, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import multimodal_fusion_amd  # noqa: F401
    import combined16_restate as cr
    import combined_xy_restate as xr
    dmod = import_module("multimodal_fusion_amd.distributed")
    F, P = (torch.from_numpy(a) for a in cr.make_data(n, d, 2, 6))
    lo, hi = dmod.shard_bounds(n, world, rank)
    kw = dict(lambda_h=xr.LH, lambda_g=xr.LG, k=k, exclude_self=True, op=xr.oracle_op)
    idx, val = dmod.sharded_simtopk_combined(F[lo:hi].contiguous(), P[lo:hi].contiguous(), n, gather_output=True, **kw)
    own_i, own_v = dmod.sharded_simtopk_combined(F[lo:hi].contiguous(), P[lo:hi].contiguous(), n, **kw)
    assert own_i.shape == (hi - lo, k) and torch.equal(own_i, idx[lo:hi]) and torch.equal(own_v.view(torch.int32), val[lo:hi].view(torch.int32))
    with pytest.raises(ValueError, match="expected"):
        dmod.sharded_simtopk_combined(F[:0], P[:0], n, **kw)               # refused on every rank, before any collective
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), idx=idx.numpy(), val=val.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n,world", [(101, 2), (67, 3)])
def test_sharded_equals_unsharded_gloo(tmp_path, n, world):
    """Uneven shards (n is no multiple of the world): every rank's rows, alone and gathered, are the unsharded composition's."""
    import combined16_restate as cr
    import combined_xy_restate as xr
    d, k = 24, 4
    port = _free_port()
    mp.spawn(_worker, args=(world, port, n, d, k, str(tmp_path)), nprocs=world, join=True)
    F, P = (torch.from_numpy(a) for a in cr.make_data(n, d, 2, 6))
    ridx, rval = xr.oracle_op(F, P, F, P, xr.LH, xr.LG, k, exclude_self=True, row_offset=0, col_offset=0)
    want_i, _ = xr.reference(F.numpy(), P.numpy(), (0, n), (0, n), k, exclude_self=True)
    assert np.array_equal(ridx.numpy(), want_i)                         # the op is the GPU test's reference
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert np.array_equal(z["idx"], ridx.numpy()) and np.array_equal(z["val"].view(np.uint32), rval.numpy().view(np.uint32))


# ---- the capacity condition of the GPU test, on the CPU ----------------------------------------------------------------
def test_a_self_case_is_the_one_graph_restatement():
    import combined16_restate as cr
    import combined_xy_restate as xr
    F, P = cr.make_data(200, 40, 2, 4)
    for operand in ("f16", "bf16"):
        a, b = xr.bands_xy(F, P, (0, 200), (0, 200), 0.5, 2e-7, 6, operand), cr.bands(F, P, 0.5, 2e-7, 6, operand)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_no_band_of_the_capacity_cases_exceeds_its_capacity(operand):
    """What tests/test_gpu_simtopk_combined_xy.py's capacity test relies on: with image, scale, maxima and the largest pn taken
    over both sides, no query's band among the candidate columns holds more columns than its lists."""
    import combined16_restate as cr
    import combined_xy_restate as xr
    assert [(c.name, c.total, c.d, c.dp, c.q, c.c) for c in xr.CASES] == [
        ("R1", 390, 40, 2, (0, 130), (130, 390)), ("R2", 400, 64, 3, (100, 300), (50, 350)), ("R3", 258, 130, 8, (0, 129), (129, 258)),
        ("R4", 600, 512, 2, (0, 300), (300, 600)), ("R5", 700, 96, 2, (175, 350), (0, 700)), ("R6", 300, 1536, 2, (0, 150), (150, 300))]
    for case in xr.CASES:
        F, P = xr.case_data(case)
        for kk in (6, 11, 12, 20):
            _, _, cnt = xr.bands_xy(F, P, case.q, case.c, xr.LH, xr.LG, kk, operand)
            cap = cr.capacity(kk)
            print(f"{case.name} {operand} k + self {kk}: largest band {int(cnt.max())} of {cap}")
            assert int((cnt > cap).sum()) == 0, (case.name, kk)
