"""The stream contract of include/mmf_hg.h on a busy non-default stream: "Every call enqueues on `hip_stream` ...
asynchronous w.r.t. the host except where noted".

Every public function of multimodal-fusion_amd/ops.py (and the C entries documented as not synchronising, through the ctypes
binding) runs behind a closed gate on a non-blocking side stream (tests/streamgate.py): its device inputs still hold a valid
DECOY when the call is made and receive the truth only when the gate opens.  The result must equal, bit for bit, the same call
made beforehand on the idle default stream, and the CPU reference (oracle.* where it has the function, numpy / torch-CPU
restatements otherwise).  That fails for
  1. a launch, memset or copy on another stream than the caller's (it sees the decoy, or runs before what it should follow);
  2. a host read of a device result before the stream was synchronised;
  3. a host table (the caller's ptr_host, a local std::vector) read after the call returned and its owner died: entries that
     do not synchronise are followed by a churn of the host heap;
  4. a workspace keyed by the device alone, or freed while a stream still uses it (the three workspace cases at the end).
SYNC below is the table of INTEGRATION.md ("Host synchronisations and host arguments"); tests/test_stream_arguments_cpu.py
checks that the two list the same entries.  Entries marked "none" must return while the gate is still closed.
"""
import ctypes
import math
import os
import sys
from contextlib import contextmanager
from importlib import import_module

import numpy as np
import pytest
import torch

import oracle
from conftest import unit_rows

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgate as sg   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5                   # scores that go through expf (test_gpu_parity.py)

# entry -> (host synchronisations, how long *_host arguments must stay valid): the table of INTEGRATION.md.
#   none            returns without waiting for the stream (check (b) of the harness)
#   once            one stream synchronisation per call
#   per iteration   one small status read per Lloyd iteration
#   data-dependent  the path decides (documented per entry in include/mmf_hg.h); the "none" paths are gated as such below
# Any entry whose cached workspace has to grow synchronises the stream once before the old buffer is freed.
CALL = "until the call returns"
NOHOST = "-"
SYNC = {
    "mmf_simtopk": ("data-dependent", NOHOST),
    "mmf_simtopk_ex": ("data-dependent", CALL),
    "mmf_simtopk_prepared": ("data-dependent", CALL),
    "mmf_simtopk_panels": ("data-dependent", CALL),
    "mmf_simtopk_segmented": ("data-dependent", CALL),
    "mmf_row_scalars": ("none", NOHOST),
    "mmf_prep_rows": ("none", NOHOST),
    "mmf_topk_merge": ("none", NOHOST),
    "mmf_edge_cosine": ("none", NOHOST),
    "mmf_sim_dense": ("none", NOHOST),
    "mmf_sim_dense_stats": ("data-dependent", NOHOST),
    "mmf_sim_dense_combined": ("none", NOHOST),
    "mmf_offdiag_lower_median": ("data-dependent", NOHOST),
    "mmf_lower_median": ("data-dependent", NOHOST),
    "mmf_array_stats": ("data-dependent", NOHOST),
    "mmf_threshold_edges": ("none", NOHOST),
    "mmf_threshold_edges_count": ("none", NOHOST),
    "mmf_threshold_edges_fill": ("none", NOHOST),
    "mmf_combined_offdiag_median": ("data-dependent", NOHOST),
    "mmf_combined_threshold_edges": ("none", NOHOST),
    "mmf_sim_dense_combined_segmented": ("none", CALL),
    "mmf_offdiag_lower_median_segmented": ("none", CALL),
    "mmf_threshold_edges_segmented_count": ("none", CALL),
    "mmf_threshold_edges_segmented_fill": ("none", CALL),
    "mmf_segment_sort": ("once", NOHOST),
    "mmf_segment_mean": ("none", NOHOST),
    "mmf_segment_offdiag_mean": ("none", NOHOST),
    "mmf_clique_pairs": ("none", NOHOST),
    "mmf_knn_pairs": ("none", NOHOST),
    "mmf_knn_clique_edges_count": ("none", CALL),
    "mmf_knn_clique_edges_fill": ("none", CALL),
    "mmf_kmeans_fit": ("per iteration", CALL),
    "mmf_kmeans_fit_segmented": ("per iteration", CALL),
    "mmf_release_workspaces": ("once", NOHOST),
}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    sg.calibrate()
    yield m
    path = os.environ.get("MMF_STREAM_RECORD")          # a run's calibration and per-case figures (profiles/stream_contract.txt)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(sg.RECORD) + "\n")


T = torch.from_numpy


def rnd(n, d, seed, scale=1.0):
    return (np.random.RandomState(seed).randn(n, d) * scale).astype(np.float32)


def dup_rows(n, d, seed, clusters=None, noise=0.02, scale=1.0):
    """tests/test_gpu_query_order.py: rows in tight clusters, scattered."""
    rng = np.random.RandomState(seed)
    c = rng.randn(clusters or max(3, n // 40), d).astype(np.float32)
    return ((c[rng.randint(0, len(c), n)] + noise * rng.randn(n, d).astype(np.float32)) * scale).astype(np.float32)


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def seeded(fn):
    """make_inputs from fn(seed): the truth is seed 1, the decoy seed 2 (valid data of the same shapes)."""
    return lambda which: [t if isinstance(t, torch.Tensor) else T(np.ascontiguousarray(t)) for t in fn(1 if which == "truth" else 2)]


@contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def ops_():
    import multimodal_fusion_amd as m
    return m.ops


def L():
    import multimodal_fusion_amd as m
    return m._lib.lib()


def st_(t):
    return ops_()._stream(t.device)       # looked up at call time: the self-test patches ops._stream


def ck(rc, what):
    import multimodal_fusion_amd as m
    m._lib.check(rc, what)


def hp(a):
    """Host pointer of a numpy array / CPU tensor."""
    return ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


P_ = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())   # noqa: E731


# ---------------------------------------------------------------------------------------------------
# the cases: name -> dict(entry, make_inputs, reference, nonsync, atol, calls, finish, covers)
# ---------------------------------------------------------------------------------------------------
CASES = {}


def case(name, covers, nonsync=False, atol=0.0, calls=None):
    def reg(fn):
        CASES[name] = dict(build=fn, covers=tuple(covers), nonsync=nonsync, atol=atol, calls=calls or (2 if nonsync else 1))
        return fn
    return reg


# ---- simtopk: every host path --------------------------------------------------------------------
def _simtopk_case(data, k, metric, expect=None, envs=None, ref_kw=None, **kw):
    """entry / inputs / reference of one simtopk call; `expect(stats)` asserts which path ran."""
    def entry(X):
        with env(**(envs or {})):
            idx, val, st = ops_().simtopk(X, metric=metric, k=k, return_stats=True, **kw)
        if expect is not None:
            assert expect(st), st
        return idx, val

    def reference(X):
        return list(oracle.simtopk(X, metric=metric, k=k, **(ref_kw or {})))
    return dict(entry=entry, make_inputs=seeded(lambda s: [data(s)]), reference=reference)


@case("simtopk_exact", ["simtopk"])
def _():
    return _simtopk_case(lambda s: unit_rows(2000, 64, 10 + s).numpy(), 5, "cosine", lambda st: st["precision_used"] == 1,
                         precision="exact")


@case("simtopk_16bit_no_flagged_rows", ["simtopk"])
def _():
    return _simtopk_case(lambda s: unit_rows(3000, 128, 20 + s).numpy(), 5, "cosine",
                         lambda st: st["precision_used"] == 2 and st["fallback_rows"] == 0, precision="fast")


@case("simtopk_overflow_lists", ["simtopk"])
def _():
    return _simtopk_case(lambda s: np.repeat(rnd(10, 64, 2 + s), 40, axis=0), 5, "neg_sq_l2",
                         lambda st: st["precision_used"] == 2 and st["fallback_rows"] == 0 and st["candidates"] >= 400 * 39,
                         precision="fast")


@case("simtopk_exact_rescan_second_slot", ["simtopk"])
def _():
    # more copies than the overflow lists hold: every row is flagged and rescanned by the exact kernel, whose f32 images
    # live in the second workspace slot, taken after the call's first synchronisation
    return _simtopk_case(lambda s: np.repeat(rnd(4, 64, 3 + s), 300, axis=0), 5, "neg_sq_l2",
                         lambda st: st["precision_used"] == 2 and st["fallback_rows"] == 1200, precision="fast")


@case("simtopk_flag_rows_49_matrix_core_rescan", ["simtopk"])
def _():
    return _simtopk_case(lambda s: dup_rows(7000, 100, 20 + s), 4, "cosine", lambda st: st["fallback_rows"] >= 49,
                         envs={"MMF_DEBUG_FLAG_ROWS": 49}, precision="fast")


@case("simtopk_k_beyond_one_pass", ["simtopk"])
def _():
    def data(s):
        X = unit_rows(1000, 128, 500 + s).numpy()
        X[50:90] = X[50]
        return X
    return _simtopk_case(data, 64, "cosine", lambda st: st["precision_used"] == 1, precision="auto")


@case("simtopk_query_order_on", ["simtopk"])
def _():
    return _simtopk_case(lambda s: dup_rows(3000, 64, 30 + s), 5, "cosine", lambda st: st["query_order"] == 1 and st["near_rows"] >= 0,
                         precision="fast", query_order="on")


@case("simtopk_query_order_auto_probe", ["simtopk"])
def _():
    # from 32768 rows AUTO probes the rows and reads the verdict back: a synchronisation in the middle of the call
    return _simtopk_case(lambda s: dup_rows(32768, 128, 40 + s, clusters=800), 5, "cosine",
                         lambda st: st["near_rows"] >= 0, precision="fast", query_order="auto")


@case("simtopk_symmetric_scan", ["simtopk"])
def _():
    def grid():
        return 2 * L().mmf_debug_symmetric_schedule((1000 + 255) // 256, 1, 0, None, 0)
    return _simtopk_case(lambda s: unit_rows(1000, 512, 50 + s).numpy(), 5, "cosine", lambda st: st["scan_grid"] == grid(),
                         envs={"MMF_SYMMETRIC": 1, "MMF_SYMMETRIC_G": 1}, precision="fast", query_order="off")


@case("simtopk_profile_events", ["simtopk"])
def _():
    def timed(st):
        ts = [st[q] for q in ("scan_ms", "prep_ms", "rerank_ms", "fallback_ms", "order_ms", "scan_wait_ms")]
        return all(math.isfinite(t) and t >= 0.0 for t in ts)
    return _simtopk_case(lambda s: unit_rows(3000, 128, 60 + s).numpy(), 5, "cosine", timed, precision="fast", profile=True)


@case("simtopk_half_rows_rect", ["simtopk"])
def _():
    def entry(X, Y):
        return ops_().simtopk(X, Y, metric="cosine", k=6, precision="fast")

    def data(s):
        return [unit_rows(900, 96, 70 + s).half(), unit_rows(2100, 96, 80 + s).half()]
    return dict(entry=entry, make_inputs=seeded(data), reference=lambda X, Y: list(oracle.simtopk(X, Y, metric="cosine", k=6)))


# ---- segmented and phase entries -----------------------------------------------------------------
def _segmented_ref(X, xp, k, metric):
    """One oracle.simtopk per segment (row_offset / col_offset = the segment's offsets), short segments padded with -1 / -inf."""
    idx = np.full((X.shape[0], k), -1, np.int64)
    val = np.full((X.shape[0], k), -np.inf, np.float32)
    for a, b in zip(xp[:-1], xp[1:]):
        ks = min(k, b - a - 1)
        if ks > 0:
            i, v = oracle.simtopk(X[a:b], X[a:b], metric=metric, k=ks, exclude_self=True, row_offset=a, col_offset=a)
            idx[a:b, :ks], val[a:b, :ks] = i, v
    return [idx, val]


@case("simtopk_segmented_short_and_flagged", ["simtopk_segmented"])
def _():
    sizes = [3, 500, 1200, 1, 40]                      # 3 rows: two admissible columns for k = 5; 1200 copies of 3 rows: flagged
    xp = offsets(sizes)

    def data(s):
        X = dup_rows(xp[-1], 48, 90 + s)
        base = rnd(3, 48, 95 + s)
        X[503:1703] = base[np.random.RandomState(s).randint(0, 3, 1200)]
        return [X]

    def entry(X):
        idx, val, st = ops_().simtopk_segmented(X, ptr=xp, metric="neg_sq_l2", k=5, precision="fast", return_stats=True)
        assert st["fallback_rows"] >= 1200, st
        return idx, val
    return dict(entry=entry, make_inputs=seeded(data), reference=lambda X: _segmented_ref(X, xp, 5, "neg_sq_l2"))


def _prep_all(ops, X, metric, n_pad):
    """row_scalars + prep_rows of all rows of X into fresh buffers (the layout of tests/test_gpu_configs.py)."""
    n, d = X.shape
    dp = ops.padded_dim(d)
    maxn = torch.zeros(1, device=X.device)
    scal = torch.zeros(n_pad + 256, device=X.device)
    ops.row_scalars(X, metric, scal[:n], maxn)
    Z = torch.zeros((n_pad + 256, dp), dtype=torch.float16, device=X.device)
    zn, rn, un = (torch.zeros(n_pad + 256, device=X.device) for _ in range(3))
    cb = torch.full((n_pad + 256,), float("-inf"), device=X.device)
    max4 = torch.zeros(4, device=X.device)
    ops.prep_rows(X, metric, "f16", scal[:n], maxn, Z[:n], zn[:n], rn[:n], un[:n], cb[:n], max4)
    return dict(Z=Z, scal=scal, zn=zn, rn=rn, un=un, cb=cb), max4


@case("row_scalars_prep_rows", ["row_scalars", "prep_rows"], nonsync=True)
def _():
    def entry(X):
        side, max4 = _prep_all(ops_(), X, "cosine", 2048)
        return side, max4
    return dict(entry=entry, make_inputs=seeded(lambda s: [unit_rows(2000, 200, 100 + s).numpy() * (1.0 + s)]), reference=None)


@case("simtopk_prepared", ["row_scalars", "prep_rows", "simtopk_prepared"])
def _():
    n, lo, hi = 4096, 1024, 2048

    def entry(X):
        ops = ops_()
        side, max4 = _prep_all(ops, X, "cosine", n)
        q = {key: v[lo:] for key, v in side.items()}
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ops.simtopk_prepared(X[lo:hi], X, q, side, n, max4, metric="cosine", k=5, exclude_self=True, row_offset=lo,
                                    wait_event=ev)
    return dict(entry=entry, make_inputs=seeded(lambda s: [unit_rows(n, 256, 110 + s).numpy()]),
                reference=lambda X: list(oracle.simtopk(X[lo:hi], X, metric="cosine", k=5, exclude_self=True, row_offset=lo)))


@case("simtopk_panels_two_ready_events", ["row_scalars", "prep_rows", "simtopk_panels"])
def _():
    n, h = 4096, 2048                                   # two panels: columns [0, h) and [h, n)

    def entry(X):
        ops = ops_()
        cur, other = torch.cuda.current_stream(), sg.streams()[1]
        side, max4 = _prep_all(ops, X, "neg_sq_l2", n)
        prepared = torch.cuda.Event()
        prepared.record(cur)
        dp = side["Z"].shape[1]
        panels, keep = [], []
        for c0, c1 in ((0, h), (h, n)):
            m = c1 - c0
            Zc = torch.zeros((m + 256, dp), dtype=torch.float16, device=X.device)     # zero operands, -inf biases: an empty panel
            cbc = torch.full((m + 256,), float("-inf"), device=X.device)              # until the copy below has run
            ready = torch.cuda.Event()
            with torch.cuda.stream(other):                                             # the exchange stream of the pipelined driver
                other.wait_event(prepared)
                Zc[:m].copy_(side["Z"][c0:c1])
                cbc[:m].copy_(side["cb"][c0:c1])
                ready.record(other)
            keep += [Zc, cbc]
            panels.append(dict(Z=Zc, cb=cbc, m=m, m_pad=m, id_base=c0, event=ready))
        q = dict(side)
        out = ops.simtopk_panels(X, X, q, side["scal"], panels, max4, metric="neg_sq_l2", k=5, exclude_self=True)
        other.synchronize()
        return out
    return dict(entry=entry, make_inputs=seeded(lambda s: [unit_rows(n, 128, 120 + s).numpy() * 2.0]),
                reference=lambda X: list(oracle.simtopk(X, metric="neg_sq_l2", k=5)))


# ---- entries that return before the stream has run ----------------------------------------------
@case("sim_dense", ["sim_dense"], nonsync=True)
def _():
    return dict(entry=lambda X, Y: ops_().sim_dense(X, Y, metric="cosine"),
                make_inputs=seeded(lambda s: [rnd(150, 64, 3 + s, 0.2), rnd(90, 64, 13 + s, 0.2)]),
                reference=lambda X, Y: oracle.sim_dense(X, Y, metric="cosine"))


@case("sim_dense_rbf_self", ["sim_dense"], nonsync=True, atol=TOL)
def _():
    return dict(entry=lambda X: ops_().sim_dense(X, metric="rbf", lam=0.7),
                make_inputs=seeded(lambda s: [rnd(700, 200, 5 + s, 0.1)]), reference=lambda X: oracle.sim_dense(X, metric="rbf", lam=0.7))


def _fp(n, d, dp, seed):
    """Features with squared distances of order one, positions in the unit box (tests/test_gpu_weighted_segmented.py)."""
    rng = np.random.RandomState(seed)
    return (rng.randn(n, d) * (0.6 / np.sqrt(d))).astype(np.float32), rng.rand(n, dp).astype(np.float32)


@case("sim_dense_combined", ["sim_dense_combined"], nonsync=True, atol=TOL)
def _():
    return dict(entry=lambda F, P: ops_().sim_dense_combined(F, P, 0.7, 1.3), make_inputs=seeded(lambda s: list(_fp(600, 48, 2, 7 + s))),
                reference=lambda F, P: oracle.sim_dense_combined(F, P, 0.7, 1.3))


def _edge_inputs(s):
    X = rnd(300, 48, 9 + s)
    X[17] = 0.0
    return [X, np.random.RandomState(s).randint(0, 300, size=(2, 5000)).astype(np.int64)]


@case("edge_cosine_c_entry", [], nonsync=True)
def _():
    def entry(X, ei):
        out = torch.empty((ei.shape[1],), dtype=torch.float32, device=X.device)
        ck(L().mmf_edge_cosine(P_(X), X.shape[0], X.shape[1], 0, P_(ei), ei.shape[1], P_(out), 0, st_(X)), "mmf_edge_cosine")
        return out
    return dict(entry=entry, make_inputs=seeded(_edge_inputs), reference=lambda X, ei: oracle.edge_cosine(X, ei))


@case("edge_cosine", ["edge_cosine"])                  # the wrapper reads the index range back before the call: one synchronisation
def _():
    return dict(entry=lambda X, ei: ops_().edge_cosine(X, ei), make_inputs=seeded(_edge_inputs),
                reference=lambda X, ei: oracle.edge_cosine(X, ei))


@case("topk_merge", ["topk_merge"], nonsync=True)
def _():
    def data(s):
        X = rnd(640, 64, 11 + s)
        a = oracle.simtopk(X, X[:200], metric="cosine", k=6, exclude_self=True)
        b = oracle.simtopk(X, X[200:], metric="cosine", k=6, exclude_self=True, col_offset=200)
        return [a[0], a[1], b[0], b[1]]
    return dict(entry=lambda ia, va, ib, vb: ops_().topk_merge(ia, va, ib, vb), make_inputs=seeded(data),
                reference=lambda ia, va, ib, vb: list(oracle.topk_merge(ia, va, ib, vb)))


def _labels_inputs(n, S, d, s):
    rng = np.random.RandomState(100 + s)
    lab = rng.randint(0, S, size=n)
    lab[lab == 1] = 0                                   # an empty segment
    order = np.argsort(lab, kind="stable").astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=S))]).astype(np.int64)
    return lab.astype(np.int64), order, off, rng


@case("segment_mean", ["segment_mean"], nonsync=True, atol=2e-6)
def _():
    n, S, d = 5000, 300, 37

    def data(s):
        lab, order, off, rng = _labels_inputs(n, S, d, s)
        return [rng.randn(n, d).astype(np.float32), order, off]

    def reference(X, order, off):
        out = np.full((S, d), np.nan, np.float32)
        for c in range(S):
            if off[c + 1] > off[c]:
                out[c] = X[order[off[c]:off[c + 1]]].astype(np.float64).mean(0)
        return out
    return dict(entry=lambda X, order, off: ops_().segment_mean(X, ops_().Segments(None, off, order, n, S)), make_inputs=seeded(data),
                reference=reference)


@case("segment_offdiag_mean", ["segment_offdiag_mean"], nonsync=True, atol=1e-10)
def _():
    n, S = 1024, 40

    def data(s):
        lab, order, off, rng = _labels_inputs(n, S, 0, s)
        return [rng.rand(n, n).astype(np.float32), order, off]

    def reference(K, order, off):
        out = np.full((S,), np.nan, np.float64)
        for c in range(S):
            idx = order[off[c]:off[c + 1]]
            if len(idx) > 1:
                sub = K[np.ix_(idx, idx)].astype(np.float64)
                out[c] = (sub.sum() - np.trace(sub)) / (len(idx) * (len(idx) - 1))
        return out
    return dict(entry=lambda K, order, off: ops_().segment_offdiag_mean(K, ops_().Segments(None, off, order, n, S)),
                make_inputs=seeded(data), reference=reference)


def _knn_inputs(s):
    X = rnd(600, 16, 3 + s)
    nbr, _ = oracle.simtopk(X, metric="neg_sq_l2", k=6)
    return [nbr, np.random.RandomState(4 + s).randint(0, 9, 600).astype(np.int64)]


def _knn_pairs_ref(nbr, lab):
    ref = {tuple(sorted((i, int(j)))) for i in range(nbr.shape[0]) for j in nbr[i]}
    ref = sorted(e for e in ref if lab[e[0]] != lab[e[1]])
    return np.array(ref, dtype=np.int64).reshape(-1, 2)


def _sorted_pairs(lo, hi, n):
    code = np.sort(lo.astype(np.int64) * n + hi)
    return np.stack([code // n, code % n], 1)


@case("knn_pairs_c_entry", [], nonsync=True)
def _():
    def entry(nbr, lab):
        n, k = nbr.shape
        lo = torch.empty((n * k,), dtype=torch.int64, device=nbr.device)
        hi = torch.empty_like(lo)
        cnt = torch.zeros((), dtype=torch.int64, device=nbr.device)
        ck(L().mmf_knn_pairs(P_(nbr), n, k, P_(lab), P_(lo), P_(hi), P_(cnt), 0, st_(nbr)), "mmf_knn_pairs")
        return lo, hi, cnt

    def finish(out):                                   # the count is read only after the stream was synchronised; order unspecified
        lo, hi, cnt = out
        E = int(cnt.item())
        return T(_sorted_pairs(lo[:E].cpu().numpy(), hi[:E].cpu().numpy(), 600))
    return dict(entry=entry, make_inputs=seeded(_knn_inputs), reference=_knn_pairs_ref, finish=finish)


@case("knn_pairs", ["knn_pairs"])                      # the wrapper reads the count back: one synchronisation
def _():
    def entry(nbr, lab):
        lo, hi = ops_().knn_pairs(nbr, lab)
        return T(_sorted_pairs(lo.cpu().numpy(), hi.cpu().numpy(), 600))
    return dict(entry=entry, make_inputs=seeded(_knn_inputs), reference=_knn_pairs_ref)


@case("offdiag_lower_median_radix", ["offdiag_lower_median"], nonsync=True)
def _():
    return dict(entry=lambda K: ops_().offdiag_lower_median(K), make_inputs=seeded(lambda s: [rnd(700, 700, 21 + s)]),
                reference=lambda K: np.float32(oracle.offdiag_lower_median(K)).reshape(()))


@case("lower_median_radix", ["lower_median"], nonsync=True)
def _():
    return dict(entry=lambda v: ops_().lower_median(v), make_inputs=seeded(lambda s: [rnd(1, 100003, 23 + s).reshape(-1)]),
                reference=lambda v: T(v).median().numpy())


def _stats_check(v):
    t = T(v)
    v64 = t.double()
    want = [float(v64.mean()), float(v64.std()), float(t.min()), float(t.max()), float(t.median())]

    def check(got):
        g = np.asarray(got, dtype=np.float64).reshape(-1).tolist()
        bad = []
        if g[2:] != want[2:]:
            bad.append(f"min / max / median {g[2:]} != {want[2:]}")
        if abs(g[0] - want[0]) > 1e-6 * abs(want[0]) + 1e-9 or abs(g[1] - want[1]) > 2e-6 * want[1] + 1e-12:
            bad.append(f"mean / std {g[:2]} != {want[:2]}")
        return bad
    return check


@case("array_stats_c_entry_radix", [], nonsync=True)
def _():
    def entry(v):
        out = torch.empty((5,), dtype=torch.float64, device=v.device)
        ck(L().mmf_array_stats(P_(v), v.numel(), P_(out), 0, st_(v)), "mmf_array_stats")
        return out
    return dict(entry=entry, make_inputs=seeded(lambda s: [0.97 + 1e-4 * rnd(1, 65539, 25 + s).reshape(-1)]), reference=_stats_check)


@case("array_stats", ["array_stats"])                  # the wrapper returns Python floats: one synchronisation
def _():
    def entry(v):
        st = ops_().array_stats(v)
        return T(np.array([st[q] for q in ("mean", "std", "min", "max", "median")]))
    return dict(entry=entry, make_inputs=seeded(lambda s: [rnd(1, 65539, 27 + s).reshape(-1)]), reference=_stats_check)


# -- segmented, with host tables: few segments, and enough of them that a table passes 1 MiB
def _median_seg_case(sizes):
    ptr = offsets(sizes)
    total = sum(v * v for v in sizes)

    def reference(K):
        kp = offsets([v * v for v in sizes])
        return np.array([oracle.offdiag_lower_median(K[kp[s]:kp[s + 1]].reshape(v, v)) for s, v in enumerate(sizes)], np.float32)
    return dict(entry=lambda K: ops_().offdiag_lower_median_segmented(K, ptr=ptr),
                make_inputs=seeded(lambda s: [np.random.RandomState(31 + s).rand(total).astype(np.float32)]), reference=reference)


@case("offdiag_lower_median_segmented_few", ["offdiag_lower_median_segmented"], nonsync=True)
def _():
    return _median_seg_case([5, 130, 2, 64, 257])


@case("offdiag_lower_median_segmented_2048_graphs", ["offdiag_lower_median_segmented"], nonsync=True)
def _():
    return _median_seg_case(np.random.RandomState(11).randint(16, 41, 2048).tolist())


def _combined_seg_case(sizes, d):
    ptr = offsets(sizes)

    def entry(F, P):
        K, kptr = ops_().sim_dense_combined_segmented(F, P, 0.7, 1.3, ptr=ptr)
        return K, kptr

    def reference(F, P):
        K = np.concatenate([oracle.sim_dense_combined(F[a:b], P[a:b], 0.7, 1.3).reshape(-1) for a, b in zip(ptr[:-1], ptr[1:])])
        return [K, np.array(offsets([v * v for v in sizes]), np.int64)]
    return dict(entry=entry, make_inputs=seeded(lambda s: list(_fp(ptr[-1], d, 2, 41 + s))), reference=reference)


@case("sim_dense_combined_segmented_few", ["sim_dense_combined_segmented"], nonsync=True, atol=TOL)
def _():
    return _combined_seg_case([300, 17, 2, 129, 6, 513], 40)


@case("sim_dense_combined_segmented_20000_graphs", ["sim_dense_combined_segmented"], nonsync=True, atol=TOL)
def _():
    # 64 bytes of work table per tile: 20000 graphs of 2 .. 4 rows pass 1 MiB
    return _combined_seg_case(np.random.RandomState(12).randint(2, 5, 20000).tolist(), 16)


def _thr_plain_inputs(s):
    return [np.random.RandomState(51 + s).rand(700, 700).astype(np.float32)]


def _c_threshold_count(K, thr):
    n = K.shape[0]
    row_off = torch.empty((n + 1,), dtype=torch.int64, device=K.device)
    cnt = torch.zeros((), dtype=torch.int64, device=K.device)
    ck(L().mmf_threshold_edges_count(P_(K), n, thr, P_(row_off), P_(cnt), 0, st_(K)), "mmf_threshold_edges_count")
    return row_off, cnt


@case("threshold_edges_count_fill_c_entries", ["threshold_edges"], nonsync=True)
def _():
    thr, cap = 0.9, 700 * 700                           # capacity of the whole matrix: the fill is enqueued without reading the count

    def entry(K):
        row_off, cnt = _c_threshold_count(K, thr)
        ei = torch.zeros((2, cap), dtype=torch.int64, device=K.device)
        ew = torch.zeros((cap,), dtype=torch.float32, device=K.device)
        ck(L().mmf_threshold_edges_fill(P_(K), 700, thr, P_(row_off), P_(ei), P_(ew), cap, 0, st_(K)), "mmf_threshold_edges_fill")
        one_ei, one_ew = torch.zeros_like(ei), torch.zeros_like(ew)
        one_cnt = torch.zeros((), dtype=torch.int64, device=K.device)
        ck(L().mmf_threshold_edges(P_(K), 700, thr, P_(one_ei), P_(one_ew), cap, P_(one_cnt), 0, st_(K)), "mmf_threshold_edges")
        return row_off, cnt, ei, ew, one_cnt, one_ei, one_ew

    def finish(out):                                   # the counts are read only after the stream was synchronised
        row_off, cnt, ei, ew, one_cnt, one_ei, one_ew = out
        E = int(cnt.item())
        assert int(one_cnt.item()) == E and int(row_off[-1]) == E
        assert torch.equal(ei[:, :E], one_ei[:, :E]) and torch.equal(ew[:E], one_ew[:E])
        return ei[:, :E].contiguous(), ew[:E].contiguous()
    return dict(entry=entry, make_inputs=seeded(_thr_plain_inputs), reference=lambda K: list(oracle.threshold_edges(K, thr)), finish=finish)


def _thr_seg_ref(K, thr, sizes):
    ptr, kp = offsets(sizes), offsets([v * v for v in sizes])
    eis, ews, counts = [], [], []
    for s, v in enumerate(sizes):
        ei, ew = oracle.threshold_edges(K[kp[s]:kp[s + 1]].reshape(v, v), float(thr[s]))
        eis.append(ei + ptr[s]), ews.append(ew), counts.append(ei.shape[1])
    return [np.concatenate(eis, 1), np.concatenate(ews), np.array(offsets(counts), np.int64)]


def _thr_seg_case(sizes, wrapper):
    ptr = offsets(sizes)
    S, n, total = len(sizes), ptr[-1], sum(v * v for v in sizes)
    p_host = np.array(ptr, dtype=np.int64)

    def data(s):
        rng = np.random.RandomState(61 + s)
        return [rng.rand(total).astype(np.float32), (0.3 + 0.5 * rng.rand(S)).astype(np.float32)]

    def entry_c(K, thr):
        p = p_host.copy()                              # a host table that dies when the entry returns, as the wrappers' does
        row_off = torch.empty((n + 1,), dtype=torch.int64, device=K.device)
        cnt = torch.zeros((), dtype=torch.int64, device=K.device)
        ck(L().mmf_threshold_edges_segmented_count(P_(K), hp(p), S, P_(thr), P_(row_off), P_(cnt), 0, st_(K)),
           "mmf_threshold_edges_segmented_count")
        ei = torch.zeros((2, total), dtype=torch.int64, device=K.device)
        ew = torch.zeros((total,), dtype=torch.float32, device=K.device)
        p2 = p_host.copy()
        ck(L().mmf_threshold_edges_segmented_fill(P_(K), hp(p2), S, P_(thr), P_(row_off), P_(ei), P_(ew), total, 0, st_(K)),
           "mmf_threshold_edges_segmented_fill")
        del p, p2
        return row_off, cnt, ei, ew

    def finish(out):
        row_off, cnt, ei, ew = out
        E = int(cnt.item())
        return ei[:, :E].contiguous(), ew[:E].contiguous(), row_off[torch.from_numpy(p_host).to(row_off.device)]

    def entry_w(K, thr):
        return ops_().threshold_edges_segmented(K, thr, ptr=ptr)
    ref = lambda K, thr: _thr_seg_ref(K, thr, sizes)   # noqa: E731
    if wrapper:
        return dict(entry=entry_w, make_inputs=seeded(data), reference=ref)
    return dict(entry=entry_c, make_inputs=seeded(data), reference=ref, finish=finish)


@case("threshold_edges_segmented_c_entries_few", [], nonsync=True)
def _():
    return _thr_seg_case([5, 130, 2, 64, 257], False)


@case("threshold_edges_segmented_c_entries_140000_graphs", [], nonsync=True)
def _():
    return _thr_seg_case([2] * 140000, False)          # 8 bytes of ptr and of kptr per graph: both tables pass 1 MiB


@case("threshold_edges_segmented", ["threshold_edges_segmented"])
def _():
    return _thr_seg_case([5, 130, 2, 64, 257, 31], True)


def _table(sizes, k, seed):
    """[n, k] neighbour table with global ids: k distinct rows of the own segment, never the row itself (vectorised)."""
    rng = np.random.RandomState(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    base = np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes)
    size = np.repeat(sizes, sizes)
    local = np.arange(sizes.sum()) - base
    step = 1 + rng.randint(0, 1 << 30, size=local.shape[0]) % np.maximum(size - k, 1)
    return (base[:, None] + (local[:, None] + step[:, None] + np.arange(k)[None, :]) % size[:, None]).astype(np.int64)


def _knn_clique_ref(nbr, lab, H, ptr):
    """The documented edge set and order of mmf_knn_clique_edges (include/mmf_hg.h), restated with numpy."""
    n, k = nbr.shape
    ptr = np.asarray(ptr, dtype=np.int64)
    seg = np.searchsorted(ptr, np.arange(n), side="right") - 1
    gl = seg * H + lab
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = nbr.reshape(-1)
    ok = (j >= 0) & (j < n) & (j != i)
    i, j = i[ok], j[ok]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    far = gl[lo] != gl[hi]
    codes = [lo[far] * n + hi[far]]
    order = np.argsort(gl, kind="stable")
    g = gl[order]
    for t in range(1, int(np.bincount(g).max()) if n else 0):
        same = g[:-t] == g[t:]
        codes.append(order[:-t][same] * n + order[t:][same])
    code = np.unique(np.concatenate(codes))
    ei = np.stack([code // n, code % n])
    return [ei, np.searchsorted(ei[0], ptr).astype(np.int64)]


def _knn_clique_case(sizes, k, H, wrapper):
    ptr = offsets(sizes)
    n, S = ptr[-1], len(sizes)
    p_host = np.array(ptr, dtype=np.int64)

    def data(s):
        return [_table(sizes, k, 71 + s), np.random.RandomState(81 + s).randint(0, H, n).astype(np.int64)]
    truth = data(1)
    cap = _knn_clique_ref(truth[0], truth[1], H, ptr)[0].shape[1]         # the count the caller would read back

    def entry_c(nbr, lab):
        p = p_host.copy()
        row_off = torch.empty((n + 1,), dtype=torch.int64, device=nbr.device)
        edge_ptr = torch.empty((S + 1,), dtype=torch.int64, device=nbr.device)
        cnt = torch.zeros((), dtype=torch.int64, device=nbr.device)
        args = (P_(nbr), n, k, P_(lab), H, hp(p), S)
        ck(L().mmf_knn_clique_edges_count(*args, P_(row_off), P_(edge_ptr), P_(cnt), 0, st_(nbr)), "mmf_knn_clique_edges_count")
        ei = torch.zeros((2, cap), dtype=torch.int64, device=nbr.device)
        p2 = p_host.copy()
        args = (P_(nbr), n, k, P_(lab), H, hp(p2), S)
        ck(L().mmf_knn_clique_edges_fill(*args, P_(row_off), P_(ei), cap, 0, st_(nbr)), "mmf_knn_clique_edges_fill")
        del p, p2
        return ei, edge_ptr, cnt
    ref = lambda nbr, lab: _knn_clique_ref(nbr, lab, H, ptr) + ([] if wrapper else [np.array(cap, np.int64)])   # noqa: E731
    if wrapper:
        return dict(entry=lambda nbr, lab: ops_().knn_clique_edges(nbr, lab, H, ptr=ptr), make_inputs=seeded(data), reference=ref)
    return dict(entry=entry_c, make_inputs=seeded(data), reference=ref)


@case("knn_clique_edges_c_entries_few", [], nonsync=True)
def _():
    return _knn_clique_case([37, 64, 65, 22, 129, 300, 1000, 23, 128], 5, 10, False)


@case("knn_clique_edges_c_entries_140000_graphs", [], nonsync=True)
def _():
    return _knn_clique_case(np.random.RandomState(13).randint(3, 6, 140000).tolist(), 2, 2, False)   # ptr passes 1 MiB


@case("knn_clique_edges", ["knn_clique_edges"])
def _():
    return _knn_clique_case([37, 64, 65, 22, 129, 300, 1000, 23, 128], 5, 10, True)


# ---- entries that synchronise ---------------------------------------------------------------------
@case("lower_median_one_sweep", ["lower_median"])
def _():
    return dict(entry=lambda v: ops_().lower_median(v), make_inputs=seeded(lambda s: [np.random.RandomState(91 + s).rand(5_000_003).astype(np.float32)]),
                reference=lambda v: T(v).median().numpy())


@case("offdiag_lower_median_one_sweep", ["offdiag_lower_median"])
def _():
    return dict(entry=lambda K: ops_().offdiag_lower_median(K), make_inputs=seeded(lambda s: [np.random.RandomState(93 + s).rand(2100, 2100).astype(np.float32)]),
                reference=lambda K: np.float32(oracle.offdiag_lower_median(K)).reshape(()))


@case("array_stats_one_sweep", ["array_stats"])
def _():
    def entry(v):
        st = ops_().array_stats(v)
        return T(np.array([st[q] for q in ("mean", "std", "min", "max", "median")]))
    return dict(entry=entry, make_inputs=seeded(lambda s: [np.random.RandomState(95 + s).rand(4_700_003).astype(np.float32)]),
                reference=_stats_check)


def _dense_stats_case(n, m, store):
    def entry(X, Y):
        S, st = ops_().sim_dense_stats(X, Y, metric="rbf_direct", lam=0.8, store=store, panel_rows=0 if store else 256)
        stats = T(np.array([st[q] for q in ("mean", "std", "min", "max", "median")]))
        return (S, stats) if store else stats

    def reference(X, Y):
        S = oracle.sim_dense(X, Y, metric="rbf_direct", lam=0.8)

        def check(got):
            st = got[1] if store else got
            bad = sg.diff(got[0], S, "S", atol=TOL) if store else []
            ref = _stats_check(got[0] if store else S)           # the statistics of the matrix the device formed
            g = np.asarray(st).tolist()
            if store:
                return bad + ref(st)
            t = T(S).double()
            if abs(g[0] - float(t.mean())) > 1e-5 or abs(g[4] - float(T(S).median())) > TOL or abs(g[3] - float(t.max())) > TOL:
                bad.append(f"statistics {g} far from the oracle matrix's")
            return bad
        return check
    return dict(entry=entry, make_inputs=seeded(lambda s: [rnd(n, 96, 97 + s, 0.2), rnd(m, 96, 99 + s, 0.2)]), reference=reference)


@case("sim_dense_stats_stored", ["sim_dense_stats"])
def _():
    return _dense_stats_case(2500, 1900, True)          # 4.75 M values: the one-sweep median


@case("sim_dense_stats_streamed", ["sim_dense_stats"])
def _():
    return _dense_stats_case(2500, 1900, False)


def _combined_edges_check(F, P, thr, lh, lg, set_tol=TOL):
    """Edges of K >= thr against the oracle's K: K is pinned to TOL (the scores go through expf), so an entry within set_tol of
    the threshold may fall on either side; every other entry must agree, and the weights are the oracle's to TOL."""
    K = oracle.sim_dense_combined(F, P, lh, lg)

    def check(got):
        ei, ew = np.asarray(got[0]), np.asarray(got[1])
        bad = []
        if ei.shape[1] and np.abs(K[ei[0], ei[1]] - ew).max() > TOL:
            bad.append("weights differ from the oracle's K")
        kept = np.zeros(K.shape, bool)
        kept[ei[0], ei[1]] = True
        if (kept & (K < thr - set_tol)).any() or (~kept & (K > thr + set_tol)).any():
            bad.append("edge set differs from the oracle's beyond the score tolerance")
        if ei.shape[1] and not (np.diff(ei[0] * K.shape[0] + ei[1]) > 0).all():
            bad.append("edges not row-major")
        return bad
    return check


@case("combined_offdiag_median_radix", ["combined_offdiag_median"], nonsync=True)      # 489300 values: the radix path
def _():
    def reference(F, P):
        want = oracle.offdiag_lower_median(oracle.sim_dense_combined(F, P, 0.7, 1.3))
        return lambda got: [] if abs(float(got) - want) <= TOL else [f"median {float(got)} vs {want}"]
    return dict(entry=lambda F, P: ops_().combined_offdiag_median(F, P, 0.7, 1.3, 128), make_inputs=seeded(lambda s: list(_fp(700, 48, 2, 101 + s))),
                reference=reference)


@case("combined_threshold_edges", ["combined_threshold_edges"])
def _():
    return dict(entry=lambda F, P: ops_().combined_threshold_edges(F, P, 0.4, 0.7, 1.3, 128),
                make_inputs=seeded(lambda s: list(_fp(700, 48, 2, 103 + s))), reference=lambda F, P: _combined_edges_check(F, P, 0.4, 0.7, 1.3))


@case("segment_sort_clique_pairs", ["segment_sort", "clique_pairs"])
def _():
    n, S = 5000, 300

    def entry(lab):
        seg = ops_().segment_sort(lab, S)
        lo, hi = ops_().clique_pairs(seg)
        return seg.counts, seg.offsets, seg.order, lo, hi

    def reference(lab):
        order = np.argsort(lab, kind="stable").astype(np.int64)
        counts = np.bincount(lab, minlength=S).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        lo, hi = [], []
        for c in range(S):
            m = order[off[c]:off[c + 1]]
            a, b = np.triu_indices(len(m), 1)
            lo.append(m[a]), hi.append(m[b])
        return [counts, off, order, np.concatenate(lo), np.concatenate(hi)]
    return dict(entry=entry, make_inputs=seeded(lambda s: [_labels_inputs(n, S, 0, s)[0]]), reference=reference)


@case("threshold_edges", ["threshold_edges"])
def _():
    return dict(entry=lambda K: ops_().threshold_edges(K, 0.9), make_inputs=seeded(_thr_plain_inputs),
                reference=lambda K: list(oracle.threshold_edges(K, 0.9)))


def _blobs(n, d, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((max(2, n // 40), d)).astype(np.float32) * 2
    return (c[rng.integers(0, len(c), n)] + rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def _lattice(seed):
    """20 x 2, duplicate rows: empty clusters, relocation (tests/test_gpu_kmeans_segmented.py, seed 27)."""
    r = np.random.default_rng(seed)
    r.choice([20, 30, 50]); r.choice([6, 8, 12])
    return r.integers(0, 4, (20, 2)).astype(np.float32) + r.standard_normal((20, 2)).astype(np.float32) * float(r.choice([0, 0.01, 0.3]))


def _kmeans_case(data, k):
    from oracle import kmeans_restate as kr

    def entry(X):
        km = import_module("multimodal_fusion_amd.kmeans")
        first, u = km.sklearn_stream(42, 10, k, X.shape[0])
        labels, centres, info, seeds = ops_().kmeans_fit(X, k, first, u, return_seeds=True)
        return labels, centres, seeds, {q: info[q] for q in ("best_init", "inertia", "n_iter", "n_iter_per_init", "inertia_per_init")}

    def reference(X):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ri = {}
            rl = kr.kmeans_fit_predict(X, k, info=ri)

        def check(got):
            bad = sg.diff(got[0], rl.astype(np.int64), "labels")
            bad += sg.diff(got[2], np.stack([p["seeds"] for p in ri["per_init"]]).astype(np.int64), "seeds")
            if got[3]["best_init"] != ri["best_init"]:
                bad.append("best restart differs from the restatement")
            return bad
        return check
    return dict(entry=entry, make_inputs=seeded(data), reference=reference)


@case("kmeans_fit", ["kmeans_fit"])
def _():
    return _kmeans_case(lambda s: [_blobs(1500, 16, 1000 + s)], 8)


@case("kmeans_fit_relocating_lattice", ["kmeans_fit"])
def _():
    return _kmeans_case(lambda s: [_lattice(27) if s == 1 else _lattice(28)], 12)


@case("kmeans_fit_segmented_two_groups", ["kmeans_fit_segmented"])
def _():
    from oracle import kmeans_restate as kr
    k, sizes = 12, [20, 37, 64] * 50                    # 150 segments x 10 restarts x 12 clusters > 16384: two lockstep groups
    ptr = np.array(offsets(sizes), dtype=np.int64)

    def data(s):
        rng = np.random.default_rng(2000 + s)
        parts = [_lattice(27 + i % 2) if n == 20 else _blobs(n, 2, int(rng.integers(1 << 30))) for i, n in enumerate(sizes)]
        return [np.concatenate(parts, 0)]

    def entry(X):
        km = import_module("multimodal_fusion_amd.kmeans")
        first, u = km.segment_streams(42, 10, k, sizes)
        labels, centres, info, seeds = ops_().kmeans_fit_segmented(X, ptr, k, first, u, return_seeds=True)
        assert len({i["lockstep_iterations"] for i in info}) >= 1
        return labels, centres, seeds, [i["best_init"] for i in info], [i["n_iter"] for i in info]

    def reference(X):
        import warnings
        rl = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for a, b in list(zip(ptr[:-1], ptr[1:]))[:24] + [(ptr[-2], ptr[-1])]:     # the first 24 segments and the last one
                rl.append((int(a), int(b), kr.kmeans_fit_predict(X[a:b], k).astype(np.int64)))
        return lambda got: [m for a, b, lab in rl for m in sg.diff(got[0][a:b], lab, f"labels[{a}:{b}]")]
    return dict(entry=entry, make_inputs=seeded(data), reference=reference)


# ---- the mirrors, as callers use them ------------------------------------------------------------
def _knn_kmeans_ref(Xs, k, H):
    from oracle import kmeans_restate as kr, ref_restate
    Xt = T(Xs)
    labels = kr.kmeans_fit_predict(Xs, H)
    pairs = np.concatenate([ref_restate.knn_pairs_exact(Xt, k), ref_restate.clique_pairs(labels, H)], axis=0)
    ei, ew = ref_restate.dedup_and_weight(Xt, pairs)
    return ei.numpy(), ew.numpy()


def _edges_check(want_ei, want_ew):
    def check(got):
        return sg.diff(got[0], want_ei, "edge_index") + sg.diff(got[1], want_ew, "edge_weights", atol=TOL)
    return check


@case("build_hypergraph_knn_kmeans", ["simtopk", "kmeans_fit", "segment_sort", "clique_pairs", "knn_pairs", "edge_cosine"])
def _():
    def entry(W, Tm):
        bh = import_module("multimodal_fusion_amd.build_hypergraph")
        ei, ew, stats = bh.build_hypergraph_knn_kmeans(W, Tm, None, 5, 6)
        return ei, ew, stats["num_edges"]

    def reference(W, Tm):
        ei, ew = _knn_kmeans_ref(np.concatenate([W, Tm], 0), 5, 6)
        inner = _edges_check(ei, ew)
        return lambda got: inner(got) + ([] if got[2] == ei.shape[1] else ["num_edges"])
    return dict(entry=entry, make_inputs=seeded(lambda s: [rnd(300, 24, 201 + s), rnd(40, 24, 211 + s)]), reference=reference)


@case("build_weighted_hypergraph_segmented", ["sim_dense_combined_segmented", "offdiag_lower_median_segmented", "threshold_edges_segmented"])
def _():
    sizes = [40, 50, 300, 60, 2, 45]
    ptr = offsets(sizes)

    def entry(F, P):
        wh = import_module("multimodal_fusion_amd.weighted_hypergraph")
        return wh.build_weighted_hypergraph_segmented(F, P, 1.0, 1.0, 0.8, ptr=ptr)

    def reference(F, P):
        def check(got):
            ei, ew, eptr = (np.asarray(g) for g in got)
            bad = [] if eptr[0] == 0 and eptr[-1] == ei.shape[1] == ew.shape[0] and len(eptr) == len(ptr) else ["edge_ptr"]
            for s, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
                K = oracle.sim_dense_combined(F[a:b], P[a:b], 1.0, 1.0)
                thr = oracle.offdiag_lower_median(K) * 0.8
                e0, e1 = int(eptr[s]), int(eptr[s + 1])
                # the threshold is 0.8 x the median of a K pinned to TOL, so it is itself within TOL: 2 TOL for the edge set
                bad += [f"segment {s}: {m}" for m in _combined_edges_check(F[a:b], P[a:b], thr, 1.0, 1.0, 2 * TOL)((ei[:, e0:e1] - a, ew[e0:e1]))]
            return bad
        return check
    return dict(entry=entry, make_inputs=seeded(lambda s: list(_fp(ptr[-1], 24, 2, 221 + s))), reference=reference)


@case("build_hypergraph_knn_kmeans_segmented", ["simtopk_segmented", "kmeans_fit_segmented", "knn_clique_edges", "edge_cosine"])
def _():
    w_sizes, t_sizes = [120, 64, 200], [10, 0, 30]
    wp, tp = offsets(w_sizes), offsets(t_sizes)

    def entry(W, Tm):
        kk = import_module("multimodal_fusion_amd.knn_kmeans_hypergraph")
        ei, ew, eptr, stats = kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, 5, 6, wsi_ptr=wp, tma_ptr=tp)
        return ei, ew, eptr, stats["num_edges"]

    def reference(W, Tm):
        eis, ews, base, counts = [], [], 0, []
        for s in range(len(w_sizes)):
            Xs = np.concatenate([W[wp[s]:wp[s + 1]], Tm[tp[s]:tp[s + 1]]], 0)
            ei, ew = _knn_kmeans_ref(Xs, 5, 6)
            eis.append(ei + base), ews.append(ew), counts.append(ei.shape[1])
            base += len(Xs)
        ei, ew, eptr = np.concatenate(eis, 1), np.concatenate(ews), np.array(offsets(counts), np.int64)
        inner = _edges_check(ei, ew)
        return lambda got: inner(got) + sg.diff(got[2], eptr, "edge_ptr") + ([] if got[3] == ei.shape[1] else ["num_edges"])
    return dict(entry=entry, make_inputs=seeded(lambda s: [rnd(sum(w_sizes), 24, 231 + s), rnd(sum(t_sizes), 24, 241 + s)]),
                reference=reference)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_entry_behind_a_closed_gate(mmf, name):
    c = CASES[name]
    kw = c["build"]()
    try:
        res = sg.run_gated(kw["entry"], kw["make_inputs"], kw["reference"], name=name, nonsync=c["nonsync"], atol=c["atol"],
                           calls=c["calls"], finish=kw.get("finish"))
    except RuntimeError as e:
        if "HIP error" in str(e) or "(code -3)" in str(e):          # a fault of the device: nothing more is started on it
            pytest.exit(f"{name}: the HIP runtime reported a failure, stopping the run: {e}", returncode=3)
        raise
    assert res.gate_ms >= 0.9 * sg.GATE_MIN_MS, f"{name}: the gate lasted {res.gate_ms:.1f} ms"
    if c["nonsync"]:
        assert res.returned_closed, name


def test_every_public_function_and_every_entry_has_a_case(mmf):
    """One gated case per public function of ops.py; every entry the table calls "none" is gated as not synchronising."""
    import inspect
    public = {n for n, f in inspect.getmembers(mmf.ops, inspect.isfunction)
              if f.__module__ == mmf.ops.__name__ and not n.startswith("_")} - {"padded_dim", "fast_scan_supported", "last_query_order"}
    covered = {f for c in CASES.values() for f in c["covers"]}
    assert public <= covered, sorted(public - covered)
    gated_none = {"mmf_" + f for c in CASES.values() if c["nonsync"] for f in c["covers"]}
    gated_none |= {"mmf_edge_cosine", "mmf_knn_pairs", "mmf_array_stats", "mmf_threshold_edges_count", "mmf_threshold_edges_fill",
                   "mmf_threshold_edges_segmented_count", "mmf_threshold_edges_segmented_fill", "mmf_knn_clique_edges_count",
                   "mmf_knn_clique_edges_fill"}                          # the *_c_entry(ies) cases above
    none = {e for e, (sync, _) in SYNC.items() if sync == "none"}
    # mmf_clique_pairs and mmf_combined_threshold_edges are count-then-fill entries whose wrappers read the count: gated through them
    assert none - gated_none <= {"mmf_clique_pairs", "mmf_combined_threshold_edges"}, sorted(none - gated_none)
    import multimodal_fusion_amd as m
    streamed = {e for e in m._lib.EXPORTS if e not in ("mmf_version", "mmf_last_error", "mmf_padded_dim", "mmf_fast_scan_supported",
                                                         "mmf_debug_query_order", "mmf_debug_symmetric_schedule")}
    assert streamed == set(SYNC), sorted(streamed ^ set(SYNC))


# ---------------------------------------------------------------------------------------------------
# the harness's self-test: a call routed to the null stream must be REPORTED
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simtopk_16bit_no_flagged_rows", "offdiag_lower_median_segmented_few"])
def test_harness_reports_a_call_on_the_wrong_stream(mmf, monkeypatch, name):
    """ops._stream hands the library the null stream while the current torch stream is the gated side stream: the call sees only
    the decoy (valid data), and run_gated must report the mismatch.  A harness that cannot see this looks like a clean library."""
    c = CASES[name]
    kw = c["build"]()
    real = mmf.ops._stream
    state = {"wrong": False}
    monkeypatch.setattr(mmf.ops, "_stream", lambda dev: ctypes.c_void_p(0) if state["wrong"] else real(dev))
    calls = {"n": 0}

    def entry(*a):
        calls["n"] += 1
        state["wrong"] = calls["n"] > 1                 # the idle call (the first) is routed properly
        try:
            return kw["entry"](*a)
        finally:
            state["wrong"] = False
    res = sg.run_gated(entry, kw["make_inputs"], kw["reference"], name="selftest_" + name, nonsync=False, atol=c["atol"],
                       report=True)
    assert any("vs idle default stream" in m for m in res.mismatches), res.mismatches
    assert any("vs reference" in m for m in res.mismatches), res.mismatches


# ---------------------------------------------------------------------------------------------------
# the workspace: per (device, stream), grown and released with work pending
# ---------------------------------------------------------------------------------------------------
def _median_blocks(sizes, seed):
    total = sum(v * v for v in sizes)
    K = np.random.RandomState(seed).rand(total).astype(np.float32)
    kp = offsets([v * v for v in sizes])
    ref = np.array([oracle.offdiag_lower_median(K[kp[s]:kp[s + 1]].reshape(v, v)) for s, v in enumerate(sizes)], np.float32)
    return T(K), ref


def _gated_pair(side, truth_pinned, decoy):
    """decoy on the device, a gate on `side`, the truth copied in behind it; returns (X, gate, produced)."""
    X = decoy.cuda()
    torch.cuda.synchronize()
    gate = sg.Gate(side, sg.GATE_MIN_MS)
    produced = torch.cuda.Event()
    with torch.cuda.stream(side):
        X.copy_(truth_pinned, non_blocking=True)
        produced.record(side)
    assert not produced.query(), "gate too short"
    return X, gate, produced


def test_two_streams_do_not_share_a_workspace(mmf):
    """s1: gate, then the segmented median of K1 (it does not synchronise).  s2, no gate: the same entry on K2 of the same shape,
    to completion.  Then s1 opens.  With a workspace keyed by the device alone the second call runs in the first call's
    scratch, and stages its host tables over the first call's, before the first has used either."""
    sizes = [5, 130, 2, 64, 257]
    # K2 has K1's shape (87074 values) in another layout: 21766 small blocks, whose select states and host tables need a far
    # larger workspace.  Were the workspace shared, the second call would have to free the one the first call is waiting to use.
    sizes2 = [3, 3] + [2] * 21764
    assert sum(v * v for v in sizes2) == sum(v * v for v in sizes)
    s1, s2 = sg.streams()
    K1, ref1 = _median_blocks(sizes, 301)
    K2, ref2 = _median_blocks(sizes2, 302)
    decoy, _ = _median_blocks(sizes, 303)
    X1, gate, produced = _gated_pair(s1, K1.pin_memory(), decoy)
    X2 = K2.cuda()                                       # a blocking copy on the default stream: it does not wait for s1
    assert not produced.query(), "gate too short"
    with torch.cuda.stream(s1):
        out1 = mmf.ops.offdiag_lower_median_segmented(X1, ptr=offsets(sizes))
    assert not produced.query(), "the entry on s1 did not return while its gate was closed"
    with torch.cuda.stream(s2):
        out2 = mmf.ops.offdiag_lower_median_segmented(X2, ptr=offsets(sizes2))
        s2.synchronize()
        got2 = out2.cpu().numpy()
    assert not produced.query(), (f"the call on s2 came back only after s1's gate ({sg.GATE_MIN_MS} ms asked) had opened: it waited for "
                                  "s1's pending work (a workspace shared between the streams?), or the gate is too short")
    sg.churn()
    s1.synchronize()
    sg.note(f"case two_streams: gate {gate.measured_ms():.1f} ms")
    assert np.array_equal(got2.view(np.uint32), ref2.view(np.uint32)), "the ungated stream's medians"
    assert np.array_equal(out1.cpu().numpy().view(np.uint32), ref1.view(np.uint32)), "the gated stream's medians"


def test_workspace_growth_behind_a_gate(mmf):
    """Behind one gate: a small call that does not synchronise, then one that needs a larger workspace.  The first call's work
    must be over before its workspace is freed (the growth synchronises the stream), and both results must be right."""
    small = [5, 130, 2, 64]
    s1 = sg.streams()[0]
    mmf._lib.lib().mmf_release_workspaces()              # so that the large call has to grow what the small one allocated
    Ks, ref_s = _median_blocks(small, 311)
    Xh = unit_rows(3000, 512, 312).numpy()               # sim_dense: 6 MB of f32 operand image, past the small call's 1 MiB of slack
    ref_l = oracle.sim_dense(Xh, metric="cosine")
    decoy, _ = _median_blocks(small, 313)
    Xs, gate, produced = _gated_pair(s1, Ks.pin_memory(), decoy)
    Xl = T(Xh).cuda()                                    # a blocking copy on the default stream: it does not wait for s1
    assert not produced.query(), "gate too short"
    with torch.cuda.stream(s1):
        out_s = mmf.ops.offdiag_lower_median_segmented(Xs, ptr=offsets(small))
        assert not produced.query(), "the small call did not return while the gate was closed"
        out_l = mmf.ops.sim_dense(Xl, metric="cosine")
        s1.synchronize()
    sg.note(f"case workspace_growth: gate {gate.measured_ms():.1f} ms")
    assert np.array_equal(out_s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32)), "the small call's medians"
    assert np.array_equal(out_l.cpu().numpy().view(np.uint32), ref_l.view(np.uint32)), "the large call's matrix"


def test_release_with_work_pending(mmf):
    """mmf_release_workspaces() with work pending behind a gate returns only after that work, whose results are right."""
    sizes = [5, 130, 2, 64, 257]
    s1 = sg.streams()[0]
    K, ref = _median_blocks(sizes, 321)
    decoy, _ = _median_blocks(sizes, 323)
    X, gate, produced = _gated_pair(s1, K.pin_memory(), decoy)
    with torch.cuda.stream(s1):
        out = mmf.ops.offdiag_lower_median_segmented(X, ptr=offsets(sizes))
        done = torch.cuda.Event()
        done.record(s1)
    assert not produced.query(), "the entry did not return while the gate was closed"
    assert mmf._lib.lib().mmf_release_workspaces() == 0
    assert done.query(), "mmf_release_workspaces returned while work was pending in a workspace it freed"
    sg.note(f"case release_pending: gate {gate.measured_ms():.1f} ms")
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    out2 = mmf.ops.offdiag_lower_median_segmented(K.cuda(), ptr=offsets(sizes))            # and the library goes on working
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), ref.view(np.uint32))
