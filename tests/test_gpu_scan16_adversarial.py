"""The 16-bit scan on worst-case rounding data (tests/adversarial16.py): rows whose true top-k columns A have approximate
values BELOW kk + 3 other columns B by 0.7 .. 0.98 of the scan's error margin.  The scan gets such a row right only if every
place that uses the margin uses all of it: the lane lists, thresholds shared between column splits and panels, the symmetric
launch's threshold image and pruned filing, select's pruning, the 5-slot-bit lists.  tests/test_scan16_margin_cpu.py certifies
the data (oracle picks A, approximation picks B, sharpness above its floor); the first test here pins the restatement that
certificate rests on to the device's prep kernel.

Every case checks ids and scores of ALL rows against the oracle bit for bit (rbf scores to 1e-5), that the 16-bit path
answered (precision_used 2 / 3) and that the exact rescan did not rescue it (fallback_rows == 0, or at most what the parent
commit measured: PARENT_FLAGGED).  With the margin halved (`margin = 1.0f * (e1 + e2)`) every candidate-side and query-side
case fails with an index mismatch.
"""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adversarial16 as adv   # noqa: E402

pytestmark = pytest.mark.gpu

PRECISION_USED = {"f16": 2, "bf16": 3}
TORCH_16 = {"f16": torch.float16, "bf16": torch.bfloat16}
SYM_KEYS = ("MMF_SYMMETRIC", "MMF_SYMMETRIC_G", "MMF_SYMMETRIC_LIVE", "MMF_SYMMETRIC_PRUNE")

# fallback_rows of commit 822c0c3 (the parent of the change that introduced this file, which touches no library code) per case
# id, where it is not zero.  The symmetric scan with bf16 operands flags one row of the 1500, in all four modes; the q rows are
# not rescued by it: with the margin halved the same cases return B columns for them.
PARENT_FLAGGED = {f"sym-bf16-live{live}-prune{prune}": 1 for live in (0, 1) for prune in (0, 1)}


@pytest.fixture(scope="module")
def mmf():
    import multimodal_fusion_amd as m
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


@contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in SYM_KEYS}
    for k in SYM_KEYS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


def check(fam, got, case, ref=None):
    idx, val, st = got
    ridx, rval = ref if ref is not None else adv.reference(fam)
    print(f"{case}: precision_used {st['precision_used']} col_splits {st['col_splits']} scan_grid {st['scan_grid']} "
          f"fallback_rows {st['fallback_rows']} overflow_rows {st['overflow_rows']} query_order {st['query_order']}")
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    bad = np.flatnonzero((idx != ridx).any(axis=1))
    assert bad.size == 0, f"indices differ from the oracle in rows {bad[:8].tolist()} (q rows: {fam.q_rows.tolist()})"
    if fam.metric == "rbf":
        assert np.allclose(val, rval, rtol=0, atol=1e-5), "scores differ from the oracle"
    else:
        assert np.array_equal(val.view(np.int32), rval.view(np.int32)), "scores differ from the oracle"
    assert st["precision_used"] == PRECISION_USED[fam.operand] and st["scan_grid"] > 0
    assert st["fallback_rows"] <= PARENT_FLAGGED.get(case, 0)
    return st


def plain(mmf, fam, **kw):
    return mmf.simtopk(cuda(fam.X), cuda(fam.Y), metric=fam.metric, lam=fam.lam, k=fam.k, exclude_self=fam.Y is None,
                       precision=fam.precision, return_stats=True, **kw)


def prepared_side(ops, X, metric, operand, maxn, pad):
    """mmf_row_scalars + mmf_prep_rows of the rows X into buffers with `pad` spare rows (zero operands, bias -inf)."""
    n, dp = X.shape[0], ops.padded_dim(X.shape[1])
    scal = torch.zeros(n + pad, device="cuda")
    ops.row_scalars(X, metric, scal[:n], maxn)
    side = dict(scal=scal, Z=torch.zeros((n + pad, dp), dtype=TORCH_16[operand], device="cuda"))
    for key in ("zn", "rn", "un", "cb"):
        side[key] = torch.full((n + pad,), float("-inf") if key == "cb" else 0.0, device="cuda")
    return side


def run_prep(ops, side, X, metric, operand, maxn, max4):
    n = X.shape[0]
    ops.prep_rows(X, metric, operand, side["scal"][:n], maxn, side["Z"][:n], side["zn"][:n], side["rn"][:n], side["un"][:n],
                  side["cb"][:n], max4)


@pytest.mark.parametrize("operand", adv.OPERANDS)
@pytest.mark.parametrize("kind,metric,d", [("cand", "dot", 128), ("cand", "neg_sq_l2", 128), ("cand", "cosine", 128),
                                           ("query", "dot", 128), ("cand", "dot", 500), ("cand", "dot", 1000)])
def test_restatement_is_the_prep_kernel(mmf, kind, metric, d, operand):
    """Z and cb bit for bit, zn / rn / un and the four maxima to 1e-5: the sharpness certified on the CPU is certified for the
    operand image the device scans."""
    fam = adv.rect_family(kind, metric, operand) if d == 128 else adv.rect_family(kind, metric, operand, "ba", d, 5, adv.DIM_COLS)
    ops = mmf.ops
    X, Y = cuda(fam.X), cuda(fam.Y)
    maxn = torch.zeros(1, device="cuda")
    q, c = prepared_side(ops, X, metric, operand, maxn, 0), prepared_side(ops, Y, metric, operand, maxn, 0)   # both sides raise maxn first
    mq, mc = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    run_prep(ops, q, X, metric, operand, maxn, mq)
    run_prep(ops, c, Y, metric, operand, maxn, mc)
    rq, rc, _ = adv.restated(fam)
    for dev, ref, m4 in ((q, rq, mq), (c, rc, mc)):
        assert np.array_equal(dev["scal"].cpu().numpy(), ref["scal"])
        assert np.array_equal(dev["Z"].view(torch.int16).cpu().numpy().view(np.uint16), ref["zbits"]), "operand image differs"
        assert np.array_equal(dev["cb"].cpu().numpy(), ref["cb"])
        for key in ("zn", "rn", "un"):
            assert np.allclose(dev[key].cpu().numpy(), ref[key], rtol=1e-5, atol=0), key
        assert np.allclose(m4.cpu().numpy(), ref["maxima"], rtol=1e-5, atol=0)
    assert float(rc["maxima"][1]) > 0 or kind == "query"      # the query-side family's columns round exactly: RB = 0


@pytest.mark.parametrize("col_splits,order", [(1, "ba"), (0, "ba"), (8, "ba"), (8, "ab")])
@pytest.mark.parametrize("operand", adv.OPERANDS)
@pytest.mark.parametrize("kind,metric", adv.KINDS)
def test_plain_rectangular(mmf, kind, metric, operand, col_splits, order):
    """col_splits = 1: one list pair per row and no pruning in select — the lane lists alone meet B (columns 64..) long before A
    (columns 3600..); 8: B in the first column range and A in the last ("ba") or the reverse ("ab"), so A has to survive a
    threshold that another workgroup's lists reached; 0: the call's own choice.  (One list pair is not run in the order "ab": a
    list that holds A already and then meets kk + 3 columns B has room for both and never consults its margin.)"""
    fam = adv.rect_family(kind, metric, operand, order)
    st = check(fam, plain(mmf, fam, col_splits=col_splits), f"rect-{kind}-{metric}-{operand}-s{col_splits}-{order}")
    assert col_splits == 0 or st["col_splits"] == col_splits


@pytest.mark.parametrize("query_order", ["on", "off"])
@pytest.mark.parametrize("operand", adv.OPERANDS)
@pytest.mark.parametrize("kind", ["cand", "query"])
def test_query_order(mmf, kind, operand, query_order):
    """The q rows sit among ordinary rows with smaller margins: under the query order their positions are not their rows."""
    fam = adv.rect_family(kind, "dot", operand)
    st = check(fam, plain(mmf, fam, query_order=query_order), f"order-{kind}-{operand}-{query_order}")
    assert st["query_order"] == (query_order == "on")


@pytest.mark.parametrize("col_splits", [1, 0])
@pytest.mark.parametrize("operand", adv.OPERANDS)
@pytest.mark.parametrize("d,k", adv.DIM_K)
def test_list_capacities_and_padded_dims(mmf, d, k, operand, col_splits):
    """15-, 16- and 32-entry lists (the last with the doubled slot term) at padded dims 128, 512 and 1024 (split-k kernel)."""
    fam = adv.rect_family("cand", "dot", operand, "ba", d, k, adv.DIM_COLS)
    check(fam, plain(mmf, fam, col_splits=col_splits), f"dims-{d}-{k}-{operand}-s{col_splits}")


@pytest.mark.parametrize("operand", adv.OPERANDS)
@pytest.mark.parametrize("d,k", [(128, 5), (128, 30), (500, 5)])
def test_plain_self(mmf, d, k, operand):
    """X against itself without the symmetric schedule: q, A and B rows in different row blocks."""
    fam = adv.self_family(operand, d, k)
    with environment(MMF_SYMMETRIC=0):
        check(fam, plain(mmf, fam), f"self-{d}-{k}-{operand}")


@pytest.mark.parametrize("prune", [0, 1])
@pytest.mark.parametrize("live", [0, 1])
@pytest.mark.parametrize("operand", adv.OPERANDS)
def test_symmetric_self(mmf, operand, live, prune):
    """The symmetric scan forced, one row block per super-block: q rows in super-blocks 0, 0, 2 and 5, B in 1, A in 4, so some
    (q, A) products are made in q's workgroup and some in A's and reach q through the log and its received list."""
    fam = adv.self_family(operand, 500, 5)
    n = len(fam.X)
    with environment(MMF_SYMMETRIC=1, MMF_SYMMETRIC_G=1, MMF_SYMMETRIC_LIVE=live, MMF_SYMMETRIC_PRUNE=prune):
        st = check(fam, plain(mmf, fam, query_order="off"), f"sym-{operand}-live{live}-prune{prune}")
    assert st["scan_grid"] == 2 * mmf._lib.lib().mmf_debug_symmetric_schedule((n + 255) // 256, 1, 0, None, 0), "not the symmetric scan"


@pytest.mark.parametrize("operand", adv.OPERANDS)
def test_segmented(mmf, operand):
    """simtopk_segmented with the family as the middle one of three segments."""
    fam = adv.self_family(operand, 128, 5, adv.SELF_ROWS, "gauss")
    rng = np.random.RandomState(7)
    before, after = adv.gauss(rng, 200, 128, 100.0, True), adv.gauss(rng, 150, 128, 100.0, True)      # like the family's own fillers
    X = np.concatenate([before, fam.X, after])
    ptr = [0, 200, 200 + len(fam.X), 350 + len(fam.X)]
    parts = [oracle.simtopk(X[a:b], X[a:b], metric="dot", k=fam.k, exclude_self=True, row_offset=a, col_offset=a) for a, b in zip(ptr[:-1], ptr[1:])]
    ref = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    assert np.array_equal(ref[0][200:ptr[2]] - 200, adv.reference(fam)[0])
    got = mmf.simtopk_segmented(cuda(X), ptr=ptr, metric="dot", k=fam.k, precision=fam.precision, return_stats=True)
    check(fam, got, f"seg-{operand}", ref=ref)


@pytest.mark.parametrize("query_order", ["off", "on"])
@pytest.mark.parametrize("operand", adv.OPERANDS)
@pytest.mark.parametrize("kind", ["cand", "query"])
def test_paneled(mmf, kind, operand, query_order):
    """mmf_simtopk_panels on two panels of 2048 columns: B in the first, A in the second.  A survives a threshold that the
    scan of another panel published."""
    fam = adv.rect_family(kind, "dot", operand)
    ops = mmf.ops
    X, Y = cuda(fam.X), cuda(fam.Y)
    n, m, P = X.shape[0], Y.shape[0], 2
    maxn = torch.zeros(1, device="cuda")
    q, c = prepared_side(ops, X, "dot", operand, maxn, 512), prepared_side(ops, Y, "dot", operand, maxn, 256)
    mq, mc = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    run_prep(ops, q, X, "dot", operand, maxn, mq)
    run_prep(ops, c, Y, "dot", operand, maxn, mc)
    seg = m // P
    panels = []
    for p in range(P):
        Zp = torch.zeros((seg + 256, c["Z"].shape[1]), dtype=TORCH_16[operand], device="cuda")
        cbp = torch.full((seg + 256,), float("-inf"), device="cuda")
        Zp[:seg], cbp[:seg] = c["Z"][p * seg:(p + 1) * seg], c["cb"][p * seg:(p + 1) * seg]
        ev = torch.cuda.Event()
        ev.record()
        panels.append(dict(Z=Zp, cb=cbp, m=seg, m_pad=seg, seg_len=seg, seg_stride=seg, id_base=p * seg, event=ev))
    assert fam.b_cols.max() < seg <= fam.a_cols.min()
    got = ops.simtopk_panels(X, Y, q, c["scal"], panels, mc, operand=operand, metric="dot", k=fam.k, exclude_self=False,
                             return_stats=True, query_order=query_order)
    st = check(fam, got, f"panels-{kind}-{operand}-{query_order}")
    assert st["query_order"] == (query_order == "on")
