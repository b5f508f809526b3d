"""The ragged-batch module without a GPU: one offsets parser for both wordings ("segment", "slide"), the two-sided description,
block offsets, segment ids, budget groups and scikit-learn's two size checks; and the import rules that keep it the one copy."""
import glob
import importlib.util
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multimodal-fusion_amd")
UNITS = [dict(unit="segment"), dict(unit="slide", min_rows=1)]


def _rg():
    import multimodal_fusion_amd  # noqa: F401
    return import_module("multimodal_fusion_amd.ragged")


# The bad inputs of the CPU tests of every module that reads offsets, on their sizes: a side of 10 rows (no prefix) and one of 6
# ("tma_").  {u} is the unit.
BAD = [
    (10, "", dict(ptr=[0, 5, 9]), r"{u} 1: ptr must end at 10 \(got 9\)"),
    (10, "", dict(ptr=[0, 5, 9]), "ptr must start at 0 and end at 10"),
    (10, "", dict(ptr=[0, 4, 9]), "end at 10"),
    (10, "", dict(ptr=[1, 5, 10]), r"{u} 0: ptr must start at 0 \(got 1\)"),
    (10, "", dict(ptr=[0, 6, 4, 10]), r"{u} 1: ptr decreases \(6 -> 4\)"),
    (10, "", dict(ptr=[0, 6, 5, 10]), r"{u} 1: ptr decreases \(6 -> 5\)"),
    (10, "", dict(ptr=[]), "{u} 0: ptr describes no {u}"),
    (10, "", dict(ptr=[0]), "{u} 0: ptr describes no {u}"),
    (10, "", dict(batch=torch.tensor([0, 0, 0, 1, 1, 1, 0, 1, 1, 1])), r"{u} 0: batch must be sorted \(row 6 follows {u} 1\)"),
    (10, "", dict(batch=torch.tensor([0, 0, 1, 0, 1, 1, 1, 1, 1, 1])), "{u} 0: batch must be sorted"),
    (10, "", dict(batch=torch.tensor([-1, -1, 0, 0, 0, 0, 0, 0, 0, 0])), "{u} -1: batch must be non-negative"),
    (10, "", dict(batch=torch.tensor([-1, 0, 0, 0, 0, 0, 0, 0, 0, 0])), "{u} -1: batch must be non-negative"),
    (10, "", dict(batch=torch.zeros(9, dtype=torch.long)), r"{u} 0: batch must hold one {u} id per row \(10\)"),
    (10, "", dict(batch=torch.zeros((2, 5), dtype=torch.long)), "batch must hold one {u} id per row"),
    (0, "", dict(batch=torch.zeros(0, dtype=torch.long)), "{u} 0: batch describes no {u}"),
    (10, "", dict(ptr=[0, 10], batch=torch.zeros(10, dtype=torch.long)), "exactly one of ptr / batch"),
    (10, "", dict(), "exactly one of ptr / batch"),
    (6, "tma_", dict(ptr=[0, 3, 5]), r"{u} 1: tma_ptr must end at 6 \(got 5\)"),
    (6, "tma_", dict(ptr=[0, 3, 5]), "tma_ptr must start at 0 and end at 6"),
    (6, "tma_", dict(ptr=[0, 4, 3, 6]), r"{u} 1: tma_ptr decreases \(4 -> 3\)"),
    (6, "tma_", dict(batch=torch.tensor([-1, 0, 0, 0, 1, 1])), "{u} -1: tma_batch must be non-negative"),
    (6, "tma_", dict(), "exactly one of tma_ptr / tma_batch"),
]
# segments without rows: an error only where the caller asks for rows
EMPTY = [
    (10, "", dict(ptr=[0, 6, 6, 10]), "{u} 1 has 0 rows in ptr, need at least 1", [0, 6, 6, 10]),
    (10, "", dict(batch=torch.tensor([0, 0, 0, 0, 0, 2, 2, 2, 2, 2])), "{u} 1 has 0 rows in batch, need at least 1", [0, 5, 5, 10]),
    (6, "tma_", dict(ptr=[0, 6, 6]), "{u} 1 has 0 rows in tma_ptr, need at least 1", [0, 6, 6]),
    (6, "tma_", dict(batch=torch.tensor([0, 0, 0, 2, 2, 2])), "{u} 1 has 0 rows in tma_batch, need at least 1", [0, 3, 3, 6]),
]


@pytest.mark.parametrize("mode", UNITS, ids=["segment", "slide"])
@pytest.mark.parametrize("rows,side,kw,match", BAD)
def test_offsets_reject_bad_input_in_both_wordings(rows, side, kw, match, mode):
    with pytest.raises(ValueError, match="^caller: .*" + match.replace("{u}", mode["unit"])):
        _rg().offsets(kw.get("ptr"), kw.get("batch"), rows, side=side, what="caller", **mode)


@pytest.mark.parametrize("rows,side,kw,match,want", EMPTY)
def test_offsets_ask_for_rows_only_where_the_caller_does(rows, side, kw, match, want):
    rg = _rg()
    assert rg.offsets(kw.get("ptr"), kw.get("batch"), rows, side=side, what="caller").tolist() == want
    with pytest.raises(ValueError, match="^caller: " + match.replace("{u}", "slide")):
        rg.offsets(kw.get("ptr"), kw.get("batch"), rows, side=side, what="caller", unit="slide", min_rows=1)


def test_offsets_from_ptr_and_from_batch_agree():
    rg = _rg()
    sizes = [3, 0, 4, 3]
    ptr = [0, 3, 3, 7, 10]
    batch = torch.tensor([0] * 3 + [2] * 4 + [3] * 3)                  # id 1 is skipped: a segment without rows
    for given in (ptr, torch.tensor(ptr), torch.tensor(ptr, dtype=torch.int32), np.array(ptr), tuple(ptr)):
        p = rg.offsets(given, None, 10, what="caller")
        assert p.dtype == torch.int64 and p.device.type == "cpu" and p.is_contiguous() and p.tolist() == ptr
    for given in (batch, batch.tolist(), batch.numpy(), batch.to(torch.int32)):
        b = rg.offsets(None, given, 10, what="caller")
        assert b.dtype == torch.int64 and b.is_contiguous() and b.tolist() == ptr
    assert (b[1:] - b[:-1]).tolist() == sizes
    # rows None: the row count is what ptr / batch say
    assert rg.offsets(ptr, None, None, what="caller").tolist() == ptr
    assert rg.offsets(None, batch, None, what="caller").tolist() == ptr
    assert rg.offsets([0, 4, 9], None, None, what="caller").tolist() == [0, 4, 9]
    with pytest.raises(ValueError, match=r"slide 1: ptr decreases \(4 -> 3\)"):
        rg.offsets([0, 4, 3], None, None, what="caller", unit="slide")
    with pytest.raises(ValueError, match="exactly one"):
        rg.offsets(None, None, None, what="caller")
    with pytest.raises(ValueError, match="segment 0 has 3 rows in ptr, need at least 4"):
        rg.offsets(ptr, None, 10, what="caller", min_rows=4)


def test_offsets_without_segments_need_the_flag():
    rg = _rg()
    assert rg.offsets([0], None, 0, what="caller", allow_no_segments=True).tolist() == [0]
    assert rg.offsets([0], None, None, what="caller", allow_no_segments=True).tolist() == [0]
    assert rg.offsets(None, torch.zeros(0, dtype=torch.long), 0, what="caller", allow_no_segments=True).tolist() == [0]
    with pytest.raises(ValueError, match="segment 0: ptr describes no segment"):
        rg.offsets([], None, 0, what="caller", allow_no_segments=True)
    with pytest.raises(ValueError, match=r"segment 0: ptr must end at 10 \(got 0\)"):
        rg.offsets([0], None, 10, what="caller", allow_no_segments=True)
    for unit in ("segment", "slide"):
        with pytest.raises(ValueError, match=f"{unit} 0: ptr describes no {unit}"):
            rg.offsets([0], None, 0, what="caller", unit=unit)


def test_two_sided_counts_and_rows_per_side():
    rg = _rg()
    sides = dict(xs="wsi_", ys="tma_", what="caller")
    wp, tp = rg.two_sided(10, 6, [0, 5, 10], None, None, torch.tensor([0, 0, 0, 1, 1, 1]), **sides)
    assert wp.tolist() == [0, 5, 10] and tp.tolist() == [0, 3, 6]
    with pytest.raises(ValueError, match="^caller: segment 2: wsi describes 2 segments, tma 3$"):
        rg.two_sided(10, 6, [0, 5, 10], None, [0, 2, 4, 6], None, **sides)
    with pytest.raises(ValueError, match="^caller: slide 2: wsi describes 3 slides, tma 2$"):
        rg.two_sided(10, 6, [0, 5, 7, 10], None, [0, 2, 6], None, unit="slide", **sides)
    with pytest.raises(ValueError, match="^caller: slide 1: wsi describes 2 slides, tma 1$"):
        rg.two_sided(10, 6, [0, 5, 10], None, None, torch.zeros(6, dtype=torch.long), unit="slide", **sides)
    with pytest.raises(ValueError, match="^caller: segment 1: x describes 2 segments, y 1$"):      # sides without a prefix of their own
        rg.two_sided(10, 6, [0, 5, 10], None, [0, 6], None, xs="", ys="y_", what="caller")
    with pytest.raises(ValueError, match="exactly one of tma_ptr / tma_batch"):
        rg.two_sided(10, 6, [0, 5, 10], None, None, None, **sides)
    # rows per side: a slide may come without tma rows where the caller says so, and never without wsi rows
    hole = dict(x_ptr=[0, 5, 10], x_batch=None, y_ptr=[0, 6, 6], y_batch=None)
    assert rg.two_sided(10, 6, unit="slide", min_rows=(1, 0), **hole, **sides)[1].tolist() == [0, 6, 6]
    with pytest.raises(ValueError, match="slide 1 has 0 rows in tma_ptr, need at least 1"):
        rg.two_sided(10, 6, unit="slide", min_rows=(1, 1), **hole, **sides)
    with pytest.raises(ValueError, match="slide 1 has 0 rows in wsi_ptr, need at least 1"):
        rg.two_sided(10, 6, [0, 10, 10], None, [0, 3, 6], None, unit="slide", min_rows=(1, 0), **sides)
    assert [p.tolist() for p in rg.two_sided(0, 0, [0], None, [0], None, allow_no_segments=True, **sides)] == [[0], [0]]


def test_block_offsets_and_segment_ids():
    rg = _rg()
    xp, yp = torch.tensor([0, 2, 2, 5]), torch.tensor([0, 4, 9, 10])         # sizes [2, 0, 3] x [4, 5, 1]
    for got, want in ((rg.block_offsets(xp, yp), [0, 8, 8, 11]), (rg.block_offsets(xp), [0, 4, 4, 13])):
        assert got.dtype == torch.int64 and got.is_contiguous() and got.tolist() == want
    assert rg.block_offsets(torch.tensor([0])).tolist() == [0]
    ids = rg.segment_ids(xp)
    assert ids.dtype == torch.int64 and ids.tolist() == [0, 0, 2, 2, 2]
    assert rg.segment_ids(yp).tolist() == [0] * 4 + [1] * 5 + [2]
    assert rg.segment_ids(torch.tensor([0])).tolist() == []
    assert rg.offsets(None, ids, 5, what="caller").tolist() == xp.tolist()         # the batch vector that has these offsets


def test_budget_groups_and_the_names_that_stay():
    import multimodal_fusion_amd as mmf
    rg, wh = _rg(), import_module("multimodal_fusion_amd.weighted_hypergraph")
    hand = [(([2, 3, 100, 5, 5, 4], 4 * 200), [(0, 2, False), (2, 3, True), (3, 6, False)]),
            (([10, 10, 10], 4 * 200), [(0, 2, False), (2, 3, False)]),
            (([40, 50, 300, 60, 70, 2, 45], 4 * 100 * 100), [(0, 2, False), (2, 3, True), (3, 6, False), (6, 7, False)]),
            (([40, 50, 300, 60, 70, 2, 45], 1 << 30), [(0, 7, False)]),
            (([10, 20, 30, 100, 10], 6000), [(0, 3, False), (3, 4, True), (4, 5, False)]),
            (([], 100), [])]
    for (sizes, budget), want in hand:
        assert rg.budget_groups(sizes, budget) == want
        assert wh._groups(sizes, budget) == want
        assert mmf.super_patches.group_plan(sizes, budget) == [(a, b) for a, b, _ in want]
    assert mmf.super_patches.group_plan.__module__ == mmf.super_patches.__name__


def test_size_checks_carry_the_texts_of_scikit_learn():
    rg = _rg()
    rg.check_kmeans_sizes([3, 5], 3, "caller")
    rg.check_knn_sizes([3, 5], 2, "caller")
    rg.check_knn_sizes([3, 5], 2, "caller", n_clusters=3)
    with pytest.raises(ValueError, match=r"^caller: segment 1: n_samples=2 should be >= n_clusters=3\.$"):
        rg.check_kmeans_sizes([5, 2], 3, "caller")
    with pytest.raises(ValueError, match=r"^caller: slide 0: n_samples=5 should be >= n_clusters=0\.$"):
        rg.check_kmeans_sizes([5, 2], 0, "caller", "slide")
    with pytest.raises(ValueError, match=r"^caller: slide 1: Expected n_neighbors <= n_samples_fit, but n_neighbors = 4, "
                                         r"n_samples_fit = 3, n_samples = 3$"):
        rg.check_knn_sizes([8, 3], 3, "caller", "slide")
    # both fail on segment 0: the neighbours are asked for first, as in the plain mirror
    with pytest.raises(ValueError, match="segment 0: Expected n_neighbors <= n_samples_fit, but n_neighbors = 6"):
        rg.check_knn_sizes([3, 8], 5, "caller", n_clusters=4)
    # and segment by segment: the first segment that fails either check is the one named
    with pytest.raises(ValueError, match=r"segment 0: n_samples=3 should be >= n_clusters=4\."):
        rg.check_knn_sizes([3, 2], 2, "caller", n_clusters=4)


def test_ragged_imports_nothing_from_the_package():
    """Loaded on its own, under a name outside the package, the module works: a relative import would fail here."""
    spec = importlib.util.spec_from_file_location("ragged_on_its_own", os.path.join(PKG, "ragged.py"))
    alone = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(alone)
    assert alone.offsets([0, 4, 10], None, 10, what="caller").tolist() == [0, 4, 10]
    with open(os.path.join(PKG, "ragged.py")) as f:
        src = f.read()
    assert not re.search(r"^\s*(from\s+\.|import\s+multimodal|from\s+multimodal)", src, re.M)


def test_no_module_imports_a_private_name_of_a_sibling():
    """ops.py's underscore helpers are the binding's shared tools; every other helper that two modules need lives in ragged."""
    found = []
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(path) as f:
            src = f.read()
        for m in re.finditer(r"^\s*from\s+\.(\w+)\s+import\s+(\([^)]*\)|[^\n]*)", src, re.M):
            names = [n.split(" as ")[0].strip() for n in re.sub(r"#[^\n]*", "", m.group(2)).strip("()").split(",")]
            found += [(os.path.basename(path), m.group(1), n) for n in names if n.startswith("_") and m.group(1) != "ops"]
    assert not found, found
