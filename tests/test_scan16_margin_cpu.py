"""The adversarial families of tests/adversarial16.py, certified on the CPU: what tests/test_gpu_scan16_adversarial.py may
take for granted about its data.  For every family a GPU test uses:

  (a) the oracle's top-k of every q row is exactly the A set;
  (b) the kk best approximate values G of the row belong to non-A columns: the scan cannot get the row right without its margin;
  (c) |G - Q| <= e1 for every (q, A or B column) pair, in float64: the proven bound, checked numerically;
  (d) the sharpness rho = (kk-th best G - min over A of G) / margin satisfies floor <= rho < 1;
and the maxima of the candidate side are the family's own, and in a rectangular call every ordinary query row has less than
half a q row's margin (except for cosine, where every row has the same un and a q row the smallest possible rn; in a scan of
X against itself the fillers are columns too and their norms, hence margins, reach the family's).

The floor is a condition on the DATA (a family below 0.5 could not tell a halved margin from a right one); it measures no kernel.
G, Q, e1 and the margin come from oracle/scan16_restate.py, which tests/test_gpu_scan16_adversarial.py pins to the device's
prep kernel.

Floors and the sharpness each construction reaches in the restatement (f16 / bf16 operands; k = 5 and 15, k = 30 within 0.005):
  candidate side, dot,             padded dim 128 : floor 0.85      reached 0.898 / 0.982   (X against itself: the same)
  candidate side, neg_sq_l2 / rbf, padded dim 128 : floor 0.85      reached 0.906 / 0.983
  candidate side, cosine,          padded dim 128 : floor 0.6       reached 0.849 / 0.962
  candidate side, dot,             padded dim 512 : floor 0.76/0.88 reached 0.848 / 0.977   (0.9 x reached; d = 500)
  candidate side, dot,             padded dim 1024: floor 0.64/0.86 reached 0.714 / 0.955   (0.9 x reached; d = 1000)
  query side,     dot,             padded dim 128 : floor 0.77/0.83 reached 0.862 / 0.929   (0.9 x reached)
Not built: query-side families for the L2 metrics and cosine and at padded dims 512 / 1024, and a cosine family for a scan of X
against itself.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adversarial16 as adv   # noqa: E402
from oracle import scan16_restate as rs   # noqa: E402

# (kind, metric or None, padded dim) -> (floor f16, floor bf16)
FLOORS = {
    ("cand", "dot", 128): (0.85, 0.85), ("cand", "neg_sq_l2", 128): (0.85, 0.85), ("cand", "rbf", 128): (0.85, 0.85),
    ("cand", "cosine", 128): (0.6, 0.6),
    ("cand", "dot", 512): (0.76, 0.88), ("cand", "dot", 1024): (0.64, 0.86),
    ("query", "dot", 128): (0.77, 0.83),
}

FAMILIES = adv.all_families()


def floor_of(fam):
    kind = fam.name.split("-")[0]
    return FLOORS[(kind, fam.metric, rs.padded_dim(fam.X.shape[1]))][0 if fam.operand == "f16" else 1]


def test_every_family_has_a_floor_above_one_half():
    assert len(FAMILIES) == len({id(f) for f in FAMILIES}) and len(FAMILIES) >= 40
    assert all(floor_of(f) > 0.5 for f in FAMILIES)


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f"{f.name}-n{len(f.X)}-a{int(f.a_cols[0])}")
def test_family(fam):
    ridx, _ = adv.reference(fam)
    r = adv.analyse(fam)
    print(f"{fam.name}: rho {r['rho']} floor {floor_of(fam)} max|G-Q|/e1 {r['err_over_e1']} margin {r['margin']} "
          f"largest other margin {r['other_margin_max']}")
    for q in fam.q_rows:                                                       # (a)
        assert sorted(ridx[q].tolist()) == sorted(fam.a_cols.tolist()), q
    assert r["top_avoids_a"]                                                   # (b)
    assert (r["err_over_e1"] <= 1.0).all()                                     # (c)
    assert (r["rho"] >= floor_of(fam)).all() and (r["rho"] < 1.0).all()       # (d)
    assert r["maxima_own"]
    if fam.metric != "cosine" and fam.Y is not None:
        assert r["other_margin_max"] < 0.5 * r["margin"].min()


def test_restated_scale_and_rounding():
    """The restatement's own pieces on values worked out by hand."""
    assert rs.common_scale(256.0 ** 2, "dot") == 1.0 and rs.common_scale(255.9 ** 2, "dot") == 2.0
    assert rs.common_scale(512.0 ** 2, "dot") == 0.5 and rs.common_scale(3.0, "cosine") == 256.0
    assert rs.common_scale(0.0, "dot") == 1.0
    v = np.array([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e38], np.float32)
    # bf16 has 8 significant bits: 1 + 2^-8 is a tie (to even: 1), 1 + 3 * 2^-8 a tie (to even: 1 + 2^-6), just above a tie rounds up
    assert rs.bf16_to_f32(rs.round_bf16(v)).tolist()[:4] == [1.0, 1.0, 1.015625, 1.0078125]
    assert [rs.list_capacity(kk) for kk in (1, 11, 12, 20, 21, 44)] == [15, 15, 16, 16, 32, 32]
    assert [rs.padded_dim(d) for d in (1, 128, 129, 500, 513, 1000)] == [128, 128, 256, 512, 1024, 1024]
    X = np.array([[3.0, 4.0], [0.0, 0.0]], np.float32)
    assert rs.row_scalars(X, "dot").tolist() == [25.0, 0.0]
    assert rs.row_scalars(X, "cosine").tolist() == [5.0, np.float32(1e-8)]
    o = rs.operands(X, "neg_sq_l2", "f16")                                     # scale 64: the norm 5 lands at 320
    assert o["scale"] == 64.0 and o["z"].tolist() == [[192.0, 256.0], [0.0, 0.0]] and o["cb"].tolist() == [-51200.0, 0.0]
    assert o["rn"].tolist() == [0.0, 0.0] and o["zbits"].shape == (2, 128)
    m4 = rs.margins(o, o["maxima"], "neg_sq_l2", 31)
    m5 = rs.margins(o, o["maxima"], "neg_sq_l2", 6)
    assert m4["slot_eps"] == 2 * m5["slot_eps"] and (m4["margin"] > m5["margin"]).all()
