"""Ragged-width segmented KMeans: one kmeans_fit_predict_ragged call for a cohort's grouping step against the
path it replaces, one kmeans_fit_predict_segmented call per distinct width.

    python scripts/kmeans_ragged_timing.py [out.txt] [--shapes 1,2,3,4] [--rounds N]

Arm A: ONE ragged call on the flat buffer.  Arm B: the grouping step's earlier path, restated here from
wsi_tma_similarity.width_plan — per distinct width one segmented fit on the concatenation of that width's blocks (a view when they
are adjacent) and one indexed store of its labels.  Both run in this process on the same buffers.

Shapes, k = 10: (1) 300 slides of (40..500) x (16..200), widths drawn freely; (2) 1000 x (100 x m), m uniform in 16..128;
controls: (3) 1000 x (100 x 64), where B is the segmented entry itself in one call; (4) 16 x (4096 x 1024).

Protocol: the outputs of both arms are compared first (labels; on the one-width controls also the centres' and the inertia's bits);
then one warm-up of each arm, then `rounds` rounds (default 7) in which the arms alternate, a device synchronisation around every
timed call; median with min .. max.  The last lines apply the three-spreads rule of DESIGN.md §4.1 to shape 3."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd  # noqa: E402,F401
from multimodal_fusion_amd import kmeans as km  # noqa: E402
from multimodal_fusion_amd import kmeans_ragged as kr  # noqa: E402
from multimodal_fusion_amd.wsi_tma_similarity import width_plan  # noqa: E402

dev = torch.device("cuda", 0)
lines = []
K = 10


def say(s):
    print(s, flush=True)
    lines.append(s)


def sim_block(n, m, rng):
    """Rows of a WSI x TMA similarity block: exp(-|a - b|^2) of clustered points, values in (0, 1)."""
    c = rng.standard_normal((6, 8)).astype(np.float32)
    a = c[rng.integers(0, 6, n)] + 0.3 * rng.standard_normal((n, 8)).astype(np.float32)
    b = c[rng.integers(0, 6, m)] + 0.3 * rng.standard_normal((m, 8)).astype(np.float32)
    return np.exp(-0.2 * ((a[:, None, :] - b[None]) ** 2).sum(-1)).astype(np.float32)


def arm_a(F, rows, widths):
    return kr.kmeans_fit_predict_ragged(F, K, rows=rows, widths=widths, return_info=True)


def arm_b(F, rows, widths, sp, wp):
    """One segmented fit per distinct width, labels back in slide order: the grouping step before the ragged entry."""
    labels = torch.empty((wp[-1],), dtype=torch.int64, device=F.device)
    fits = 0
    for fit in width_plan(rows, widths):
        sl, m = fit["slides"], fit["width"]
        if fit["adjacent"]:
            X = F[sp[sl[0]]:sp[sl[-1] + 1]].view(-1, m)
        else:
            X = torch.cat([F[sp[s]:sp[s + 1]].view(-1, m) for s in sl], dim=0)
        lab, _, _ = km.kmeans_fit_predict_segmented(X, K, ptr=fit["fit_ptr"])
        if fit["adjacent"]:
            labels[wp[sl[0]]:wp[sl[-1] + 1]] = lab
        else:
            dest = torch.cat([torch.arange(wp[s], wp[s + 1]) for s in sl])
            labels[dest.to(F.device)] = lab
        fits += 1
    return labels, fits


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ts):
    return f"{np.median(ts):9.2f} ms ({min(ts):.2f} .. {max(ts):.2f})"


def run(name, sizes, rounds, rng, one_width=False):
    rows, widths = [n for n, _ in sizes], [m for _, m in sizes]
    F = torch.from_numpy(np.concatenate([sim_block(n, m, rng).reshape(-1) for n, m in sizes])).to(dev)
    sp = [0] + [int(v) for v in np.cumsum([n * m for n, m in sizes])]
    wp = [0] + [int(v) for v in np.cumsum(rows)]
    la, ca, ia, info = arm_a(F, rows, widths)
    lb, fits = arm_b(F, rows, widths, sp, wp)
    same = torch.equal(la, lb)
    if one_width:
        _, cb, ib = km.kmeans_fit_predict_segmented(F.view(-1, widths[0]), K, ptr=wp)
        same = same and all(torch.equal(ca[s].view(torch.int32), cb[s].view(torch.int32)) for s in range(len(sizes))) and \
            np.array_equal(ia.view(np.uint64), ib.view(np.uint64))
    order = np.argsort((np.array(widths) + 31) // 32, kind="stable")
    bounds, _ = kr.ragged_groups(np.array(rows)[order], np.array(widths)[order], K)
    lock = sum(info[int(order[b])]["lockstep_iterations"] for b in bounds[:-1])
    say(f"{name}: slides = {len(sizes)}, rows = {wp[-1]}, values = {sp[-1]}, distinct widths = {len(set(widths))}, k = {K}")
    say(f"  outputs identical: {same}   A: {len(bounds) - 1} lockstep groups, {lock} Lloyd iterations in all; B: {fits} segmented fits")
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(clock(lambda: arm_a(F, rows, widths))[0])
        tb.append(clock(lambda: arm_b(F, rows, widths, sp, wp))[0])
    say(f"  A one ragged call:       {fmt(ta)}")
    say(f"  B one fit per width:     {fmt(tb)}")
    say(f"  A / B = {np.median(ta) / np.median(tb):.3f}   (B / A = {np.median(tb) / np.median(ta):.2f}x)")
    return same, ta, tb


def main():
    out, shapes, rounds = None, [1, 2, 3, 4], 7
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a == "--shapes":
            shapes = [int(v) for v in args.pop(0).split(",")]
        elif a == "--rounds":
            rounds = int(args.pop(0))
        else:
            out = a
    say(f"device: {torch.cuda.get_device_name(0)}; arms alternating, {rounds} rounds after one warm-up of each, median (min .. max)")
    ok = True
    rng = np.random.default_rng(0)
    if 1 in shapes:
        sizes = list(zip(rng.integers(40, 501, 300).tolist(), rng.integers(16, 201, 300).tolist()))
        ok &= run("(1) 300 ragged slides (40..500) x (16..200)", sizes, rounds, rng)[0]
    if 2 in shapes:
        sizes = [(100, int(m)) for m in rng.integers(16, 129, 1000)]
        ok &= run("(2) 1000 x (100 x m), m in 16..128", sizes, rounds, rng)[0]
    if 3 in shapes:
        same, ta, tb = run("(3) control: 1000 x (100 x 64), one width", [(100, 64)] * 1000, rounds, rng, one_width=True)
        ok &= same
        diff, spread = float(np.median(ta) - np.median(tb)), max(max(ta) - min(ta), max(tb) - min(tb))
        verdict = "no clear difference" if abs(diff) <= 3 * spread else ("the ragged entry is slower" if diff > 0 else "the ragged entry is faster")
        say(f"  three-spreads rule: A - B = {diff:+.2f} ms against 3 x the larger spread = {3 * spread:.2f} ms: {verdict}")
    if 4 in shapes:
        ok &= run("(4) control: 16 x (4096 x 1024), one width", [(4096, 1024)] * 16, rounds, rng, one_width=True)[0]
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
