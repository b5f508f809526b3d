"""Segmented KMeans: one mmf_kmeans_fit_segmented call against the Python loop of kmeans_fit_predict per segment.

    python scripts/kmeans_segmented_timing.py [out.txt] [--shapes 1,2,3,4] [--reps N] [--seg-only]

Shapes: (1) 64 x 16384 x 512, k = 100, g9 "clustered"-style rows (unit rows around 128 directions, one draw per segment);
(2) a ragged mix of 1000 .. 30000 rows, d = 512, k = 100; (3) 1000 x (100 + 64) x 512, k = 10 (the clique step);
(4) 1000 x 100 x 256, k = 10 (group_by_similarity's shape, one width).  Same process, one warm-up call of each form, then the
median of `reps` timed calls with a synchronise around each timed window.  The outputs of both forms are compared in the same
run (labels, centres, inertia: same bits).  Also: Lloyd lockstep iterations and host status reads per call (the loop reads
once per iteration of each fit; the segmented call once per iteration of each group).  Relocation reads are not counted.  --seg-only times the segmented call alone (for a kernel trace)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd  # noqa: E402,F401
from multimodal_fusion_amd import kmeans as km  # noqa: E402

dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def clustered(n, d, rng):
    c = rng.standard_normal((128, d)).astype(np.float32)
    X = (c[rng.integers(0, 128, n)] + 0.7 * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def sim_rows(n, d, rng):
    a = rng.standard_normal((n, 16)).astype(np.float32)
    b = rng.standard_normal((d, 16)).astype(np.float32)
    return np.exp(-0.05 * ((a[:, None, :] - b[None]) ** 2).sum(-1)).astype(np.float32)


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def loop(X, ptr, k):
    labels, centres, inertia, iters = [], [], [], 0
    for s in range(len(ptr) - 1):
        l, c, i, info = km.kmeans_fit_predict(X[ptr[s]:ptr[s + 1]], k, return_info=True)
        labels.append(l); centres.append(c); inertia.append(i); iters += info["lockstep_iterations"]
    return torch.cat(labels), torch.stack(centres), np.array(inertia), iters


def groups(ptr, k, n_init=10):
    """First segment of every group under the cluster and label limits of mmf_kmeans_fit_segmented (its scratch bound, 2 GiB,
    does not bind on these shapes)."""
    firsts, c, rows = [], 0, 0
    for s in range(len(ptr) - 1):
        n = ptr[s + 1] - ptr[s]
        if not firsts or c + n_init * k > 16384 or (rows + n) * n_init >= 2 ** 31:
            firsts.append(s); c = rows = 0
        c += n_init * k; rows += n
    return firsts


def seg(X, ptr, k):
    l, c, i, info = km.kmeans_fit_predict_segmented(X, k, ptr=ptr, return_info=True)
    firsts = groups(ptr, k)
    return l, c, i, sum(info[s]["lockstep_iterations"] for s in firsts), len(firsts)


def run(name, parts, k, reps, seg_only=False):
    X = torch.from_numpy(np.concatenate(parts, 0)).to(dev)
    ptr = [0] + [int(v) for v in np.cumsum([len(p) for p in parts])]
    t_seg, (l1, c1, i1, it_seg, ngrp) = timed(lambda: seg(X, ptr, k), reps)
    if seg_only:                        # for a kernel trace of the segmented call alone
        say(f"{name}: segmented call {t_seg:.2f} ms, lockstep iterations {it_seg} in {ngrp} groups")
        return True
    t_loop, (l2, c2, i2, it_loop) = timed(lambda: loop(X, ptr, k), reps)
    same = torch.equal(l1, l2) and torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and np.array_equal(i1, i2)
    say(f"{name}: n_seg = {len(parts)}, rows = {ptr[-1]}, d = {X.shape[1]}, k = {k}")
    say(f"  segmented call: {t_seg:9.2f} ms   lockstep iterations {it_seg} in {ngrp} groups -> {it_seg + ngrp} host reads")
    say(f"  loop of fits:   {t_loop:9.2f} ms   lockstep iterations {it_loop} -> {it_loop + len(parts)} host reads")
    say(f"  speed-up {t_loop / t_seg:.2f}x, outputs identical: {same}")
    return same


def main():
    out = None
    shapes = [1, 2, 3, 4]
    reps = 3
    seg_only = False
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a == "--shapes":
            shapes = [int(v) for v in args.pop(0).split(",")]
        elif a == "--reps":
            reps = int(args.pop(0))
        elif a == "--seg-only":
            seg_only = True
        else:
            out = a
    say(f"device: {torch.cuda.get_device_name(0)}; median of {reps} timed calls after one warm-up")
    ok = True
    rng = np.random.default_rng(0)
    if 1 in shapes:
        ok &= run("(1) 64 x 16384 x 512, clustered", [clustered(16384, 512, rng) for _ in range(64)], 100, reps, seg_only)
    if 2 in shapes:
        sizes = rng.integers(1000, 30001, 40)
        ok &= run("(2) ragged 1000..30000 rows x 512", [clustered(int(n), 512, rng) for n in sizes], 100, reps, seg_only)
    if 3 in shapes:
        ok &= run("(3) 1000 x 164 x 512 (clique step)", [clustered(164, 512, rng) for _ in range(1000)], 10, reps, seg_only)
    if 4 in shapes:
        ok &= run("(4) 1000 x 100 x 256 (grouping shape)", [sim_rows(100, 256, rng) for _ in range(1000)], 10, reps, seg_only)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
