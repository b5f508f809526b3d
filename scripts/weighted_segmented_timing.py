"""Segmented weighted hypergraph: one build_weighted_hypergraph_segmented call against the Python loop of
build_weighted_hypergraph per segment (ratio 1.0, lambda_h = lambda_g = 1, d = 512, dp = 2).

    python scripts/weighted_segmented_timing.py [out.txt] [--shapes 1,2,3,4] [--reps N] [--seg-only]

Shapes: (1) 2048 x 128 rows; (2) 256 x 1024; (3) 64 x 4096; (4) a ragged mix of 60 segments of 64 .. 8192 rows (log-uniform
sizes, fixed seed, both ends included).  Features are randn / sqrt(d) * 0.6 (similarities spread over (0, 1)), positions uniform in the unit square.  Same
process, one warm-up call of each form per shape, then the median of `reps` timed calls with a device synchronisation around
each timed window.  The outputs of both forms are compared in the same run (edge ids equal, weights the same bits, edge_ptr
equal to the loop's edge counts).  --seg-only times the segmented call alone (for a kernel trace)."""
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd  # noqa: E402,F401

wh = import_module("multimodal_fusion_amd.weighted_hypergraph")
bh = import_module("multimodal_fusion_amd.build_hypergraph")
dev = torch.device("cuda", 0)
lines = []
D, RATIO = 512, 1.0


def say(s):
    print(s, flush=True)
    lines.append(s)


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


def loop(F, P, ptr):
    eis, ews, cnt = [], [], []
    for s in range(len(ptr) - 1):
        a, b = ptr[s], ptr[s + 1]
        ei, ew = bh.build_weighted_hypergraph(F[a:b], P[a:b], 1.0, 1.0, RATIO)
        eis.append(ei + a); ews.append(ew); cnt.append(ew.numel())
    return torch.cat(eis, 1), torch.cat(ews), cnt


def shapes():
    rng = np.random.RandomState(7)
    ragged = np.exp(rng.uniform(np.log(64), np.log(8192), 60)).astype(np.int64).tolist()
    ragged[0], ragged[-1] = 64, 8192                   # both ends of the range
    return {1: ("small 2048 x 128", [128] * 2048), 2: ("256 x 1024", [1024] * 256), 3: ("64 x 4096", [4096] * 64),
            4: ("ragged 64..8192", ragged)}


def main():
    args = sys.argv[1:]
    out_path = next((a for a in args if a.endswith(".txt")), None)
    sel = [1, 2, 3, 4]
    if "--shapes" in args:
        sel = [int(v) for v in args[args.index("--shapes") + 1].split(",")]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    seg_only = "--seg-only" in args
    for key in sel:
        name, sizes = shapes()[key]
        ptr = [0] + [int(v) for v in np.cumsum(sizes)]
        n = ptr[-1]
        g = torch.Generator().manual_seed(key)
        F = (torch.randn(n, D, generator=g) * (0.6 / D ** 0.5)).to(dev)
        P = torch.rand(n, 2, generator=g).to(dev)
        kbytes = 4 * sum(v * v for v in sizes)
        t_seg, (ei, ew, eptr) = timed(lambda: wh.build_weighted_hypergraph_segmented(F, P, 1.0, 1.0, RATIO, ptr=ptr), reps)
        head = (f"{name}: segments {len(sizes)}  rows {n}  rows/segment {min(sizes)}..{max(sizes)}  d {D}  ratio {RATIO}  "
                f"blocks {kbytes / 2 ** 30:.3f} GiB  edges {ew.numel()}")
        if seg_only:
            say(head)
            say(f"  segmented call {t_seg:9.3f} ms")
            continue
        t_loop, (rei, rew, cnt) = timed(lambda: loop(F, P, ptr), reps)
        same = (torch.equal(ei, rei) and torch.equal(ew.view(torch.int32), rew.view(torch.int32))
                and (eptr[1:] - eptr[:-1]).tolist() == cnt)
        say(head)
        say(f"  segmented call {t_seg:9.3f} ms   loop of {len(sizes)} build_weighted_hypergraph {t_loop:9.3f} ms   "
            f"speed-up {t_loop / t_seg:6.2f}x   same edges and bits {same}")
        del ei, ew, rei, rew
        torch.cuda.empty_cache()
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
