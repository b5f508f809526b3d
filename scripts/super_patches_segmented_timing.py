"""Segmented super-patch aggregation: one cohort call (A) against the Python loop of the plain mirror per slide (B).
d = 512, positions 2-D, lambda_h = lambda_g = 1.

    python scripts/super_patches_segmented_timing.py [out.txt] [--shapes 1,2,3,4] [--reps N] [--a-only]

    A   aggregate_wsi_super_patches_segmented(keep_similarity=False)      (one KMeans call, one sort, one pooling call per group)
    B   loop of aggregate_wsi_super_patches                               (parent code)

Shapes: (1) 1000 slides of 400 patches, C = 100; (2) 2048 x 128, C = 16; (3) 300 ragged slides of 150..2000 patches (fixed seed),
C = 100; (4) 16 x 8192, C = 100.  Rows are clustered Gaussians (ten centres per slide), scaled so that squared distances are
about 1.  Same process, one warm-up call of each variant per shape, then `reps` rounds that time the variants in turn with a
device synchronisation around every timed call; median and min .. max are reported.  Before anything is timed the outputs are
compared in the same run: super features and positions bit for bit, the stats dicts equal.  --a-only times A alone (for a kernel
trace)."""
import json
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402,F401

sp = import_module("multimodal_fusion_amd.super_patches")
bh = import_module("multimodal_fusion_amd.build_hypergraph")
dev = torch.device("cuda", 0)
lines = []
D, LAM = 512, (1.0, 1.0)


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def shapes():
    n_r = np.random.RandomState(7).randint(150, 2001, 300).tolist()
    n_r[0], n_r[-1] = 150, 2000
    return {1: ("1000 x 400, C = 100", [400] * 1000, 100), 2: ("2048 x 128, C = 16", [128] * 2048, 16),
            3: ("ragged 300 x (150..2000), C = 100", n_r, 100), 4: ("16 x 8192, C = 100", [8192] * 16, 100)}


def cohort(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    n, S = sum(sizes), len(sizes)
    centres = torch.randn(S, 10, D, generator=g) * (0.9 / np.sqrt(D))
    slide = torch.repeat_interleave(torch.arange(S), torch.tensor(sizes))
    F = centres[slide, torch.randint(0, 10, (n,), generator=g)] + torch.randn(n, D, generator=g) * (0.25 / np.sqrt(D))
    return F.to(dev), torch.rand(n, 2, generator=g).to(dev)


def a(F, P, ptr, C):
    return sp.aggregate_wsi_super_patches_segmented(F, P, C, *LAM, ptr=ptr, keep_similarity=False, return_info=True)


def b(F, P, ptr, C):
    out = []
    for s in range(len(ptr) - 1):
        sf, spos, st, _ = bh.aggregate_wsi_super_patches(F[ptr[s]:ptr[s + 1]], P[ptr[s]:ptr[s + 1]], C, *LAM)
        out.append((sf, spos, st))
    return out


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def verdict(ta, tb):
    """A difference is called a gain only where it exceeds three times the larger spread (DESIGN.md's rule)."""
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    diff = np.median(tb) - np.median(ta)
    word = "gain" if diff > 3 * spread else ("loss" if -diff > 3 * spread else "no difference")
    return f"B / A {np.median(tb) / np.median(ta):7.2f}x   {word} (difference {diff:.3f} ms, larger spread {spread:.3f} ms)"


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    sel = [int(v) for v in args[args.index("--shapes") + 1].split(",")] if "--shapes" in args else [1, 2, 3, 4]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    a_only = "--a-only" in args
    for key in sel:
        name, sizes, C = shapes()[key]
        ptr = offsets(sizes)
        F, P = cohort(sizes, key)
        _, (sf, spos, stats, _, k_ptr, info) = once(lambda: a(F, P, ptr, C))
        head = (f"{name}: slides {len(sizes)}  patches {ptr[-1]}  super patches {len(sizes) * C}  similarities {int(k_ptr[-1])}  d {D}  "
                f"groups {len(info['groups'])}  ambiguous slides {sum(1 for v in info['ambiguous_draws'] if v)}")
        if a_only:
            ta = [once(lambda: a(F, P, ptr, C))[0] for _ in range(reps)]
            say(head)
            say(f"  A segmented aggregation                  {stat(ta)}")
            continue
        _, ref = once(lambda: b(F, P, ptr, C))
        for s, (f_s, p_s, st_s) in enumerate(ref):
            assert torch.equal(sf[s * C:(s + 1) * C].view(torch.int32), f_s.view(torch.int32)), f"slide {s}: super features differ"
            assert torch.equal(spos[s * C:(s + 1) * C].view(torch.int32), p_s.view(torch.int32)), f"slide {s}: super positions differ"
            assert json.dumps(stats[s], sort_keys=True) == json.dumps(st_s, sort_keys=True), f"slide {s}: stats differ"
        del ref
        ta, tb = [], []
        for _ in range(reps):
            ta.append(once(lambda: a(F, P, ptr, C))[0])
            tb.append(once(lambda: b(F, P, ptr, C))[0])
        say(head)
        say(f"  A segmented aggregation                  {stat(ta)}")
        say(f"  B loop of aggregate_wsi_super_patches    {stat(tb)}   {verdict(ta, tb)}")
        say("  same super features, positions and stats in A and B: True")
        del sf, spos, F, P
        torch.cuda.empty_cache()
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
