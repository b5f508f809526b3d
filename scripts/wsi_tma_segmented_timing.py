"""Segmented WSI x TMA similarity and grouping: one cohort call (A) against the Python loop of the plain mirrors per slide (B).
d = 512, lambda_h = 1, G = 10.

    python scripts/wsi_tma_segmented_timing.py [out.txt] [--shapes 1,2,3,4] [--reps N] [--a-only]

    A1  compute_wsi_tma_similarity_segmented                              (similarity + statistics)
    A2  A1 + group_by_similarity_segmented                                (+ grouping)
    B1  loop of compute_wsi_tma_similarity                                (parent code)
    B2  loop of compute_wsi_tma_similarity + group_by_similarity          (parent code)

Shapes: (1) 1000 slides of 100 x 64; (2) 2048 x (64 x 64); (3) 300 ragged slides of (40..500) x (16..200), the TMA counts drawn
from ten distinct widths (fixed seed); (4) 16 x (4096 x 1024).  Rows are Gaussian, scaled so that squared distances are about 1.
Same process, one warm-up call of each variant per shape, then `reps` rounds that time the variants in turn with a device
synchronisation around every timed call; median and min .. max are reported.  Before anything is timed the outputs are
compared in the same run: blocks and statistics bit for bit, labels and group sizes equal.  --a-only times A1 and A2 alone (for
a kernel trace)."""
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402,F401

wt = import_module("multimodal_fusion_amd.wsi_tma_similarity")
bh = import_module("multimodal_fusion_amd.build_hypergraph")
dev = torch.device("cuda", 0)
lines = []
D, G, LAM = 512, 10, 1.0


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
    rng = np.random.RandomState(7)
    widths = sorted(rng.choice(np.arange(16, 201), 10, replace=False).tolist())
    widths[0], widths[-1] = 16, 200
    n_r = rng.randint(40, 501, 300).tolist()
    m_r = [widths[i] for i in rng.randint(0, 10, 300)]
    n_r[0], n_r[-1] = 40, 500
    return {1: ("1000 x (100 x 64)", [100] * 1000, [64] * 1000), 2: ("2048 x (64 x 64)", [64] * 2048, [64] * 2048),
            3: ("ragged 300 x (40..500) x (16..200)", n_r, m_r), 4: ("16 x (4096 x 1024)", [4096] * 16, [1024] * 16)}


def a1(W, Tm, wp, tp):
    return wt.compute_wsi_tma_similarity_segmented(W, None, Tm, lambda_h=LAM, wsi_ptr=wp, tma_ptr=tp)


def a2(W, Tm, wp, tp):
    S_flat, s_ptr, st = a1(W, Tm, wp, tp)
    return (S_flat, s_ptr, st) + tuple(wt.group_by_similarity_segmented(S_flat, G, wsi_ptr=wp, tma_ptr=tp))


def b1(W, Tm, wp, tp):
    return [bh.compute_wsi_tma_similarity(W[wp[s]:wp[s + 1]], None, Tm[tp[s]:tp[s + 1]], lambda_h=LAM) for s in range(len(wp) - 1)]


def b2(W, Tm, wp, tp):
    out = []
    for s in range(len(wp) - 1):
        S, st = bh.compute_wsi_tma_similarity(W[wp[s]:wp[s + 1]], None, Tm[tp[s]:tp[s + 1]], lambda_h=LAM)
        out.append((S, st) + tuple(bh.group_by_similarity(S, G)))
    return out


def stat(ts):
    return f"{np.median(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def verdict(ta, tb):
    """A difference is called a gain only where it exceeds three times the larger spread (DESIGN.md's rule)."""
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    diff = np.median(tb) - np.median(ta)
    word = "gain" if diff > 3 * spread else ("loss" if -diff > 3 * spread else "no difference")
    return f"B / A {np.median(tb) / np.median(ta):7.2f}x   {word} (difference {diff:.3f} ms, larger spread {spread:.3f} ms)"


def main():
    args = sys.argv[1:]
    out_path = next((a for a in args if a.endswith(".txt")), None)
    sel = [int(v) for v in args[args.index("--shapes") + 1].split(",")] if "--shapes" in args else [1, 2, 3, 4]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    a_only = "--a-only" in args
    for key in sel:
        name, nw, nt = shapes()[key]
        wp, tp = offsets(nw), offsets(nt)
        g = torch.Generator().manual_seed(key)
        scale = 0.7 / np.sqrt(D)
        W, Tm = (torch.randn(wp[-1], D, generator=g) * scale).to(dev), (torch.randn(tp[-1], D, generator=g) * scale).to(dev)
        _, (S_flat, s_ptr, st, labels, gst, info) = once(lambda: a2(W, Tm, wp, tp))
        fits = len(wt.width_plan(nw, nt))
        head = (f"{name}: slides {len(nw)}  wsi rows {wp[-1]}  tma rows {tp[-1]}  similarities {int(s_ptr[-1])}  d {D}  G {G}  "
                f"distinct widths (KMeans fits) {fits}  ambiguous slides {sum(1 for v in info['ambiguous_draws'] if v)}")
        if a_only:
            t1 = [once(lambda: a1(W, Tm, wp, tp))[0] for _ in range(reps)]
            t2 = [once(lambda: a2(W, Tm, wp, tp))[0] for _ in range(reps)]
            say(head)
            say(f"  A1 segmented similarity + statistics   {stat(t1)}")
            say(f"  A2 A1 + segmented grouping             {stat(t2)}")
            continue
        _, ref = once(lambda: b2(W, Tm, wp, tp))
        once(lambda: a1(W, Tm, wp, tp))
        once(lambda: b1(W, Tm, wp, tp))
        for s, (S, st_s, lab_s, gst_s) in enumerate(ref):
            assert torch.equal(S_flat[int(s_ptr[s]):int(s_ptr[s + 1])].view(torch.int32), S.reshape(-1).view(torch.int32)), f"slide {s}: blocks differ"
            assert repr(st[s]) == repr(st_s), f"slide {s}: statistics differ"
            assert np.array_equal(labels[wp[s]:wp[s + 1]], lab_s) and gst[s] == gst_s, f"slide {s}: grouping differs"
        del ref
        t_a1, t_a2, t_b1, t_b2 = [], [], [], []
        for _ in range(reps):
            t_a1.append(once(lambda: a1(W, Tm, wp, tp))[0])
            t_b1.append(once(lambda: b1(W, Tm, wp, tp))[0])
            t_a2.append(once(lambda: a2(W, Tm, wp, tp))[0])
            t_b2.append(once(lambda: b2(W, Tm, wp, tp))[0])
        say(head)
        say(f"  A1 segmented similarity + statistics   {stat(t_a1)}")
        say(f"  B1 loop of compute_wsi_tma_similarity  {stat(t_b1)}   {verdict(t_a1, t_b1)}")
        say(f"  A2 A1 + segmented grouping             {stat(t_a2)}")
        say(f"  B2 loop of similarity + grouping       {stat(t_b2)}   {verdict(t_a2, t_b2)}")
        say("  same blocks, statistics, labels and group sizes in A and B: True")
        del S_flat, W, Tm
        torch.cuda.empty_cache()
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
