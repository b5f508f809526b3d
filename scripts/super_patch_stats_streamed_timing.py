"""Streamed super-patch statistics (A) against the stored path (B): the six numbers aggregate_wsi_super_patches takes from
K = K_h * K_g.  d = 512, positions 2-D, lambda_h = lambda_g = 1, C = 100 clusters (random covering labels).

    python scripts/super_patch_stats_streamed_timing.py [out.txt] [--sizes 16384,32768] [--alone 131072,262144] [--reps N]

    A   super_patch_stats_streamed(F, P, order, offsets, C)                          (K recomputed in row panels, never stored)
    B   ops.sim_dense_combined -> ops.segment_offdiag_mean -> mmf_array_stats        (parent code: K stored, n^2 floats)

--sizes: both variants in the same process, one warm-up call of each, then `reps` rounds that time them in turn with a device
synchronisation around every timed call; median and min .. max.  Before anything is timed the two outputs are compared bit for
bit.  --alone: A only, at sizes whose K cannot be stored (64 and 256 GiB); `none` skips either list.

Every row states the bound that applies and A's share of it.  The least time the hardware could take for one recomputation of K
is the larger of 2 n^2 d flop over the f32 matrix-core peak (157.3 TF, MI355X) and the panel traffic (n^2 floats written once
and read once for the statistics sweep, once more for the row sums: 12 n^2 bytes) over 8 TB/s of HBM; A recomputes K once on the
one-sweep path and four times above its cap (n of about 103,000), which the row says.  The share is a whole-call figure (the
call also samples, sorts the bracket and waits once for its verdict), not a kernel's."""
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402

sps = import_module("multimodal_fusion_amd.super_patch_stats")
dev = torch.device("cuda", 0)
lines = []
D, C, LAM = 512, 100, (1.0, 1.0)
F32_MFMA_FLOPS, HBM_BYTES = 157.3e12, 8.0e12


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def slide(n, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(10, D, generator=g) * (0.9 / np.sqrt(D))
    F = centres[torch.randint(0, 10, (n,), generator=g)] + torch.randn(n, D, generator=g) * (0.25 / np.sqrt(D))
    lab = torch.cat([torch.arange(C), torch.randint(0, C, (n - C,), generator=g)])[torch.randperm(n, generator=g)]
    return F.to(dev), torch.rand(n, 2, generator=g).to(dev), mmf.ops.segment_sort(lab.to(dev), C)


def a(F, P, seg):
    return sps.super_patch_stats_streamed(F, P, seg.order, seg.offsets, C, *LAM)


def b(F, P, seg):
    K = mmf.ops.sim_dense_combined(F, P, *LAM)
    intra = mmf.ops.segment_offdiag_mean(K, seg)
    v = K.reshape(-1)
    out = torch.empty((5,), dtype=torch.float64, device=dev)
    mmf._lib.check(mmf._lib.lib().mmf_array_stats(mmf.ops._p(v), v.numel(), mmf.ops._p(out), 0, mmf.ops._stream(dev)), "mmf_array_stats")
    return intra, out


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def bound(n, ta):
    """The bound of one recomputation of K and the median call's share of (recomputations x bound)."""
    sweeps = 1 if n * n * 4 // 20 <= (2 << 30) and not os.environ.get("MMF_MEDIAN_RADIX") else 4
    mfma_ms, hbm_ms = 2.0 * n * n * D / F32_MFMA_FLOPS * 1e3, 12.0 * n * n / HBM_BYTES * 1e3
    which, least = ("f32 MFMA", mfma_ms) if mfma_ms >= hbm_ms else ("HBM", hbm_ms)
    return (f"bound: {which} ({mfma_ms:.2f} ms of matrix cores, {hbm_ms:.2f} ms of HBM per recomputation), K recomputed {sweeps}x, "
            f"least time {sweeps * least:.2f} ms, share {sweeps * least / np.median(ta):.2f}")


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)

    def sizes(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        return [] if v == "none" else [int(x) for x in v.split(",")]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    say(f"d {D}  clusters {C}  lambdas {LAM}  rounds {reps}  panel_rows 0 (about 1 GiB)")
    for n in sizes("--sizes", [16384, 32768]):
        F, P, seg = slide(n, n)
        _, got = once(lambda: a(F, P, seg))
        _, want = once(lambda: b(F, P, seg))
        same = all(torch.equal(g.view(torch.int64), w.view(torch.int64)) for g, w in zip(got, want))
        assert same, f"n = {n}: streamed and stored outputs differ"
        ta, tb = [], []
        for _ in range(reps):
            ta.append(once(lambda: a(F, P, seg))[0])
            tb.append(once(lambda: b(F, P, seg))[0])
        say(f"n {n}: K would take {n * n * 4 / 2 ** 30:.1f} GiB, streamed workspace {sps.streamed_workspace_bytes(n, D, 2, C) / 2 ** 30:.2f} GiB")
        say(f"  A streamed                               {stat(ta)}   {bound(n, ta)}")
        say(f"  B stored K, offdiag mean, array_stats    {stat(tb)}   B / A {np.median(tb) / np.median(ta):.2f}x")
        say("  same bits in A and B: True")
        del F, P, seg, got, want
        torch.cuda.empty_cache()
    for n in sizes("--alone", [131072]):
        F, P, seg = slide(n, n)
        once(lambda: a(F, P, seg))
        ta = [once(lambda: a(F, P, seg))[0] for _ in range(reps)]
        say(f"n {n}: K would take {n * n * 4 / 2 ** 30:.1f} GiB, streamed workspace {sps.streamed_workspace_bytes(n, D, 2, C) / 2 ** 30:.2f} GiB")
        say(f"  A streamed (alone)                       {stat(ta)}   {bound(n, ta)}")
        del F, P, seg
        torch.cuda.empty_cache()
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
