"""The 16-bit top-k of the combined similarity (combined_topk16.simtopk_combined_fast) against the exact entry
(combined_topk.simtopk_combined).  dp = 2, k = 5, lambda_h = 0.5, lambda_g = 2e-7; unit-norm planted features (12 Gaussian
centres + 0.05 noise, rows L2-normalised) with distinct pixel positions (cells of a grid of side 4 ceil(sqrt(N)) x 224);
whole-call times.

    python scripts/simtopk_combined_fast_timing.py [out.txt] [--reps N] [--skip-large] [--exact-only]

    arms  A  precision="fast" (f16 operands)   A' precision="fast_bf16"   B  simtopk_combined (exact f32 scan)
    shapes N = 16384, 65536, 262144 at d = 512; N = 65536 at d = 1536

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max.  A and A' are checked against B bit for bit before they
are timed.  The scan's own time comes from the call's event timers (profile=True, one separate call); its share of the 16-bit
matrix-core peak is 2 d flop per pair over that time.  The device memory a call takes is measured on the first call of a
fresh process state (workspaces released before).  --exact-only times B alone: run on a build of the parent commit
(MMF_HG_LIBRARY) it shows that the exact arm did not move.

The AUTO rule: MMF_PREC_AUTO takes the fast path only for the (d, k) ranges where A beats B by more than
three times B's spread at every measured N of that range."""
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402

ct = import_module("multimodal_fusion_amd.combined_topk")
dev = torch.device("cuda", 0)
lines = []
K, LH, LG = 5, 0.5, 2e-7
B16_MFMA_FLOPS = 2.5e15
F32_MFMA_FLOPS = 157.3e12


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(12, d, generator=g)
    F = centres[torch.randint(0, 12, (n,), generator=g)] + 0.05 * torch.randn(n, d, generator=g)
    F = F / F.norm(dim=1, keepdim=True)
    side = 4 * int(np.ceil(np.sqrt(n)))
    cells = torch.randperm(side * side, generator=g)[:n]
    P = torch.stack([(cells // side) * 224, (cells % side) * 224], dim=1).float()
    return F.contiguous().to(dev), P.contiguous().to(dev)


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def alternate(arms, reps):
    for fn in arms:
        once(fn)
    ts = [[] for _ in arms]
    for _ in range(reps):
        for t, fn in zip(ts, arms):
            t.append(once(fn)[0])
    return ts


def release():
    mmf._lib.check(mmf._lib.lib().mmf_release_workspaces(), "mmf_release_workspaces")
    torch.cuda.empty_cache()


def taken(fn):
    release()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    once(fn)
    return (free0 - torch.cuda.mem_get_info(dev)[0]) / 2 ** 30


def events(fn, n, d, peak):
    st = fn(return_stats=True, profile=True)[2]
    share = 2.0 * d * n * n / (st["scan_ms"] * 1e-3) / peak if st["scan_ms"] > 0 else float("nan")
    return (f"events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms ({share:.3f} of the {peak / 1e12:.1f} TF peak), re-rank "
            f"{st['rerank_ms']:.3f} ms, rescan {st['fallback_ms']:.3f} ms; grid {st['scan_grid']}, col_splits {st['col_splits']}, candidates "
            f"per row {st['candidates'] / n:.1f}, fallback_rows {st['fallback_rows']}")


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    exact_only = "--exact-only" in args
    fast = None if exact_only else import_module("multimodal_fusion_amd.combined_topk16").simtopk_combined_fast
    say(f"dp 2  k {K}  lambda_h {LH}  lambda_g {LG}  rounds {reps}  whole-call times, median (min .. max)"
        + ("  [exact arm alone]" if exact_only else ""))
    shapes = [(16384, 512), (65536, 512), (65536, 1536)] + ([] if "--skip-large" in args else [(262144, 512)])
    for n, d in shapes:
        F, P = rows(n, d, n // 1024 + d)

        def B(**kw):
            return ct.simtopk_combined(F, P, LH, LG, K, **kw)
        say(f"N = {n}, d = {d}")
        if exact_only:
            tb = alternate([B], max(3, reps if n < 262144 else reps // 2))[0]
            say(f"   B  simtopk_combined (exact)   {stat(tb)}   spread {(max(tb) - min(tb)) / np.median(tb):.4f}")
            del F, P
            release()
            continue

        def A(**kw):
            return fast(F, P, LH, LG, K, precision="fast", **kw)

        def A2(**kw):
            return fast(F, P, LH, LG, K, precision="fast_bf16", **kw)
        mem = [taken(fn) for fn in (A, A2, B)]
        want = B()
        for name, fn in (("fast", A), ("fast_bf16", A2)):
            got = fn()
            assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), f"{name} differs from the exact entry"
        del want, got
        r = reps if n < 262144 else max(3, reps // 2)
        ta, ta2, tb = alternate([A, A2, B], r)
        spread = max(tb) - min(tb)
        say(f"   A  fast (f16)                 {stat(ta)}   B / A {np.median(tb) / np.median(ta):.2f}x   B - A = {np.median(tb) - np.median(ta):.3f} ms = "
            f"{(np.median(tb) - np.median(ta)) / spread if spread > 0 else float('inf'):.0f} x B's spread   memory {mem[0]:.2f} GiB")
        say(f"   A' fast_bf16                  {stat(ta2)}   B / A' {np.median(tb) / np.median(ta2):.2f}x   memory {mem[1]:.2f} GiB")
        say(f"   B  simtopk_combined (exact)   {stat(tb)}   spread {spread:.3f} ms ({spread / np.median(tb):.4f})   memory {mem[2]:.2f} GiB")
        say(f"   A  {events(A, n, d, B16_MFMA_FLOPS)}")
        say(f"   A' {events(A2, n, d, B16_MFMA_FLOPS)}")
        say(f"   B  {events(B, n, d, F32_MFMA_FLOPS)}")
        del F, P
        release()
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
