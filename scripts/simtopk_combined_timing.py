"""Top-k of the combined similarity K_h * K_g (combined_topk.simtopk_combined) against what a user has without it.
d = 512, positions 2-D in pixel units (grid cells x 224), lambda_h = 0.5, lambda_g = 2e-7, k = 5; whole-call times.

    python scripts/simtopk_combined_timing.py [out.txt] [--reps N] [--skip-large]

    1  N = 65536: simtopk_combined against ops.simtopk(F, metric="rbf", precision="exact") on the same rows — the same scan
       without the position term.  The difference is the price of the position term in the scan's epilogue and the re-rank; the
       ratio stands next to the spread of the rbf arm and is not gated.
    2  N = 16384: against the materialised form, ops.sim_dense_combined + torch.sort per row (N^2 floats stored and sorted).
    3  64 segments of 4096 rows: one call against a Python loop of single-graph calls.
    4  N = 262144, where nothing can be stored: the call alone, and the device memory the first call took (its workspace).

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max.  The scan's own time comes from the call's event timers
(profile=True, one separate call); its share of the f32 matrix-core peak is 2 d flop per pair over that time.  With several
segments the launches of scan and re-rank alternate and one timer covers them all."""
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
D, K, LH, LG = 512, 5, 0.5, 2e-7
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


def rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(12, D, generator=g)
    F = centres[torch.randint(0, 12, (n,), generator=g)] + 0.05 * torch.randn(n, D, generator=g)
    P = (torch.randint(0, 24, (n, 2), generator=g) * 224).float()
    return F.to(dev), P.to(dev)


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


def scan_share(n_pairs, F, P, **kw):
    st = ct.simtopk_combined(F, P, LH, LG, K, return_stats=True, profile=True, **kw)[2]
    share = 2.0 * D * n_pairs / (st["scan_ms"] * 1e-3) / F32_MFMA_FLOPS if st["scan_ms"] > 0 else float("nan")
    if "ptr" in kw:   # several segments: the launches alternate, one timer covers the image and every segment's scan and re-rank
        return (f"events: row scalars {st['prep_ms']:.3f} ms, image + every segment's scan and re-rank {st['scan_ms']:.3f} ms: "
                f"{share:.2f} of the f32 matrix-core peak ({F32_MFMA_FLOPS / 1e12:.1f} TF); workgroups {st['scan_grid']}, col_splits "
                f"{st['col_splits']} per segment, candidates per row {st['candidates'] / F.shape[0]:.1f}")
    return (f"events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms, re-rank {st['rerank_ms']:.3f} ms; scan at "
            f"{share:.2f} of the f32 matrix-core peak ({F32_MFMA_FLOPS / 1e12:.1f} TF); grid {st['scan_grid']}, col_splits {st['col_splits']}, "
            f"candidates per row {st['candidates'] / F.shape[0]:.1f}")


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    say(f"d {D}  dp 2  k {K}  lambda_h {LH}  lambda_g {LG}  rounds {reps}  whole-call times, median (min .. max)")

    # 4 first: the workspace it takes is the process's largest, so the figure is that call's own
    if "--skip-large" not in args:
        n = 262144
        F, P = rows(n, 4)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(dev)[0]
        once(lambda: ct.simtopk_combined(F, P, LH, LG, K))
        took = free0 - torch.cuda.mem_get_info(dev)[0]
        ta = [once(lambda: ct.simtopk_combined(F, P, LH, LG, K))[0] for _ in range(max(3, reps // 2))]
        say(f"4  N = {n}, one graph: K would take {n * n * 4 / 2 ** 30:.0f} GiB")
        say(f"   simtopk_combined (alone)                {stat(ta)}   device memory taken by the first call "
            f"(workspace + outputs): {took / 2 ** 30:.2f} GiB")
        say(f"   {scan_share(n * n, F, P)}")
        del F, P
        mmf._lib.check(mmf._lib.lib().mmf_release_workspaces(), "mmf_release_workspaces")
        torch.cuda.empty_cache()

    n = 65536
    F, P = rows(n, 1)
    a, b = ct.simtopk_combined(F, P, LH, 0.0, K), mmf.ops.simtopk(F, metric="rbf", lam=LH, k=K, precision="exact")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "lambda_g = 0 must give the rbf top-k"
    ta, tb = alternate([lambda: ct.simtopk_combined(F, P, LH, LG, K),
                        lambda: mmf.ops.simtopk(F, metric="rbf", lam=LH, k=K, precision="exact")], reps)
    say(f"1  N = {n}, one graph")
    say(f"   A simtopk_combined                      {stat(ta)}")
    say(f"   B simtopk rbf exact (no position term)  {stat(tb)}   A / B {np.median(ta) / np.median(tb):.3f}, spread of B "
        f"{(max(tb) - min(tb)) / np.median(tb):.3f}")
    say(f"   A {scan_share(n * n, F, P)}")
    del F, P

    n = 16384
    F, P = rows(n, 2)

    def stored():
        Kd = mmf.ops.sim_dense_combined(F, P, LH, LG)
        Kd.fill_diagonal_(-1.0)
        v, i = torch.sort(Kd, dim=1, descending=True, stable=True)
        return i[:, :K].contiguous(), v[:, :K].contiguous()
    ta, tb = alternate([lambda: ct.simtopk_combined(F, P, LH, LG, K), stored], reps)
    say(f"2  N = {n}, one graph: the stored form holds {n * n * 4 / 2 ** 30:.0f} GiB of K and sorts it")
    say(f"   A simtopk_combined                      {stat(ta)}")
    say(f"   B sim_dense_combined + torch.sort       {stat(tb)}   B / A {np.median(tb) / np.median(ta):.1f}x")
    del F, P
    torch.cuda.empty_cache()

    S, ns = 64, 4096
    F, P = rows(S * ns, 3)
    ptr = torch.arange(S + 1, dtype=torch.int64) * ns

    def loop():
        return [ct.simtopk_combined(F[s * ns:(s + 1) * ns], P[s * ns:(s + 1) * ns], LH, LG, K) for s in range(S)]
    one = ct.simtopk_combined(F, P, LH, LG, K, ptr=ptr)
    parts = loop()
    assert torch.equal(one[0], torch.cat([p[0] + s * ns for s, p in enumerate(parts)])) and torch.equal(one[1], torch.cat([p[1] for p in parts]))
    ta, tb = alternate([lambda: ct.simtopk_combined(F, P, LH, LG, K, ptr=ptr), loop], reps)
    say(f"3  {S} segments of {ns} rows")
    say(f"   A one call                              {stat(ta)}")
    say(f"   B Python loop of single-graph calls     {stat(tb)}   B / A {np.median(tb) / np.median(ta):.2f}x   (same bits)")
    say(f"   A {scan_share(S * ns * ns, F, P, ptr=ptr)}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
