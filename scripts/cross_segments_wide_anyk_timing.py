"""The wide 16-bit cross-segment top-k for any k against the exact cross-segment call of the same k, whole-call times.

    python scripts/cross_segments_wide_anyk_timing.py [out.txt] [--reps N] [--skip-large]

    A   cross_segments_wide_anyk.simtopk_cross_segments_wide_any_k(precision="fast")   f16 operands, passes of the masked wide scan under ceilings
    A'  the same with precision="fast_bf16" (one shape only)                           bf16 operands
    B   cross_segments.simtopk_cross_segments                                          the table-driven f32 scan in passes of 44: what these k get today

Cases (f32 Gaussian rows, cosine, X against itself).  The first four are the cohorts of profiles/cross_segments_wide_timing.txt at
k = 32: 64 segments of 1024 rows, 512 slides of 128 rows and 250 ragged slides of 100 .. 300 rows at d = 1536, 16 segments of 4096
rows at d = 2560; then 64 x 1024 at d = 1536 with k = 64.  The bf16 row is 64 x 1024 at d = 1536, k = 32.  --skip-large leaves out
the d = 2560 cohort.

Everything runs in one process.  Every case is warmed by one call of each arm (whose results are compared bit for bit), then `reps`
rounds time the arms in turn with a device synchronisation around every timed call: median and min .. max of the whole call.  Per
case the passes, yields, ghost_max and rows rescanned per pass (exact_rows) of A.  The verdict applies the project's rule to each
case: the new call is ahead only if median(B) - median(A) is at least three times B's spread (max - min)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402

dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def alternate(arms, reps):
    ts = [[] for _ in arms]
    for _ in range(reps):
        for t, fn in zip(ts, arms):
            t.append(once(fn)[0])
    return ts


def case(name, sizes, d, k, reps, bf16=False):
    n = int(sum(sizes))
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    X = torch.randn(n, d, generator=torch.Generator(device=dev).manual_seed(n + d + k), device=dev)
    fast = lambda p: mmf.simtopk_cross_segments_wide_any_k(X, ptr=ptr, metric="cosine", k=k, precision=p, return_info=True)   # noqa: E731
    exact = lambda: mmf.cross_segments.simtopk_cross_segments(X, ptr=ptr, metric="cosine", k=k)                               # noqa: E731
    b = exact()                                   # the warm-up calls double as the comparison of the bits
    precisions = ("fast", "fast_bf16") if bf16 else ("fast",)
    infos, same = [], True
    for p in precisions:
        i, v, info = fast(p)
        torch.cuda.synchronize()
        same &= torch.equal(i, b[0]) and torch.equal(v.view(torch.int32), b[1].view(torch.int32))
        infos.append(info)
        del i, v
    del b
    assert same, f"{name}: the new call differs from the exact call"
    ts = alternate([(lambda p=p: fast(p)) for p in precisions] + [exact], reps)
    tb = ts[-1]
    spread = max(tb) - min(tb)
    say(f"{name}: {len(sizes)} segments, N = {n}  d = {d}  k = {k}  rounds {reps}  same bits as exact: {same}")
    ahead = []
    for tag, t, info in zip(("A  fast     ", "A' fast_bf16"), ts[:-1], infos):
        ok = bool(same and np.median(tb) - np.median(t) >= 3.0 * spread)
        ahead.append(ok)
        say(f"   {tag} {stat(t)}   A / B {np.median(t) / np.median(tb):.3f}   B - A = {(np.median(tb) - np.median(t)) / spread if spread > 0 else float('inf'):.1f} "
            f"spreads of B: {'ahead' if ok else 'NOT ahead'}")
        say(f"        passes {info['passes']}  yields {info['yield']}  ghost_max {info['ghost_max']}  rows rescanned per pass {info['exact_rows']}")
    say(f"   B  exact     {stat(tb)}   spread of B {spread:.3f} ms")
    del X
    torch.cuda.empty_cache()
    return ahead


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    large = "--skip-large" not in args
    say("cosine, f32 Gaussian rows, X against itself, every row against all other segments; whole-call times, median (min .. max)")
    verdict = {}
    ragged = np.random.default_rng(2024).integers(100, 301, size=250).tolist()      # scripts/cross_segments_wide_timing.py's: 47943 rows
    verdict[("64 x 1024", 1536, 32)] = case("64 x 1024", [1024] * 64, 1536, 32, reps, bf16=True)
    verdict[("512 x 128", 1536, 32)] = case("512 x 128", [128] * 512, 1536, 32, reps)
    verdict[("250 ragged 100..300", 1536, 32)] = case("250 ragged slides of 100 .. 300 rows", ragged, 1536, 32, reps)
    if large:
        verdict[("16 x 4096", 2560, 32)] = case("16 x 4096", [4096] * 16, 2560, 32, reps)
    verdict[("64 x 1024", 1536, 64)] = case("64 x 1024", [1024] * 64, 1536, 64, reps)
    say("three-spreads rule, per case (fast[, fast_bf16]): " + "; ".join(f"{name} d={d} k={k}: {a}" for (name, d, k), a in verdict.items()))
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
