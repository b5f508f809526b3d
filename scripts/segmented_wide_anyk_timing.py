"""The segmented wide 16-bit top-k for any k against the exact segmented call of the same k, whole-call times.

    python scripts/segmented_wide_anyk_timing.py [out.txt] [--reps N] [--skip-large]

    A   segmented_wide_anyk.simtopk_segmented_wide_any_k(precision="fast")   f16 operands, passes of the table-driven wide 16-bit scan under ceilings
    A'  the same with precision="fast_bf16" (one shape only)                 bf16 operands
    B   segmented_exact.simtopk_segmented_exact                              the table-driven f32 scan: what these (d, k) get today

Cases (f32 Gaussian rows, cosine, X against itself, 262144 rows): 4 segments of 65536 rows, 16 of 16384, 64 of 4096 and 2048 of 128
at d = 1536 with k = 32; 16 x 16384 at d = 2560, k = 32 and at d = 1536, k = 64; bf16 operands on 64 x 4096 at d = 1536, k = 32.
--skip-large leaves out the 4 x 65536 cohort.

Everything runs in one process.  Every case is warmed by one call of each arm, whose results are compared bit for bit (the script
asserts it before it times anything), then `reps` rounds time the arms in turn with a device synchronisation around every timed
call: median and min .. max of the whole call.  Per case the passes, yields and exact_rows (rows rescanned per pass) of A.  The
verdict applies the project's rule to each case: the new call is ahead only if median(B) - median(A) exceeds three times B's
spread (max - min)."""
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
    fast = lambda p: mmf.simtopk_segmented_wide_any_k(X, ptr=ptr, metric="cosine", k=k, precision=p, return_info=True)   # noqa: E731
    exact = lambda: mmf.simtopk_segmented_exact(X, ptr=ptr, metric="cosine", k=k)                                      # noqa: E731
    b = exact()                                   # the warm-up calls double as the comparison of the bits
    precisions = ("fast", "fast_bf16") if bf16 else ("fast",)
    infos = []
    for p in precisions:
        i, v, info = fast(p)
        torch.cuda.synchronize()
        assert torch.equal(i, b[0]) and torch.equal(v.view(torch.int32), b[1].view(torch.int32)), f"{name} d={d} k={k} {p}: bits differ from the exact call"
        infos.append(info)
        del i, v
    del b
    ts = alternate([(lambda p=p: fast(p)) for p in precisions] + [exact], reps)
    tb = ts[-1]
    spread = max(tb) - min(tb)
    say(f"{name}: {len(sizes)} segments, N = {n}  d = {d}  k = {k}  rounds {reps}  same bits as exact: True")
    ahead = []
    for tag, t, info in zip(("A  fast     ", "A' fast_bf16"), ts[:-1], infos):
        ok = bool(np.median(tb) - np.median(t) > 3.0 * spread)
        ahead.append(ok)
        say(f"   {tag} {stat(t)}   A / B {np.median(t) / np.median(tb):.3f}   B - A = {(np.median(tb) - np.median(t)) / spread if spread > 0 else float('inf'):.1f} "
            f"spreads of B: {'ahead' if ok else 'NOT ahead'}")
        say(f"        passes {info['passes']}  yields {info['yield']}  ghost_max {info['ghost_max']}  exact_rows {info['exact_rows']}")
    say(f"   B  exact     {stat(tb)}   spread of B {spread:.3f} ms")
    del X
    torch.cuda.empty_cache()
    return ahead


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    say("cosine, f32 Gaussian rows, X against itself per segment; whole-call times, median (min .. max)")
    verdict = {}
    cohorts = [] if "--skip-large" in args else [("4 x 65536", [65536] * 4)]
    cohorts += [("16 x 16384", [16384] * 16), ("64 x 4096", [4096] * 64), ("2048 x 128", [128] * 2048)]
    for name, sizes in cohorts:
        verdict[(name, 1536, 32)] = case(name, sizes, 1536, 32, reps, bf16=(name == "64 x 4096"))
    verdict[("16 x 16384", 2560, 32)] = case("16 x 16384", [16384] * 16, 2560, 32, reps)
    verdict[("16 x 16384", 1536, 64)] = case("16 x 16384", [16384] * 16, 1536, 64, reps)
    say("three-spreads rule, per case (fast[, fast_bf16]): " + "; ".join(f"{name} d={d} k={k}: {a}" for (name, d, k), a in verdict.items()))
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
