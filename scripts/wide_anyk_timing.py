"""The wide 16-bit top-k for any k against the exact call of the same k, whole-call times.

    python scripts/wide_anyk_timing.py [out.txt] [--reps N] [--skip-large] [--only-exact]

    A   wide_anyk.simtopk_wide_any_k(precision="fast")        f16 operands, several passes of the wide 16-bit scan under per-row ceilings
    A'  wide_anyk.simtopk_wide_any_k(precision="fast_bf16")   bf16 operands
    B   ops.simtopk(precision="exact")                        the f32 matrix-core scan: what these k get today above d = 1024

Cases (f32 rows, cosine, X against itself, seeded unit-variance Gaussian rows): N = 16384 and 65536 at d = 1536 with k = 32;
N = 65536 at d = 1536 with k = 64; N = 65536 at d = 2560 with k = 32; N = 262144 at d = 1536 with k = 32 (--skip-large leaves it out).

Everything runs in one process, the method of scripts/fast_anyk_timing.py.  Every case is warmed by one call of each arm (whose
results are compared bit for bit), then `reps` rounds (5; 3 at N = 262144) time the arms in turn with a device synchronisation
around every timed call: median and min .. max of the whole call.  Per case the passes, yields and exact_rows of A and A'.  The
verdict applies the project's rule to each case: the new call is ahead only if median(B) - median(A) exceeds three times B's
spread (max - min).  --only-exact times B alone, on a build that has no wide any-k call (the parent's), to confirm B."""
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


def rows(n, d, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, d, generator=g, device=dev)


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def alternate(arms, reps):
    ts = [[] for _ in arms]
    for _ in range(reps):
        for t, fn in zip(ts, arms):
            t.append(once(fn)[0])
    return ts


def case(n, d, k, reps, only_exact):
    X = rows(n, d, n + d + k)
    exact = lambda: mmf.ops.simtopk(X, metric="cosine", k=k, precision="exact")                       # noqa: E731
    b = exact()                                   # the warm-up calls double as the comparison of the bits
    if only_exact:
        del b
        tb, = alternate([exact], reps)
        say(f"N = {n}  d = {d}  k = {k}  rounds {reps}")
        say(f"   B  exact     {stat(tb)}   spread of B {max(tb) - min(tb):.3f} ms")
        return None
    fast = lambda p: mmf.simtopk_wide_any_k(X, metric="cosine", k=k, precision=p, return_info=True)   # noqa: E731
    infos, same = [], True
    for p in ("fast", "fast_bf16"):
        i, v, info = fast(p)
        same &= torch.equal(i, b[0]) and torch.equal(v.view(torch.int32), b[1].view(torch.int32))
        infos.append(info)
        del i, v
    del b
    ta, ta2, tb = alternate([lambda: fast("fast"), lambda: fast("fast_bf16"), exact], reps)
    spread = max(tb) - min(tb)
    ahead = [bool(same and np.median(tb) - np.median(t) > 3.0 * spread) for t in (ta, ta2)]
    say(f"N = {n}  d = {d}  k = {k}  rounds {reps}  same bits as exact: {same}")
    for tag, t, info, ok in (("A  fast     ", ta, infos[0], ahead[0]), ("A' fast_bf16", ta2, infos[1], ahead[1])):
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
    only_exact = "--only-exact" in args
    say("cosine, f32 rows, X against itself, gaussian; whole-call times, median (min .. max)")
    cases = [(16384, 1536, 32), (65536, 1536, 32), (65536, 1536, 64), (65536, 2560, 32)]
    if "--skip-large" not in args:
        cases += [(262144, 1536, 32)]
    verdict = {}
    for n, d, k in cases:
        verdict[(n, d, k)] = case(n, d, k, reps if n < 262144 else max(3, reps // 2), only_exact)
        if out_path:                               # what is measured so far survives a run that is cut short
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")
    if not only_exact:
        say("three-spreads rule, per case (fast, fast_bf16): " + "; ".join(f"N={n} d={d} k={k}: {a}" for (n, d, k), a in verdict.items()))
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
