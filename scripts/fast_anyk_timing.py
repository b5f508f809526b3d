"""The 16-bit top-k for any k against the exact call of the same k, whole-call times.

    python scripts/fast_anyk_timing.py [out.txt] [--reps N] [--skip-large] [--data gaussian|clustered]

    A   fast_anyk.simtopk_fast_any_k(precision="fast")        f16 operands, several passes of the 16-bit scan under per-row ceilings
    A'  fast_anyk.simtopk_fast_any_k(precision="fast_bf16")   bf16 operands
    B   ops.simtopk(precision="exact")                        the f32 matrix-core scan in passes of 44: what these k get today

Cases (f32 rows, cosine, X against itself): N = 65536 and 262144 at d = 512 with k = 64 and 128; N = 65536 at d = 768 with k = 32;
N = 65536 at d = 1024 with k = 32 and 64; and, whatever --data says, clustered rows at N = 65536, d = 512, k = 64.  Gaussian rows
are seeded unit-variance noise; clustered rows are planted clusters of 32 (row = a * centre + sqrt(1 - a^2) * unit noise, a graded
0.95 .. 0.60, normalised).  Then the operating point: MMF_ANYK_SHORT_DIV = 16 / 64 / 256 at N = 65536, d = 512, k = 128.

Everything runs in one process.  Every case is warmed by one call of each arm (whose results are compared bit for bit), then
`reps` rounds time the arms in turn with a device synchronisation around every timed call: median and min .. max of the whole
call.  Per case the passes, yields and exact_rows of A and A'.  The verdict applies the project's rule to each case: the new call
is ahead only if median(B) - median(A) exceeds three times B's spread (max - min)."""
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


def rows(n, d, seed, data):
    g = torch.Generator(device=dev).manual_seed(seed)
    if data == "gaussian":
        return torch.randn(n, d, generator=g, device=dev)
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)   # noqa: E731
    per = 32
    centres = unit(torch.randn(n // per, 1, d, generator=g, device=dev))
    a = torch.linspace(0.95, 0.60, per, device=dev)[None, :, None]
    X = a * centres + torch.sqrt(1.0 - a * a) * unit(torch.randn(n // per, per, d, generator=g, device=dev))
    return unit(X).reshape(n, d).contiguous()


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def alternate(arms, reps):
    ts = [[] for _ in arms]
    for _ in range(reps):
        for t, fn in zip(ts, arms):
            t.append(once(fn)[0])
    return ts


def case(n, d, k, data, reps):
    X = rows(n, d, n + d + k, data)
    fast = lambda p: mmf.simtopk_fast_any_k(X, metric="cosine", k=k, precision=p, return_info=True)   # noqa: E731
    exact = lambda: mmf.ops.simtopk(X, metric="cosine", k=k, precision="exact")                       # noqa: E731
    b = exact()                                   # the warm-up calls double as the comparison of the bits
    infos, same = [], True
    for p in ("fast", "fast_bf16"):
        i, v, info = fast(p)
        same &= torch.equal(i, b[0]) and torch.equal(v.view(torch.int32), b[1].view(torch.int32))
        infos.append(info)
        del i, v
    del b
    ta, ta2, tb = alternate([lambda: fast("fast"), lambda: fast("fast_bf16"), exact], reps)
    spread = max(tb) - min(tb)
    ahead = [same and np.median(tb) - np.median(t) > 3.0 * spread for t in (ta, ta2)]
    say(f"N = {n}  d = {d}  k = {k}  {data}  rounds {reps}  same bits as exact: {same}")
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
    data = args[args.index("--data") + 1] if "--data" in args else "gaussian"
    say("cosine, f32 rows, X against itself; whole-call times, median (min .. max)")
    cases = [(65536, 512, 64), (65536, 512, 128), (65536, 768, 32), (65536, 1024, 32), (65536, 1024, 64)]
    if "--skip-large" not in args:
        cases += [(262144, 512, 64), (262144, 512, 128)]
    verdict = {}
    for n, d, k in cases:
        verdict[(n, d, k, data)] = case(n, d, k, data, reps if n < 262144 else max(3, reps // 2))
    if data != "clustered":
        verdict[(65536, 512, 64, "clustered")] = case(65536, 512, 64, "clustered", reps)
    say("operating point: MMF_ANYK_SHORT_DIV at N = 65536, d = 512, k = 128, gaussian, precision fast")
    X = rows(65536, 512, 65536 + 512 + 128, "gaussian")
    ref = None
    arms = []
    for div in ("16", "64", "256"):
        def arm(div=div):
            os.environ["MMF_ANYK_SHORT_DIV"] = div
            try:
                return mmf.simtopk_fast_any_k(X, metric="cosine", k=128, return_info=True)
            finally:
                del os.environ["MMF_ANYK_SHORT_DIV"]
        i, v, info = arm()
        ref = ref or (i, v)
        say(f"   div {div:>3}: same bits as div 16: {torch.equal(i, ref[0]) and torch.equal(v.view(torch.int32), ref[1].view(torch.int32))}  "
            f"passes {info['passes']}  yields {info['yield']}  exact_rows {info['exact_rows']}")
        arms.append(arm)
    for div, t in zip(("16", "64", "256"), alternate(arms, reps)):
        say(f"   div {div:>3}: {stat(t)}")
    say("three-spreads rule, per case (fast, fast_bf16): " + "; ".join(f"N={n} d={d} k={k} {dt}: {a}" for (n, d, k, dt), a in verdict.items()))
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
