"""The wide 16-bit scan against the exact scan at feature dims above 1024: ops.simtopk, cosine, k = 5.

    python scripts/wide_scan_timing.py [out.txt] [--reps N] [--skip-large] [--baseline-only]

    A   precision="fast"        f16 operands, scan_b16w_kernel + exact re-rank
    A'  precision="fast_bf16"   bf16 operands
    B   precision="exact"       the f32 matrix-core scan: what these shapes get without the wide scan

Shapes: N in {16384, 65536, 262144} x d in {1536, 2560}.  Rows are planted clusters of 32 (row = a * centre + sqrt(1 - a^2) * unit
noise, a graded 0.95 .. 0.60, normalised) — the data of tests/test_gpu_wide_scan.py at size.

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max of the whole call.  Scan and re-rank times come from the
call's event timers (profile=True, one separate call per arm); the scan's share of the 2.5 PFLOP/s 16-bit peak (B: of the 157.3
TFLOP/s f32 matrix-core peak) is 2 N^2 d flop over the scan time.  The verdict line applies the rule MMF_PREC_AUTO follows: the
wide scan is AUTO's choice only if the whole call beats B by more than three times B's spread at N = 16384 and at N = 65536, d =
1536.  --baseline-only times B alone at N = 65536, d = 1536 (run on a build of the parent commit: the baseline is the parent's)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402

dev = torch.device("cuda", 0)
lines = []
K = 5
PEAK16, PEAK32 = 2.5e15, 157.3e12


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
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)   # noqa: E731
    per = 32
    centres = unit(torch.randn(n // per, 1, d, generator=g, device=dev))
    a = torch.linspace(0.95, 0.60, per, device=dev)[None, :, None]
    X = a * centres + torch.sqrt(1.0 - a * a) * unit(torch.randn(n // per, per, d, generator=g, device=dev))
    return unit(X).reshape(n, d).contiguous()


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


def events(X, precision, peak):
    st = mmf.ops.simtopk(X, metric="cosine", k=K, precision=precision, profile=True, return_stats=True)[2]
    n, d = X.shape
    share = 2.0 * n * n * d / (st["scan_ms"] * 1e-3) / peak if st["scan_ms"] > 0 else float("nan")
    return (f"events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms = {share:.3f} of the {'16-bit' if peak == PEAK16 else 'f32'} "
            f"peak, re-rank {st['rerank_ms']:.3f} ms, rescan {st['fallback_ms']:.3f} ms; precision_used {st['precision_used']}, grid "
            f"{st['scan_grid']}, col_splits {st['col_splits']}, candidates per row {st['candidates'] / n:.1f}, fallback_rows {st['fallback_rows']}")


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    exact = lambda X: mmf.ops.simtopk(X, metric="cosine", k=K, precision="exact")   # noqa: E731
    if "--baseline-only" in args:
        X = rows(65536, 1536, 65536 + 1536)
        tb, = alternate([lambda: exact(X)], reps)
        say(f"N = 65536  d = 1536  cosine  k = {K}  B exact alone  {stat(tb)}   spread {(max(tb) - min(tb)) / np.median(tb):.3f}")
        say(f"   B {events(X, 'exact', PEAK32)}")
    else:
        say(f"cosine  k = {K}  rounds {reps} (N = 262144: {max(2, reps // 2)})  whole-call times, median (min .. max)")
        verdict = []
        for d in (1536, 2560):
            for n in (16384, 65536, 262144):
                if n == 262144 and "--skip-large" in args:
                    continue
                X = rows(n, d, n + d)
                a, a2, b = (mmf.ops.simtopk(X, metric="cosine", k=K, precision=p) for p in ("fast", "fast_bf16", "exact"))
                same = all(torch.equal(x[0], b[0]) and torch.equal(x[1], b[1]) for x in (a, a2))
                del a, a2, b
                ta, ta2, tb = alternate([lambda: mmf.ops.simtopk(X, metric="cosine", k=K, precision="fast"),
                                         lambda: mmf.ops.simtopk(X, metric="cosine", k=K, precision="fast_bf16"),
                                         lambda: exact(X)], reps if n < 262144 else max(2, reps // 2))
                spread = max(tb) - min(tb)
                say(f"N = {n}  d = {d}  2 N^2 d = {2.0 * n * n * d:.3e} flop  same bits as exact: {same}")
                say(f"   A  fast        {stat(ta)}   B / A  {np.median(tb) / np.median(ta):.2f}x")
                say(f"   A' fast_bf16   {stat(ta2)}   B / A' {np.median(tb) / np.median(ta2):.2f}x")
                say(f"   B  exact       {stat(tb)}   spread of B {spread:.3f} ms; B - A = {np.median(tb) - np.median(ta):.3f} ms = "
                    f"{(np.median(tb) - np.median(ta)) / spread if spread > 0 else float('inf'):.1f} spreads")
                say(f"   A  {events(X, 'fast', PEAK16)}")
                say(f"   A' {events(X, 'fast_bf16', PEAK16)}")
                say(f"   B  {events(X, 'exact', PEAK32)}")
                if d == 1536 and n in (16384, 65536):
                    verdict.append(same and np.median(tb) - np.median(ta) > 3.0 * spread)
                del X
                torch.cuda.empty_cache()
        say(f"AUTO rule (whole call beats B by more than 3 spreads of B at N = 16384 and N = 65536, d = 1536): "
            f"{'met' if len(verdict) == 2 and all(verdict) else 'NOT met'}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
