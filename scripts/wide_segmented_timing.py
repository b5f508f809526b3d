"""The segmented wide 16-bit scan against what a cohort above a feature dim of 1024 gets without it: cosine, k = 5.

    python scripts/wide_segmented_timing.py [out.txt] [--reps N] [--baseline-only]

    A   wide_scan.simtopk_segmented(precision="auto")        one launch of the wide scan (f16 operands) + exact re-rank
    A'  wide_scan.simtopk_segmented(precision="fast_bf16")   bf16 operands
    B   ops.simtopk_segmented(precision="auto")              the exact pass, two launches per segment: these shapes before §4.16
    C   a Python loop of ops.simtopk(precision="fast")       one wide-scan call (and one host synchronisation) per segment

Shapes (f32 planted rows, the clusters of tests/test_gpu_wide_scan.py cut into segments): 2048 x 128 rows at d = 1536; 1000 ragged
segments of 100 .. 300 rows at d = 1536 and d = 2560; 64 x 4096 at d = 1536; 4 x 4096 at d = 1536 with the automatic column splits
and with col_splits = 1.

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max of the whole call.  The scan's share comes from the call's
event timers (profile=True, one separate call per arm).  Two verdict lines apply the project's rule — the whole call wins by more
than three times the other arm's spread: A against B on every shape decides the cohort routing, the automatic splits against
col_splits = 1 at 4 x 4096 decide the automatic splits rule.  --baseline-only times B alone at 2048 x 128, d = 1536 (run on a build
of the parent commit: the baseline is the parent's)."""
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
    nc = (n + per - 1) // per
    centres = unit(torch.randn(nc, 1, d, generator=g, device=dev))
    a = torch.linspace(0.95, 0.60, per, device=dev)[None, :, None]
    X = a * centres + torch.sqrt(1.0 - a * a) * unit(torch.randn(nc, per, d, generator=g, device=dev))
    return unit(X).reshape(nc * per, d)[:n].contiguous()


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


def events(fn):
    st = fn(profile=True, return_stats=True)[2]
    whole = st["prep_ms"] + st["scan_ms"] + st["rerank_ms"] + st["fallback_ms"]
    return (f"events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms = {st['scan_ms'] / whole if whole > 0 else float('nan'):.2f} of "
            f"the timed stages, re-rank {st['rerank_ms']:.3f} ms, exact pass {st['fallback_ms']:.3f} ms; precision_used {st['precision_used']}, "
            f"col_splits {st['col_splits']}, scan_grid {st['scan_grid']}, fallback_rows {st['fallback_rows']}")


def loop_fast(X, ptr):
    out = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        out.append(mmf.ops.simtopk(X[a:b], metric="cosine", k=K, precision="fast", row_offset=a, col_offset=a))
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def spreads(t_win, t_other):
    s = max(t_other) - min(t_other)
    gain = np.median(t_other) - np.median(t_win)
    return gain, s, (gain / s if s > 0 else float("inf"))


def shape(name, sizes, d, reps, routing, with_loop=True):
    ptr = [0] + np.cumsum(sizes).tolist()
    X = rows(ptr[-1], d, ptr[-1] + d)
    wide = lambda **kw: mmf.wide_scan.simtopk_segmented(X, ptr=ptr, metric="cosine", k=K, **kw)   # noqa: E731
    narrow = lambda **kw: mmf.ops.simtopk_segmented(X, ptr=ptr, metric="cosine", k=K, precision="auto", **kw)   # noqa: E731
    a, a2, b = wide(precision="auto"), wide(precision="fast_bf16"), narrow()
    same = all(torch.equal(x[0], b[0]) and torch.equal(x[1], b[1]) for x in (a, a2))
    del a, a2, b
    arms = [lambda: wide(precision="auto"), lambda: wide(precision="fast_bf16"), narrow] + ([lambda: loop_fast(X, ptr)] if with_loop else [])
    ts = alternate(arms, reps)
    gain, s, n_spreads = spreads(ts[0], ts[2])
    say(f"{name}  d = {d}  {len(sizes)} segments, {ptr[-1]} rows  same bits as B: {same}")
    say(f"   A  wide auto        {stat(ts[0])}   B / A  {np.median(ts[2]) / np.median(ts[0]):.2f}x")
    say(f"   A' wide fast_bf16   {stat(ts[1])}   B / A' {np.median(ts[2]) / np.median(ts[1]):.2f}x")
    say(f"   B  ops auto (exact) {stat(ts[2])}   spread of B {s:.3f} ms; B - A = {gain:.3f} ms = {n_spreads:.1f} spreads")
    if with_loop:
        say(f"   C  loop of fast     {stat(ts[3])}   C / A  {np.median(ts[3]) / np.median(ts[0]):.2f}x")
    say(f"   A  {events(lambda **kw: wide(precision='auto', **kw))}")
    say(f"   A' {events(lambda **kw: wide(precision='fast_bf16', **kw))}")
    say(f"   B  {events(narrow)}")
    routing.append(bool(same and gain > 3.0 * s))
    return X, ptr


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    rng = np.random.default_rng(2024)
    if "--baseline-only" in args:
        sizes = [128] * 2048
        ptr = [0] + np.cumsum(sizes).tolist()
        X = rows(ptr[-1], 1536, ptr[-1] + 1536)
        narrow = lambda **kw: mmf.ops.simtopk_segmented(X, ptr=ptr, metric="cosine", k=K, precision="auto", **kw)   # noqa: E731
        tb, = alternate([narrow], reps)
        say(f"2048 x 128  d = 1536  cosine  k = {K}  B ops.simtopk_segmented(auto) alone  {stat(tb)}   spread {(max(tb) - min(tb)) / np.median(tb):.3f}")
        say(f"   B {events(narrow)}")
    else:
        say(f"cosine  k = {K}  rounds {reps}  whole-call times, median (min .. max)")
        routing = []
        shape("2048 x 128", [128] * 2048, 1536, reps, routing)
        torch.cuda.empty_cache()
        ragged = rng.integers(100, 301, size=1000).tolist()
        for d in (1536, 2560):
            shape("1000 ragged 100..300", ragged, d, reps, routing)
            torch.cuda.empty_cache()
        shape("64 x 4096", [4096] * 64, 1536, reps, routing)
        torch.cuda.empty_cache()
        X, ptr = shape("4 x 4096", [4096] * 4, 1536, reps, routing)
        say(f"cohort routing (A beats B by more than 3 spreads of B, same bits, on every shape): {'met' if all(routing) else 'NOT met'}")
        wide = lambda **kw: mmf.wide_scan.simtopk_segmented(X, ptr=ptr, metric="cosine", k=K, precision="auto", **kw)   # noqa: E731
        forced = [1, 2, 4, 8, 16]
        ts = alternate([wide] + [lambda c=c: wide(col_splits=c) for c in forced], 2 * reps)
        st = wide(return_stats=True)[2]
        say(f"4 x 4096  d = 1536  column splits, rounds {2 * reps}")
        say(f"   automatic (col_splits {st['col_splits']}, scan_grid {st['scan_grid']})   {stat(ts[0])}")
        for c, t in zip(forced, ts[1:]):
            s1 = wide(col_splits=c, profile=True, return_stats=True)[2]
            say(f"   col_splits = {c:2d} (scan_grid {s1['scan_grid']:4d}, scan {s1['scan_ms']:.3f} ms, re-rank {s1['rerank_ms']:.3f} ms, fallback_rows "
                f"{s1['fallback_rows']})   {stat(t)}")
        gain, s, n_spreads = spreads(ts[0], ts[1])
        say(f"automatic splits rule (the automatic choice beats col_splits = 1 by more than 3 spreads of col_splits = 1): one - automatic = "
            f"{gain:.3f} ms = {n_spreads:.1f} spreads of {s:.3f} ms: {'met' if gain > 3.0 * s else 'NOT met'}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
