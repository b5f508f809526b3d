"""The segmented exact scan against what a cohort gets today where no 16-bit scan applies.

    python scripts/segmented_exact_timing.py [out.txt] [--reps N] [--baseline-only]

    A   segmented_exact.simtopk_segmented_exact / simtopk_combined_exact    one table-driven scan launch + one re-rank
    B   ops.simtopk_segmented(precision="exact" | "auto") / combined_topk.simtopk_combined(ptr=...)    the launch loop inside one call
    C   a Python loop of ops.simtopk(precision="exact") / combined_topk.simtopk_combined per segment   one call and one host sync each

Shapes (f32 planted rows cut into segments, cosine unless noted): 2048 x 128, 1000 ragged segments of 100 .. 300 rows, 64 x 4096 and
16 x 16384 at d = 512, k = 5 (col_splits = 0, the automatic rule, everywhere); 2048 x 128 at d = 768, k = 32 (what AUTO sends to the exact pass today); k = 60 on 64 x 4096 (B refuses
k + self > 44: C is the only other arm); the combined key at 2048 x 128 and 64 x 4096 with dp = 2; forced column ranges 1 / 2 / 4 / 8 against
the automatic rule at 4 x 4096.

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max of the whole call.  The verdict lines apply the project's rule
(DESIGN.md §4.1): a default is adopted only where A's whole call beats the other arm by more than three times that arm's spread.
--baseline-only times B alone at 2048 x 128, d = 512 (it uses ops.* only: run it on a build of the parent commit, the baseline is
the parent's)."""
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


def spreads(t_win, t_other):
    s = max(t_other) - min(t_other)
    gain = np.median(t_other) - np.median(t_win)
    return gain, s, (gain / s if s > 0 else float("inf"))


def same_bits(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def events(st):
    return (f"events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms, re-rank {st['rerank_ms']:.3f} ms; col_splits {st['col_splits']}, "
            f"scan_grid {st['scan_grid']}")


def loop_exact(X, ptr, k):
    out = [mmf.ops.simtopk(X[a:b], metric="cosine", k=k, precision="exact", row_offset=a, col_offset=a) for a, b in zip(ptr[:-1], ptr[1:])]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def loop_combined(F, P, ptr, k):
    out = [mmf.combined_topk.simtopk_combined(F[a:b], P[a:b], 0.7, 0.3, k) for a, b in zip(ptr[:-1], ptr[1:])]
    return torch.cat([o[0] + a for o, a in zip(out, ptr[:-1])]), torch.cat([o[1] for o in out])


def report(name, ts, same, verdicts, st, with_b=True):
    other = 1 if with_b else 2
    gain, s, n_spreads = spreads(ts[0], ts[other])
    say(f"{name}  same bits as {'B' if with_b else 'C'}: {same}")
    say(f"   A  one launch      {stat(ts[0])}   {events(st)}")
    if with_b:
        say(f"   B  launch loop     {stat(ts[1])}   B / A {np.median(ts[1]) / np.median(ts[0]):.2f}x   spread of B {s:.3f} ms; B - A = {gain:.3f} ms = {n_spreads:.1f} spreads")
        say(f"   C  Python loop     {stat(ts[2])}   C / A {np.median(ts[2]) / np.median(ts[0]):.2f}x")
    else:
        say(f"   B  refused (k + self > 44)")
        say(f"   C  Python loop     {stat(ts[2])}   C / A {np.median(ts[2]) / np.median(ts[0]):.2f}x   spread of C {s:.3f} ms; C - A = {gain:.3f} ms = {n_spreads:.1f} spreads")
    verdicts.append((name, bool(same and gain > 3.0 * s)))


def plain(name, sizes, d, k, reps, verdicts, b_precision="exact", with_b=True):
    ptr = [0] + np.cumsum(sizes).tolist()
    X = rows(ptr[-1], d, ptr[-1] + d)
    A = lambda **kw: mmf.segmented_exact.simtopk_segmented_exact(X, ptr=ptr, metric="cosine", k=k, **kw)   # noqa: E731
    B = lambda: mmf.ops.simtopk_segmented(X, ptr=ptr, metric="cosine", k=k, precision=b_precision)          # noqa: E731
    C = lambda: loop_exact(X, ptr, k)                                                                        # noqa: E731
    same = same_bits(A(), B() if with_b else C())
    ts = alternate([A, B if with_b else C, C], reps)
    st = A(profile=True, return_stats=True)[2]
    report(f"{name}  d = {d}  k = {k}  {len(sizes)} segments, {ptr[-1]} rows", ts, same, verdicts, st, with_b)
    return X, ptr


def combined(name, sizes, d, k, reps, verdicts):
    ptr = [0] + np.cumsum(sizes).tolist()
    F = rows(ptr[-1], d, ptr[-1] + d)
    P = torch.rand(ptr[-1], 2, generator=torch.Generator(device=dev).manual_seed(5), device=dev) * 4.0
    A = lambda **kw: mmf.segmented_exact.simtopk_combined_exact(F, P, 0.7, 0.3, k, ptr=ptr, **kw)   # noqa: E731
    B = lambda: mmf.combined_topk.simtopk_combined(F, P, 0.7, 0.3, k, ptr=ptr)                       # noqa: E731
    C = lambda: loop_combined(F, P, ptr, k)                                                          # noqa: E731
    same = same_bits(A(), B())
    ts = alternate([A, B, C], reps)
    st = A(profile=True, return_stats=True)[2]
    report(f"combined  {name}  d = {d}  dp = 2  k = {k}  {len(sizes)} segments, {ptr[-1]} rows", ts, same, verdicts, st)


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    rng = np.random.default_rng(2024)
    if "--baseline-only" in args:
        ptr = [0] + np.cumsum([128] * 2048).tolist()
        X = rows(ptr[-1], 512, ptr[-1] + 512)
        B = lambda: mmf.ops.simtopk_segmented(X, ptr=ptr, metric="cosine", k=5, precision="exact")   # noqa: E731
        tb, = alternate([B], reps)
        say(f"2048 x 128  d = 512  cosine  k = 5  B ops.simtopk_segmented(exact) alone  {stat(tb)}   spread {(max(tb) - min(tb)) / np.median(tb):.3f}")
    else:
        say(f"cosine  rounds {reps}  whole-call times, median (min .. max)")
        v = []
        plain("2048 x 128", [128] * 2048, 512, 5, reps, v)
        plain("1000 ragged 100..300", rng.integers(100, 301, size=1000).tolist(), 512, 5, reps, v)
        plain("64 x 4096", [4096] * 64, 512, 5, reps, v)
        torch.cuda.empty_cache()
        plain("16 x 16384", [16384] * 16, 512, 5, reps, v)
        torch.cuda.empty_cache()
        plain("2048 x 128 (AUTO -> exact)", [128] * 2048, 768, 32, reps, v, b_precision="auto")
        plain("64 x 4096 large k", [4096] * 64, 512, 60, reps, v, with_b=False)
        torch.cuda.empty_cache()
        combined("2048 x 128", [128] * 2048, 512, 5, reps, v)
        combined("64 x 4096", [4096] * 64, 512, 5, reps, v)
        torch.cuda.empty_cache()
        for name, ok in v:
            say(f"A beats the other arm by more than 3 of its spreads, same bits: {'met    ' if ok else 'NOT met'}  {name}")
        # column ranges at 4 x 4096: forced counts and the automatic runs against one range
        ptr = [0] + np.cumsum([4096] * 4).tolist()
        X = rows(ptr[-1], 512, ptr[-1] + 512)
        A = lambda **kw: mmf.segmented_exact.simtopk_segmented_exact(X, ptr=ptr, metric="cosine", k=5, **kw)   # noqa: E731
        B = lambda: mmf.ops.simtopk_segmented(X, ptr=ptr, metric="cosine", k=5, precision="exact")              # noqa: E731

        forced = [1, 2, 4, 8]
        ts = alternate([lambda c=c: A(col_splits=c) for c in forced] + [A, B], 2 * reps)
        say(f"4 x 4096  d = 512  k = 5  column ranges, rounds {2 * reps}")
        for c, t in zip(forced, ts):
            say(f"   col_splits = {c}   {stat(t)}   {events(A(col_splits=c, profile=True, return_stats=True)[2])}")
        say(f"   automatic (0)    {stat(ts[4])}   {events(A(profile=True, return_stats=True)[2])}")
        say(f"   B  launch loop   {stat(ts[5])}")
        gain, s, n_spreads = spreads(ts[4], ts[0])
        say(f"automatic range rule (the runs beat one range by more than 3 spreads of one range): one - runs = {gain:.3f} ms = {n_spreads:.1f} "
            f"spreads of {s:.3f} ms: {'met' if gain > 3.0 * s else 'NOT met'}")
        gain, s, n_spreads = spreads(ts[4], ts[5])
        say(f"with the runs against the launch loop at 4 x 4096: B - A = {gain:.3f} ms = {n_spreads:.1f} spreads of {s:.3f} ms: "
            f"{'met' if gain > 3.0 * s else 'NOT met'}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
