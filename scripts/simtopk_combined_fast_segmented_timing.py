"""The segmented 16-bit top-k of the combined similarity (combined_topk16_segmented.simtopk_combined_fast_segmented)
against what a ragged batch gets without it.  dp = 2, k = 5, lambda_h = 0.5, lambda_g = 2e-7; per segment the data of
scripts/simtopk_combined_fast_timing.py (unit-norm planted features, distinct pixel positions); whole-call times.

    python scripts/simtopk_combined_fast_segmented_timing.py [out.txt] [--reps N] [--baseline-only]

    A   simtopk_combined_fast_segmented(precision="fast")        one launch of the combined-key scan (f16 operands) + exact re-rank
    A'  simtopk_combined_fast_segmented(precision="fast_bf16")   bf16 operands
    B   combined_topk.simtopk_combined(ptr=...)                  the exact pass, two launches per segment: these shapes before §4.18
    C   a Python loop of combined_topk16.simtopk_combined_fast(precision="fast") per segment (one host synchronisation each)

Shapes: 2048 x 128, 1000 ragged 100 .. 300, 64 x 4096 and 16 x 16384 at d = 512; 64 x 4096 at d = 1536; 4 x 4096 at d = 512 with
col_splits 1 / 2 / 4.

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max of the whole call.  Every arm is checked against B's bits
before it is timed.  The scan's share of the 16-bit matrix-core peak comes from the call's event timers (profile=True, one separate
call): 2 d flop per pair of a segment over the scan's time.  Two verdict lines apply the project's rule — the whole call wins by
more than three times the other arm's spread: A against B at every shape of a (d, k) range decides what precision="auto" does
there, two ranges against one at 4 x 4096 decide the automatic splits.  --baseline-only times B alone at 64 x 4096, d = 512 and touches
nothing this feature added: copied into a checkout of the parent commit and run there, it gives the parent's baseline."""
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
    return F.contiguous(), P.contiguous()


def batch(sizes, d):
    parts = [rows(n_s, d, 7 * s + n_s + d) for s, n_s in enumerate(sizes)]
    ptr = torch.tensor([0] + np.cumsum(sizes).tolist(), dtype=torch.int64)
    return torch.cat([p[0] for p in parts]).to(dev), torch.cat([p[1] for p in parts]).to(dev), ptr


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


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def events(fn, pairs, d, n):
    st = fn(profile=True, return_stats=True)[2]
    whole = st["prep_ms"] + st["scan_ms"] + st["rerank_ms"] + st["fallback_ms"]
    share = 2.0 * d * pairs / (st["scan_ms"] * 1e-3) / B16_MFMA_FLOPS if st["precision_used"] != 1 and st["scan_ms"] > 0 else float("nan")
    return (f"events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms = {st['scan_ms'] / whole if whole > 0 else float('nan'):.2f} of "
            f"the timed stages and {share:.3f} of the 16-bit peak, re-rank {st['rerank_ms']:.3f} ms, exact pass {st['fallback_ms']:.3f} ms; "
            f"precision_used {st['precision_used']}, col_splits {st['col_splits']}, scan_grid {st['scan_grid']}, fallback_rows "
            f"{st['fallback_rows']}, candidates per row {st['candidates'] / max(1, n):.1f}")


def loop_fast(F, P, ptr):
    out = [mmf.simtopk_combined_fast(F[a:b], P[a:b], LH, LG, K, precision="fast") for a, b in zip(ptr[:-1], ptr[1:])]
    return torch.cat([o[0] + a for o, a in zip(out, ptr[:-1])]), torch.cat([o[1] for o in out])


def spreads(t_win, t_other):
    s = max(t_other) - min(t_other)
    gain = np.median(t_other) - np.median(t_win)
    return gain, s, (gain / s if s > 0 else float("inf"))


def shape(name, sizes, d, reps, verdicts):
    F, P, ptr = batch(sizes, d)
    pl = ptr.tolist()
    pairs = float(sum(n_s * n_s for n_s in sizes))
    seg = lambda **kw: mmf.simtopk_combined_fast_segmented(F, P, LH, LG, K, ptr=ptr, **kw)   # noqa: E731
    exact = lambda **kw: ct.simtopk_combined(F, P, LH, LG, K, ptr=ptr, **kw)   # noqa: E731
    b = exact()
    same = [same_bits(seg(precision="fast"), b), same_bits(seg(precision="fast_bf16"), b), same_bits(loop_fast(F, P, pl), b)]
    del b
    arms = [lambda: seg(precision="fast"), lambda: seg(precision="fast_bf16"), exact, lambda: loop_fast(F, P, pl)]
    ts = alternate(arms, reps)
    gain, s, n_spreads = spreads(ts[0], ts[2])
    say(f"{name}  d = {d}  {len(sizes)} segments, {pl[-1]} rows  same bits as B (A, A', C): {same}")
    say(f"   A  segmented fast        {stat(ts[0])}   B / A  {np.median(ts[2]) / np.median(ts[0]):.2f}x")
    say(f"   A' segmented fast_bf16   {stat(ts[1])}   B / A' {np.median(ts[2]) / np.median(ts[1]):.2f}x")
    say(f"   B  simtopk_combined(ptr) {stat(ts[2])}   spread of B {s:.3f} ms; B - A = {gain:.3f} ms = {n_spreads:.1f} spreads")
    say(f"   C  loop of one-graph fast{stat(ts[3])}   C / A  {np.median(ts[3]) / np.median(ts[0]):.2f}x")
    say(f"   A  {events(lambda **kw: seg(precision='fast', **kw), pairs, d, pl[-1])}")
    say(f"   A' {events(lambda **kw: seg(precision='fast_bf16', **kw), pairs, d, pl[-1])}")
    verdicts.append((name, d, bool(all(same) and gain > 3.0 * s)))
    return F, P, ptr


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    rng = np.random.default_rng(2024)
    if "--baseline-only" in args:
        F, P, ptr = batch([4096] * 64, 512)
        exact = lambda: ct.simtopk_combined(F, P, LH, LG, K, ptr=ptr)   # noqa: E731
        tb, = alternate([exact], reps)
        say(f"64 x 4096  d = 512  k = {K}  B combined_topk.simtopk_combined(ptr) alone  {stat(tb)}   spread {(max(tb) - min(tb)) / np.median(tb):.3f}")
    else:
        say(f"simtopk_combined_fast_segmented  dp = 2  k = {K}  lambda_h = {LH}  lambda_g = {LG}  rounds {reps}  whole-call times, median (min .. max)")
        verdicts = []
        shape("2048 x 128", [128] * 2048, 512, reps, verdicts)
        torch.cuda.empty_cache()
        shape("1000 ragged 100..300", rng.integers(100, 301, size=1000).tolist(), 512, reps, verdicts)
        torch.cuda.empty_cache()
        shape("64 x 4096", [4096] * 64, 512, reps, verdicts)
        torch.cuda.empty_cache()
        shape("16 x 16384", [16384] * 16, 512, reps, verdicts)
        torch.cuda.empty_cache()
        shape("64 x 4096", [4096] * 64, 1536, reps, verdicts)
        torch.cuda.empty_cache()
        for name, d, ok in verdicts:
            say(f"auto rule at {name}, d = {d} (A beats B by more than 3 spreads of B, same bits): {'met' if ok else 'NOT met'}")
        say(f"auto rule, 512 <= d <= 1536, k + self <= 11 (every measured shape): {'met' if all(v[2] for v in verdicts) else 'NOT met'}")
        F, P, ptr = batch([4096] * 4, 512)
        seg = lambda **kw: mmf.simtopk_combined_fast_segmented(F, P, LH, LG, K, ptr=ptr, precision="fast", **kw)   # noqa: E731
        want = ct.simtopk_combined(F, P, LH, LG, K, ptr=ptr)
        forced = [1, 2, 4]
        same = [same_bits(seg(col_splits=c), want) for c in forced]
        ts = alternate([lambda c=c: seg(col_splits=c) for c in forced], 2 * reps)
        say(f"4 x 4096  d = 512  column splits, rounds {2 * reps}  same bits as B: {same}")
        for c, t in zip(forced, ts):
            s1 = seg(col_splits=c, profile=True, return_stats=True)[2]
            say(f"   col_splits = {c:2d} (scan_grid {s1['scan_grid']:4d}, scan {s1['scan_ms']:.3f} ms, re-rank {s1['rerank_ms']:.3f} ms, fallback_rows "
                f"{s1['fallback_rows']})   {stat(t)}")
        best = min(range(1, len(forced)), key=lambda i: np.median(ts[i]))
        gain, s, n_spreads = spreads(ts[best], ts[0])
        say(f"automatic splits rule (col_splits = {forced[best]} beats col_splits = 1 by more than 3 spreads of col_splits = 1): one - split = "
            f"{gain:.3f} ms = {n_spreads:.1f} spreads of {s:.3f} ms: {'met' if gain > 3.0 * s else 'NOT met'}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
