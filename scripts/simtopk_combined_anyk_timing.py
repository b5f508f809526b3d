"""The combined top-k for any k: the new entry against the existing ones in their range, and what a pass costs.

    python scripts/simtopk_combined_anyk_timing.py [out.txt] [--reps N]

    A   mmf_simtopk_combined_anyk, called directly (combined_topk_anyk.simtopk_combined_any_k routes k + self <= 44 to B itself)
    B   combined_topk.simtopk_combined (one graph) / segmented_exact.simtopk_combined_exact (a batch): k + self <= 44 only
    D   ops.sim_dense_combined + diagonal fill + torch.topk (one graph at N = 16384, where the 1 GiB matrix fits; for a batch a
        Python loop of that per segment)

Shapes: d = 512, dp = 2; one graph of N = 16384 and 65536 rows; batches of 64 x 4096 and 2048 x 128 rows.  k = 43 (one pass: A
and B run the same launches, so A must not be slower than B by more than three of B's spreads), then k = 64 (two
passes) and k = 128 (three): the time per pass against the k = 43 call of the same arm.

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max of the whole call.  Before anything is timed every result
is checked bit for bit against the other arm where one exists: A against B at k = 43, and the first 43 columns of A at k = 64 /
128 against B's k = 43."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402
from multimodal_fusion_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
LH, LG = 0.7, 0.3
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


def same_bits(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def entry(F, P, k, ptr=None, profile=False):
    """mmf_simtopk_combined_anyk itself: (idx, val, stats)."""
    n, d = F.shape
    idx = torch.empty((n, k), dtype=torch.int64, device=dev)
    val = torch.empty((n, k), dtype=torch.float32, device=dev)
    stats = _lib.SimtopkStats()
    opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], int(profile), 0, _lib.QUERY_ORDERS["off"], None)
    ops._call("mmf_simtopk_combined_anyk", dev, ops._p(F), ops._p(P), n, d, P.shape[1], LH, LG, k, 1, ops._hp(ptr),
              0 if ptr is None else ptr.numel() - 1, ops._p(idx), ops._p(val), ctypes.byref(opts), ctypes.byref(stats))
    return idx, val, stats.as_dict()


def dense_topk(F, P, k):
    K = ops.sim_dense_combined(F, P, LH, LG)
    K.fill_diagonal_(float("-inf"))
    v, i = torch.topk(K, k, dim=1)
    return i, v


def dense_topk_loop(F, P, ptr, k):
    out = [dense_topk(F[a:b], P[a:b], k) for a, b in zip(ptr[:-1], ptr[1:])]
    return torch.cat([o[0] + a for o, a in zip(out, ptr[:-1])]), torch.cat([o[1] for o in out])


def events(st):
    return f"events: prep {st['prep_ms']:.3f}, scan {st['scan_ms']:.3f}, re-rank {st['rerank_ms']:.3f} ms; col_splits {st['col_splits']}, scan_grid {st['scan_grid']}"


def shape(name, sizes, reps, verdicts, dense):
    n = int(sum(sizes))
    one = len(sizes) == 1
    ptr_l = [0] + np.cumsum(sizes).tolist()
    ptr = None if one else torch.tensor(ptr_l, dtype=torch.int64)
    F = rows(n, 512, n + 512)
    P = torch.rand(n, 2, generator=torch.Generator(device=dev).manual_seed(5), device=dev) * 4.0
    A = lambda k, **kw: entry(F, P, k, ptr, **kw)   # noqa: E731
    if one:
        B = lambda: mmf.combined_topk.simtopk_combined(F, P, LH, LG, 43)   # noqa: E731
    else:
        B = lambda: mmf.segmented_exact.simtopk_combined_exact(F, P, LH, LG, 43, ptr=ptr)   # noqa: E731
    # bits before anything is timed
    b43 = B()
    same = same_bits(A(43)[:2], b43)
    prefix = all(same_bits((o[0][:, :43].contiguous(), o[1][:, :43].contiguous()), b43) for o in (A(64), A(128)))
    say(f"{name}  d = 512  dp = 2  {len(sizes)} segment(s), {n} rows   A(k = 43) has B's bits: {same}; the first 43 columns of A(64), A(128) are B's: {prefix}")
    # three alternations of their own: A against B alone, the passes, the dense arms.  In one alternation of all six arms the
    # arm behind the host-bound Python loop of D (it was A k = 43) measured 7.20 ms at 2048 x 128 against B's 6.37; alone with B
    # it is 6.15 against 6.18
    ts = alternate([lambda: A(43), B], reps) + alternate([lambda: A(64), lambda: A(128)], reps)
    if dense:
        D = (lambda k: dense_topk(F, P, k)) if one else (lambda k: dense_topk_loop(F, P, ptr_l, k))
        ts += alternate([lambda: D(64), lambda: D(128)], reps)
    med = [float(np.median(t)) for t in ts]
    sb = max(ts[1]) - min(ts[1])
    slower = med[0] - med[1]
    say(f"   A  k = 43   {stat(ts[0])}   {events(A(43, profile=True)[2])}")
    say(f"   B  k = 43   {stat(ts[1])}   spread of B {sb:.3f} ms; A - B = {slower:+.3f} ms = {slower / sb if sb > 0 else float('inf'):+.1f} spreads")
    for j, (k, passes) in ((2, (64, 2)), (3, (128, 3))):
        say(f"   A  k = {k:<3d}  {stat(ts[j])}   {passes} passes: {med[j] / passes:.3f} ms per pass = {med[j] / passes / med[0]:.2f} x the k = 43 call   "
            f"{events(A(k, profile=True)[2])}")
    if dense:
        for j, k, a in ((4, 64, 2), (5, 128, 3)):
            say(f"   D  k = {k:<3d}  {stat(ts[j])}   dense + topk{'' if one else ', Python loop'}; D / A {med[j] / med[a]:.2f}x")
    verdicts.append((name, bool(same and prefix and slower <= 3.0 * sb)))
    del F, P
    torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    say(f"combined key, lambda_h = {LH}, lambda_g = {LG}, exclude_self; rounds {reps}; whole-call times, median (min .. max)")
    v = []
    shape("one graph N = 16384", [16384], reps, v, dense=True)
    shape("one graph N = 65536", [65536], reps, v, dense=False)
    shape("batch 64 x 4096", [4096] * 64, reps, v, dense=True)
    shape("batch 2048 x 128", [128] * 2048, reps, v, dense=True)
    for name, ok in v:
        say(f"A (k = 43) not slower than B by more than 3 of B's spreads, same bits: {'met    ' if ok else 'NOT met'}  {name}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
