"""The 16-bit combined top-k for any k against the exact any-k call, whole-call times.

    python scripts/simtopk_combined_fast_anyk_timing.py [out.txt] [--reps N] [--only SUBSTRING]

    A    mmf_simtopk_combined_fast_anyk, f16 operands   (combined_topk16_anyk.simtopk_combined_fast_any_k, precision="fast")
    A'   the same call, bf16 operands                    (precision="fast_bf16")
    B    mmf_simtopk_combined_anyk with the same k, called directly (the exact scan in passes of 44 - self entries)

Data as in scripts/simtopk_combined_fast_timing.py / _segmented_timing.py: unit-norm planted features (12 centres + 0.05 noise),
distinct pixel positions (cells of a grid x 224), dp = 2, lambda_h = 0.5, lambda_g = 2e-7, self excluded.  Shapes: one graph of
N = 16384 / 65536 / 262144 rows at d = 512 and N = 65536 at d = 1536 with k = 32 and 64; batches of 64 x 4096 and 16 x 16384 rows at
d = 512 and 1536, and 2048 x 128 rows at d = 512, with k = 32.

Everything runs in one process.  Per shape and k: A and A' are checked bit for bit against B before anything is timed; every arm
is warmed by one call; then `reps` rounds (3 at 262144 rows of one graph) time the arms in turn with a device synchronisation
around every timed call; median and min .. max of the whole call.  Per A / A' the passes of one call are listed: yields, rows that
took the exact rescan and the largest ghost count, per pass.  "B - A in spreads of B" is what the router's rule
reads: "auto" takes A on a shape class only where it exceeds 3 at every measured size of the class."""
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
LH, LG = 0.5, 2e-7
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
    ptr = None if len(sizes) == 1 else torch.tensor([0] + np.cumsum(sizes).tolist(), dtype=torch.int64)
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
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def exact_entry(F, P, k, ptr):
    """mmf_simtopk_combined_anyk itself: (idx, val)."""
    n, d = F.shape
    idx = torch.empty((n, k), dtype=torch.int64, device=dev)
    val = torch.empty((n, k), dtype=torch.float32, device=dev)
    opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], 0, 0, _lib.QUERY_ORDERS["off"], None)
    ops._call("mmf_simtopk_combined_anyk", dev, ops._p(F), ops._p(P), n, d, P.shape[1], LH, LG, k, 1, ops._hp(ptr),
              0 if ptr is None else ptr.numel() - 1, ops._p(idx), ops._p(val), ctypes.byref(opts), None)
    return idx, val


def passes(info):
    return f"passes {info['passes']}: yields {info['yield']}, rows rescanned {info['exact_rows']}, ghost_max {info['ghost_max']}"


def shape(name, sizes, d, ks, reps, table):
    F, P, ptr = batch(sizes, d)
    n = F.shape[0]
    ak16 = mmf.combined_topk16_anyk
    for k in ks:
        A = lambda prec="fast", **kw: ak16.simtopk_combined_fast_any_k(F, P, LH, LG, k, ptr=ptr, precision=prec, **kw)   # noqa: E731
        B = lambda: exact_entry(F, P, k, ptr)   # noqa: E731
        want = B()
        a, a2 = A(return_info=True), A("fast_bf16", return_info=True)
        ok = same_bits(a[:2], want) and same_bits(a2[:2], want)
        say(f"{name}  d = {d}  k = {k}  {len(sizes)} segment(s), {n} rows   A and A' have B's bits: {ok}")
        del want
        ts = alternate([A, lambda: A("fast_bf16"), B], reps)
        med = [float(np.median(t)) for t in ts]
        sb = max(ts[2]) - min(ts[2])
        say(f"   A   f16   {stat(ts[0])}   {passes(a[2])}")
        say(f"   A'  bf16  {stat(ts[1])}   {passes(a2[2])}")
        say(f"   B   exact {stat(ts[2])}   spread of B {sb:.3f} ms;  A / B = {med[0] / med[2]:.3f}, B - A = {(med[2] - med[0]) / sb if sb > 0 else float('inf'):+.1f} spreads of B;  "
            f"A' / B = {med[1] / med[2]:.3f}, B - A' = {(med[2] - med[1]) / sb if sb > 0 else float('inf'):+.1f} spreads of B")
        table.append((name, d, k, ok, med[0], med[1], med[2], sb))
        del a, a2
    del F, P
    torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    only = args[args.index("--only") + 1] if "--only" in args else ""
    say(f"mmf_simtopk_combined_fast_anyk  dp = 2  lambda_h = {LH}  lambda_g = {LG}  self excluded  rounds {reps} (3 at 262144 rows of one graph)  "
        f"whole-call times, median (min .. max)")
    shapes = [("one graph N = 16384", [16384], 512, (32, 64), reps), ("one graph N = 65536", [65536], 512, (32, 64), reps),
              ("one graph N = 262144", [262144], 512, (32, 64), min(reps, 3)), ("one graph N = 65536", [65536], 1536, (32, 64), reps),
              ("batch 64 x 4096", [4096] * 64, 512, (32,), reps), ("batch 16 x 16384", [16384] * 16, 512, (32,), reps),
              ("batch 64 x 4096", [4096] * 64, 1536, (32,), reps), ("batch 16 x 16384", [16384] * 16, 1536, (32,), reps),
              ("batch 2048 x 128", [128] * 2048, 512, (32,), reps)]
    table = []
    for name, sizes, d, ks, r in shapes:
        if only in f"{name} d = {d}":
            shape(name, sizes, d, ks, r, table)
    say("")
    say("shape, d, k: same bits | A / B | (B - A) / spread of B | A' / B | (B - A') / spread of B")
    for name, d, k, ok, a, a2, b, sb in table:
        say(f"  {name:22s} d = {d:4d} k = {k:2d}: {str(ok):5s} | {a / b:5.3f} | {(b - a) / sb if sb > 0 else float('inf'):+8.1f} | {a2 / b:5.3f} | {(b - a2) / sb if sb > 0 else float('inf'):+8.1f}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
