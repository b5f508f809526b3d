"""The 16-bit combined top-k for two node sets and any k against the exact two-set any-k call, whole-call times.

    python scripts/simtopk_combined_xy_fast_anyk_timing.py [out.txt] [--reps N] [--limit SECONDS] [--only SUBSTRING]

    A    mmf_simtopk_combined_xy_fast_anyk, f16 operands   (combined_topk16_xy_anyk.simtopk_combined_xy_fast_any_k, precision="fast")
    A'   the same call, bf16 operands                       (precision="fast_bf16")
    B    mmf_simtopk_combined_xy_anyk with the same arguments, called directly (the exact scan in passes of 44 - self entries)

Data as in scripts/simtopk_combined_xy_timing.py: unit-norm planted features (12 centres + 0.05 noise), distinct pixel positions
(cells of a grid x 224), dp = 2, lambda_h = 0.5, lambda_g = 2e-7.  Shapes (DESIGN.md §4.19's), each at k = 32 and 64: the row panel
[24576, 32768) of N = 65536 and [98304, 131072) of N = 262144 at d = 512 (views of one array: the library sees a row slice, self
excluded), 16384 queries against 65536 distinct candidates at d = 512 (arrays of their own, ids apart), and the first and the third
at d = 1536.

The protocol of DESIGN.md §4.24: every shape runs in a child process of its own under `timeout -k 10` (--limit, default 280 s); a
child that fails or runs out of time ends the run.  Per shape and k: A and A' are checked bit for bit against B before anything is
timed; every arm is warmed by one call; then `reps` rounds (default 5) time the arms in turn with a device synchronisation around
every timed call; median and min .. max of the whole call.  Per A / A' the passes of one call are listed: yields, queries that took
the exact rescan and the largest ghost count, per pass.  "B - A in spreads of B" is what the routers' rule reads:
"auto" takes A on a shape class only where it exceeds 3 at every measured shape of the class."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LH, LG = 0.5, 2e-7
KS = (32, 64)
# name, rows of the data set, d, queries [q0, q1), candidates [c0, c1), views of one array
SHAPES = [("panel 8192 of 65536", 65536, 512, (24576, 32768), (0, 65536), True),
          ("panel 32768 of 262144", 262144, 512, (98304, 131072), (0, 262144), True),
          ("16384 x 65536 distinct", 81920, 512, (65536, 81920), (0, 65536), False),
          ("panel 8192 of 65536", 65536, 1536, (24576, 32768), (0, 65536), True),
          ("16384 x 65536 distinct", 81920, 1536, (65536, 81920), (0, 65536), False)]


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


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def same_bits(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def passes(info):
    return f"passes {info['passes']}: yields {info['yield']}, queries rescanned {info['exact_rows']}, ghost_max {info['ghost_max']}"


def child(which, reps):
    import multimodal_fusion_amd as mmf
    from multimodal_fusion_amd import _lib, ops
    dev = torch.device("cuda", 0)
    name, total, d, (q0, q1), (c0, c1), views = SHAPES[which]
    F, P = rows(total, d, total % 1000 + d)
    F, P = F.to(dev), P.to(dev)
    if views:
        Fq, Pq, Fc, Pc = F[q0:q1], P[q0:q1], F[c0:c1], P[c0:c1]
    else:
        Fq, Pq, Fc, Pc = F[q0:q1].clone(), P[q0:q1].clone(), F[c0:c1].clone(), P[c0:c1].clone()
        del F, P
    ex = views                       # a panel of one graph drops the row itself; distinct sets have no self
    nq, nc = q1 - q0, c1 - c0
    m = mmf.combined_topk16_xy_anyk

    def exact_entry(k):
        idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
        val = torch.empty((nq, k), dtype=torch.float32, device=dev)
        opts = _lib.SimtopkOpts(_lib.PRECISIONS["exact"], 0, 0, _lib.QUERY_ORDERS["off"], None)
        ops._call("mmf_simtopk_combined_xy_anyk", dev, ops._p(Fq), ops._p(Pq), nq, ops._p(Fc), ops._p(Pc), nc, d, 2, LH, LG, k, int(ex), q0, c0,
                  ops._p(idx), ops._p(val), ctypes.byref(opts), None)
        return idx, val

    met = {}
    for k in KS:
        A = lambda prec="fast", **kw: m.simtopk_combined_xy_fast_any_k(Fq, Pq, Fc, Pc, LH, LG, k, exclude_self=ex, row_offset=q0, col_offset=c0,   # noqa: E731
                                                                       precision=prec, **kw)
        B = lambda: exact_entry(k)   # noqa: E731
        want = B()
        a, a2 = A(return_info=True), A("fast_bf16", return_info=True)
        ok = same_bits(a[:2], want) and same_bits(a2[:2], want)
        print(f"{name}  d = {d}  k = {k}  {nq} queries x {nc} candidates{' (row slice, self excluded)' if views else ''}   A and A' have B's bits: {ok}", flush=True)
        del want
        arms = [A, lambda: A("fast_bf16"), B]
        for fn in arms:
            once(fn)
        ts = [[] for _ in arms]
        for _ in range(reps):
            for t, fn in zip(ts, arms):
                t.append(once(fn)[0])
        med = [float(np.median(t)) for t in ts]
        sb = max(ts[2]) - min(ts[2])
        inf = float("inf")
        print(f"   A   f16   {stat(ts[0])}   {passes(a[2])}")
        print(f"   A'  bf16  {stat(ts[1])}   {passes(a2[2])}")
        print(f"   B   exact {stat(ts[2])}   spread of B {sb:.3f} ms;  A / B = {med[0] / med[2]:.3f}, B - A = {(med[2] - med[0]) / sb if sb > 0 else inf:+.1f} spreads of B;  "
              f"A' / B = {med[1] / med[2]:.3f}, B - A' = {(med[2] - med[1]) / sb if sb > 0 else inf:+.1f} spreads of B", flush=True)
        met[k] = (ok, med[2] - med[0] > 3.0 * sb, med[2] - med[1] > 3.0 * sb)
        del a, a2
    print(f"verdict {name} d = {d}: " + "; ".join(f"k = {k}: bit for bit {o}, A beats B by more than 3 of B's spreads: {'met' if x else 'NOT met'}, A': "
                                                  f"{'met' if y else 'NOT met'}" for k, (o, x, y) in met.items()))
    if which == len(SHAPES) - 1:
        print(f"device: {torch.cuda.get_device_name(0)}")
    return 0 if all(o for o, _, _ in met.values()) else 1


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    if "--child" in args:
        return child(int(args[args.index("--child") + 1]), reps)
    out_path = next((v for v in args if v.endswith(".txt")), None)
    limit = int(args[args.index("--limit") + 1]) if "--limit" in args else 280
    only = args[args.index("--only") + 1] if "--only" in args else ""
    lines = [f"mmf_simtopk_combined_xy_fast_anyk  dp = 2  lambda_h = {LH}  lambda_g = {LG}  rounds {reps}  whole-call times, median (min .. max)"]
    print(lines[0], flush=True)
    for which, shape in enumerate(SHAPES):
        if only not in f"{shape[0]} d = {shape[2]}":
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(which), "--reps", str(reps)],
                           capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:                            # nothing more is started on the GPU behind a failed step
            print(r.stderr[-4000:], flush=True)
            lines.append(f"{shape[0]} d = {shape[2]}: the step ended with status {r.returncode}; the run stops here")
            break
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if lines and not lines[-1].endswith("the run stops here") else 1


if __name__ == "__main__":
    sys.exit(main())
