"""The two-set top-k of the combined similarity (combined_topk_xy, mmf_simtopk_combined_xy): a row panel of one
graph against all of it, and queries against distinct candidates.  d = 512 and 1536, dp = 2, k = 5, lambda_h = 0.5, lambda_g = 2e-7;
unit-norm planted features (12 Gaussian centres + 0.05 noise, rows L2-normalised) with distinct pixel positions (cells of a grid
of side 4 ceil(sqrt(N)) x 224); whole-call times.

    python scripts/simtopk_combined_xy_timing.py [out.txt] [--reps N] [--skip-large]

    (a) one eighth of N = 65536 (rows [3N/8, N/2) against all N): simtopk_combined_rows exact / f16 / bf16, against one eighth of
        the full self call's time (combined_topk.simtopk_combined / combined_topk16.simtopk_combined_fast) in the same process
    (b) the same at N = 262144 (d = 512 only)
    (c) 16384 queries against 65536 distinct candidates: simtopk_combined_xy exact / f16 / bf16

Everything runs in one process.  Every shape is warmed by one call of each arm, then `reps` rounds time the arms in turn with a
device synchronisation around every timed call; median and min .. max.  The panels are checked against the rows of the self call
bit for bit, the 16-bit arms of (c) against its exact arm, before anything is timed.  The stage times come from the call's event
timers (profile=True, one separate call).

The AUTO rule: MMF_PREC_AUTO of this entry may take the 16-bit scan only for a (d, k) range where the whole call
beat this entry's own exact arm by more than three times that arm's spread at every measured shape."""
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402

ct = import_module("multimodal_fusion_amd.combined_topk")
ct16 = import_module("multimodal_fusion_amd.combined_topk16")
xy = import_module("multimodal_fusion_amd.combined_topk_xy")
dev = torch.device("cuda", 0)
lines = []
K, LH, LG = 5, 0.5, 2e-7


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
    return F.contiguous().to(dev), P.contiguous().to(dev)


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


def release():
    mmf._lib.check(mmf._lib.lib().mmf_release_workspaces(), "mmf_release_workspaces")
    torch.cuda.empty_cache()


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def events(fn, nq):
    st = fn(return_stats=True, profile=True)[2]
    return (f"events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms, re-rank {st['rerank_ms']:.3f} ms, rescan {st['fallback_ms']:.3f} ms; "
            f"grid {st['scan_grid']}, col_splits {st['col_splits']}, candidates per query {st['candidates'] / nq:.1f}, "
            f"fallback_rows {st['fallback_rows']}, precision_used {st['precision_used']}")


def verdict(name, ta, te):
    spread = max(te) - min(te)
    gain = np.median(te) - np.median(ta)
    return (f"   {name:<28}{stat(ta)}   exact / this {np.median(te) / np.median(ta):.2f}x   exact - this = {gain:.3f} ms = "
            f"{gain / spread if spread > 0 else float('inf'):.0f} x the exact arm's spread")


def panel(n, D, reps):
    F, P = rows(n, D, n // 1024 + D)
    lo, hi = 3 * n // 8, n // 2
    say(f"rows [{lo}, {hi}) of N = {n} against all N, d = {D}")
    full = {"exact": lambda **kw: ct.simtopk_combined(F, P, LH, LG, K, **kw),
            "fast": lambda **kw: ct16.simtopk_combined_fast(F, P, LH, LG, K, precision="fast", **kw),
            "fast_bf16": lambda **kw: ct16.simtopk_combined_fast(F, P, LH, LG, K, precision="fast_bf16", **kw)}
    part = {p: (lambda p=p, **kw: xy.simtopk_combined_rows(F, P, lo, hi, LH, LG, K, precision=p, **kw)) for p in full}
    for p in full:
        want, got = full[p](), part[p]()
        assert same(got, (want[0][lo:hi], want[1][lo:hi])), f"{p}: the panel differs from the rows of the self call"
        del want, got
    r = reps if n < 262144 else max(3, reps // 2)
    te, ta, ta2 = alternate([part["exact"], part["fast"], part["fast_bf16"]], r)
    tfe, tfa = alternate([full["exact"], full["fast"]], max(3, r // 2))
    spread = max(te) - min(te)
    say(f"   panel exact                 {stat(te)}   spread {spread:.3f} ms ({spread / np.median(te):.4f})   full exact call / 8 = "
        f"{np.median(tfe) / 8:.3f} ms (full {np.median(tfe):.3f})")
    say(verdict("panel fast (f16)", ta, te) + f"   full f16 call / 8 = {np.median(tfa) / 8:.3f} ms (full {np.median(tfa):.3f})")
    say(verdict("panel fast_bf16", ta2, te))
    for p in ("exact", "fast", "fast_bf16"):
        say(f"   {p:<10} {events(part[p], hi - lo)}")
    del F, P
    release()


def two_sets(nq, nc, D, reps):
    F, P = rows(nq + nc, D, 77)
    Fq, Pq, Fc, Pc = F[:nq].clone(), P[:nq].clone(), F[nq:].clone(), P[nq:].clone()
    del F, P
    say(f"{nq} queries against {nc} distinct candidates, d = {D}")
    arm = {p: (lambda p=p, **kw: xy.simtopk_combined_xy(Fq, Pq, Fc, Pc, LH, LG, K, precision=p, **kw)) for p in ("exact", "fast", "fast_bf16")}
    want = arm["exact"]()
    for p in ("fast", "fast_bf16"):
        assert same(arm[p](), want), f"{p} differs from the exact arm"
    del want
    te, ta, ta2 = alternate([arm["exact"], arm["fast"], arm["fast_bf16"]], reps)
    spread = max(te) - min(te)
    say(f"   exact                       {stat(te)}   spread {spread:.3f} ms ({spread / np.median(te):.4f})")
    say(verdict("fast (f16)", ta, te))
    say(verdict("fast_bf16", ta2, te))
    for p in arm:
        say(f"   {p:<10} {events(arm[p], nq)}")
    release()


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    say(f"dp 2  k {K}  lambda_h {LH}  lambda_g {LG}  rounds {reps}  whole-call times, median (min .. max)")
    for D in (512, 1536):
        say(f"(a) d = {D}")
        panel(65536, D, reps)
        if D == 512 and "--skip-large" not in args:
            say(f"(b) d = {D}")
            panel(262144, D, reps)
        say(f"(c) d = {D}")
        two_sets(16384, 65536, D, reps)
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
