"""The 16-bit hypergraph branch against the float32 kernels and against what a caller under autocast had to do before,
whole-call times on one device.

    python scripts/hg16_timing.py [out.txt] [--reps N] [--only CLASS]

    A    the 16-bit call over ready plans: mmf.hypergraph_propagate_16(x16, plan=plan, bias=bias) / mmf.attention_readout_16(x16, gate, plan=plan)
    C    the float32 call on an x.float() prepared ahead: mmf.hypergraph_propagate(x32, plan=plan) (no bias) / mmf.attention_readout(x32, ...)
    D    what a caller has to do without A: x16.float() -> the float32 call -> (+ bias).to(dtype)   (the readout's result is float32: no cast down)
    -fb  forward + backward of each (gradient in x; A and D also in the bias), the output gradient ready in the output's dtype

The four shape classes of scripts/hgconv_timing.py (P1 .. P4) and the first four of scripts/readout_timing.py (R1 .. R4), float16 and
bfloat16.  Protocol: that of scripts/hgpair_timing.py — same process; before anything is timed, A against A bit for bit and max |A - D|
for the propagation (A rounds Y once more than D, so the two differ by design), A against C and grad_x of A against D bit for bit for
the readout; one warm-up of every arm; then `reps` rounds (default 7) that time the arms in turn, each measurement a window of calls of
at least 20 ms between two
device synchronisations; median and min .. max per call.  The minimal traffic of the propagation is x, Y (written and read) and out
once each in their storage type, both id lists, both offset lists and both scale vectors; the gathers ask the caches for one row per
pair and step.  A machine without a GPU fails."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hgpair_timing import HBM_PEAK, WINDOW_MS, cohort_class, knn_class, threshold_class, window      # noqa: E402


def main():
    import multimodal_fusion_amd as mmf
    if not torch.cuda.is_available():
        raise SystemExit("hg16_timing: no GPU: nothing is measured on a CPU")
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    only = args[args.index("--only") + 1] if "--only" in args else None
    out_path = args[0] if args and not args[0].startswith("--") else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                    "profiles", "hg16_timing.txt")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    def measure(arms):
        inner = {}
        for key, fn in arms:
            window(fn, 1)
            inner[key] = max(1, int(np.ceil(WINDOW_MS / max(window(fn, 2), 1e-3))))
        t = {key: [] for key, _ in arms}
        for _ in range(reps):
            for key, fn in arms:
                t[key].append(window(fn, inner[key]))
        return t, {k: float(np.median(v)) for k, v in t.items()}, inner

    def report(t, med, inner, fwd_extra):
        def row(key, label, extra=""):
            say(f"   {key:<6}{label:<58}{med[key]:9.3f} ms ({min(t[key]):.3f} .. {max(t[key]):.3f})   calls per window {inner[key]}{extra}")

        def ratio(a, b):
            slow = a if med[a] >= med[b] else b
            spread, gap = max(t[slow]) - min(t[slow]), abs(med[a] - med[b])
            return f"{a} / {b} = {med[a] / med[b]:.2f} (gap {gap:.3f} ms = {gap / max(spread, 1e-9):.1f} spreads of the slower arm)"

        row("A", "the 16-bit call", fwd_extra)
        row("C", "the float32 call on x.float() prepared ahead", ";  " + ratio("A", "C"))
        row("D", "x16.float() -> float32 call -> cast down", ";  " + ratio("A", "D"))
        row("A-fb", "forward + backward, 16-bit")
        row("C-fb", "forward + backward, float32", ";  " + ratio("A-fb", "C-fb"))
        row("D-fb", "forward + backward through the casts", ";  " + ratio("A-fb", "D-fb"))

    say(f"# scripts/hg16_timing.py --reps {reps} ({torch.cuda.get_device_name(0)}; same process, one warm-up of every arm, then {reps} rounds "
        f"timing the arms in turn; windows of >= {WINDOW_MS:.0f} ms between device synchronisations; per call: median (min .. max))")
    classes = [("P1", "k-NN incidence, N = 262144, k = 5 with self", lambda: knn_class(mmf, 262144, 1), 256),
               ("P2", "cohort of 2048 graphs x 128 nodes, k-NN + KMeans edges", lambda: cohort_class(mmf, 2), 256),
               ("P3", "median-threshold graph, N = 4096", lambda: threshold_class(mmf, 3), 256),
               ("P4", "k-NN incidence, N = 262144, k = 5 with self", lambda: knn_class(mmf, 262144, 1), 16)]
    for tag, name, make, C in classes:
        if only is not None and only != tag:
            continue
        ei, _, N, M = make()
        E = ei.shape[1]
        plan = mmf.incidence_plan(ei, N, M)
        gen = torch.Generator().manual_seed(10 + int(tag[1]))
        x32_0 = torch.randn(N, C, generator=gen).cuda()
        G32_0 = torch.randn(N, C, generator=gen).cuda()
        bias = torch.randn(C, generator=gen).cuda()
        say(f"class {tag}: {name}, C = {C}: N {N}  M {M}  pairs {E}")
        for dt, dname in ((torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
            x16, G16 = x32_0.to(dt), G32_0.to(dt)
            x32, G32 = x16.float(), G16.float()

            def fb_a():
                xd, bd = x16.detach().requires_grad_(), bias.detach().requires_grad_()
                mmf.hypergraph_propagate_16(xd, plan=plan, bias=bd).backward(G16)
                return xd.grad, bd.grad

            def fb_c():
                xd = x32.detach().requires_grad_()
                mmf.hypergraph_propagate(xd, plan=plan).backward(G32)
                return xd.grad

            def fb_d():
                xd, bd = x16.detach().requires_grad_(), bias.detach().requires_grad_()
                (mmf.hypergraph_propagate(xd.float(), plan=plan) + bd).to(dt).backward(G16)
                return xd.grad, bd.grad

            arms = [("A", lambda: mmf.hypergraph_propagate_16(x16, plan=plan, bias=bias)),
                    ("C", lambda: mmf.hypergraph_propagate(x32, plan=plan)),
                    ("D", lambda: (mmf.hypergraph_propagate(x16.float(), plan=plan) + bias).to(dt)),
                    ("A-fb", fb_a), ("C-fb", fb_c), ("D-fb", fb_d)]
            fns = dict(arms)
            a0, a1, d0 = fns["A"](), fns["A"](), fns["D"]()
            torch.cuda.synchronize()
            say(f"  {dname}: A against A bit for bit: {bool(torch.equal(a0, a1))};  max |A - D| = {float((a0.float() - d0.float()).abs().max()):.3e} at max |D| = "
                f"{float(d0.float().abs().max()):.3e} (A rounds Y once more than D)")
            t, med, inner = measure(arms)
            ids = 2 * E * 4 + (N + M + 2) * 8 + (N + M) * 4
            min16, min32 = 2 * (N + M) * C * 2 + ids + C * 4, 2 * (N + M) * C * 4 + ids
            asked16 = 2 * E * C * 2 + (N + M) * C * 2
            r16, r32 = min16 / (med["A"] * 1e-3), min32 / (med["C"] * 1e-3)
            report(t, med, inner, f";  minimal traffic {min16 / 1e6:.1f} MB -> {r16 / 1e12:.3f} TB/s = {100 * r16 / HBM_PEAK:.1f} % of the 8 TB/s HBM peak "
                   f"(C: {min32 / 1e6:.1f} MB -> {r32 / 1e12:.3f} TB/s = {100 * r32 / HBM_PEAK:.1f} %);  the gathers ask for {asked16 / 1e6:.1f} MB -> "
                   f"{asked16 / (med['A'] * 1e-3) / 1e12:.3f} TB/s (C: {2 * asked16 / (med['C'] * 1e-3) / 1e12:.3f} TB/s)")
        del plan, x32_0, G32_0, x16, G16, x32, G32, ei
        torch.cuda.empty_cache()

    for tag, S, n, C in (("R1", 2048, 128, 256), ("R2", 64, 4096, 256), ("R3", 1, 262144, 256), ("R4", 1, 200, 256)):
        if only is not None and only != tag:
            continue
        N = S * n
        rp = mmf.readout_plan(ptr=(torch.arange(S + 1) * n))
        gen = torch.Generator().manual_seed(20 + int(tag[1]))
        x32_0 = torch.randn(N, C, generator=gen).cuda()
        gate = (3 * torch.randn(N, generator=gen)).cuda()
        G = torch.randn(S, C, generator=gen).cuda()
        say(f"class {tag}: readout, {S} segments x {n} rows, C = {C}: N {N}  chunks {rp.num_chunks}")
        for dt, dname in ((torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
            x16 = x32_0.to(dt)
            x32 = x16.float()

            def fb(fn, x, cast):
                def run():
                    xd, gd = x.detach().requires_grad_(), gate.detach().requires_grad_()
                    fn(xd.float() if cast else xd, gd, plan=rp).backward(G)
                    return xd.grad, gd.grad
                return run

            arms = [("A", lambda: mmf.attention_readout_16(x16, gate, plan=rp)),
                    ("C", lambda: mmf.attention_readout(x32, gate, plan=rp)),
                    ("D", lambda: mmf.attention_readout(x16.float(), gate, plan=rp)),
                    ("A-fb", fb(mmf.attention_readout_16, x16, False)), ("C-fb", fb(mmf.attention_readout, x32, False)),
                    ("D-fb", fb(mmf.attention_readout, x16, True))]
            fns = dict(arms)
            a0, c0 = fns["A"](), fns["C"]()
            ga, gd_ = fns["A-fb"](), fns["D-fb"]()
            torch.cuda.synchronize()
            say(f"  {dname}: A against C bit for bit: {bool(torch.equal(a0, c0))};  grad_x of A against D bit for bit: {bool(torch.equal(ga[0], gd_[0]))}")
            t, med, inner = measure(arms)
            min16, min32 = N * C * 2 + N * 8 + S * C * 4, N * C * 4 + N * 8 + S * C * 4
            r16, r32 = min16 / (med["A"] * 1e-3), min32 / (med["C"] * 1e-3)
            report(t, med, inner, f";  minimal traffic {min16 / 1e6:.1f} MB -> {r16 / 1e12:.3f} TB/s = {100 * r16 / HBM_PEAK:.1f} % of the 8 TB/s HBM peak "
                   f"(C: {min32 / 1e6:.1f} MB -> {r32 / 1e12:.3f} TB/s = {100 * r32 / HBM_PEAK:.1f} %)")
        del rp, x32_0, x16, x32, gate, G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
