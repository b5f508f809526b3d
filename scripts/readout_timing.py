"""The attention readout against the same operator composed in torch, whole-call times on one device.

    python scripts/readout_timing.py [out.txt] [--reps N] [--only CLASS]

    A    mmf.attention_readout(x, gate, plan=plan) over a ready plan (mmf_attention_readout: five enqueues), and with its backward
    A'   mmf.readout_plan(ptr=ptr): the plan build (host chunk table, two uploads out of pinned memory)
    B    the same operator as torch_geometric's GlobalAttention computes it, written in torch on the same device with the segment id
         of every row ready: m = scatter_reduce amax; e = exp(gate - m[seg]); Z = zeros.index_add_(0, seg, e); alpha = e / Z[seg];
         out = zeros.index_add_(0, seg, alpha * x).  Float atomics: its bits change from run to run.  It is the only baseline there
         is (torch_geometric itself is not installable next to this library), and it is not the code under test.

Shape classes, C = 256 unless said otherwise:
    1  2048 segments of 128 rows          2  64 segments of 4096 rows          3  one segment of 262144 rows (4096 chunk partials
    chained by one thread per column)     4  one segment of 200 rows (the reference's single slide)          5  class 1 at C = 16

Protocol: same process; A against B to a tolerance and A against A bit for bit before anything is timed; one warm-up call of every arm;
then `reps` rounds (default 7) that time the arms in turn, each measurement a window of calls of at least 20 ms between two device
synchronisations; median and min .. max per call.  Forward, then forward + backward (gradients for x and gate).  For A's forward
also the bytes of the minimal traffic (x and gate read once, out and alpha written once) over the median time, as a share of the
8 TB/s HBM peak.  A machine without a GPU fails."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
WINDOW_MS = 20.0


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def torch_arm(x, gate, seg, S):
    m = torch.full((S,), float("-inf"), dtype=gate.dtype, device=gate.device).scatter_reduce(0, seg, gate, "amax", include_self=True)
    e = torch.exp(gate - m[seg])
    Z = torch.zeros((S,), dtype=gate.dtype, device=gate.device).index_add_(0, seg, e)
    alpha = e / Z[seg]
    return torch.zeros((S, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, seg, alpha.unsqueeze(1) * x)


def main():
    import multimodal_fusion_amd as mmf
    if not torch.cuda.is_available():
        raise SystemExit("readout_timing: no GPU: nothing is measured on a CPU")
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    only = args[args.index("--only") + 1] if "--only" in args else None
    out_path = args[0] if args and not args[0].startswith("--") else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                    "profiles", "readout_timing.txt")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"# scripts/readout_timing.py --reps {reps} ({torch.cuda.get_device_name(0)}; same process, one warm-up of every arm, then {reps} rounds "
        f"timing the arms in turn; windows of >= {WINDOW_MS:.0f} ms between device synchronisations; per call: median (min .. max))")
    classes = [("1", 2048, 128, 256), ("2", 64, 4096, 256), ("3", 1, 262144, 256), ("4", 1, 200, 256), ("5", 2048, 128, 16)]
    for tag, S, n, C in classes:
        if only is not None and only != tag:
            continue
        N = S * n
        g = torch.Generator().manual_seed(int(tag))
        x = torch.randn(N, C, generator=g).cuda()
        gate = (3.0 * torch.randn(N, generator=g)).cuda()
        G = torch.randn(S, C, generator=g).cuda()
        ptr = torch.arange(S + 1, dtype=torch.int64) * n
        seg = torch.repeat_interleave(torch.arange(S), n).cuda()
        plan = mmf.readout_plan(ptr=ptr)
        xg, gg = x.clone().requires_grad_(), gate.clone().requires_grad_()

        def both(fn):
            xg.grad = gg.grad = None
            fn(xg, gg).backward(G)

        run_a = lambda: mmf.attention_readout(x, gate, plan=plan)
        run_p = lambda: mmf.readout_plan(ptr=ptr)
        run_b = lambda: torch_arm(x, gate, seg, S)
        run_ab = lambda: both(lambda a, b: mmf.attention_readout(a, b, plan=plan))
        run_bb = lambda: both(lambda a, b: torch_arm(a, b, seg, S))
        a0, a1, b0 = run_a(), run_a(), run_b()
        run_ab()
        gxa, gga = xg.grad.clone(), gg.grad.clone()
        run_bb()
        torch.cuda.synchronize()
        say(f"class {tag}: {S} segments x {n} rows, C = {C}: N {N}  chunks {plan.num_chunks}")
        say(f"   A against A bit for bit: {bool(torch.equal(a0, a1))};  max |A - B| = {float((a0 - b0).abs().max()):.3e} at max |B| = {float(b0.abs().max()):.3e};"
            f"  grad_x max |A - B| = {float((gxa - xg.grad).abs().max()):.3e}, grad_gate {float((gga - gg.grad).abs().max()):.3e}"
            f"  (B against B bit for bit: {bool(torch.equal(b0, run_b()))})")
        arms = (("A", run_a), ("A'", run_p), ("B", run_b), ("A+bwd", run_ab), ("B+bwd", run_bb))
        inner = {}
        for key, fn in arms:
            window(fn, 1)
            inner[key] = max(1, int(np.ceil(WINDOW_MS / max(window(fn, 2), 1e-3))))
        t = {key: [] for key, _ in arms}
        for _ in range(reps):
            for key, fn in arms:
                t[key].append(window(fn, inner[key]))
        med = {k: float(np.median(v)) for k, v in t.items()}
        minimal = (N * C + N + S * C + N) * 4
        rate = minimal / (med["A"] * 1e-3)

        def row(key, name, extra=""):
            say(f"   {key:6s} {name:34s} {med[key]:9.4f} ms ({min(t[key]):.4f} .. {max(t[key]):.4f})   calls per window {inner[key]}{extra}")

        row("A", "readout, ready plan", f";  minimal traffic {minimal / 1e6:.1f} MB -> {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
        AP = "A'"
        row(AP, "plan build", f";  = {med[AP] / med['A']:.1f} readouts")
        row("B", "composed in torch", f";  B / A = {med['B'] / med['A']:.2f}, B - A = {(med['B'] - med['A']) / max(max(t['B']) - min(t['B']), 1e-9):+.1f} spreads of B")
        row("A+bwd", "readout forward + backward")
        row("B+bwd", "torch forward + backward", f";  B / A = {med['B+bwd'] / med['A+bwd']:.2f}")
        del plan, x, gate, G, seg, xg, gg, a0, a1, b0, gxa, gga
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
