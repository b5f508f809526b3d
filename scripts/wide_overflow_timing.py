"""The wide 16-bit scan's overflow lists on near-duplicate rows: ops.simtopk, cosine, k = 5, d = 1536.

    python scripts/wide_overflow_timing.py [out.txt] [--reps N] [--parent-lib PATH/libmmf_hg.so]

    A    precision="fast"                          the overflow lists on (the default)
    A0   precision="fast", MMF_WIDE_SINK=0         the kernels without them: a crowded row is flagged and rescanned exactly
    B    precision="exact"                         the f32 matrix-core scan
    P    A0's call through the parent commit's library (--parent-lib: built into a scratch directory; left out without it)

Shapes, at N = 16384 and 65536:
    (i)  near-duplicate clusters as bench.py --data clustered builds them (a unit centre + 0.03 / sqrt(d) noise, normalised), with
         N / 128 centres: clusters of about 128 rows
    (ii) the planted clusters of scripts/wide_scan_timing.py (32 rows, graded 0.95 .. 0.60): no row is crowded

The method is scripts/wide_scan_timing.py's: one process, every shape warmed by one call of each arm, then `reps` rounds time the
arms in turn with a device synchronisation around every timed call; median and min .. max of the whole call.  The bits of A, A0
and P are checked against B before anything is timed.  fallback_rows, candidates per row and the scan / re-rank / rescan times
come from the call's own stats (profile=True, one separate call per arm).  The verdict lines apply the three-spreads rule
(DESIGN.md §4.1): the lists stay on by default only if A beats A0 by more than three of A0's spreads on (i) at both N, and on (ii)
A - P (A - A0 without P) has to lie within three of P's spreads."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402
from multimodal_fusion_amd import _lib  # noqa: E402

dev = torch.device("cuda", 0)
lines = []
K, D, SIGMA = 5, 1536, 0.03


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def near_duplicate_rows(n, d, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = unit(torch.randn(n // 128, d, generator=g, device=dev))
    assign = torch.randint(0, n // 128, (n,), generator=g, device=dev)
    return unit(centres[assign] + (SIGMA / d ** 0.5) * torch.randn(n, d, generator=g, device=dev)).contiguous()


def planted_rows(n, d, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    per = 32
    centres = unit(torch.randn(n // per, 1, d, generator=g, device=dev))
    a = torch.linspace(0.95, 0.60, per, device=dev)[None, :, None]
    X = a * centres + torch.sqrt(1.0 - a * a) * unit(torch.randn(n // per, per, d, generator=g, device=dev))
    return unit(X).reshape(n, d).contiguous()


def stat(ts):
    return f"{np.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


class Arm:
    """One arm: the library it calls through, the switch, the precision."""

    def __init__(self, name, library, sink, precision):
        self.name, self.library, self.sink, self.precision = name, library, sink, precision

    def __call__(self, X, **kw):
        _lib._lib = self.library
        if self.sink is None:
            os.environ.pop("MMF_WIDE_SINK", None)
        else:
            os.environ["MMF_WIDE_SINK"] = self.sink
        try:
            return mmf.ops.simtopk(X, metric="cosine", k=K, precision=self.precision, **kw)
        finally:
            os.environ.pop("MMF_WIDE_SINK", None)


def load_parent(path):
    """A second handle on another build of the library, bound like the first (the parent has the same ABI)."""
    own = _lib.lib()
    so = _lib.SO_PATH
    _lib._lib, _lib.SO_PATH = None, path
    try:
        parent = _lib.lib()
    finally:
        _lib._lib, _lib.SO_PATH = own, so
    return parent


def events(arm, X):
    st = arm(X, profile=True, return_stats=True)[2]
    return (f"events: scan {st['scan_ms']:.3f} ms, re-rank {st['rerank_ms']:.3f} ms, rescan {st['fallback_ms']:.3f} ms; fallback_rows "
            f"{st['fallback_rows']}, candidates per row {st['candidates'] / X.shape[0]:.1f}, col_splits {st['col_splits']}")


def main():
    args = sys.argv[1:]
    out_path = next((v for v in args if v.endswith(".txt")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    own = _lib.lib()
    arms = [Arm("A ", own, None, "fast"), Arm("A0", own, "0", "fast"), Arm("B ", own, None, "exact")]
    if "--parent-lib" in args:
        arms.append(Arm("P ", load_parent(os.path.abspath(args[args.index("--parent-lib") + 1])), "0", "fast"))
    say(f"cosine  k = {K}  d = {D}  rounds {reps}  whole-call times, median (min .. max)")
    on_ok, flat_ok = [], []
    for shape, make in (("(i) near-duplicate clusters of ~128 rows", near_duplicate_rows), ("(ii) planted clusters of 32 rows", planted_rows)):
        for n in (16384, 65536):
            X = make(n, D, n + D)
            outs = [arm(X) for arm in arms]                                  # the warm-up, and the bits
            ref = outs[2]
            same = all(torch.equal(o[0], ref[0]) and torch.equal(o[1], ref[1]) for o in outs)
            del outs, ref
            ts = [[] for _ in arms]
            for _ in range(reps):
                for t, arm in zip(ts, arms):
                    t.append(once(lambda: arm(X))[0])
            med = [float(np.median(t)) for t in ts]
            spread = [max(t) - min(t) for t in ts]
            say(f"{shape}  N = {n}  same bits as exact: {same}")
            for arm, t, s in zip(arms, ts, spread):
                say(f"   {arm.name} {stat(t)}   spread {s:.3f} ms")
            for arm in arms:
                say(f"   {arm.name} {events(arm, X)}")
            base = 3 if len(arms) == 4 else 1                                # P, or A0 in its place
            if shape.startswith("(i)"):
                say(f"   A0 - A = {med[1] - med[0]:.3f} ms = {(med[1] - med[0]) / spread[1] if spread[1] > 0 else float('inf'):.1f} spreads of A0;  "
                    f"B / A = {med[2] / med[0]:.2f}x  B / A0 = {med[2] / med[1]:.2f}x"
                    + (f";  A0 - P = {med[1] - med[3]:.3f} ms ({spread[3]:.3f} ms spread of P)" if len(arms) == 4 else ""))
                on_ok.append(same and med[1] - med[0] > 3.0 * spread[1])
            else:
                say(f"   A - {arms[base].name.strip()} = {med[0] - med[base]:.3f} ms against 3 spreads = {3.0 * spread[base]:.3f} ms;  B / A = {med[2] / med[0]:.2f}x")
                flat_ok.append(same and med[0] - med[base] <= 3.0 * spread[base])
            del X
            torch.cuda.empty_cache()
    say(f"default-on rule (A beats A0 by more than 3 spreads of A0 on (i) at both N): {'met' if len(on_ok) == 2 and all(on_ok) else 'NOT met'}")
    say(f"uncrowded rule (A - {'P' if len(arms) == 4 else 'A0'} within 3 spreads on (ii) at both N): {'met' if len(flat_ok) == 2 and all(flat_ok) else 'NOT met'}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
