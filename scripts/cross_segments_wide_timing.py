"""The wide 16-bit cross-segment top-k against the exact entry it reproduces and against the plain wide 16-bit scan.

    python scripts/cross_segments_wide_timing.py [out.txt] [--reps N] [--limit SECONDS]

    A   cross_segments_wide.simtopk_cross_segments_wide, f16 operands   one table-driven launch of the wide scan with the per-row mask + one re-rank
    A'  the same call with bf16 operands
    B   cross_segments.simtopk_cross_segments                            the exact entry: unchanged from the parent commit, so the parent's time
    C   ops.simtopk(X, precision="fast")                                 the plain wide scan on the same rows: a DIFFERENT answer (a row's lists fill
                                                                         with its own slide) over the same pairs plus the block diagonal

Shapes (f32 planted rows cut into segments, cosine, k = 5): 64 x 1024 at d = 1536 (§4.24's fifth shape), 512 x 128 at d = 1536, 250 ragged
segments of 100 .. 300 rows at d = 1536, 16 x 4096 at d = 2560, and one small call — 8 x 1024 at d = 1536 — where forced col_splits
1, 2, 4, 8, 16 are timed beside the automatic rule (arms S1 .. S16).

Every shape runs in a child process of its own under `timeout -k 10` (--limit, default 240 s); a child that fails or runs out of time
ends the run.  Inside a child: every arm is warmed by one call, A and A' are checked bit for bit against B (indices equal, values
bitwise equal), then `reps` rounds time the arms in turn with a device synchronisation around every timed call; median and
min .. max of the whole call.  Reported: B / A, (B - A) in spreads of B, A / C, A's event split under `profile`, the work table's
entries, its tiles and masked tiles (the tiles of all entries' mask windows), and fallback_rows."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("64 x 1024", "uniform", 64, 1024, 1536), ("512 x 128", "uniform", 512, 128, 1536), ("250 ragged 100..300", "ragged", 250, 0, 1536),
          ("16 x 4096", "uniform", 16, 4096, 2560), ("8 x 1024 (small)", "uniform", 8, 1024, 1536)]
SWEEP = (1, 2, 4, 8, 16)


def sizes_of(kind, count, rows):
    if kind == "uniform":
        return [rows] * count
    return np.random.default_rng(2024).integers(100, 301, size=count).tolist()


def child(which, reps):
    import torch
    sys.path.insert(0, ROOT)
    import multimodal_fusion_amd as mmf
    dev = torch.device("cuda", 0)

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

    def same_bits(a, b):
        return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))

    name, kind, count, per_seg, d = SHAPES[which]
    k = 5
    small = which == len(SHAPES) - 1
    sizes = sizes_of(kind, count, per_seg)
    ptr = [0] + np.cumsum(sizes).tolist()
    X = rows(ptr[-1], d, ptr[-1] + d)
    wide = mmf.cross_segments_wide.simtopk_cross_segments_wide
    A = lambda **kw: wide(X, ptr=ptr, metric="cosine", k=k, **kw)                                              # noqa: E731
    A16 = lambda **kw: wide(X, ptr=ptr, metric="cosine", k=k, precision="fast_bf16", **kw)                     # noqa: E731
    B = lambda: mmf.cross_segments.simtopk_cross_segments(X, ptr=ptr, metric="cosine", k=k)                   # noqa: E731
    C = lambda: mmf.ops.simtopk(X, metric="cosine", k=k, precision="fast")                                    # noqa: E731
    forced = [(lambda cs=cs: A(col_splits=cs)) for cs in SWEEP] if small else []
    arms = [A, B, C, A16] + forced
    ref = B()
    same = same_bits(A(), ref) and same_bits(A16(), ref) and all(same_bits(fn(), ref) for fn in forced)
    for fn in arms:
        once(fn)
    ts = [[] for _ in arms]
    for _ in range(reps):
        for t, fn in zip(ts, arms):
            t.append(once(fn)[0])
    st = A(profile=True, return_stats=True)[2]
    s16 = A16(return_stats=True)[2]
    table, lists = mmf.cross_segments_wide_table(ptr, d=d, k=k)
    masked = int((table[:, 7] - table[:, 5]).sum())
    tiles = int((table[:, 4] - table[:, 3]).sum())
    a, b, c = (float(np.median(t)) for t in ts[:3])
    spread_b, spread_c = max(ts[1]) - min(ts[1]), max(ts[2]) - min(ts[2])
    print(f"{name}  d = {d}  k = {k}  {len(sizes)} segments, {ptr[-1]} rows   A, A' same bits as B: {same}")
    print(f"   A  wide 16-bit, f16   {stat(ts[0])}   events: prep {st['prep_ms']:.3f} ms, scan {st['scan_ms']:.3f} ms, re-rank {st['rerank_ms']:.3f} ms, "
          f"fallback {st['fallback_ms']:.3f} ms; entries {st['scan_grid']} (at most {st['col_splits']} per block), tiles {tiles}, masked tiles {masked}, "
          f"fallback_rows {st['fallback_rows']}")
    print(f"   A' wide 16-bit, bf16  {stat(ts[3])}   fallback_rows {s16['fallback_rows']}")
    print(f"   B  exact entry        {stat(ts[1])}   B / A {b / a:.2f}x   spread of B {spread_b:.3f} ms; B - A = {b - a:.3f} ms = "
          f"{((b - a) / spread_b if spread_b > 0 else float('inf')):.1f} spreads")
    print(f"   C  plain wide call    {stat(ts[2])}   A / C {a / c:.3f}   spread of C {spread_c:.3f} ms; A - C = {a - c:.3f} ms = "
          f"{((a - c) / spread_c if spread_c > 0 else float('inf')):.1f} spreads")
    spread_a = max(ts[0]) - min(ts[0])
    for cs, t in zip(SWEEP, ts[4:]):
        sf = A(col_splits=cs, return_stats=True)[2]
        s = float(np.median(t))
        print(f"   S{cs:<2d} col_splits = {cs:<2d}    {stat(t)}   entries {sf['scan_grid']} (at most {sf['col_splits']} per block), fallback_rows {sf['fallback_rows']}; "
              f"automatic - forced = {a - s:.3f} ms = {((a - s) / spread_a if spread_a > 0 else float('inf')):.1f} spreads of the automatic arm")
    print(f"verdict {name}: bit for bit {same}; A beats B by more than 3 of B's spreads: {'met' if b - a > 3.0 * spread_b else 'NOT met'}")
    if small:
        print(f"device: {torch.cuda.get_device_name(0)}")


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    if "--child" in args:
        return child(int(args[args.index("--child") + 1]), reps)
    out_path = next((v for v in args if v.endswith(".txt")), None)
    limit = int(args[args.index("--limit") + 1]) if "--limit" in args else 240
    lines = [f"cosine  k = 5  rounds {reps}  whole-call times, median (min .. max)"]
    print(lines[0], flush=True)
    for which in range(len(SHAPES)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(which), "--reps", str(reps)],
                           capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:                            # nothing more is started on the GPU behind a failed step
            print(r.stderr[-4000:], flush=True)
            lines.append(f"{SHAPES[which][0]}: the step ended with status {r.returncode}; the run stops here")
            break
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if lines and not lines[-1].endswith("the run stops here") else 1


if __name__ == "__main__":
    sys.exit(main())
