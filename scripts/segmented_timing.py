"""Segmented simtopk: one mmf_simtopk_segmented call against the Python loop of one simtopk per segment.

    python scripts/segmented_timing.py [out.txt]

64 segments x 4096 rows, d = 512, cosine, k = 5, f32 rows: ms per call (median of 10 after 3 warm-up calls), the scan
kernel's time (profile = 1) and its fraction of the 2.5 PFLOP/s 16-bit peak on the block-diagonal flops 2 sum(n_s m_s d).
The loop's result is checked against the segmented call (same bits).  Then a ragged mix: sizes drawn from 64 to 16384 rows
with the same total; the exact path (precision="exact": one exact f32 scan and re-rank per segment) at 64 x 4096; many
small segments (2048 x 128) on both paths; and, for scale, the scan of ONE plain simtopk call of 4096 rows."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402

PEAK = 2.5e15
PEAK_F32 = 157.3e12
dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def loop(X, xp, k, precision="auto"):
    idx = torch.empty((X.shape[0], k), dtype=torch.int64, device=X.device)
    val = torch.empty((X.shape[0], k), dtype=torch.float32, device=X.device)
    for s in range(len(xp) - 1):
        a, b = xp[s], xp[s + 1]
        i, v = mmf.simtopk(X[a:b], X[a:b], row_offset=a, col_offset=a, exclude_self=True, k=k, precision=precision)
        idx[a:b] = i
        val[a:b] = v
    return idx, val


def run(name, sizes, d=512, k=5, precision="auto", reps=10):
    xp = [0] + [int(v) for v in np.cumsum(sizes)]
    X = torch.randn(xp[-1], d, device=dev)
    flops = 2.0 * sum(int(s) * int(s) for s in sizes) * d
    t_seg, seg = timed(lambda: mmf.simtopk_segmented(X, ptr=xp, k=k, precision=precision), reps=reps)
    t_loop, ref = timed(lambda: loop(X, xp, k, precision), reps=reps)
    same = bool(torch.equal(seg[0], ref[0]) and torch.equal(seg[1].view(torch.int32), ref[1].view(torch.int32)))
    scan = []
    for _ in range(5):
        _, _, st = mmf.simtopk_segmented(X, ptr=xp, k=k, precision=precision, profile=True, return_stats=True)
        scan.append(st["scan_ms"])
    scan_ms = float(np.median(scan))
    say(f"{name} [{precision}]: segments {len(sizes)}  rows {xp[-1]}  d {d}  k {k}  block-diagonal flops {flops:.3e}")
    say(f"  segmented call {t_seg:8.3f} ms   loop of {len(sizes)} simtopk {t_loop:8.3f} ms   speed-up {t_loop / t_seg:5.2f}x   same bits {same}")
    peak, what = (PEAK, "16-bit peak") if precision != "exact" else (PEAK_F32, "f32 MFMA peak; scan = the exact pass: scans + re-ranks")
    say(f"  segmented scan {scan_ms:8.3f} ms   = {flops / (scan_ms * 1e-3) / peak:.3f} of the {what}   (whole call: "
        f"{flops / (t_seg * 1e-3) / peak:.3f})   scan_grid {st['scan_grid']}  fallback_rows {st['fallback_rows']}")
    return same


ok = run("uniform 64 x 4096", [4096] * 64)
rng = np.random.RandomState(0)
total = 64 * 4096
sizes = []
while sum(sizes) < total:
    sizes.append(int(np.exp(rng.uniform(np.log(64), np.log(16384)))))
sizes[-1] -= sum(sizes) - total
if sizes[-1] < 64:
    sizes[-2] += sizes[-1]
    sizes.pop()
ok &= run("ragged 64..16384", sizes)
ok &= run("uniform 64 x 4096", [4096] * 64, precision="exact", reps=3)
ok &= run("small 2048 x 128", [128] * 2048, reps=3)
ok &= run("small 2048 x 128", [128] * 2048, precision="exact", reps=3)
X1 = torch.randn(4096, 512, device=dev)
one = []
for _ in range(5):
    _, _, st1 = mmf.simtopk(X1, k=5, profile=True, return_stats=True)
    one.append(st1["scan_ms"])
one_ms = float(np.median(one))
say(f"one plain simtopk of 4096 rows: scan {one_ms:.4f} ms = {2.0 * 4096 * 4096 * 512 / (one_ms * 1e-3) / PEAK:.3f} of the 16-bit peak "
    f"(col_splits {st1['col_splits']}, scan_grid {st1['scan_grid']}); x 64 = {64 * one_ms:.3f} ms")
say(f"device: {torch.cuda.get_device_name(0)}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
