"""A/B of the symmetric 16-bit scan in ONE process on one library: rounds of the bench workload with MMF_SYMMETRIC=0 and =1
interleaved (boxes of the pool differ by a few per cent, and so do separate processes).
    scripts/ab_symmetric.py [--rows N] [--rounds R] [--prec fast|fast_bf16] [--group G]
Per arm: wall time of a whole call (as bench.py's step), scan and re-rank time, candidates per row, flagged rows; the two arms'
results are compared bit for bit.  The last line is the verdict rule of profiles/r04_symmetric_ab.txt: a gain counts when the
medians differ by more than three times the larger min-max spread."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimodal_fusion_amd as mmf   # noqa: E402
from bench import make_rows            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=262144)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--prec", default="auto")
ap.add_argument("--topk", type=int, default=5)
ap.add_argument("--group", type=int, default=0, help="MMF_SYMMETRIC_G (0: the library's default)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
X = make_rows(0, a.rows, a.dim, dev)
if a.group > 0:
    os.environ["MMF_SYMMETRIC_G"] = str(a.group)

arms = ("off", "on")
wall, scan, rerank, info, ref = {n: [] for n in arms}, {n: [] for n in arms}, {n: [] for n in arms}, {}, None
for r in range(a.rounds + 1):
    for n in arms:
        os.environ["MMF_SYMMETRIC"] = "1" if n == "on" else "0"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        i, v, st = mmf.simtopk(X, metric="cosine", k=a.topk, precision=a.prec, profile=True, return_stats=True)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if r == 0:                      # warm-up round: also the parity check
            if ref is None:
                ref = (i, v)
            else:
                assert torch.equal(i, ref[0]) and torch.equal(v, ref[1]), "the symmetric scan's result differs"
            continue
        wall[n].append(dt)
        scan[n].append(st["scan_ms"])
        rerank[n].append(st["rerank_ms"])
        info[n] = (st["candidates"] / a.rows, st["fallback_rows"], st["scan_grid"])
for n in arms:
    w = wall[n]
    print(f"{n:4s} step_ms median {statistics.median(w):7.3f}  min {min(w):7.3f}  max {max(w):7.3f}   scan_ms median "
          f"{statistics.median(scan[n]):7.3f}   rerank_ms median {statistics.median(rerank[n]):6.3f}   candidates/row {info[n][0]:6.1f}  "
          f"flagged {info[n][1]}  scan_grid {info[n][2]}", flush=True)
spread = max(max(wall[n]) - min(wall[n]) for n in arms)
gain = statistics.median(wall["off"]) - statistics.median(wall["on"])
print(f"rows {a.rows}: off - on = {gain:.3f} ms ({100.0 * gain / statistics.median(wall['off']):.1f} %), larger min-max spread {spread:.3f} ms: "
      f"{'a gain' if gain > 3.0 * spread else 'NOT a clear gain'}", flush=True)
