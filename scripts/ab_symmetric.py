"""A/B of the symmetric 16-bit scan in ONE process on one library: rounds of the bench workload with the plain scan
(MMF_SYMMETRIC=0), the symmetric scan with frozen thresholds and the forward schedule (MMF_SYMMETRIC_LIVE=0) and the symmetric
scan with live thresholds and the backward schedule (the default) interleaved (boxes of the pool differ by a few per cent, and
so do separate processes).
    scripts/ab_symmetric.py [--rows N] [--rounds R] [--prec fast|fast_bf16] [--group G] [--all-four]
--all-four adds the two mixed arms (MMF_SYMMETRIC_LIVE=2: live, forward; =3: frozen, backward).
Per arm: wall time of a whole call (as bench.py's step), scan and re-rank time, candidates per row, flagged rows; the arms'
results are compared bit for bit.  With MMF_SYMMETRIC_DEBUG=1 the library prints the received-entry line of every symmetric
call of the warm-up round (stderr).  The last lines are the verdict rule of profiles/r04_symmetric_ab.txt: a gain counts when
the medians differ by more than three times the larger min-max spread."""
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
ap.add_argument("--all-four", action="store_true", help="also live + forward and frozen + backward")
a = ap.parse_args()
dev = torch.device("cuda", 0)
X = make_rows(0, a.rows, a.dim, dev)
if a.group > 0:
    os.environ["MMF_SYMMETRIC_G"] = str(a.group)

# arm -> (MMF_SYMMETRIC, MMF_SYMMETRIC_LIVE)
ARMS = {"off": ("0", "1"), "frozen": ("1", "0"), "live": ("1", "1"), "live-fwd": ("1", "2"), "frozen-back": ("1", "3")}
arms = ("off", "frozen", "live") + (("live-fwd", "frozen-back") if a.all_four else ())
debug = os.environ.pop("MMF_SYMMETRIC_DEBUG", None)
wall, scan, rerank, info, ref = {n: [] for n in arms}, {n: [] for n in arms}, {n: [] for n in arms}, {}, None
for r in range(a.rounds + 1):
    for n in arms:
        os.environ["MMF_SYMMETRIC"], os.environ["MMF_SYMMETRIC_LIVE"] = ARMS[n]
        if debug and r == 0 and n != "off":      # the dump synchronises and reads back: warm-up round only
            print(f"{n}:", file=sys.stderr, flush=True)
            os.environ["MMF_SYMMETRIC_DEBUG"] = debug
        else:
            os.environ.pop("MMF_SYMMETRIC_DEBUG", None)
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
    print(f"{n:11s} step_ms median {statistics.median(w):7.3f}  min {min(w):7.3f}  max {max(w):7.3f}   scan_ms median "
          f"{statistics.median(scan[n]):7.3f}   rerank_ms median {statistics.median(rerank[n]):6.3f}   candidates/row {info[n][0]:6.1f}  "
          f"flagged {info[n][1]}  scan_grid {info[n][2]}", flush=True)
for x, y in (("off", "live"), ("frozen", "live")):
    spread = max(max(wall[n]) - min(wall[n]) for n in (x, y))
    gain = statistics.median(wall[x]) - statistics.median(wall[y])
    print(f"rows {a.rows}: {x} - {y} = {gain:.3f} ms ({100.0 * gain / statistics.median(wall[x]):.1f} %), larger min-max spread {spread:.3f} ms: "
          f"{'a gain' if gain > 3.0 * spread else 'NOT a clear gain'}", flush=True)
