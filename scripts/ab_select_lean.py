"""A/B of the re-rank's lean gather in ONE process (the pattern of scripts/ab_inproc.py): MMF_SELECT_LEAN=0 and 1 interleaved,
scripts/ab_select_lean.py [--rows N] [--rounds R] [--prec fast|fast_bf16].  The switch is read per call.  Reports rerank_ms
(device events around the re-rank) and the whole call (host clock around a call that ends in a synchronise), medians with
min - max, and compares the two arms' results bit for bit."""
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
ap.add_argument("--prec", default="fast")
ap.add_argument("--data", default="gaussian")
ap.add_argument("--topk", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
X = make_rows(0, a.rows, a.dim, dev, data=a.data)
arms = {"lean=0": "0", "lean=1": "1"}
call, rerank, scan, ref = {n: [] for n in arms}, {n: [] for n in arms}, {n: [] for n in arms}, None
for r in range(a.rounds + 1):
    for name, val in arms.items():
        os.environ["MMF_SELECT_LEAN"] = val
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        i, v, st = mmf.simtopk(X, metric="cosine", k=a.topk, precision=a.prec, profile=True, return_stats=True)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        if r == 0:                      # warm-up round: also the parity check
            if ref is None:
                ref = (i, v)
            else:
                assert torch.equal(i, ref[0]) and torch.equal(v, ref[1]), f"{name}: result differs"
            continue
        call[name].append(ms)
        rerank[name].append(st["rerank_ms"])
        scan[name].append(st["scan_ms"])
os.environ.pop("MMF_SELECT_LEAN", None)


def line(t):
    return f"median {statistics.median(t):7.3f}  min {min(t):7.3f}  max {max(t):7.3f}"


for name in arms:
    print(f"{name}  rerank_ms {line(rerank[name])}   call_ms {line(call[name])}   scan_ms {line(scan[name])}", flush=True)
for what, t in (("rerank_ms", rerank), ("call_ms", call)):
    d = statistics.median(t["lean=0"]) - statistics.median(t["lean=1"])
    spread = max(max(x) - min(x) for x in t.values())
    print(f"{what}: lean=0 - lean=1 = {d:.3f} ms, larger min-max spread {spread:.3f} ms: "
          f"{'a gain' if d > 3 * spread else 'NOT a clear gain'}", flush=True)
