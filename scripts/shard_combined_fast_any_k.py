"""Two ranks on ONE GPU (gloo + host staging): every rank runs distributed.sharded_simtopk_combined_fast_any_k on its uneven shard
of n = 401 rows (d = 40, dp = 2, k = 45, self excluded; f16 and bf16 operands) and checks its rows against the unsharded exact call
combined_topk_anyk.simtopk_combined_any_k, bit for bit; the gathered output against all of it.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P \
        scripts/shard_combined_fast_any_k.py

tests/test_gpu_simtopk_combined_xy_fast_anyk.py runs this under pytest -m gpu."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from importlib import import_module   # noqa: E402

import multimodal_fusion_amd as mmf   # noqa: E402

dmod = import_module("multimodal_fusion_amd.distributed")
torch.cuda.set_device(0)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda", 0)
N, D, K, LH, LG = 401, 40, 45, 0.5, 2e-7

g = torch.Generator().manual_seed(77)
F = (torch.randn(N, D, generator=g) * (8.0 / D) ** 0.5).to(dev)
P = (torch.randint(0, 48, (N, 2), generator=g) * 224).float().to(dev)
want = mmf.combined_topk_anyk.simtopk_combined_any_k(F, P, LH, LG, K)
lo, hi = dmod.shard_bounds(N, world, rank)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


for precision in ("fast", "fast_bf16"):
    i, v, st = dmod.sharded_simtopk_combined_fast_any_k(F[lo:hi].clone(), P[lo:hi].clone(), N, lambda_h=LH, lambda_g=LG, k=K, precision=precision,
                                                        return_stats=True)
    ok = same((i, v), (want[0][lo:hi], want[1][lo:hi])) and st["driver"] == "simple" and st["precision_used"] == mmf._lib.PRECISIONS[precision]
    gi, gv = dmod.sharded_simtopk_combined_fast_any_k(F[lo:hi].clone(), P[lo:hi].clone(), N, lambda_h=LH, lambda_g=LG, k=K, precision=precision,
                                                      gather_output=True)
    ok = ok and same((gi, gv), want)
    print(f"rank {rank}/{world} rows [{lo}, {hi}) {precision}: {'OK' if ok else 'MISMATCH'}", flush=True)
    assert ok, precision
dist.barrier()
if rank == 0:
    print("SHARDED FAST ANY-K OK", flush=True)
dist.destroy_process_group()
