"""Attention readout over a ragged batch: torch_geometric's GlobalAttention (include/ext/mmf_hg_readout.h).

The reference's HypergraphNetwork ends with ``GlobalAttention(gate_nn)(x, batch)`` (downstream_survival/models/cust_omics.py:69,108):
inside every graph of the batch a softmax of a per-node gate, then the gate-weighted sum of the node rows — the ``[batch_size, C]``
token the rest of the model consumes.  Underneath that is a scatter-max, an exp and two scatter-adds with float atomics; here it is one
pass over x whose sums are sequential chains at two levels (the rows of a chunk of 64, then the chunks of a segment), with an
exponential the header defines itself, so the result has the same bits from call to call and from toolchain to toolchain.

    plan = readout_plan(ptr=ptr)                                  # once per batch layout: every layer, call and epoch reuses it
    out = attention_readout(x, gate, plan=plan)                   # [S, C]; differentiable in x and gate
    out, alpha = attention_readout(x, gate, batch=batch, return_attention=True)      # alpha [N]: the weight of every node
    pool = GlobalAttention(gate_nn)                               # drop-in for torch_geometric.nn.GlobalAttention

Limits: x and gate float32; rows, segments and channels below 2^31.  Segments may be empty (a zero row).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops, ragged

__all__ = ["ReadoutPlan", "readout_plan", "attention_readout", "GlobalAttention"]

_LIMIT = 2 ** 31


class ReadoutPlan:
    """The description of a ragged batch as the readout kernels read it:

        ptr_host int64 [S + 1] (host), ptr int64 [S + 1] (device)      segment s has the rows ptr[s] .. ptr[s + 1]
        table int32 [num_chunks, 2] (device)                          (segment id, first row) of every chunk of 64 rows
        num_rows, num_segments, num_chunks

    It depends on the offsets alone: reusable across layers, calls and epochs."""

    def __init__(self, ptr_host, ptr, table, num_chunks):
        self.ptr_host, self.ptr, self.table = ptr_host, ptr, table
        self.num_rows, self.num_segments, self.num_chunks = int(ptr_host[-1]), int(ptr_host.numel()) - 1, int(num_chunks)

    @property
    def device(self) -> torch.device:
        return self.ptr.device


def _to_device(host: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """A host table on its way to the device without waiting for the stream: out of pinned memory, on the current stream."""
    if dev.type != "cuda":
        return host.to(dev)
    return host.pin_memory().to(dev, non_blocking=True)


def readout_plan(ptr=None, batch=None, *, rows: Optional[int] = None, size: Optional[int] = None, device=None) -> ReadoutPlan:
    """The plan of a batch given by exactly one of ``ptr`` (offsets [S + 1]) / ``batch`` (sorted segment id per row, PyG's
    convention).  ``rows``: the row count the description must have.  ``size``: the number of segments (PyG's ``size``) — trailing
    segments without rows are appended; fewer than the description holds is an error.  ``device``: where the plan lives (default:
    the device of ptr / batch if it is a tensor on one, else the current ROCm device).  A ptr or batch on the device costs one
    device -> host copy; the chunk table is built on the host (mmf_attention_readout_table) and uploaded without waiting."""
    what = "readout_plan"
    p = ragged.offsets(ptr, batch, rows, what=what, min_rows=0, allow_no_segments=True)
    if size is not None:
        size = int(size)
        if size < p.numel() - 1:
            raise ValueError(f"{what}: size = {size}, but the description holds {p.numel() - 1} segments")
        if size > p.numel() - 1:
            p = torch.cat([p, p[-1:].expand(size - (p.numel() - 1))]).contiguous()
    if int(p[-1]) >= _LIMIT or p.numel() - 1 >= _LIMIT:
        raise ValueError(f"{what}: {int(p[-1])} rows in {p.numel() - 1} segments: both must stay below 2^31")
    if device is None:
        src = ptr if ptr is not None else batch
        if isinstance(src, torch.Tensor) and src.is_cuda:
            device = src.device
        else:
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: device {dev}; this op runs only on a ROCm device (the package has no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    L = ops._lib.lib()
    S = p.numel() - 1
    chunks = int(L.mmf_attention_readout_table(ops._hp(p), S, None, 0))
    if chunks < 0:
        ops._lib.check(chunks, "mmf_attention_readout_table")
    table = torch.empty((chunks, 2), dtype=torch.int32)
    got = int(L.mmf_attention_readout_table(ops._hp(p), S, ops._hp(table), chunks))
    if got < 0:
        ops._lib.check(got, "mmf_attention_readout_table")
    return ReadoutPlan(p, _to_device(p, dev), _to_device(table, dev), chunks)


def _rows(x: torch.Tensor) -> torch.Tensor:
    """x as the kernel reads it: unit column stride and a row pitch of at least C (a slice of a larger tensor stays a view)."""
    n, c = x.shape
    if n == 0 or c == 0 or (c > 1 and x.stride(1) != 1) or (n > 1 and x.stride(0) < c):
        return x.contiguous()
    return x


class _Readout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gate, plan):
        xr, g = _rows(x.detach()), gate.detach().contiguous()
        N, C, S, dev = xr.shape[0], xr.shape[1], plan.num_segments, xr.device
        out = torch.empty((S, C), dtype=torch.float32, device=dev)
        alpha = torch.empty((N,), dtype=torch.float32, device=dev)
        seg_max = torch.empty((S,), dtype=torch.float32, device=dev)
        seg_sum = torch.empty((S,), dtype=torch.float32, device=dev)
        ops._call("mmf_attention_readout", dev, ops._p(xr), xr.stride(0) if N > 1 else C, ops._p(g), ops._p(plan.ptr), ops._p(plan.table),
                  plan.num_chunks, N, S, C, ops._p(out), ops._p(alpha), ops._p(seg_max), ops._p(seg_sum), what="attention_readout")
        ctx.plan = plan
        ctx.save_for_backward(xr, alpha, out)
        ctx.mark_non_differentiable(alpha, seg_max, seg_sum)
        return out, alpha, seg_max, seg_sum

    @staticmethod
    def backward(ctx, g_out, _ga, _gm, _gs):
        plan = ctx.plan
        xr, alpha, out = ctx.saved_tensors
        N, C, S, dev = xr.shape[0], xr.shape[1], plan.num_segments, xr.device
        need_x, need_gate = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_gate):
            return None, None, None
        G = g_out.contiguous()
        gx = torch.empty((N, C), dtype=torch.float32, device=dev)
        gg = torch.empty((N,), dtype=torch.float32, device=dev) if need_gate else None      # without it the kernel does not read x
        ops._call("mmf_attention_readout_backward", dev, ops._p(xr), xr.stride(0) if N > 1 else C, ops._p(alpha), ops._p(plan.ptr),
                  ops._p(plan.table), plan.num_chunks, ops._p(out), ops._p(G), N, S, C, ops._p(gx), ops._p(gg), what="attention_readout")
        return (gx if need_x else None), gg, None


def attention_readout(x: torch.Tensor, gate: torch.Tensor, ptr=None, batch=None, *, plan: Optional[ReadoutPlan] = None,
                      size: Optional[int] = None, return_attention: bool = False):
    """out [S, C] = sum over the rows i of segment s of alpha_i x[i], alpha = softmax of ``gate`` inside each segment: torch_geometric's
    GlobalAttention after its two networks, with the bits of the chain definition in include/ext/mmf_hg_readout.h.  x f32 [N, C]; gate
    f32 [N] or [N, 1].  The segments: ``plan`` (readout_plan: reusable), or one of ``ptr`` / ``batch`` (with ``size`` as PyG's), or
    nothing — all rows are one segment (PyG's ``batch=None``).  Differentiable in x and gate; the gate's share of the backward kernel
    is skipped when gate needs no gradient.  ``return_attention=True`` returns (out, alpha) with alpha [N] the weight of every row
    (not differentiable)."""
    what = "attention_readout"
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what}: x must be a float32 tensor [N, C]")
    if x.dtype != torch.float32:
        raise ValueError(f"{what}: x must be float32 (got {x.dtype})")
    N, C = x.shape
    if not isinstance(gate, torch.Tensor) or gate.dtype != torch.float32:
        raise ValueError(f"{what}: gate must be float32 (got {gate.dtype if isinstance(gate, torch.Tensor) else type(gate).__name__})")
    if not (gate.shape == (N,) or gate.shape == (N, 1)):
        raise ValueError(f"{what}: gate must have shape [N] or [N, 1] with N = {N} (got {tuple(gate.shape)})")
    if gate.device != x.device:
        raise ValueError(f"{what}: gate is on {gate.device}, x on {x.device}")
    if N >= _LIMIT or C >= _LIMIT:
        raise ValueError(f"{what}: x is {N} x {C}: rows and channels must stay below 2^31")
    if plan is not None:
        if ptr is not None or batch is not None or size is not None:
            raise ValueError(f"{what}: pass either plan or a description (ptr / batch / size), not both")
        if plan.num_rows != N:
            raise ValueError(f"{what}: the plan was built for {plan.num_rows} rows, x has {N}")
        if plan.device != x.device:
            raise ValueError(f"{what}: the plan is on {plan.device}, x on {x.device}")
    else:
        if ptr is not None and batch is not None:
            raise ValueError(f"{what}: give exactly one of ptr / batch (or neither: one segment, or a plan)")
        if ptr is None and batch is None:
            ptr = [0, N]
        host = ragged.offsets(ptr, batch, N, what=what, min_rows=0, allow_no_segments=True)
        if size is not None and int(size) < host.numel() - 1:
            raise ValueError(f"{what}: size = {int(size)}, but the description holds {host.numel() - 1} segments")
    ops._need_gpu(x, what)
    if plan is None:
        plan = readout_plan(ptr=host, size=size, device=x.device)
    out, alpha, _, _ = _Readout.apply(x, gate.reshape(N), plan)
    return (out, alpha) if return_attention else out


class GlobalAttention(torch.nn.Module):
    """torch_geometric.nn.GlobalAttention (aggr.AttentionalAggregation): forward = attention_readout(nn(x) if nn else x, gate_nn(x)).
    The parameter prefixes are torch_geometric's, ``gate_nn.`` and ``nn.``, so its checkpoints load."""

    def __init__(self, gate_nn: torch.nn.Module, nn: Optional[torch.nn.Module] = None):
        super().__init__()
        self.gate_nn = gate_nn
        self.nn = nn

    def forward(self, x: torch.Tensor, batch=None, ptr=None, size: Optional[int] = None, *, plan: Optional[ReadoutPlan] = None,
                return_attention: bool = False):
        gate = self.gate_nn(x)
        h = self.nn(x) if self.nn is not None else x
        if h.dtype in (torch.float16, torch.bfloat16):                       # autocast: the 16-bit kernels; the token stays float32
            from . import hg16
            return hg16.attention_readout_16(h, gate, ptr=ptr, batch=batch, plan=plan, size=size, return_attention=return_attention)
        return attention_readout(h, gate, ptr=ptr, batch=batch, plan=plan, size=size, return_attention=return_attention)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(gate_nn={self.gate_nn}, nn={self.nn})"
