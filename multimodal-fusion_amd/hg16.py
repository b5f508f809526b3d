"""16-bit activations for the hypergraph branch: f16 / bf16 x, f32 chains (include/ext/mmf_hg_hg16.h).

Under ``torch.autocast`` every ``Linear`` emits f16 or bf16.  The functions here are ``hgconv.hypergraph_propagate``,
``hgpair.hypergraph_propagate_pairs`` and ``readout.attention_readout`` for such an x: storage is 16-bit, arithmetic is float32, and
every stored 16-bit tensor is rounded once (to nearest, ties to even).  So each result equals the float32 function on ``x.float()``
followed by ``.to(x.dtype)`` at every store, bit for bit — without the cast up, the cast down and the float32 copy of ``[N, C]``.

    out = hypergraph_propagate_16(h16, plan=plan, bias=conv.bias)                     # h16.dtype; Y is rounded once, out once
    out = hypergraph_propagate_pairs_16(h16, edge_weights, plan=pair_plan, normalization="weight")
    token = attention_readout_16(h16, gate, plan=readout_plan)                        # float32 [S, C]

The plans are the existing ``IncidencePlan`` / ``IncidencePairPlan`` / ``ReadoutPlan``.  ``HypergraphConv``,
``PairWeightedHypergraphConv``, ``HypergraphAttentionConv`` and ``GlobalAttention`` route a 16-bit input here.

Limits: x float16 or bfloat16; pair weights, hyperedge weights, scales, bias and gate float32; sizes below 2^31.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops, ragged
from .hgconv import IncidencePlan, LIMIT, check_edge_index, check_weight, incidence_plan, unit_stride_rows
from .hgpair import NORMALIZATIONS, IncidencePairPlan, check_pair_plan, check_pairs, pair_scales
from .readout import ReadoutPlan, readout_plan

__all__ = ["hypergraph_propagate_16", "hypergraph_propagate_pairs_16", "attention_readout_16"]

DTYPES = (torch.float16, torch.bfloat16)


# ---- checks, all before any device work ---------------------------------------------------------------------------------------------
def _check_x16(x, what: str, f32_name: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what}: x must be a float16 or bfloat16 tensor [N, C]")
    if x.dtype not in DTYPES:
        raise ValueError(f"{what}: x must be float16 or bfloat16 (got {x.dtype}); the float32 function is {f32_name}")
    if x.shape[1] >= LIMIT:
        raise ValueError(f"{what}: {x.shape[1]} channels: must stay below 2^31")


def _check_plan_for(x, plan: IncidencePlan, what: str) -> None:
    if plan.num_nodes != x.shape[0]:
        raise ValueError(f"{what}: the plan was built for {plan.num_nodes} nodes, x has {x.shape[0]} rows")
    if plan.device != x.device:
        raise ValueError(f"{what}: the plan is on {plan.device}, x on {x.device}")


def _check_bias(bias, x, what: str) -> None:
    if bias is None:
        return
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or bias.shape != (x.shape[1],):
        raise ValueError(f"{what}: bias must be a float32 vector [C] with C = {x.shape[1]} "
                         f"(got {bias.dtype if isinstance(bias, torch.Tensor) else type(bias).__name__}"
                         f"{tuple(bias.shape) if isinstance(bias, torch.Tensor) else ''})")
    if bias.device != x.device:
        raise ValueError(f"{what}: bias is on {bias.device}, x on {x.device}")


def _run(plan: IncidencePlan, a, x: torch.Tensor, edge_scale, node_scale, bias, transpose: bool, what: str):
    """(out [N, C], Y [M, C]) of mmf_hypergraph_propagate_16 in x's dtype; x with unit column stride, a None or f32 [E]."""
    N, M, C = plan.num_nodes, plan.num_edges, x.shape[1]
    dev = x.device
    Y = torch.empty((M, C), dtype=x.dtype, device=dev)
    out = torch.empty((N, C), dtype=x.dtype, device=dev)
    pair = a is not None
    ops._call("mmf_hypergraph_propagate_16", dev, ops._p(plan.eptr), ops._p(plan.emem), ops._p(plan.epos if pair else None), ops._p(plan.nptr),
              ops._p(plan.nmem), ops._p(plan.npos if pair else None), ops._p(edge_scale), ops._p(node_scale), ops._p(plan.hyperedge_weight),
              ops._p(a), plan.num_pairs, ops._p(x), x.stride(0) if N > 1 else C, N, M, C, ops._DT[x.dtype], ops._p(bias), ops._p(Y), ops._p(out),
              1 if transpose else 0, what=what)
    return out, Y


def _grad_bias(g_out: torch.Tensor) -> torch.Tensor:
    return g_out.sum(0, dtype=torch.float32)


# ---- propagation --------------------------------------------------------------------------------------------------------------------
class _Propagate16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, plan):
        b = None if bias is None else bias.detach().contiguous()
        out, Y = _run(plan, None, unit_stride_rows(x.detach()), plan.edge_scale, plan.node_scale, b, False, "hypergraph_propagate_16")
        ctx.plan = plan
        ctx.mark_non_differentiable(Y)
        return out, Y

    @staticmethod
    def backward(ctx, g_out, _g_y):
        # P^T g = H (W Binv) H^T (Dinv . g): the transposed form takes Dinv as the hyperedge step's scale per source row, so g goes in
        # as it is — no float32 copy of [N, C]
        plan = ctx.plan
        gx = None
        if ctx.needs_input_grad[0]:
            gx, _ = _run(plan, None, unit_stride_rows(g_out), plan.edge_scale, plan.node_scale, None, True, "hypergraph_propagate_16 (backward)")
        return gx, (_grad_bias(g_out) if ctx.needs_input_grad[1] else None), None


def hypergraph_propagate_16(x: torch.Tensor, edge_index: Optional[torch.Tensor] = None, *, plan: Optional[IncidencePlan] = None,
                            num_edges: Optional[int] = None, hyperedge_weight: Optional[torch.Tensor] = None,
                            bias: Optional[torch.Tensor] = None, return_edge_features: bool = False):
    """``hgconv.hypergraph_propagate`` for x float16 / bfloat16 [N, C]: the hyperedge features Y are stored in x's dtype, rounded
    once; the node step reads the rounded Y; out is stored in x's dtype, rounded once, after the optional ``bias`` (float32 [C]) —
    bit for bit ``(propagate32 of the widened operands [+ bias]).to(x.dtype)`` at each of the two stores (include/ext/mmf_hg_hg16.h).
    Differentiable in x (the transposed form over the same plan, in x's dtype) and in bias (``g_out.sum(0, dtype=float32)``).
    ``return_edge_features=True`` returns (out, Y) with Y [M, C] in x's dtype (not differentiable)."""
    what = "hypergraph_propagate_16"
    _check_x16(x, what, "hypergraph_propagate")
    if (plan is None) == (edge_index is None):
        raise ValueError(f"{what}: pass either edge_index or plan")
    if plan is not None:
        if num_edges is not None or hyperedge_weight is not None:
            raise ValueError(f"{what}: num_edges and hyperedge_weight belong to the plan; pass them to incidence_plan")
        if not isinstance(plan, IncidencePlan):
            raise ValueError(f"{what}: plan must be an IncidencePlan (incidence_plan)")
        _check_plan_for(x, plan, what)
    else:
        check_edge_index(edge_index, what)
        if edge_index.device != x.device:
            raise ValueError(f"{what}: edge_index is on {edge_index.device}, x on {x.device}")
        check_weight(hyperedge_weight, None if num_edges is None else int(num_edges), x.device, what)
    _check_bias(bias, x, what)
    ops._need_gpu(x, what)
    if plan is None:
        plan = incidence_plan(edge_index, x.shape[0], num_edges, hyperedge_weight)
    out, Y = _Propagate16.apply(x, bias, plan)
    return (out, Y) if return_edge_features else out


class _PropagatePairs16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, bias, plan, edge_scale, node_scale):
        xr = unit_stride_rows(x.detach())
        ad = a.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        out, Y = _run(plan, ad, xr, edge_scale, node_scale, b, False, "hypergraph_propagate_pairs_16")
        ctx.plan, ctx.scales = plan, (edge_scale, node_scale)
        ctx.save_for_backward(ad, xr, Y)
        ctx.mark_non_differentiable(Y)
        return out, Y

    @staticmethod
    def backward(ctx, g_out, _g_y):
        plan = ctx.plan
        edge_scale, node_scale = ctx.scales
        a, x, Y = ctx.saved_tensors
        g = g_out.contiguous()                                                   # dense: the weight gradient reads it with pitch C
        gx = ga = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx, T = _run(plan, a, g, edge_scale, node_scale, None, True, "hypergraph_propagate_pairs_16 (backward)")
        if ctx.needs_input_grad[1]:
            ga = torch.empty((plan.num_pairs,), dtype=torch.float32, device=a.device)
            C = x.shape[1]
            ops._call("mmf_pair_weight_grad_16", a.device, ops._p(plan.eptr), ops._p(plan.emem), ops._p(plan.epos), ops._p(g), ops._p(node_scale),
                      ops._p(x), x.stride(0) if plan.num_nodes > 1 else C, ops._p(Y), ops._p(T), plan.num_nodes, plan.num_edges, C, plan.num_pairs,
                      ops._DT[x.dtype], ops._p(ga), what="hypergraph_propagate_pairs_16 (backward)")
        return (gx if ctx.needs_input_grad[0] else None), ga, (_grad_bias(g_out) if ctx.needs_input_grad[2] else None), None, None, None


def hypergraph_propagate_pairs_16(x: torch.Tensor, pair_weight: torch.Tensor, *, plan: IncidencePairPlan, normalization: str = "count",
                                  scales=None, bias: Optional[torch.Tensor] = None, return_edge_features: bool = False):
    """``hgpair.hypergraph_propagate_pairs`` for x float16 / bfloat16 [N, C]; ``pair_weight``, the hyperedge weights and the scales
    stay float32.  Y and out are stored in x's dtype, each rounded once, out after the optional ``bias`` (float32 [C]).
    Differentiable in x, in bias and, under ``normalization="count"``, in pair_weight (float32: the two dot64 of
    include/ext/mmf_hg_hgpair.h over the widened rows); under ``"weight"`` a pair_weight that requires grad is refused."""
    what = "hypergraph_propagate_pairs_16"
    if normalization not in NORMALIZATIONS:
        raise ValueError(f"{what}: unknown normalization {normalization!r} (one of {NORMALIZATIONS})")
    check_pair_plan(plan, what)
    _check_x16(x, what, "hypergraph_propagate_pairs")
    _check_plan_for(x, plan, what)
    check_pairs(pair_weight, "pair_weight", plan, what)
    if normalization == "weight" and pair_weight.requires_grad:
        raise ValueError(f"{what}: pair_weight requires grad under normalization='weight': the scales depend on it, and there is no "
                         "gradient through them (use normalization='count')")
    if scales is not None and normalization != "weight":
        raise ValueError(f"{what}: scales belong to normalization='weight'")
    _check_bias(bias, x, what)
    ops._need_gpu(x, what)
    if normalization == "weight":
        edge_scale, node_scale = pair_scales(pair_weight, plan=plan) if scales is None else scales
        if edge_scale.shape != (plan.num_edges,) or node_scale.shape != (plan.num_nodes,) or edge_scale.dtype != torch.float32 or \
                node_scale.dtype != torch.float32 or edge_scale.device != x.device or node_scale.device != x.device:
            raise ValueError(f"{what}: scales must be pair_scales' two float32 vectors [num_edges] and [num_nodes] on x's device")
    else:
        edge_scale, node_scale = plan.edge_scale, plan.node_scale
    out, Y = _PropagatePairs16.apply(x, pair_weight, bias, plan, edge_scale.contiguous(), node_scale.contiguous())
    return (out, Y) if return_edge_features else out


# ---- readout ------------------------------------------------------------------------------------------------------------------------
class _Readout16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gate, plan):
        xr, g = unit_stride_rows(x.detach()), gate.detach().contiguous()
        N, C, S, dev = xr.shape[0], xr.shape[1], plan.num_segments, xr.device
        out = torch.empty((S, C), dtype=torch.float32, device=dev)
        alpha = torch.empty((N,), dtype=torch.float32, device=dev)
        seg_max = torch.empty((S,), dtype=torch.float32, device=dev)
        seg_sum = torch.empty((S,), dtype=torch.float32, device=dev)
        ops._call("mmf_attention_readout_16", dev, ops._p(xr), xr.stride(0) if N > 1 else C, ops._DT[xr.dtype], ops._p(g), ops._p(plan.ptr),
                  ops._p(plan.table), plan.num_chunks, N, S, C, ops._p(out), ops._p(alpha), ops._p(seg_max), ops._p(seg_sum),
                  what="attention_readout_16")
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
        gx = torch.empty((N, C), dtype=xr.dtype, device=dev)
        gg = torch.empty((N,), dtype=torch.float32, device=dev) if need_gate else None      # without it the kernel does not read x
        ops._call("mmf_attention_readout_backward_16", dev, ops._p(xr), xr.stride(0) if N > 1 else C, ops._DT[xr.dtype], ops._p(alpha),
                  ops._p(plan.ptr), ops._p(plan.table), plan.num_chunks, ops._p(out), ops._p(G), N, S, C, ops._p(gx), ops._p(gg),
                  what="attention_readout_16")
        return (gx if need_x else None), gg, None


def attention_readout_16(x: torch.Tensor, gate: torch.Tensor, ptr=None, batch=None, *, plan: Optional[ReadoutPlan] = None,
                         size: Optional[int] = None, return_attention: bool = False):
    """``readout.attention_readout`` for x float16 / bfloat16 [N, C].  ``gate`` [N] or [N, 1] is float32; a 16-bit gate is widened
    here (one torch cast of N values, differentiable).  out [S, C] and alpha [N] are float32 and equal, bit for bit, the float32
    function on ``x.float()``.  Differentiable in x (grad_x in x's dtype, each element ``alpha_i * G[s, c]`` rounded once) and in gate
    (float32)."""
    what = "attention_readout_16"
    _check_x16(x, what, "attention_readout")
    N, C = x.shape
    if not isinstance(gate, torch.Tensor) or gate.dtype not in (torch.float32,) + DTYPES:
        raise ValueError(f"{what}: gate must be float32, float16 or bfloat16 "
                         f"(got {gate.dtype if isinstance(gate, torch.Tensor) else type(gate).__name__})")
    if not (gate.shape == (N,) or gate.shape == (N, 1)):
        raise ValueError(f"{what}: gate must have shape [N] or [N, 1] with N = {N} (got {tuple(gate.shape)})")
    if gate.device != x.device:
        raise ValueError(f"{what}: gate is on {gate.device}, x on {x.device}")
    if N >= LIMIT:
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
    out, alpha, _, _ = _Readout16.apply(x, gate.reshape(N).float(), plan)
    return (out, alpha) if return_attention else out
