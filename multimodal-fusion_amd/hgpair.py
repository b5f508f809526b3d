"""Hypergraph propagation with one weight per (node, hyperedge) pair, the softmax over the pairs of a hyperedge or of a node, and
two modules on top (include/ext/mmf_hg_hgpair.h).

Every builder of this library returns ``edge_index [2, E]`` and ``edge_weights [E]``, one weight per column — a cosine, an RBF value,
a ``K_h * K_g`` entry.  ``hgconv.hypergraph_propagate`` uses the first alone, as torch_geometric's ``HypergraphConv`` without
attention does.  Here a value per pair multiplies the message in both gather steps:

    plan = incidence_pair_plan(edge_index, num_nodes, num_edges)          # an IncidencePlan that remembers the columns
    out = hypergraph_propagate_pairs(x, edge_weights, plan=plan, normalization="weight")
    alpha = pair_softmax(score, plan=plan, group="edge")                  # torch_geometric's softmax(score, edge_index[1])
    conv = PairWeightedHypergraphConv(in_channels, out_channels)          # HypergraphConv's parameters, the builders' weights
    att = HypergraphAttentionConv(in_channels, out_channels, heads=3)     # torch_geometric's HypergraphConv(use_attention=True)

Sums are sequential float32 chains in the plan's order, products rounded float32 multiplies: the bits depend neither on the order of
the columns (for an incidence without repeated pairs) nor on the run.  Limits: x, pair_weight and score float32; sizes below 2^31.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import ops
from .hgconv import IncidencePlan, LIMIT, check_edge_index, plan_arguments, unit_stride_rows

__all__ = ["IncidencePairPlan", "incidence_pair_plan", "pair_scales", "hypergraph_propagate_pairs", "pair_softmax",
           "PairWeightedHypergraphConv", "HypergraphAttentionConv"]

NORMALIZATIONS = ("count", "weight")
GROUPS = ("edge", "node")


class IncidencePairPlan(IncidencePlan):
    """An ``IncidencePlan`` (same arrays, same bits: it is accepted wherever one is) with the two position arrays of
    mmf_incidence_pair_plan:

        epos int32 [E]    slot j of emem came from column epos[j] of edge_index
        npos int32 [E]    slot j of nmem came from column npos[j]

    The copies of a pair that occurs several times sit in ascending column order.  Slots past eptr[M] hold 0."""

    def __init__(self, num_nodes, num_edges, num_pairs, eptr, emem, nptr, nmem, edge_scale, node_scale, weight, status, epos, npos):
        super().__init__(num_nodes, num_edges, num_pairs, eptr, emem, nptr, nmem, edge_scale, node_scale, weight, status)
        self.epos, self.npos = epos, npos


def incidence_pair_plan(edge_index: torch.Tensor, num_nodes: int, num_edges: Optional[int] = None,
                        hyperedge_weight: Optional[torch.Tensor] = None, *, check: bool = True) -> IncidencePairPlan:
    """``hgconv.incidence_plan`` with the columns remembered: the arguments, the checks, the host read of ``num_edges=None`` and of
    ``check=True`` are the same, and so is every array the two have in common.  One plan serves weighted and unweighted layers."""
    what = "incidence_pair_plan"
    N, M, E, w = plan_arguments(edge_index, num_nodes, num_edges, hyperedge_weight, what)
    dev = edge_index.device
    eptr = torch.empty((M + 1,), dtype=torch.int64, device=dev)
    nptr = torch.empty((N + 1,), dtype=torch.int64, device=dev)
    emem, nmem, epos, npos = (torch.empty((E,), dtype=torch.int32, device=dev) for _ in range(4))
    edge_scale = torch.empty((M,), dtype=torch.float32, device=dev)
    node_scale = torch.empty((N,), dtype=torch.float32, device=dev)
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    ops._call("mmf_incidence_pair_plan", dev, ops._p(edge_index), E, N, M, ops._p(w), ops._p(eptr), ops._p(emem), ops._p(epos), ops._p(nptr),
              ops._p(nmem), ops._p(npos), ops._p(edge_scale), ops._p(node_scale), ops._p(status), what=what)
    plan = IncidencePairPlan(N, M, E, eptr, emem, nptr, nmem, edge_scale, node_scale, w, status, epos, npos)
    return plan.check() if check else plan


# ---- checks, all before any device work ---------------------------------------------------------------------------------------------
def _check_pair_plan(plan, what: str) -> None:
    if not isinstance(plan, IncidencePlan):
        raise ValueError(f"{what}: plan must be an IncidencePairPlan (incidence_pair_plan)")
    if not isinstance(plan, IncidencePairPlan):
        raise ValueError(f"{what}: a plain IncidencePlan does not know the columns of its slots; build the plan with incidence_pair_plan")


def _check_pairs(t, name: str, plan: IncidencePlan, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 1:
        raise ValueError(f"{what}: {name} must be a float32 vector [E], one value per column of edge_index")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32 (got {t.dtype})")
    if t.numel() != plan.num_pairs:
        raise ValueError(f"{what}: {name} has {t.numel()} entries, the plan was built for {plan.num_pairs} pairs")
    if t.device != plan.device:
        raise ValueError(f"{what}: {name} is on {t.device}, the plan on {plan.device}")


check_pair_plan, check_pairs = _check_pair_plan, _check_pairs          # for hg16, which runs the same checks


def _check_x(x, plan: IncidencePlan, what: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what}: x must be a float32 tensor [N, C]")
    if x.dtype != torch.float32:
        raise ValueError(f"{what}: x must be float32 (got {x.dtype})")
    if plan.num_nodes != x.shape[0]:
        raise ValueError(f"{what}: the plan was built for {plan.num_nodes} nodes, x has {x.shape[0]} rows")
    if plan.device != x.device:
        raise ValueError(f"{what}: the plan is on {plan.device}, x on {x.device}")
    if x.shape[1] >= LIMIT:
        raise ValueError(f"{what}: {x.shape[1]} channels: must stay below 2^31")


# ---- the scales of the "weight" normalisation ---------------------------------------------------------------------------------------
def pair_scales(pair_weight: torch.Tensor, *, plan: IncidencePairPlan):
    """(edge_scale f32 [M], node_scale f32 [N]) of ``normalization="weight"``: 1 / B_e with B_e the chain of a over the hyperedge's
    slots, 1 / D_v with D_v the chain of a * w_e (without hyperedge weights: of a) over the node's slots, 0 for a degree of 0.
    They depend on ``pair_weight`` alone: compute them once and pass them as ``scales=`` to every layer that shares the weights."""
    what = "pair_scales"
    _check_pair_plan(plan, what)
    _check_pairs(pair_weight, "pair_weight", plan, what)
    ops._need_gpu(pair_weight, what)
    a = pair_weight.detach().contiguous()
    dev = a.device
    es = torch.empty((plan.num_edges,), dtype=torch.float32, device=dev)
    ns = torch.empty((plan.num_nodes,), dtype=torch.float32, device=dev)
    ops._call("mmf_pair_scales", dev, ops._p(plan.eptr), ops._p(plan.epos), ops._p(plan.nptr), ops._p(plan.nmem), ops._p(plan.npos), ops._p(a),
              ops._p(plan.hyperedge_weight), plan.num_nodes, plan.num_edges, plan.num_pairs, ops._p(es), ops._p(ns), what=what)
    return es, ns


# ---- propagation --------------------------------------------------------------------------------------------------------------------
def _run(plan: IncidencePairPlan, a: torch.Tensor, x: torch.Tensor, edge_scale, node_scale, transpose: bool):
    """(out [N, C], Y [M, C]) of mmf_hypergraph_propagate_pairs; x f32 [N, C] with unit column stride."""
    N, M, C = plan.num_nodes, plan.num_edges, x.shape[1]
    dev = x.device
    Y = torch.empty((M, C), dtype=torch.float32, device=dev)
    out = torch.empty((N, C), dtype=torch.float32, device=dev)
    ops._call("mmf_hypergraph_propagate_pairs", dev, ops._p(plan.eptr), ops._p(plan.emem), ops._p(plan.epos), ops._p(plan.nptr),
              ops._p(plan.nmem), ops._p(plan.npos), ops._p(edge_scale), ops._p(node_scale), ops._p(plan.hyperedge_weight), ops._p(a),
              plan.num_pairs, ops._p(x), x.stride(0) if N > 1 else C, N, M, C, ops._p(Y), ops._p(out), 1 if transpose else 0,
              what="hypergraph_propagate_pairs")
    return out, Y


class _PropagatePairs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, plan, edge_scale, node_scale):
        xr = unit_stride_rows(x.detach())
        ad = a.detach().contiguous()
        out, Y = _run(plan, ad, xr, edge_scale, node_scale, False)
        ctx.plan, ctx.scales = plan, (edge_scale, node_scale)
        ctx.save_for_backward(ad, xr, Y)
        ctx.mark_non_differentiable(Y)
        return out, Y

    @staticmethod
    def backward(ctx, g_out, _g_y):
        # P_a^T g = A (W Binv) A^T (Dinv . g): the pre-scale is one torch multiply, the rest the same two weighted gather-sums; the
        # gradient in a reads both passes' hyperedge features: grad_a[p] = dot64(g'_v, Y_e) + dot64(x_v, T_e)
        plan = ctx.plan
        edge_scale, node_scale = ctx.scales
        a, x, Y = ctx.saved_tensors
        g = g_out.contiguous() * node_scale.unsqueeze(1)
        gx, T = _run(plan, a, g, edge_scale, None, True)
        ga = None
        if ctx.needs_input_grad[1]:
            ga = torch.empty((plan.num_pairs,), dtype=torch.float32, device=a.device)
            C = x.shape[1]
            ops._call("mmf_pair_weight_grad", a.device, ops._p(plan.eptr), ops._p(plan.emem), ops._p(plan.epos), ops._p(g), ops._p(x),
                      x.stride(0) if plan.num_nodes > 1 else C, ops._p(Y), ops._p(T), plan.num_nodes, plan.num_edges, C, plan.num_pairs,
                      ops._p(ga), what="hypergraph_propagate_pairs (backward)")
        return (gx if ctx.needs_input_grad[0] else None), ga, None, None, None


def hypergraph_propagate_pairs(x: torch.Tensor, pair_weight: torch.Tensor, *, plan: IncidencePairPlan, normalization: str = "count",
                               return_edge_features: bool = False, scales=None):
    """out [N, C] = Dinv A (W Binv) A^T x with A[v, e] the sum of ``pair_weight`` over the columns (v, e) of edge_index, for x f32
    [N, C] (a row or column slice with unit column stride stays a view) and pair_weight f32 [E], with the bits of the rule in
    include/ext/mmf_hg_hgpair.h.

    ``normalization="count"``: the plan's own scales (1 / B_e from the pair count, 1 / D_v from the hyperedge weights) —
    torch_geometric's attention-mode norm.  Differentiable in x and in pair_weight.
    ``normalization="weight"``: the real-valued incidence normalised by its own degrees (``pair_scales``; pass its result as
    ``scales=`` to reuse it) — what suits similarity weights.  Differentiable in x; a pair_weight that requires grad is refused,
    because the scales depend on it.
    With pair_weight all ones both modes equal ``hypergraph_propagate`` bit for bit.  ``return_edge_features=True`` returns
    (out, Y) with Y [M, C] the hyperedge features (not differentiable)."""
    what = "hypergraph_propagate_pairs"
    if normalization not in NORMALIZATIONS:
        raise ValueError(f"{what}: unknown normalization {normalization!r} (one of {NORMALIZATIONS})")
    _check_pair_plan(plan, what)
    _check_x(x, plan, what)
    _check_pairs(pair_weight, "pair_weight", plan, what)
    if normalization == "weight" and pair_weight.requires_grad:
        raise ValueError(f"{what}: pair_weight requires grad under normalization='weight': the scales depend on it, and there is no "
                         "gradient through them (use normalization='count')")
    if scales is not None and normalization != "weight":
        raise ValueError(f"{what}: scales belong to normalization='weight'")
    ops._need_gpu(x, what)
    if normalization == "weight":
        edge_scale, node_scale = pair_scales(pair_weight, plan=plan) if scales is None else scales
        if edge_scale.shape != (plan.num_edges,) or node_scale.shape != (plan.num_nodes,) or edge_scale.dtype != torch.float32 or \
                node_scale.dtype != torch.float32 or edge_scale.device != x.device or node_scale.device != x.device:
            raise ValueError(f"{what}: scales must be pair_scales' two float32 vectors [num_edges] and [num_nodes] on x's device")
    else:
        edge_scale, node_scale = plan.edge_scale, plan.node_scale
    out, Y = _PropagatePairs.apply(x, pair_weight, plan, edge_scale.contiguous(), node_scale.contiguous())
    return (out, Y) if return_edge_features else out


# ---- softmax over the pairs of a row ------------------------------------------------------------------------------------------------
def _group(plan: IncidencePairPlan, group: str):
    return (plan.eptr, plan.epos, plan.num_edges) if group == "edge" else (plan.nptr, plan.npos, plan.num_nodes)


class _PairSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, plan, group):
        s = score.detach().contiguous()
        ptr, pos, rows = _group(plan, group)
        alpha = torch.empty_like(s)
        ops._call("mmf_pair_softmax", s.device, ops._p(ptr), ops._p(pos), rows, plan.num_pairs, ops._p(s), ops._p(alpha), what="pair_softmax")
        ctx.plan, ctx.group = plan, group
        ctx.save_for_backward(alpha)
        return alpha

    @staticmethod
    def backward(ctx, g):
        (alpha,) = ctx.saved_tensors
        ptr, pos, rows = _group(ctx.plan, ctx.group)
        g = g.contiguous()
        out = torch.empty_like(alpha)
        ops._call("mmf_pair_softmax_backward", alpha.device, ops._p(ptr), ops._p(pos), rows, ctx.plan.num_pairs, ops._p(alpha), ops._p(g),
                  ops._p(out), what="pair_softmax (backward)")
        return out, None, None


def pair_softmax(score: torch.Tensor, *, plan: IncidencePairPlan, group: str = "edge") -> torch.Tensor:
    """alpha f32 [E]: torch_geometric's ``softmax(score, index)`` over the pairs.  ``group="edge"`` groups by row 1 of edge_index
    (normalises over the nodes of a hyperedge: attention mode 'node'), ``group="node"`` by row 0.  Inside a group, in plan order:
    the exact maximum, e = cexp(score - max) with the canonical exponential of include/ext/mmf_hg_readout.h, Z the sequential chain
    of e, alpha = e / Z.  Columns with an id outside its range get 0.  Differentiable in score."""
    what = "pair_softmax"
    if group not in GROUPS:
        raise ValueError(f"{what}: unknown group {group!r} (one of {GROUPS})")
    _check_pair_plan(plan, what)
    _check_pairs(score, "score", plan, what)
    ops._need_gpu(score, what)
    return _PairSoftmax.apply(score, plan, group)


# ---- modules ------------------------------------------------------------------------------------------------------------------------
def _glorot(t: torch.Tensor) -> None:
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)


def _plan_for(plan, hyperedge_index, num_nodes, num_edges, hyperedge_weight, what: str) -> IncidencePairPlan:
    if (plan is None) == (hyperedge_index is None):
        raise ValueError(f"{what}: pass either hyperedge_index or plan")
    if plan is None:
        return incidence_pair_plan(hyperedge_index, num_nodes, num_edges, hyperedge_weight)
    if num_edges is not None or hyperedge_weight is not None:
        raise ValueError(f"{what}: num_edges and hyperedge_weight belong to the plan; pass them to incidence_pair_plan")
    _check_pair_plan(plan, what)
    return plan


class PairWeightedHypergraphConv(torch.nn.Module):
    """``HypergraphConv`` over the builders' per-pair weights: forward = propagate_pairs(lin(x), pair_weight) + bias.  The parameters
    are ``lin.weight`` and ``bias``, so a ``HypergraphConv`` (or torch_geometric) checkpoint loads."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True, normalization: str = "weight"):
        super().__init__()
        if normalization not in NORMALIZATIONS:
            raise ValueError(f"PairWeightedHypergraphConv: unknown normalization {normalization!r} (one of {NORMALIZATIONS})")
        self.in_channels, self.out_channels, self.normalization = int(in_channels), int(out_channels), normalization
        self.lin = torch.nn.Linear(self.in_channels, self.out_channels, bias=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _glorot(self.lin.weight)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def forward(self, x: torch.Tensor, hyperedge_index: Optional[torch.Tensor] = None, pair_weight: Optional[torch.Tensor] = None,
                hyperedge_weight: Optional[torch.Tensor] = None, num_edges: Optional[int] = None,
                plan: Optional[IncidencePairPlan] = None) -> torch.Tensor:
        what = "PairWeightedHypergraphConv"
        if pair_weight is None:
            raise ValueError(f"{what}: pair_weight is required (one value per column of hyperedge_index)")
        plan = _plan_for(plan, hyperedge_index, x.shape[0], num_edges, hyperedge_weight, what)
        h = self.lin(x)
        if h.dtype in (torch.float16, torch.bfloat16):                       # autocast: the 16-bit kernels, the bias inside
            from . import hg16
            bias = None if self.bias is None else self.bias.float()           # a module cast as a whole: its bias is widened
            return hg16.hypergraph_propagate_pairs_16(h, pair_weight, plan=plan, normalization=self.normalization, bias=bias)
        out = hypergraph_propagate_pairs(h, pair_weight, plan=plan, normalization=self.normalization)
        return out if self.bias is None else out + self.bias

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, normalization={self.normalization!r})"


class HypergraphAttentionConv(torch.nn.Module):
    """torch_geometric's ``HypergraphConv(use_attention=True)``: per pair (v, e) and head h a score
    leaky_relu(<lin(x)[v, h], att[h, :F]> + <lin(hyperedge_attr)[e, h], att[h, F:]>), a softmax of it over the nodes of a hyperedge
    (``attention_mode="node"``) or over the hyperedges of a node (``"edge"``), dropout on it in training, and the propagation with it
    as the pair weight under the count normalisation, one call per head; the heads are concatenated or averaged, then the bias.
    Parameters: ``lin.weight [heads * F, in]``, ``att [1, heads, 2 F]`` (both glorot), ``bias`` (zeros)."""

    def __init__(self, in_channels: int, out_channels: int, attention_mode: str = "node", heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, bias: bool = True):
        super().__init__()
        if attention_mode not in ("node", "edge"):
            raise ValueError(f"HypergraphAttentionConv: unknown attention_mode {attention_mode!r} (one of ('node', 'edge'))")
        if int(heads) < 1:
            raise ValueError(f"HypergraphAttentionConv: heads must be >= 1 (got {heads})")
        self.in_channels, self.out_channels, self.heads, self.concat = int(in_channels), int(out_channels), int(heads), bool(concat)
        self.attention_mode, self.negative_slope, self.dropout = attention_mode, float(negative_slope), float(dropout)
        self.lin = torch.nn.Linear(self.in_channels, self.heads * self.out_channels, bias=False)
        self.att = torch.nn.Parameter(torch.empty(1, self.heads, 2 * self.out_channels))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.heads * self.out_channels if self.concat else self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _glorot(self.lin.weight)
        _glorot(self.att)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def forward(self, x: torch.Tensor, hyperedge_index: torch.Tensor, hyperedge_weight: Optional[torch.Tensor] = None,
                hyperedge_attr: Optional[torch.Tensor] = None, num_edges: Optional[int] = None,
                plan: Optional[IncidencePairPlan] = None) -> torch.Tensor:
        """``hyperedge_index`` is always needed (the scores are gathered by it); a ``plan`` of it may be passed next to it."""
        what = "HypergraphAttentionConv"
        if hyperedge_attr is None:
            raise ValueError(f"{what}: hyperedge_attr [num_edges, in_channels] is required")
        check_edge_index(hyperedge_index, what)
        if plan is None:
            plan = incidence_pair_plan(hyperedge_index, x.shape[0], hyperedge_attr.shape[0] if num_edges is None else num_edges, hyperedge_weight)
        else:
            if num_edges is not None or hyperedge_weight is not None:
                raise ValueError(f"{what}: num_edges and hyperedge_weight belong to the plan; pass them to incidence_pair_plan")
            _check_pair_plan(plan, what)
            if plan.num_pairs != hyperedge_index.shape[1]:
                raise ValueError(f"{what}: the plan was built for {plan.num_pairs} pairs, hyperedge_index has {hyperedge_index.shape[1]}")
        N, M, H, F = x.shape[0], plan.num_edges, self.heads, self.out_channels
        if hyperedge_attr.dim() != 2 or hyperedge_attr.shape[0] != M:
            raise ValueError(f"{what}: hyperedge_attr must be [num_edges = {M}, in_channels] (got {tuple(hyperedge_attr.shape)})")
        xh = self.lin(x).view(N, H, F)
        eh = self.lin(hyperedge_attr).view(M, H, F)
        sx = (xh * self.att[:, :, :F]).sum(-1)                                   # [N, H]
        se = (eh * self.att[:, :, F:]).sum(-1)                                   # [M, H]
        # a column with an id outside its range is in no CSR: its score is never read, any row will do for the gather
        v = hyperedge_index[0].clamp(0, max(N - 1, 0))
        e = hyperedge_index[1].clamp(0, max(M - 1, 0))
        score = torch.nn.functional.leaky_relu(sx[v] + se[e], self.negative_slope)        # [E, H]
        group = "edge" if self.attention_mode == "node" else "node"
        if xh.dtype in (torch.float16, torch.bfloat16):
            return self._forward_16(xh, score.float(), plan, group)            # the scores are widened: the softmax stays float32
        outs = []
        for h in range(H):
            alpha = pair_softmax(score[:, h].contiguous(), plan=plan, group=group)
            alpha = torch.nn.functional.dropout(alpha, p=self.dropout, training=self.training)
            outs.append(hypergraph_propagate_pairs(xh[:, h], alpha, plan=plan, normalization="count"))
        out = torch.cat(outs, dim=1) if self.concat else torch.stack(outs, dim=0).mean(0)
        return out if self.bias is None else out + self.bias

    def _forward_16(self, xh: torch.Tensor, score: torch.Tensor, plan: IncidencePairPlan, group: str) -> torch.Tensor:
        """The heads of a 16-bit ``xh`` [N, H, F] under float32 scores [E, H]; the result keeps xh's dtype.  Concatenated heads take
        their slice of the bias inside the kernel; averaged heads are averaged in float32, biased, and rounded once."""
        from . import hg16
        H, F = self.heads, self.out_channels
        outs = []
        for h in range(H):
            alpha = pair_softmax(score[:, h].contiguous(), plan=plan, group=group)
            alpha = torch.nn.functional.dropout(alpha, p=self.dropout, training=self.training)
            bias = self.bias[h * F:(h + 1) * F].float() if self.concat and self.bias is not None else None
            outs.append(hg16.hypergraph_propagate_pairs_16(xh[:, h], alpha, plan=plan, normalization="count", bias=bias))
        if self.concat:
            return torch.cat(outs, dim=1)
        out = torch.stack(outs, dim=0).float().mean(0)
        return (out if self.bias is None else out + self.bias).to(xh.dtype)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads}, attention_mode={self.attention_mode!r})"
