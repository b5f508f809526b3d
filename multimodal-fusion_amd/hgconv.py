"""Hypergraph propagation on the incidence: out = D^-1 H W B^-1 H^T x (include/ext/mmf_hg_hgconv.h).

The reference's model reads every edge list this library builds in one place: torch_geometric's ``HypergraphConv(x, edge_index)``
with ``use_attention=False`` (downstream_survival/models/cust_omics.py:58,101), row 1 of ``edge_index`` being the hyperedge id.
Underneath that is two scatter-adds with float atomics; here it is two gather-sums over a canonical CSR (an ``IncidencePlan``), so
the result does not depend on the order of the columns of ``edge_index`` and has the same bits from call to call.

    plan = incidence_plan(edge_index, num_nodes, num_edges)       # once per graph: every layer, call and epoch reuses it
    out = hypergraph_propagate(x, plan=plan)                      # differentiable in x
    conv = HypergraphConv(in_channels, out_channels)              # drop-in for torch_geometric.nn.HypergraphConv (no attention)

Limits: x float32; num_nodes, num_edges and the pair count below 2^31.  No gradient with respect to the hyperedge weights.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import ops

__all__ = ["IncidencePlan", "incidence_plan", "hypergraph_propagate", "knn_incidence", "HypergraphConv"]

LIMIT = 2 ** 31


class IncidencePlan:
    """Both CSRs and both scale vectors of an incidence, on the device (mmf_incidence_plan):

        eptr int64 [M + 1], emem int32 [E]    hyperedge e has the nodes emem[eptr[e]:eptr[e + 1]], ascending
        nptr int64 [N + 1], nmem int32 [E]    node v has the hyperedges nmem[nptr[v]:nptr[v + 1]], ascending
        edge_scale f32 [M] = 1 / B_e, node_scale f32 [N] = 1 / D_v  (0 for an empty row)
        status int64 [2]                      lowest column of edge_index with a bad node / hyperedge id, -1 for none

    ``check()`` reads ``status`` once (one host synchronisation) and raises ValueError for an id outside its range; such pairs
    are in neither CSR, so a plan is safe to apply whatever ``status`` says."""

    def __init__(self, num_nodes, num_edges, num_pairs, eptr, emem, nptr, nmem, edge_scale, node_scale, weight, status):
        self.num_nodes, self.num_edges, self.num_pairs = int(num_nodes), int(num_edges), int(num_pairs)
        self.eptr, self.emem, self.nptr, self.nmem = eptr, emem, nptr, nmem
        self.edge_scale, self.node_scale, self.hyperedge_weight, self.status = edge_scale, node_scale, weight, status
        self._checked = False

    @property
    def device(self) -> torch.device:
        return self.eptr.device

    def check(self) -> "IncidencePlan":
        if not self._checked:
            bad_node, bad_edge = (int(v) for v in self.status.tolist())
            if bad_node >= 0:
                raise ValueError(f"incidence_plan: edge_index[0, {bad_node}] is no node id in [0, {self.num_nodes})")
            if bad_edge >= 0:
                raise ValueError(f"incidence_plan: edge_index[1, {bad_edge}] is no hyperedge id in [0, {self.num_edges})")
            self._checked = True
        return self


def check_edge_index(edge_index, what: str) -> None:
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"{what}: edge_index must be an int64 tensor of shape [2, E]"
                         f" (got {tuple(edge_index.shape) if isinstance(edge_index, torch.Tensor) else type(edge_index).__name__})")
    if edge_index.dtype != torch.int64:
        raise ValueError(f"{what}: edge_index must be int64 (got {edge_index.dtype})")
    if not edge_index.is_contiguous():
        raise ValueError(f"{what}: edge_index must be contiguous (row 0 the node ids, row 1 the hyperedge ids)")
    if edge_index.shape[1] >= LIMIT:
        raise ValueError(f"{what}: {edge_index.shape[1]} pairs: the pair count must stay below 2^31")


def _check_weight(w, num_edges: Optional[int], dev: torch.device, what: str) -> None:
    if w is None:
        return
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.dtype != torch.float32:
        raise ValueError(f"{what}: hyperedge_weight must be a float32 vector [num_edges]")
    if w.requires_grad:
        raise ValueError(f"{what}: hyperedge_weight requires grad: there is no gradient with respect to the weights")
    if num_edges is not None and w.numel() != num_edges:
        raise ValueError(f"{what}: hyperedge_weight has {w.numel()} entries for {num_edges} hyperedges")
    if w.device != dev:
        raise ValueError(f"{what}: hyperedge_weight is on {w.device}, edge_index on {dev}")


check_weight = _check_weight          # for hg16, which runs the same checks


def plan_arguments(edge_index, num_nodes, num_edges, hyperedge_weight, what: str):
    """The checks of a plan build, before any device work, and its sizes: (N, M, E, contiguous hyperedge_weight or None).
    ``num_edges=None`` costs the one host read of max + 1."""
    check_edge_index(edge_index, what)
    N = int(num_nodes)
    if N < 0 or N >= LIMIT:
        raise ValueError(f"{what}: num_nodes must lie in [0, 2^31) (got {N})")
    if num_edges is not None and not 0 <= int(num_edges) < LIMIT:
        raise ValueError(f"{what}: num_edges must lie in [0, 2^31) (got {num_edges})")
    dev = edge_index.device
    _check_weight(hyperedge_weight, None if num_edges is None else int(num_edges), dev, what)
    E = edge_index.shape[1]
    if num_edges is None:
        M = int(edge_index[1].max()) + 1 if E else 0                    # the one host read
        if not 0 <= M < LIMIT:
            raise ValueError(f"{what}: the largest hyperedge id gives num_edges = {M}, outside [0, 2^31)")
        _check_weight(hyperedge_weight, M, dev, what)
    else:
        M = int(num_edges)
    ops._need_gpu(edge_index, what)
    return N, M, E, None if hyperedge_weight is None else hyperedge_weight.contiguous()


def incidence_plan(edge_index: torch.Tensor, num_nodes: int, num_edges: Optional[int] = None,
                   hyperedge_weight: Optional[torch.Tensor] = None, *, check: bool = True) -> IncidencePlan:
    """The plan of ``edge_index`` int64 [2, E] (row 0 node ids in [0, num_nodes), row 1 hyperedge ids in [0, num_edges)); a pair
    that occurs t times counts t times.  ``num_edges=None`` means max + 1, which costs one host read: pass it to avoid the read.
    ``hyperedge_weight`` f32 [num_edges] enters the node degrees D_v and every propagation over the plan.  The plan is meant to be
    reused: a network applies the same incidence at every layer, call and epoch.
    ``check=True`` reads the plan's status word (one host synchronisation) and raises ValueError for an id outside its range;
    ``check=False`` returns without waiting for the stream (``plan.check()`` does the read later)."""
    what = "incidence_plan"
    N, M, E, w = plan_arguments(edge_index, num_nodes, num_edges, hyperedge_weight, what)
    dev = edge_index.device
    eptr = torch.empty((M + 1,), dtype=torch.int64, device=dev)
    nptr = torch.empty((N + 1,), dtype=torch.int64, device=dev)
    emem = torch.empty((E,), dtype=torch.int32, device=dev)
    nmem = torch.empty((E,), dtype=torch.int32, device=dev)
    edge_scale = torch.empty((M,), dtype=torch.float32, device=dev)
    node_scale = torch.empty((N,), dtype=torch.float32, device=dev)
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    ops._call("mmf_incidence_plan", dev, ops._p(edge_index), E, N, M, ops._p(w), ops._p(eptr), ops._p(emem), ops._p(nptr), ops._p(nmem),
              ops._p(edge_scale), ops._p(node_scale), ops._p(status), what=what)
    plan = IncidencePlan(N, M, E, eptr, emem, nptr, nmem, edge_scale, node_scale, w, status)
    return plan.check() if check else plan


def _run(plan: IncidencePlan, x: torch.Tensor, transpose: bool):
    """(out [N, C], Y [M, C]) of mmf_hypergraph_propagate; x f32 [N, C] with unit column stride."""
    N, M, C = plan.num_nodes, plan.num_edges, x.shape[1]
    dev = x.device
    Y = torch.empty((M, C), dtype=torch.float32, device=dev)
    out = torch.empty((N, C), dtype=torch.float32, device=dev)
    ops._call("mmf_hypergraph_propagate", dev, ops._p(plan.eptr), ops._p(plan.emem), ops._p(plan.nptr), ops._p(plan.nmem),
              ops._p(plan.edge_scale), ops._p(plan.node_scale), ops._p(plan.hyperedge_weight), ops._p(x), x.stride(0) if N > 1 else C,
              N, M, C, ops._p(Y), ops._p(out), 1 if transpose else 0, what="hypergraph_propagate")
    return out, Y


def unit_stride_rows(x: torch.Tensor) -> torch.Tensor:
    """x as the kernel reads it: unit column stride and a row pitch of at least C (a row slice of a larger tensor stays a view)."""
    n, c = x.shape
    if n == 0 or c == 0 or (c > 1 and x.stride(1) != 1) or (n > 1 and x.stride(0) < c):
        return x.contiguous()
    return x


class _Propagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        out, Y = _run(plan, unit_stride_rows(x.detach()), False)
        ctx.plan = plan
        ctx.mark_non_differentiable(Y)
        return out, Y

    @staticmethod
    def backward(ctx, g_out, _g_y):
        # P^T g = H (W Binv) H^T (Dinv . g): the pre-scale is one torch multiply, the rest the same two gather-sums
        plan = ctx.plan
        g = g_out.contiguous() * plan.node_scale.unsqueeze(1)
        gx, _ = _run(plan, g, True)
        return gx, None


def hypergraph_propagate(x: torch.Tensor, edge_index: Optional[torch.Tensor] = None, *, plan: Optional[IncidencePlan] = None,
                         num_edges: Optional[int] = None, hyperedge_weight: Optional[torch.Tensor] = None,
                         return_edge_features: bool = False):
    """out [N, C] = D^-1 H W B^-1 H^T x for x f32 [N, C]: torch_geometric's HypergraphConv propagation with use_attention=False,
    with the bits of the sequential-chain definition in include/ext/mmf_hg_hgconv.h.  Pass ``plan`` (incidence_plan: reusable), or
    ``edge_index`` (and optionally ``num_edges`` / ``hyperedge_weight``) to have one built for this call.  Differentiable in x
    (the backward is the transposed form over the same plan).  ``return_edge_features=True`` returns (out, Y) with Y [M, C] the
    hyperedge features w_e B_e^-1 sum_v x_v (not differentiable)."""
    what = "hypergraph_propagate"
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what}: x must be a float32 tensor [N, C]")
    if x.dtype != torch.float32:
        raise ValueError(f"{what}: x must be float32 (got {x.dtype})")
    if (plan is None) == (edge_index is None):
        raise ValueError(f"{what}: pass either edge_index or plan")
    if plan is not None:
        if num_edges is not None or hyperedge_weight is not None:
            raise ValueError(f"{what}: num_edges and hyperedge_weight belong to the plan; pass them to incidence_plan")
        if plan.num_nodes != x.shape[0]:
            raise ValueError(f"{what}: the plan was built for {plan.num_nodes} nodes, x has {x.shape[0]} rows")
        if plan.device != x.device:
            raise ValueError(f"{what}: the plan is on {plan.device}, x on {x.device}")
    else:
        check_edge_index(edge_index, what)
        if edge_index.device != x.device:
            raise ValueError(f"{what}: edge_index is on {edge_index.device}, x on {x.device}")
        _check_weight(hyperedge_weight, None if num_edges is None else int(num_edges), x.device, what)
        plan = incidence_plan(edge_index, x.shape[0], num_edges, hyperedge_weight)
    ops._need_gpu(x, what)
    if x.shape[1] >= LIMIT:
        raise ValueError(f"{what}: {x.shape[1]} channels: must stay below 2^31")
    out, Y = _Propagate.apply(x, plan)
    return (out, Y) if return_edge_features else out


def knn_incidence(idx: torch.Tensor, include_self: bool = True) -> torch.Tensor:
    """The incidence of a k-NN table: ``idx`` int64 [N, k] (simtopk's first result; the global ids of the segmented and
    cross-segment calls work unchanged — a block-diagonal cohort is an incidence with global ids) -> edge_index int64 [2, E] where
    row i's hyperedge i is {i} ∪ idx[i].  Negative ids (rows short of k neighbours) are dropped; with ``include_self`` an entry
    idx[i, j] == i is dropped too, so that i is in its hyperedge once.  One host read (the number of pairs kept)."""
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype != torch.int64:
        raise ValueError("knn_incidence: idx must be an int64 tensor [N, k]")
    n = idx.shape[0]
    rows = torch.arange(n, dtype=torch.int64, device=idx.device).unsqueeze(1)
    keep = idx >= 0
    nodes = idx
    if include_self:
        keep = keep & (idx != rows)
        nodes = torch.cat([rows, idx], dim=1)
        keep = torch.cat([torch.ones((n, 1), dtype=torch.bool, device=idx.device), keep], dim=1)
    edges = rows.expand_as(nodes)
    return torch.stack([nodes[keep], edges[keep]]).contiguous()


class HypergraphConv(torch.nn.Module):
    """torch_geometric.nn.HypergraphConv without attention: forward = propagate(lin(x)) + bias, with ``lin`` a bias-free Linear
    (glorot) and ``bias`` zeros — the parameter names ``lin.weight`` and ``bias`` of torch_geometric, so its checkpoints load."""

    def __init__(self, in_channels: int, out_channels: int, use_attention: bool = False, bias: bool = True, *, heads: int = 1, **kwargs):
        super().__init__()
        if use_attention:
            raise NotImplementedError("HypergraphConv: use_attention=True is not implemented (DESIGN.md §4.35)")
        if heads != 1:
            raise NotImplementedError("HypergraphConv: heads != 1 belongs to the attention mode, which is not implemented")
        if kwargs:
            raise NotImplementedError(f"HypergraphConv: unsupported arguments {sorted(kwargs)}")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.lin = torch.nn.Linear(self.in_channels, self.out_channels, bias=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))                 # glorot
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x: torch.Tensor, hyperedge_index: Optional[torch.Tensor] = None, hyperedge_weight: Optional[torch.Tensor] = None,
                hyperedge_attr=None, num_edges: Optional[int] = None, plan: Optional[IncidencePlan] = None) -> torch.Tensor:
        if hyperedge_attr is not None:
            raise NotImplementedError("HypergraphConv: hyperedge_attr belongs to the attention mode, which is not implemented")
        h = self.lin(x)
        if h.dtype in (torch.float16, torch.bfloat16):                       # autocast: the 16-bit kernels, the bias inside
            from . import hg16
            bias = None if self.bias is None else self.bias.float()           # a module cast as a whole: its bias is widened
            if plan is not None:
                return hg16.hypergraph_propagate_16(h, plan=plan, bias=bias)
            return hg16.hypergraph_propagate_16(h, hyperedge_index, num_edges=num_edges, hyperedge_weight=hyperedge_weight, bias=bias)
        if plan is not None:
            out = hypergraph_propagate(h, plan=plan)
        else:
            out = hypergraph_propagate(h, hyperedge_index, num_edges=num_edges, hyperedge_weight=hyperedge_weight)
        return out if self.bias is None else out + self.bias

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"
