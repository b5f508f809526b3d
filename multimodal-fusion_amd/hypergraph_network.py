"""The hypergraph branch of the reference's model on this library: ``HypergraphNetwork`` with the constructor
signature, the forward and the state-dict keys of downstream_survival/models/cust_omics.py:11-110, built from ``hgconv.HypergraphConv``
and ``readout.GlobalAttention``.

    first_h (Linear, BatchNorm1d, ReLU) -> dropout -> [HypergraphConv -> dropout] x (len(hidden_dims) - 1) -> output_layer -> attention_pool

    net = HypergraphNetwork(input_dim, [256, 256], output_dim)
    net.load_state_dict(torch.load("reference_checkpoint.pt"))          # the keys are the reference module's
    token = net(x, edge_index, batch)                                    # [batch_size, output_dim]; batch = zeros for one slide

One incidence plan is built per forward and shared by every conv layer; ``incidence=`` / ``readout=`` take plans the caller keeps
across calls and epochs.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

from . import hgconv, readout as readout_mod

__all__ = ["HypergraphNetwork"]


class HypergraphNetwork(torch.nn.Module):
    """State-dict keys: first_h.0.{weight,bias}, first_h.1.{weight,bias,running_mean,running_var,num_batches_tracked},
    convs.{i}.lin.weight, convs.{i}.bias, output_layer.{weight,bias}, attention_pool.gate_nn.0.{weight,bias},
    attention_pool.gate_nn.2.{weight,bias}.  ``use_attention=True`` raises NotImplementedError (hgconv.HypergraphConv).
    As in the reference, the gate network takes hidden_dims[-1] inputs but reads the output layer's result, so a forward needs
    output_dim == hidden_dims[-1] (the reference runs 256 / 256); the shapes are kept so that its checkpoints load."""

    def __init__(self, input_dim: int, hidden_dims: List[int], output_dim: int, dropout: float = 0.2, use_attention: bool = False):
        super().__init__()
        hidden_dims = list(hidden_dims)
        if not hidden_dims:
            raise ValueError("HypergraphNetwork: hidden_dims must name at least one layer")
        self.dropout = dropout
        self.hidden_dims = hidden_dims
        self.num_layers = len(hidden_dims)
        self.first_h = torch.nn.Sequential(torch.nn.Linear(input_dim, hidden_dims[0]), torch.nn.BatchNorm1d(hidden_dims[0]), torch.nn.ReLU())
        self.convs = torch.nn.ModuleList(hgconv.HypergraphConv(hidden_dims[i - 1], hidden_dims[i], use_attention=use_attention)
                                         for i in range(1, self.num_layers))
        self.output_layer = torch.nn.Linear(hidden_dims[-1], output_dim)
        gate_nn = torch.nn.Sequential(torch.nn.Linear(hidden_dims[-1], hidden_dims[-1] // 2), torch.nn.Tanh(),
                                      torch.nn.Linear(hidden_dims[-1] // 2, 1))
        self.attention_pool = readout_mod.GlobalAttention(gate_nn=gate_nn)

    def forward(self, x: torch.Tensor, edge_index: Optional[torch.Tensor] = None, batch: Optional[torch.Tensor] = None, *,
                incidence: Optional[hgconv.IncidencePlan] = None, readout: Optional[readout_mod.ReadoutPlan] = None,
                return_attention: bool = False):
        """x [N, input_dim]; edge_index int64 [2, E] (row 1 the hyperedge id); batch [N] the sorted graph id of every node (None: one
        graph).  ``incidence`` / ``readout``: ready plans, used in place of edge_index / batch (which may then be None).  Returns the
        graph tokens [batch_size, output_dim], with ``return_attention=True`` also the weight of every node."""
        if incidence is None and edge_index is None:
            raise ValueError("HypergraphNetwork: pass edge_index or incidence")
        if readout is not None:
            batch = None                                                      # a plan given: it is the description (as for incidence)
        h = self.first_h(x)
        h = F.dropout(h, p=self.dropout, training=self.training)
        if incidence is None and len(self.convs):
            incidence = hgconv.incidence_plan(edge_index, x.shape[0])         # one plan for every layer
        for conv in self.convs:
            h = conv(h, plan=incidence)
            h = F.dropout(h, p=self.dropout, training=self.training)
        h = self.output_layer(h)
        return self.attention_pool(h, batch, plan=readout, return_attention=return_attention)
