"""The adaptive layer-wise sampler of AS-GCN [AS-GCN-recall: Huang et al., "Adaptive Sampling Towards Fast Graph Representation
Learning", NeurIPS 2018: the layer-wise sampler with the self-dependent function g(x(u_j))], the one baseline of the reference's
analysis/significance.py whose sampler is learned, on the gfx950 kernels of csrc/asgcn_kernels.hip, the LADIES set work of
modules/ladies.py and the project's exact-k draw.

Notation is that of modules/ladies.py: V = A + I over the DeviceGraph CSR (a stored (i, i) makes v_ii = 2), P = D^-1 V,
D_i = deg_i + 1; layers are drawn from the targets inward, prev_0 = the targets as given.  The sampler's parameters are w_g
(fp32 [F], initialised as nn.Linear(F, 1)'s weight) and b_g (fp32 [1], zero).

Per layer d, m = |prev_d|:
  1. candidates = the ascending union of prev_d and its neighbours (LADIES step 1);
  2. per candidate j (ops.asgcn_importance, one wavefront each): a_j = <x_j, w_g> + b_g, g_j = max(a_j, 0) + 1,
     c_j = sum_{i in prev_d} P_ij (the paper's sum_i p(u_j | v_i), > 0), q_j = c_j g_j, logq_j = logf(q_j),
     logit_j = (logq_j - max_k logq_k) - 20 <= -20, where log sigmoid(l) = l in fp32: ops.gumbel_topk (mode 0) on these logits
     samples without replacement in proportion to q.  The sampler kernels are untouched;
  3. s = min(#candidates, samp_num) of them through the draw (all of them, and no stream advance, when there are no more than
     samp_num); after_d = the ascending union of the sampled nodes and the targets;
  4. ops.ladies_layer with the table holding q: w_ij = (v_ij / q_j) / sum_{j' kept} (v_ij' / q_j');
  5. prev_{d + 1} = after_d.

Where this departs from the paper (the project's LADIES conventions, taken where the paper leaves a choice or differs): nodes are
sampled WITHOUT replacement; the targets are forced into every layer; the weights are row-normalised (the estimator is the
self-normalised one) instead of divided by q alone.  The paper's skip connections and its node-wise variant are not built.

A batch is a LADIES batch (modules/ladies.py) plus, per layer, c, a, q, logq and logit over its candidates, and per batch `a` (the
kernel's a over node_idx, which the trainer's ReLU mask reads) and `local_prev` (per layer the rows' ranks in node_idx).
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import torch
from torch import nn

from .. import ops
from .ladies import LayerWiseSampler


class AdaptiveSampler(nn.Module, LayerWiseSampler):
    """AdaptiveSampler(data_or_graph, samp_num, num_layers, in_features, seed=None, e_cap=None): an nn.Module owning w_g and b_g;
    the other arguments, the Philox stream and check() are LayerWiseSampler's."""

    def __init__(self, data_or_graph, samp_num: int, num_layers: int, in_features: int, seed: Optional[int] = None,
                 e_cap: Optional[int] = None):
        nn.Module.__init__(self)
        LayerWiseSampler.__init__(self, data_or_graph, samp_num, num_layers, kind="ladies", seed=seed, e_cap=e_cap)
        self._name = "asgcn"                                             # (check()'s message; kind stays "ladies": that branch of sample())
        if int(in_features) < 1:
            raise ValueError("AdaptiveSampler: in_features is at least 1")
        self.in_features = int(in_features)
        dev = self.graph.device
        w = torch.empty(1, self.in_features)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))                      # nn.Linear(F, 1).weight
        self.w_g = nn.Parameter(w.reshape(-1).to(dev))
        self.b_g = nn.Parameter(torch.zeros(1, device=dev))
        self.a_table = torch.zeros(self.graph.num_nodes, dtype=torch.float32, device=dev)

    def sample(self, targets, x, uniforms=None) -> SimpleNamespace:
        """targets, uniforms: as LayerWiseSampler.sample, whose set work, draw and layer kernel this runs.  x: fp32 [N, F], the node
        features the importance reads.  Returns the LADIES namespace (pi = q) with c, a, q, logq, logit per layer, and `a` /
        `local_prev` per batch (module docstring)."""
        if x.shape[0] != self.graph.num_nodes or x.shape[1] != self.in_features:
            raise ValueError(f"AdaptiveSampler.sample: x is [{self.graph.num_nodes}, {self.in_features}]")
        self._x = x
        try:
            return LayerWiseSampler.sample(self, targets, uniforms)
        finally:
            self._x = None

    def _importance(self, cand, m: int):
        g = self.graph
        c, a, q, logq, logit = ops.asgcn_importance(g.rowptr, self.rowptr_t, self.col_t, g.num_nodes, self._x, self.w_g.detach(),
                                                    self.b_g.detach(), ids=cand, prev_bits=g.prev_bits, m=m, q_table=self.pi_table,
                                                    a_table=self.a_table, status=self.status)
        return q, logit, dict(c=c, a=a, q=q, logq=logq)

    def _batch_fields(self, node_idx, layers) -> dict:
        return dict(local_prev=[ops.tensormap_map(self.graph.node_map, L.prev.contiguous()) for L in layers],
                    a=self.a_table[node_idx.long()])
