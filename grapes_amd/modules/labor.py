"""LABOR, the layer-neighbour sampler [Balin and Catalyurek, NeurIPS 2023; LABOR-recall: DGL's LaborSampler(fanouts,
importance_sampling=i, layer_dependency=...)] on the gfx950 kernels of csrc/labor_kernels.hip (ops.labor_sample_layer,
ops.labor_importance).  The paper is recalled, not read: the rule written here and in include/grapes_hip.h is the contract.

It is neighbour sampling's per-row estimator with ONE uniform r_t per candidate vertex t, shared by every row that sees t.  Rows
therefore agree on which neighbours to keep, and a layer's union of sources is far smaller than under independent per-row draws.

Layers are drawn from the targets inward, exactly as modules.sage.NeighborSampler draws them: d = 0 is the layer next to the output,
prev_0 = the targets as given, fanouts[0] belongs to the hop next to the output;
  1. layer d keeps entries of the rows of prev_d (source = the neighbour, target = the row, in prev_d's order and within a row in
     the CSR's order; duplicates are separate entries, a stored loop is an ordinary entry);
  2. prev_{d + 1} = the ascending union of prev_d and the kept sources.
For layer d, fanout k, row s with d_s = deg(s) stored entries, entry t:
  variates     r_t = 32-bit word t & 3 of philox4x32_10(base + (t >> 2), seed), t the GLOBAL node id; base = philox_offset +
               d ceil(N / 4) (layer_dependency=False), or philox_offset for every layer (True, DGL's option: a vertex kept in one
               layer is likely kept in the next).  sample() advances philox_offset by num_layers ceil(N / 4) in both settings.
  LABOR-0      (importance_iters = 0) d_s <= k keeps every entry; else t is kept iff (uint64) r_t d_s < (uint64) k << 32: probability
               k / d_s, integers only.
  LABOR-i      (importance_iters = i >= 1) from pi = 1: c_s(pi) solves sum_t 1 / min(1, c pi_t) = d_s^2 / k for a row with d_s > k;
               one iteration is pi_t <- pi_t max_{s in prev_d, d_s > k, t in N(s)} c_s(pi); after i of them c_s is solved once more
               and t is kept iff (r_t >> 8) 2^-24 < p_st = fminf(1, c_s pi_t).  Rows with d_s <= k have p = 1.
  weights      (Hajek) w_st = (1 / p_st) / sum_{t' kept in row s} (1 / p_st'); LABOR-0: 1 / kept_s.  A row that keeps nothing has no
               entry.
A fanout of -1 is the expansion with weights 1 / d_s.

A batch has NeighborSampler's fields — node_idx, num_nodes, targets, local_targets, edge_index (per layer a local int32 [2, e_d] list,
row 0 the sources), layers (prev, after, edge_src, edge_dst, edge_pos, fanout; plus edge_weight, and c / pi under importance) — plus
edge_weight (one fp32 vector per layer) and uniform (importance_iters == 0: every kept entry of a row weighs the same, so a mean over
them is the Hajek estimator).  Each layer reads two counts on the host: this is the eager form.  The DeviceGraph's bitmaps and the
sampler's N-sized scratch are zero again when sample() returns.

Not built: a captured step, multi-GPU forms, DGL's batch_dependency, sequential Poisson (exact-k) sampling.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from .. import ops
from .sampling import InwardSampler

_EVERY = 2 ** 31 - 1                # the fanout of a -1 layer: past every degree


class LaborSampler(InwardSampler):
    """LaborSampler(data_or_graph, fanouts, importance_iters=0, layer_dependency=False, seed=None).  data_or_graph: a DeviceGraph, or
    a data object as the GraphSAINT samplers take.  fanouts: one entry per layer, fanouts[0] next to the output; -1 keeps every
    neighbour, else 1 .. ops.SAGE_MAX_FANOUT.  importance_iters: 0 .. ops.LABOR_MAX_ITERS.  seed: the Philox key of the draws (None:
    from torch's generator)."""

    _KIND = "layer-neighbour"

    def __init__(self, data_or_graph, fanouts: Sequence[int], importance_iters: int = 0, layer_dependency: bool = False,
                 seed: Optional[int] = None):
        self.importance_iters = int(importance_iters)
        if not 0 <= self.importance_iters <= ops.LABOR_MAX_ITERS:
            raise ValueError(f"LaborSampler: importance_iters {importance_iters} is not built (0 .. {ops.LABOR_MAX_ITERS})")
        self.layer_dependency = bool(layer_dependency)
        super().__init__(data_or_graph, fanouts, seed)
        self.scratch = ops.labor_scratch(self.graph.num_nodes, self.graph.device) if self.importance_iters else None

    def layer_base(self, d: int) -> int:
        """The Philox counter of node 0's variates in layer d of the NEXT sample() call."""
        return self.philox_offset + (0 if self.layer_dependency else d * ((self.graph.num_nodes + 3) // 4))

    def _layer(self, d, k, prev, eoff, deg_sum, keys):
        g = self.graph
        c = pi = None
        if self.importance_iters and k != -1:
            c, pi = ops.labor_importance(g.rowptr, g.col, g.num_nodes, prev, k, self.importance_iters, self.scratch, status=self.status)
        src, dst, pos, w, d_l = ops.labor_sample_layer(g.rowptr, g.col, g.num_nodes, prev, _EVERY if k == -1 else k, keys=keys,
                                                       philox_seed=self.seed, philox_base=self.layer_base(d), c=c, pi=pi,
                                                       deg_sum=deg_sum, want_pos=k != -1, status=self.status)
        return dict(edge_src=src, edge_dst=dst, edge_pos=pos, edge_weight=w, c=c, pi=pi), d_l   # (a -1 layer: no edge_pos, rows whole)

    def _empty_layer(self, dev):
        return dict(super()._empty_layer(dev), edge_weight=torch.zeros(0, dtype=torch.float32, device=dev), c=None, pi=None)

    def sample(self, targets, keys=None) -> SimpleNamespace:
        """targets: node ids (any integer tensor; taken in the given order).  keys: per layer one int32 table of N words indexed by
        GLOBAL node id — one word per node, not per entry — replacing the layer's variates (tests); None entries and layers past the
        list draw from the stream.  Returns the batch namespace described in the module docstring."""
        batch = super().sample(targets, keys)
        self.philox_offset += self.num_layers * ((self.graph.num_nodes + 3) // 4)
        batch.edge_weight = [L.edge_weight for L in batch.layers]
        batch.uniform = self.importance_iters == 0
        return batch
