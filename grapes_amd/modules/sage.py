"""GraphSAGE's node-wise neighbour sampler [Hamilton et al., NeurIPS 2017; PyG-recall: NeighborLoader(num_neighbors=[25, 10])] on
the gfx950 kernel of csrc/sage_kernels.hip (ops.sage_sample_layer): for each row of a layer keep at most `fanout` of its stored
neighbours, uniformly without replacement.

Layers are drawn from the targets inward, as the layer-wise samplers of modules.ladies do: d = 0 is the layer next to the output,
prev_0 = the targets as given;
  1. layer d keeps min(deg_i, fanouts[d]) entries of every row i of prev_d (fanout -1: every entry) — source = the neighbour,
     target = the row, in prev_d's order and within a row in the CSR's order;
  2. prev_{d + 1} = the ascending union of prev_d and the kept sources.
So fanouts[0] belongs to the hop next to the output, as in PyG's num_neighbors.  The draw's rule (which entries are kept for a
Philox stream or for given keys) is the kernel's, stated in include/grapes_hip.h; a layer consumes ceil(sum deg / 4) counters.

A batch has the fields of a LADIES batch without the weights: node_idx = the ascending union of the targets and every layer's
sources, num_nodes, targets, local_targets, edge_index = per layer a local int32 [2, e_d] list (row 0 the sources) — GCN's routing
(edge_index[-i] for hidden layer i, [0] for the last) applies as is — and layers (prev, after, edge_src and edge_dst in global ids,
edge_pos = the kept entries' positions in col; None for a -1 layer, which keeps its rows whole).
Each layer reads two counts on the host (the rows' entry count and the kept count): this is the eager form.  The DeviceGraph's
bitmaps are zero again when sample() returns.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from .. import ops
from .sampling import _graph_of, as_targets, draw_seed, local_edge_lists, raise_on_status, union_of_lists


def check_fanouts(fanouts: Sequence[int]) -> "list[int]":
    """The fanouts as a list of ints: each -1 (every neighbour) or 1 .. ops.SAGE_MAX_FANOUT; at least one layer."""
    out = [int(k) for k in fanouts]
    if not out:
        raise ValueError("NeighborSampler: at least one fanout")
    for k in out:
        if k != -1 and not 1 <= k <= ops.SAGE_MAX_FANOUT:
            raise ValueError(f"NeighborSampler: fanout {k} is not built (-1 for every neighbour, or 1 .. {ops.SAGE_MAX_FANOUT})")
    return out


class NeighborSampler:
    """NeighborSampler(data_or_graph, fanouts, seed=None).  data_or_graph: a DeviceGraph, or a data object as the GraphSAINT
    samplers take.  fanouts: one entry per layer, fanouts[0] next to the output; -1 keeps every neighbour.  seed: the Philox key of
    the draws (None: from torch's generator); the stream position advances by ceil(sum deg / 4) counters per layer."""

    def __init__(self, data_or_graph, fanouts: Sequence[int], seed: Optional[int] = None):
        self.fanouts = check_fanouts(fanouts)
        self.num_layers = len(self.fanouts)
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("neighbour sampling over a graph with 2^31 or more entries is not built: the layer's entry offsets are "
                             "32-bit")
        self.seed, self.philox_offset = draw_seed(seed), 0
        self.status = torch.zeros(1, dtype=torch.int32, device=g.device)
        if ops.csr_symmetric_check(g.rowptr, g.col, g.num_nodes) & 2:
            raise ops._lib.GrapesHipError("NeighborSampler: a column id is outside [0, num_nodes)")

    def sample(self, targets, keys=None) -> SimpleNamespace:
        """targets: node ids (any integer tensor; taken in the given order).  keys: per layer one tensor of 32-bit words (int32 bit
        patterns), one per entry of the layer's rows in order, replacing the Philox words (tests); None entries and layers past the
        list draw from the stream.  Returns the batch namespace described in the module docstring."""
        g = self.graph
        dev, N = g.device, g.num_nodes
        targets = as_targets(targets, dev, "NeighborSampler")
        keys = list(keys) if keys is not None else []
        prev, layers = targets, []
        for d, k in enumerate(self.fanouts):
            m = prev.numel()
            eoff, d_e = ops.frontier_offsets(g.rowptr, prev)
            deg_sum = int(d_e.item())                                    # the rows' entry count (host read)
            if deg_sum >= 2 ** 31:
                raise ValueError("NeighborSampler.sample: a layer's rows hold 2^31 or more entries")
            if deg_sum == 0:
                empty = torch.zeros(0, dtype=torch.int32, device=dev)
                src, dst, pos = empty, empty, torch.zeros(0, dtype=torch.int64, device=dev)
            elif k == -1:                                                # every neighbour: the expansion itself
                dst, src, _ = ops.frontier_expand(g.rowptr, g.col, prev, eoff, deg_sum, status=self.status)
                pos = None                                               # (every entry of the rows, in order)
            else:
                kd = keys[d] if d < len(keys) else None
                src, dst, pos, d_l = ops.sage_sample_layer(g.rowptr, g.col, N, prev, k, e_cap=min(m * k, deg_sum), keys=kd,
                                                           philox_seed=self.seed, philox_offset=self.philox_offset,
                                                           deg_sum=deg_sum, status=self.status)
                e = int(d_l.item())                                      # the layer's entry count (host read)
                src, dst, pos = src[:e], dst[:e], pos[:e]
            if k != -1:
                self.philox_offset += (deg_sum + 3) // 4
            after = union_of_lists(g, [prev, src], self.status) if src.numel() else union_of_lists(g, [prev], self.status)
            layers.append(SimpleNamespace(prev=prev, after=after, edge_src=src, edge_dst=dst, edge_pos=pos, fanout=k))
            prev = after
        node_idx = prev                                  # the last union holds every earlier layer, and left node_map[id] = rank
        return SimpleNamespace(node_idx=node_idx, num_nodes=node_idx.numel(), targets=targets,
                               local_targets=ops.tensormap_map(g.node_map, targets), edge_index=local_edge_lists(g, layers, dev),
                               layers=layers)

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError on an edge overflow or a bad id, and clears it (and, as
        DeviceGraph.check_status does, the bitmaps a truncated batch may have left marked)."""
        raise_on_status(self.status, "neighbour sampler", graph=self.graph)
