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

from .. import ops
from .sampling import InwardSampler, check_fanouts  # noqa: F401  (check_fanouts: imported from here by its users)


class NeighborSampler(InwardSampler):
    """NeighborSampler(data_or_graph, fanouts, seed=None).  data_or_graph: a DeviceGraph, or a data object as the GraphSAINT
    samplers take.  fanouts: one entry per layer, fanouts[0] next to the output; -1 keeps every neighbour.  seed: the Philox key of
    the draws (None: from torch's generator); the stream position advances by ceil(sum deg / 4) counters per layer.
    sample(targets, keys=None): keys is per layer one tensor of 32-bit words (int32 bit patterns), one per entry of the layer's rows
    in order."""

    _KIND = "neighbour"

    def _layer(self, d, k, prev, eoff, deg_sum, keys):
        g = self.graph
        if k == -1:                                                      # every neighbour: the expansion itself
            dst, src, _ = ops.frontier_expand(g.rowptr, g.col, prev, eoff, deg_sum, status=self.status)
            return dict(edge_src=src, edge_dst=dst, edge_pos=None), None     # (every entry of the rows, in order)
        src, dst, pos, d_l = ops.sage_sample_layer(g.rowptr, g.col, g.num_nodes, prev, k, e_cap=min(prev.numel() * k, deg_sum),
                                                   keys=keys, philox_seed=self.seed, philox_offset=self.philox_offset,
                                                   deg_sum=deg_sum, status=self.status)
        self.philox_offset += (deg_sum + 3) // 4
        return dict(edge_src=src, edge_dst=dst, edge_pos=pos), d_l
