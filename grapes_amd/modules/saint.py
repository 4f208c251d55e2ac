"""Drop-in ``GraphSAINTRandomWalkSampler`` (PyG 2.5, used at reference graphsaint.py:104) on the gfx950 kernels of
csrc/saint_kernels.hip.

Per batch (num_steps batches per epoch): B roots, B random walks of L steps (torch_cluster random_walk, p = q = 1),
node_idx = walks.view(-1).unique() (ascending), the induced subgraph relabelled to local ids in CSR order (local row ascending,
then local column ascending; stored self-loops stay), and every node-sized tensor gathered at node_idx.  sample_coverage > 0
(GraphSAINT's node / edge normalisation) is not built: the reference runs with sample_coverage 0.

The draws come from the project's Philox stream (seed, device offset): see ops.saint_walk_nodes and DESIGN.md.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from .. import ops


def _graph_of(data_or_graph):
    from ..graph import DeviceGraph
    if isinstance(data_or_graph, DeviceGraph):
        return data_or_graph, None
    g = getattr(data_or_graph, "graph", None)
    if isinstance(g, DeviceGraph):
        return g, data_or_graph
    dev = torch.device("cuda", torch.cuda.current_device())
    if getattr(data_or_graph, "rowptr", None) is not None:
        g = DeviceGraph(data_or_graph.rowptr.to(dev), data_or_graph.col.to(dev), int(data_or_graph.num_nodes))
    else:
        g = DeviceGraph.from_edge_index(data_or_graph.edge_index.to(dev), int(data_or_graph.num_nodes), device=dev)
    return g, data_or_graph


class GraphSAINTRandomWalkSampler:
    """Iterable of `num_steps` batches.  data_or_graph: a DeviceGraph, or a data object with edge_index (or rowptr / col) and
    num_nodes (x, y and *_mask are then gathered into every batch).  Each batch has node_idx (int64), num_nodes, edge_index
    (local, int64, [2, E], on the device) and the data's node-sized tensors at node_idx.
    seed: the Philox key (None: drawn from torch's generator).  e_cap: edge capacity of a batch (None: B (L + 1) squared, capped
    at the graph's entry count — no batch can exceed it); more edges set a status bit that check() raises on."""

    def __init__(self, data_or_graph, batch_size: int, walk_length: int, num_steps: int = 1, sample_coverage: int = 0,
                 seed: Optional[int] = None, e_cap: Optional[int] = None):
        if sample_coverage:
            raise NotImplementedError("GraphSAINT normalisation (sample_coverage > 0) is not built; the reference "
                                      "(graphsaint.py:104) uses sample_coverage=0")
        self.batch_size, self.walk_length, self.num_steps = int(batch_size), int(walk_length), int(num_steps)
        if self.batch_size * (self.walk_length + 1) > ops.SAINT_MAX_IDS:
            raise ValueError(f"batch_size * (walk_length + 1) must be at most {ops.SAINT_MAX_IDS}")
        self.graph, self.data = _graph_of(data_or_graph)
        dev = self.graph.device
        self.n_cap = self.batch_size * (self.walk_length + 1)
        self.e_cap = int(e_cap) if e_cap is not None else max(1, min(self.n_cap * self.n_cap, self.graph.nnz))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.seed = int(seed)
        self.philox_offset = torch.zeros(1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def __len__(self):
        return self.num_steps

    def sample(self, roots=None, uniforms=None):
        """One batch's device arrays (no host read): dict of walks, node_idx (int32 [n_cap]), count, edge_src / edge_dst
        (int32 [e_cap]), e_count, rowptr_l."""
        g = self.graph
        walks, node_idx, count = ops.saint_walk_nodes(g.rowptr, g.col, g.num_nodes, self.batch_size, self.walk_length,
                                                      roots=roots, uniforms=uniforms, philox_seed=self.seed,
                                                      d_philox_offset=None if roots is not None else self.philox_offset,
                                                      node_map=g.node_map, status=self.status)
        src, dst, d_e, rowptr_l = ops.saint_subgraph(g.rowptr, g.col, node_idx, count, g.node_map, self.e_cap, status=self.status)
        return dict(walks=walks, node_idx=node_idx, count=count, edge_src=src, edge_dst=dst, e_count=d_e, rowptr_l=rowptr_l)

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError on an edge overflow or a bad id, and clears it."""
        s = int(self.status.item())
        if s:
            self.status.zero_()
            bits = [n for b, n in ((1, "edge buffer overflow (raise e_cap)"), (4, "index out of range")) if s & b]
            raise ops._lib.GrapesHipError("GraphSAINT sampler: " + ", ".join(bits))

    def batch(self, roots=None, uniforms=None) -> SimpleNamespace:
        """One batch in PyG's form (two host reads: the node and edge counts)."""
        s = self.sample(roots, uniforms)
        self.check()
        n, e = int(s["count"].item()), int(s["e_count"].item())
        node_idx = s["node_idx"][:n].long()
        out = SimpleNamespace(node_idx=node_idx, num_nodes=n, walks=s["walks"],
                              edge_index=torch.stack([s["edge_src"][:e], s["edge_dst"][:e]]).long())
        if self.data is not None:
            for k in ("x", "y", "train_mask", "val_mask", "test_mask"):
                t = getattr(self.data, k, None)
                if t is not None:
                    t = t.to(node_idx.device)
                    setattr(out, k, ops.gather_rows(t, s["node_idx"][:n]) if (k == "x" and t.dtype == torch.float32 and
                                                                              t.dim() == 2 and t.is_contiguous()) else t[node_idx])
        return out

    def __iter__(self):
        for _ in range(self.num_steps):
            yield self.batch()
