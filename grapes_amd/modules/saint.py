"""Drop-in GraphSAINT samplers (PyG 2.5 loader/graph_saint.py; the reference imports GraphSAINTNodeSampler and
GraphSAINTRandomWalkSampler at graphsaint.py:8 and uses the latter at graphsaint.py:104) on the gfx950 kernels of
csrc/saint_kernels.hip.

Per batch (num_steps batches per epoch) a sampler draws node ids, node_idx = their ascending duplicate-free set, the induced
subgraph relabelled to local ids in CSR order (local row ascending, then local column ascending; stored self-loops stay), and
every node-sized tensor gathered at node_idx.  The three samplers differ in the draw alone:

* GraphSAINTRandomWalkSampler: B roots, B random walks of L steps (torch_cluster random_walk, p = q = 1); the ids are the
  B (L + 1) visited nodes (walks.view(-1)).
* GraphSAINTNodeSampler: B independent draws of a stored entry e uniform in [0, nnz); the id is the CSR row that holds e (PyG:
  adj.storage.row()[randint(0, E, (B,))] — a node is drawn in proportion to its row length, with replacement).
* GraphSAINTEdgeSampler: B independent draws of a stored entry e = (r, c) with probability proportional to the integer weight
  w_e = colcount[r] + rowcount[c] (PyG: prob = 1 / deg_in[row] + 1 / deg_out[col] with deg_in = 1 / colcount and
  deg_out = 1 / rowcount; deg(r) + deg(c) on a symmetric graph); both endpoints are ids.  PyG takes the top-1 of
  rand(B, E).log() / (prob + 1e-10) per row, which is one weighted draw per row: the distribution is built here, not the key
  arithmetic, and the 1e-10 is dropped — an entry of weight 0 is never drawn.

GraphSAINT's node / edge normalisation [PyG-recall: PyG 2.5 GraphSAINTSampler._compute_norm / __collate__] comes through
estimate_norm(sample_coverage), not through the constructors: they keep refusing sample_coverage > 0 (the reference runs with 0)
and name that method.  estimate_norm draws passes of num_steps batches with the sampler's own draw on its Philox stream while
total_sampled_nodes < N * sample_coverage (tested before each pass, so at least one runs), counting per batch node_count[v] += 1
over the node set and edge_count[j] += 1 over the stored entries j with both ends in it (ops.saint_coverage_count: integers,
exact), then forms
    edge_norm[j] = fp32(node_count[row(j)]) / fp32(edge_count[j]) clamped to [0, 1e4], 0 / 0 -> 0.1 (so x / 0 -> 1e4),
    node_norm[v] = (fp32(num_samples) / fp32(node_count[v])) / fp32(N), a count of 0 taken as 0.1
(ops.saint_norms).  Afterwards every batch also carries node_norm = node_norm[node_idx] ([n]), edge_id (int64 [E], the position in
col of every edge, in the batch's edge order) and edge_norm = edge_norm[edge_id] ([E]) — what modules.gcn.GCNConv.forward(...,
edge_weight=) and ops.saint_masked_loss(..., node_norm=) take.  Without the call batches are what they were.

The draws come from the project's Philox stream (seed, device offset): see ops.saint_walk_nodes, ops.saint_draw_nodes and DESIGN.md.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from .. import ops
from .sampling import _graph_of, draw_seed, raise_on_status


class _SaintSampler:
    """What the three samplers share.  Iterable of `num_steps` batches.  data_or_graph: a DeviceGraph, or a data object with
    edge_index (or rowptr / col) and num_nodes (x, y and *_mask are then gathered into every batch).  Each batch has node_idx
    (int64), num_nodes, edge_index (local, int64, [2, E], on the device) and the data's node-sized tensors at node_idx.
    seed: the Philox key (None: drawn from torch's generator).  e_cap: edge capacity of a batch (None: n_cap squared, capped at
    the graph's entry count — no batch can exceed it); more edges set a status bit that check() raises on.
    A subclass gives n_cap (the ids of one batch), draw() and the names of the draw's own arrays a batch carries (_extras)."""

    _extras = ()

    def __init__(self, data_or_graph, batch_size: int, num_steps: int, sample_coverage: int, seed: Optional[int],
                 e_cap: Optional[int], n_cap: int, limit: str):
        if sample_coverage:
            raise NotImplementedError("GraphSAINT normalisation does not come through the constructor's sample_coverage (the "
                                      "reference, graphsaint.py:104, passes 0): build the sampler without it and call "
                                      "estimate_norm(sample_coverage)")
        self.batch_size, self.num_steps, self.n_cap = int(batch_size), int(num_steps), int(n_cap)
        if self.n_cap > ops.SAINT_MAX_IDS:
            raise ValueError(f"{limit} must be at most {ops.SAINT_MAX_IDS}")
        self.graph, self.data = _graph_of(data_or_graph)
        dev = self.graph.device
        self.e_cap = int(e_cap) if e_cap is not None else max(1, min(self.n_cap * self.n_cap, self.graph.nnz))
        self.seed = draw_seed(seed)
        self.philox_offset = torch.zeros(1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        # set by estimate_norm
        self.sample_coverage, self.num_samples, self.total_sampled_nodes = 0, 0, 0
        self.node_count = self.edge_count = self.node_norm = self.edge_norm = None

    def weights(self):
        """The draw's one-time table (the edge sampler's alone)."""
        return None

    def estimate_norm(self, sample_coverage: int):
        """GraphSAINT's coverage estimate and the two norm vectors (the module docstring has the rules).  Each batch is a draw and
        one counting launch; nothing is read back but the running total, once per pass.  Keeps node_count / edge_count (int32
        tensors holding the uint32 counts), num_samples, total_sampled_nodes, node_norm [N], edge_norm [nnz] and sample_coverage;
        from then on batches carry their norms.  Returns self."""
        cov = int(sample_coverage)
        if cov <= 0:
            raise ValueError(f"estimate_norm: sample_coverage must be positive, not {sample_coverage!r}")
        g = self.graph
        self.weights()                                   # the edge sampler's table is built first, as before a first draw
        counts = None
        num_samples = total = 0
        while total < g.num_nodes * cov:
            for _ in range(self.num_steps):
                d = self.draw()
                counts = ops.saint_coverage_count(g.rowptr, g.col, g.num_nodes, d["node_idx"], d["count"], g.node_map, out=counts)
            num_samples += self.num_steps
            total = int(counts[2].item())
        self.node_count, self.edge_count = counts[0], counts[1]
        self.num_samples, self.total_sampled_nodes, self.sample_coverage = num_samples, total, cov
        self.edge_norm, self.node_norm = ops.saint_norms(g.rowptr, g.num_nodes, self.node_count, self.edge_count, num_samples)
        return self

    def __len__(self):
        return self.num_steps

    def draw(self, *inject, out=None, **kw):
        """The batch's ids and their set, on the device: dict with node_idx (int32 [n_cap]), count and the sampler's own arrays.
        inject: arrays that replace the Philox draws (tests).  out: the tensors to write (captured steps)."""
        raise NotImplementedError

    def draw_buffers(self):
        """Zeroed tensors for draw(out=...): what a captured step keeps."""
        raise NotImplementedError

    def sample(self, *inject, **kw):
        """One batch's device arrays (no host read): the dict of draw() plus edge_src / edge_dst (int32 [e_cap]), e_count,
        rowptr_l; after estimate_norm also edge_id (int64 [e_cap]), edge_norm (fp32 [e_cap], the edges' norms) and node_norm
        (fp32 [N], the whole table: a kernel reads it through node_idx)."""
        g = self.graph
        d = self.draw(*inject, **kw)
        src, dst, d_e, rowptr_l, *ids = ops.saint_subgraph(g.rowptr, g.col, d["node_idx"], d["count"], g.node_map, self.e_cap,
                                                           edge_norm=self.edge_norm, status=self.status)
        d.update(edge_src=src, edge_dst=dst, e_count=d_e, rowptr_l=rowptr_l)
        if ids:
            d.update(edge_id=ids[0], edge_norm=ids[1], node_norm=self.node_norm)
        return d

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError on an edge overflow or a bad id, and clears it."""
        raise_on_status(self.status, "GraphSAINT sampler", hints={1: " (raise e_cap)", 2: None})

    def batch(self, *inject, **kw) -> SimpleNamespace:
        """One batch in PyG's form (two host reads: the node and edge counts)."""
        s = self.sample(*inject, **kw)
        self.check()
        n, e = int(s["count"].item()), int(s["e_count"].item())
        node_idx = s["node_idx"][:n].long()
        out = SimpleNamespace(node_idx=node_idx, num_nodes=n, edge_index=torch.stack([s["edge_src"][:e], s["edge_dst"][:e]]).long(),
                              **{k: s[k] for k in self._extras})
        if "edge_id" in s:
            out.node_norm, out.edge_norm, out.edge_id = s["node_norm"][node_idx], s["edge_norm"][:e], s["edge_id"][:e]
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


class GraphSAINTRandomWalkSampler(_SaintSampler):
    """B roots and their random walks of walk_length steps; n_cap = B (L + 1).  See _SaintSampler for the arguments and a batch's
    fields; a batch also carries walks (int32 [B, L + 1])."""

    _extras = ("walks",)

    def __init__(self, data_or_graph, batch_size: int, walk_length: int, num_steps: int = 1, sample_coverage: int = 0,
                 seed: Optional[int] = None, e_cap: Optional[int] = None):
        self.walk_length = int(walk_length)
        super().__init__(data_or_graph, batch_size, num_steps, sample_coverage, seed, e_cap,
                         int(batch_size) * (self.walk_length + 1), "batch_size * (walk_length + 1)")

    def draw_buffers(self):
        i32 = dict(dtype=torch.int32, device=self.graph.device)
        return (torch.zeros((self.batch_size, self.walk_length + 1), **i32), torch.zeros(self.n_cap, **i32), torch.zeros(1, **i32))

    def draw(self, roots=None, uniforms=None, out=None):
        g = self.graph
        walks, node_idx, count = ops.saint_walk_nodes(g.rowptr, g.col, g.num_nodes, self.batch_size, self.walk_length,
                                                      roots=roots, uniforms=uniforms, philox_seed=self.seed,
                                                      d_philox_offset=None if roots is not None else self.philox_offset,
                                                      node_map=g.node_map, status=self.status, out=out)
        return dict(walks=walks, node_idx=node_idx, count=count)


class _SaintEntrySampler(_SaintSampler):
    """The node and edge samplers: B draws of a stored entry, one integer t in [0, total) each.  A batch also carries ids (int32,
    the drawn node ids in draw order) and entries (int64 [B], the drawn entries' positions in col).
    draws: int64 [B] values t that replace the Philox draws; a value outside [0, total) sets the bad-index status bit."""

    _extras = ("ids", "entries")
    _ids_per_draw = 1

    def __init__(self, data_or_graph, batch_size: int, num_steps: int = 1, sample_coverage: int = 0, seed: Optional[int] = None,
                 e_cap: Optional[int] = None):
        k = self._ids_per_draw
        super().__init__(data_or_graph, batch_size, num_steps, sample_coverage, seed, e_cap, k * int(batch_size),
                         "batch_size" if k == 1 else f"{k} * batch_size")
        if self.graph.nnz <= 0:
            raise ValueError(f"{type(self).__name__}: the graph has no stored entry to draw")

    def draw_buffers(self):
        dev = self.graph.device
        return (torch.zeros(self.n_cap, dtype=torch.int32, device=dev), torch.zeros(self.n_cap, dtype=torch.int32, device=dev),
                torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(self.batch_size, dtype=torch.int64, device=dev))

    def draw(self, draws=None, out=None):
        g = self.graph
        ids, node_idx, count, entries = ops.saint_draw_nodes(g.rowptr, g.col, g.num_nodes, self.batch_size, weights=self.weights(),
                                                             draws=draws, philox_seed=self.seed,
                                                             d_philox_offset=None if draws is not None else self.philox_offset,
                                                             node_map=g.node_map, status=self.status, out=out)
        return dict(ids=ids, entries=entries, node_idx=node_idx, count=count)


class GraphSAINTNodeSampler(_SaintEntrySampler):
    """PyG's GraphSAINTNodeSampler(data, batch_size, num_steps, sample_coverage=0): B draws of a stored entry uniform in
    [0, nnz), the drawn node being the row that holds it (degree-proportional, with replacement); n_cap = B.  rowptr is the
    draw's cumulative table, so nothing is precomputed."""


class GraphSAINTEdgeSampler(_SaintEntrySampler):
    """PyG's GraphSAINTEdgeSampler(data, batch_size, num_steps, sample_coverage=0): B draws of a stored entry (r, c) in proportion
    to colcount[r] + rowcount[c]; both endpoints join the node set; n_cap = 2 B.  The weight table (ops.saint_edge_weights) is
    built at the first use and kept; building it reads the total weight once, and a graph whose total weight is 0 (no node has
    both a stored row entry and a stored column entry) raises ValueError there — an empty graph already at construction.
    Fewer than 2^31 stored entries (the weights are 32-bit)."""

    _ids_per_draw = 2

    def __init__(self, data_or_graph, batch_size: int, num_steps: int = 1, sample_coverage: int = 0, seed: Optional[int] = None,
                 e_cap: Optional[int] = None):
        super().__init__(data_or_graph, batch_size, num_steps, sample_coverage, seed, e_cap)
        if self.graph.nnz >= 2 ** 31:
            raise ValueError("GraphSAINTEdgeSampler: the entry weights are 32-bit: fewer than 2^31 stored entries")
        self._weights = None

    def weights(self):
        """(colcount, blockw, roww) of ops.saint_edge_weights, built once (one host read: the total weight)."""
        if self._weights is None:
            g = self.graph
            w = ops.saint_edge_weights(g.rowptr, g.col, g.num_nodes, status=self.status)
            if int(w[2][-1].item()) <= 0:
                raise ValueError("GraphSAINTEdgeSampler: every stored entry has weight 0 (no node has both a stored row entry "
                                 "and a stored column entry)")
            self._weights = w
        return self._weights


SAMPLERS = {"rw": GraphSAINTRandomWalkSampler, "node": GraphSAINTNodeSampler, "edge": GraphSAINTEdgeSampler}


def make_sampler(kind: str, data_or_graph, batch_size: int, walk_length: int = 2, **kw):
    """The sampler `kind` (rw | node | edge); walk_length is the random-walk sampler's alone."""
    if kind not in SAMPLERS:
        raise ValueError(f"sampler must be one of {', '.join(SAMPLERS)}, not {kind!r}")
    if kind == "rw":
        return GraphSAINTRandomWalkSampler(data_or_graph, batch_size, walk_length, **kw)
    return SAMPLERS[kind](data_or_graph, batch_size, **kw)
