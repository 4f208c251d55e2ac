"""VR-GCN [Chen, Zhu and Song, "Stochastic Training of Graph Convolutional Networks with Variance Reduction", ICML 2018]: the
project's GCN trained on a NeighborSampler batch with the control-variate estimator over historical activations, on the gfx950
kernels of csrc/vrgcn_kernels.hip (ops.vrgcn_aggregate_fwd / _bwd).

Every term is taken over a loop-free graph (VRGraph): d_u = the stored entries of row u, dinv_u = (d_u + 1)^-1/2,
P = D^-1/2 (A + I) D^-1/2, duplicate entries counting once each.  A model of L layers keeps for l = 1 .. L - 1 a history Hbar^(l),
fp32 [N, hidden_l] on global rows, zero at first (HistoryStore).  Layer l + 1 >= 2 computes, for the rows u it has to produce and the
k_u = min(d_u, fanout) entries the sampler kept of each,

    A[u] = dinv_u^2 H[loc u] + (d_u / k_u) sum_{kept v} dinv_u dinv_v (H[loc v] - Hbar[v]) + sum_{every entry v of row u} dinv_u dinv_v Hbar[v]
    Z[u] = A[u] W^T + b

with H = H^(l) on the batch's local rows (loc = rank in node_idx) and Hbar = Hbar^(l) a constant for autograd.  The first layer's
history is X itself, so it is exact: Z[u] = (P X)[u] W^T + b, with P X computed once (VRGraph.propagate) and gathered per step.
Each level computes only the rows the next one reads: layers[d].prev of the batch (d = 0 next to the output).  The histories are
written by the caller AFTER the forward (HistoryStore.update), with the post-ReLU activations of exactly the computed rows.
Dropout is not built (the paper's estimator under dropout is another one).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Sequence

import torch

from .. import ops
from .gcn import GCN, _LinearFn


class VRGraph:
    """What the estimator reads of a loop-free DeviceGraph: rowptr / col, dinv = (d + 1)^-1/2 (fp32 [N]) and the largest row."""

    def __init__(self, graph):
        self.graph = graph
        self.rowptr, self.col, self.num_nodes = graph.rowptr, graph.col, graph.num_nodes
        deg = graph.rowptr[1:] - graph.rowptr[:-1]
        self.dinv = (deg + 1).to(torch.float64).rsqrt().to(torch.float32).contiguous()
        self.max_degree = graph.max_degree

    def propagate(self, x):
        """P x for every node, by the full-graph aggregation (the graph is symmetric: its CSR is the CSR by target)."""
        return ops.gcn_aggregate_fwd(x.contiguous(), self.graph.gcn_prepared())


class HistoryStore:
    """HistoryStore(N, widths, device): one fp32 [N, widths[l - 1]] table per level l = 1 .. len(widths), zero at construction,
    indexed by global node id."""

    def __init__(self, num_nodes: int, widths: Sequence[int], device):
        self.num_nodes = int(num_nodes)
        self.tables = [torch.zeros((self.num_nodes, int(w)), dtype=torch.float32, device=device) for w in widths]

    def __getitem__(self, level: int) -> torch.Tensor:
        return self.tables[level - 1]

    def update(self, level: int, node_idx, rows_local, H):
        """Hbar^(level)[node_idx[r]] = H[r] for r in rows_local (int32 local ids); H: [n_local, width] on the batch's local rows."""
        if rows_local.numel() == 0:
            return
        ids = node_idx[rows_local.long()].contiguous()
        ops.scatter_rows(self.tables[level - 1], ids, ops.gather_rows(H.detach().contiguous(), rows_local.contiguous()))

    def reset(self):
        for t in self.tables:
            t.zero_()


class VRGCNLayerFn(torch.autograd.Function):
    """A = the control-variate aggregate of h [n_local, f] for the rows of `lay` (a namespace: node_idx, dinv, rowptr, col, rows_g,
    rows_l, prep, pos, item_cap, status); hbar [N, f] is a constant: its gradient is None."""

    @staticmethod
    def forward(ctx, h, hbar, lay):
        out, coef = ops.vrgcn_aggregate_fwd(h, lay.node_idx, hbar, lay.dinv, lay.rowptr, lay.col, lay.rows_g, lay.rows_l, lay.prep,
                                            item_cap=lay.item_cap, status=lay.status)
        ctx.lay, ctx.coef = lay, coef
        return out

    @staticmethod
    def backward(ctx, da):
        lay = ctx.lay
        dh = ops.vrgcn_aggregate_bwd(da.contiguous(), ctx.coef, lay.pos, lay.node_idx, lay.dinv, lay.prep, status=lay.status)
        return dh, None, None


class _ToLocalRows(torch.autograd.Function):
    """out [n_local, f] = 0 with out[ids[r]] = rows[r] (ids duplicate-free); backward: the gather of those rows."""

    @staticmethod
    def forward(ctx, rows, ids, n_local):
        ctx.ids = ids
        out = torch.zeros((n_local, rows.shape[1]), dtype=torch.float32, device=rows.device)
        return ops.scatter_rows(out, ids, rows.contiguous())

    @staticmethod
    def backward(ctx, dout):
        return ops.gather_rows(dout.contiguous(), ctx.ids), None, None


class _KeptEntries:
    """A layer's kept entries over the batch's local ids as both CSRs (the fields of ops.PreparedGraph the kernels read); a layer
    without an entry has empty rows."""

    def __init__(self, edge_index, n_local: int, status):
        self.n, self.status = n_local, status
        if edge_index.shape[1]:
            prep = ops.PreparedGraph(edge_index[0].contiguous(), edge_index[1].contiguous(), n_local, status=status)
            self.rowptr_t, self.csr_src, self.rowptr_s, self.csr_dst = prep.rowptr_t, prep.csr_src, prep.rowptr_s, prep.csr_dst
        else:
            dev = edge_index.device
            self.rowptr_t = self.rowptr_s = torch.zeros(n_local + 1, dtype=torch.int32, device=dev)
            self.csr_src = self.csr_dst = torch.zeros(1, dtype=torch.int32, device=dev)


def local_ids(node_idx, rows):
    """The ranks (int32) of the global ids `rows` in the ascending node_idx."""
    return torch.searchsorted(node_idx, rows).to(torch.int32)


def layer_inputs(vg: VRGraph, batch, d: int, status=None) -> SimpleNamespace:
    """What VRGCNLayerFn takes for the batch's layer d: the rows layers[d].prev in global and local ids, the layer's kept entries
    prepared over local ids, pos (a local node's position among the rows, or -1) and the long rows' chunk count."""
    rows_g = batch.layers[d].prev.contiguous()
    rows_l = local_ids(batch.node_idx, rows_g)
    n_local, m = batch.num_nodes, rows_g.numel()
    pos = torch.full((n_local,), -1, dtype=torch.int32, device=rows_g.device)
    pos[rows_l.long()] = torch.arange(m, dtype=torch.int32, device=rows_g.device)
    item_cap = ops.vrgcn_item_cap(vg.rowptr, rows_g) if vg.max_degree > ops.VRGCN_LONG_ROW else 0
    return SimpleNamespace(node_idx=batch.node_idx, dinv=vg.dinv, rowptr=vg.rowptr, col=vg.col, rows_g=rows_g, rows_l=rows_l,
                           prep=_KeptEntries(batch.edge_index[d], n_local, status), pos=pos, item_cap=item_cap, status=status)


def vrgcn_forward(model: GCN, batch, px, store: HistoryStore, vg: VRGraph, status=None):
    """(logits [B, C] on the targets' rows in the targets' order, acts) of the estimator with the model's weights
    (gcn_layers.i.lin.weight, .bias); px = P X [N, F] (VRGraph.propagate).  acts: per level l = 1 .. L - 1 the tuple
    (l, rows_local, H^(l) on the batch's local rows, detached) to push into the history after the step's forward."""
    if not isinstance(model, GCN):
        raise TypeError("vrgcn_forward runs the project's GCN")
    if model.dropout != 0.0:
        raise ValueError("VR-GCN with dropout is not built (the paper's estimator under dropout is another one)")
    convs = model.gcn_layers
    L = len(convs)
    if L != len(batch.layers):
        raise ValueError(f"vrgcn_forward: {L} layers take a batch of {L} sampled layers, not {len(batch.layers)}")
    rows = batch.layers[L - 1].prev.contiguous()
    z = _LinearFn.apply(ops.gather_rows(px, rows), convs[0].lin.weight, convs[0].bias, L > 1)      # exact: the history of X is X
    acts = []
    for i in range(1, L):
        rows_l = local_ids(batch.node_idx, rows)
        h = _ToLocalRows.apply(z, rows_l, batch.num_nodes)
        acts.append((i, rows_l, h.detach()))
        lay = layer_inputs(vg, batch, L - 1 - i, status)
        a = VRGCNLayerFn.apply(h, store[i], lay)
        z = _LinearFn.apply(a, convs[i].lin.weight, convs[i].bias, i < L - 1)
        rows = lay.rows_g
    return z, acts
