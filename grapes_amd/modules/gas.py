"""GNNAutoScale, "GAS" [Fey, Lenssen, Weichert and Leskovec, ICML 2021; pyg_autoscale-recall: ScalableGNN, History, SubgraphLoader]:
the project's GCN trained on cluster batches whose rows aggregate their WHOLE global neighbourhood, on the gfx950 kernels of
csrc/gas_kernels.hip (ops.gas_resolve, ops.gas_aggregate_fwd / _bwd).  The paper and the library are recalled, not read: the rule
written in include/grapes_hip.h is the contract.

Cluster-GCN discards every edge that leaves the batch; GAS keeps them all.  An in-batch neighbour contributes its current
activation, an out-of-batch neighbour the last activation pushed for it into a per-level history table (modules.vrgcn.HistoryStore).
Nothing is sampled and no edge is dropped: the forward is exact once the histories are fresh.

Every term is taken over a loop-free symmetric graph (modules.vrgcn.VRGraph): d_u = the stored entries of row u, dinv_u =
(d_u + 1)^-1/2, P = D^-1/2 (A + I) D^-1/2.  A batch is ClusterLoader.batch's: n rows, node_idx[i] = the global id of row i.  Once per
batch every entry of every batch row is resolved to a code — the local row of an in-batch neighbour, -1 - v for an out-of-batch v.
The first layer is exact, the history of X being X: Z1 = (P X)[node_idx] W1^T + b1.  Layer l + 1 >= 2 computes, for every row,

    A[i] = dinv_u (dinv_u H[i] + sum_t dinv_{v_t} (code_t >= 0 ? H[code_t] : Hbar[-1 - code_t]))        Z = A W^T + b

with H = H^(l) on the batch's rows and Hbar = Hbar^(l) a constant for autograd, read in place: no halo is materialised and nothing is
concatenated.  The backward runs over the batch's induced entries.  The histories are written by the caller AFTER the forward
(push), with the post-ReLU activations of all n rows; in-batch nodes never read their own history inside a step.  Dropout is not
built.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from .. import ops
from .cluster import _E_CEIL, _E_FLOOR, ClusterData, ClusterLoader
from .gcn import GCN, _LinearFn
from .vrgcn import HistoryStore, VRGraph, _KeptEntries


class GasLoader:
    """GasLoader(cluster_data, batch_size, seed=None): a ClusterLoader over `cluster_data` (built on the loop-free graph) whose
    batches also carry
      rowptr_h  int32 [n + 1]: the prefix sum of the rows' global degrees;
      code      int32 [rowptr_h[n]]: every entry of every row, the local row of an in-batch neighbour or -1 - v;
      num_in, num_halo: the in-batch and the out-of-batch entries;
      prep      the batch's induced entries (edge_index) prepared once, for the backward of every layer;
      item_cap  the chunks of the rows longer than ops.VRGCN_LONG_ROW entries.
    The code buffer starts near the last batch's size; a batch that does not fit is resolved again into one that does (rowptr_h[n]
    reports the total).  This is the eager form: batch() reads counts on the host."""

    def __init__(self, cluster_data: ClusterData, batch_size: int, seed: Optional[int] = None):
        self.loader = ClusterLoader(cluster_data, batch_size, seed=seed)
        self.cluster_data, self.status = cluster_data, self.loader.status
        self._h_hint = _E_FLOOR

    def __len__(self) -> int:
        return len(self.loader)

    def batch(self, clusters) -> SimpleNamespace:
        """ClusterLoader.batch(clusters) with the fields above added."""
        ld, cd = self.loader, self.cluster_data
        g = cd.graph
        b = ld.batch(clusters)
        n = b.num_nodes
        if n < 1:
            raise ValueError("GasLoader.batch: the chosen clusters hold no node")
        # the items of the batch's rows: at most the chosen clusters' (ClusterData.items bounds any batch of them)
        item_cap = min(max(1, int(cd.items[b.clusters.long()].sum().item())), ops.GAS_ITEM_CAP_MAX)
        hc = self._h_hint
        while True:
            rowptr_h, code, counts = ops.gas_resolve(g.rowptr, g.col, g.num_nodes, b.node_idx, n, cd.where, ld.stamp, ld.serial, hc,
                                                     item_cap=item_cap, status=self.status)
            total = int(rowptr_h[n].item())                          # the rows' entries (host read)
            if total <= hc or hc >= _E_CEIL:
                break
            self.status.bitwise_and_(~1)                             # the buffer was too small: the same batch into one that fits
            hc = min(max(total, 2 * hc), _E_CEIL)
        self._h_hint = max(_E_FLOOR, min(total + total // 4, _E_CEIL))
        num_in, num_halo = (int(v) for v in counts.tolist())
        b.rowptr_h, b.code, b.num_in, b.num_halo = rowptr_h, code[:total], num_in, num_halo
        b.prep = _KeptEntries(b.edge_index, n, self.status)
        b.item_cap = ops.gas_item_cap(rowptr_h) if int((rowptr_h[1:] - rowptr_h[:-1]).max()) > ops.VRGCN_LONG_ROW else 0
        return b

    def __iter__(self):
        order = torch.randperm(self.cluster_data.num_parts, generator=self.loader._gen)
        for i in range(0, order.numel(), self.loader.batch_size):
            yield self.batch(order[i:i + self.loader.batch_size])

    def check(self):
        self.loader.check()


class GasLayerFn(torch.autograd.Function):
    """A = the GAS aggregate of h [n, f] over the batch `lay` (a namespace: node_idx, dinv, rowptr_h, code, prep, item_cap, status);
    hbar [N, f] is a constant: its gradient is None."""

    @staticmethod
    def forward(ctx, h, hbar, lay):
        ctx.lay = lay
        return ops.gas_aggregate_fwd(h, hbar, lay.dinv, lay.node_idx, lay.rowptr_h, lay.code, item_cap=lay.item_cap, status=lay.status)

    @staticmethod
    def backward(ctx, da):
        lay = ctx.lay
        return ops.gas_aggregate_bwd(da.contiguous(), lay.node_idx, lay.dinv, lay.prep, status=lay.status), None, None


def gas_forward(model: GCN, batch, px, store: HistoryStore, vg: VRGraph, status=None):
    """(logits [n, C] on the batch's rows, acts) with the model's weights (gcn_layers.i.lin.weight, .bias); px = P X [N, F]
    (VRGraph.propagate), batch a GasLoader batch.  acts: per level l = 1 .. L - 1 the pair (l, H^(l) on the batch's rows, detached)
    to push into the history after the step's forward (push)."""
    if not isinstance(model, GCN):
        raise TypeError("gas_forward runs the project's GCN")
    if model.dropout != 0.0:
        raise ValueError("GAS with dropout is not built")
    convs = model.gcn_layers
    L = len(convs)
    lay = SimpleNamespace(node_idx=batch.node_idx, dinv=vg.dinv, rowptr_h=batch.rowptr_h, code=batch.code, prep=batch.prep,
                          item_cap=batch.item_cap, status=status)
    z = _LinearFn.apply(ops.gather_rows(px, batch.node_idx), convs[0].lin.weight, convs[0].bias, L > 1)   # exact: the history of X is X
    acts = []
    for i in range(1, L):
        acts.append((i, z.detach()))
        a = GasLayerFn.apply(z, store[i], lay)
        z = _LinearFn.apply(a, convs[i].lin.weight, convs[i].bias, i < L - 1)
    return z, acts


def push(store: HistoryStore, batch, acts) -> None:
    """Hbar^(l)[node_idx] = H^(l) for every level of `acts` (gas_forward's), all n rows of the batch."""
    for level, h in acts:
        ops.scatter_rows(store[level], batch.node_idx, h)
