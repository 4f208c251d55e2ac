"""LINKX [Lim et al., NeurIPS 2021; PyG-recall: LINKX, SparseLinear — the rules in include/grapes_hip.h are the contract] on the gfx950
kernels of csrc/bag_kernels.hip (ops.bag_batch, ops.bag_fwd, ops.bag_bwd, ops.bag_bwd_adam).  A node's row of the adjacency matrix is
a feature vector of length N pushed through a learned table,

    h_A[i] = b + sum_{j in row(i)} W_A[j],

so nothing is sampled: a batch is m rows of A.  The table's gradient is row-sparse — a batch touches the columns its rows store and
no other — and is never materialised densely.

BagBatcher(graph).batch(rows) returns a namespace: rows int32 [m] (= node_idx = targets: the trainer gathers their feature rows;
local_targets = arange(m)), bptr int32 [m + 1], uniq int32 [num_unique] — the ascending distinct columns, the indices of the sparse
gradient — tptr int32 [num_unique + 1] and trow int32 [num_entries] — per column the batch rows that store it, ascending;
seg_max / row_max: the longest segment and row; graph; check().

AdjacencyBag is the layer, BagAdam the fused lazy Adam of its table, LINKX the model.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
from torch import nn

from .. import ops
from .._lib import GrapesHipError
from .sampling import _graph_of, as_targets, raise_on_status

GRADS = ("fused", "sparse")


class BagBatcher:
    """BagBatcher(data_or_graph).  batch(rows): rows are node ids (any integer tensor, at most ops.BAG_MAX_ROWS, in the given order;
    ids may repeat, each occurrence is its own batch row).  The capacities start from the last batch's and grow on an overflow,
    whose true totals the kernel reports (as GasLoader retries): one host read per try."""

    def __init__(self, data_or_graph):
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("BagBatcher: a graph with 2^31 or more entries is not built")
        self.status = torch.zeros(1, dtype=torch.int32, device=g.device)
        self._scratch = (g.bits, g.node_map)                         # (the graph's frontier bitmap is zero at rest, and left so)
        self._u_cap, self._e_cap = 1024, 4096

    def batch(self, rows) -> SimpleNamespace:
        g = self.graph
        rows = as_targets(rows, g.device, type(self).__name__)
        m = rows.numel()
        if m > ops.BAG_MAX_ROWS:
            raise ValueError(f"BagBatcher.batch: at most {ops.BAG_MAX_ROWS} rows per batch")
        for _ in range(3):
            bptr, uniq, tptr, trow, counts = ops.bag_batch(g.rowptr, g.col, g.num_nodes, rows, self._scratch, self._u_cap, self._e_cap,
                                                           status=self.status)
            n_u, e, seg_max, row_max = counts.tolist()               # (the host read)
            if n_u <= self._u_cap and e <= self._e_cap:
                break
            self.status.bitwise_and_(~3)                             # (the two overflow bits: the retry has the room)
            self._u_cap = max(self._u_cap, min(n_u + n_u // 4, g.num_nodes), 1)
            self._e_cap = max(self._e_cap, e + e // 4)
        else:
            raise GrapesHipError("BagBatcher.batch: the batch does not fit the capacities its own totals asked for")
        return SimpleNamespace(rows=rows, node_idx=rows, targets=rows, local_targets=torch.arange(m, dtype=torch.int32, device=g.device),
                               bptr=bptr, uniq=uniq[:n_u], tptr=tptr[:n_u + 1], trow=trow[:e], num_unique=n_u, num_entries=e,
                               seg_max=seg_max, row_max=row_max, graph=g, check=self.check)

    sample = batch

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError("LINKX batcher: ...") on a bad id and clears it."""
        if int(self.status.item()):
            self.graph.bits.zero_()
        raise_on_status(self.status, "LINKX batcher")


class _BagFn(torch.autograd.Function):
    """out = bias + A[rows] W (ops.bag_fwd).  Backward: d bias = the column sums of G; d W is row-sparse — a sparse COO tensor built from
    ops.bag_bwd (grad="sparse"), or nothing at all while (batch, G) waits for BagAdam (grad="fused")."""

    @staticmethod
    def forward(ctx, weight, bias, batch, bag):
        ctx.batch, ctx.bag, ctx.has_bias = batch, bag, bias is not None
        g = batch.graph
        return ops.bag_fwd(g.rowptr, g.col, g.num_nodes, batch.rows, weight.detach(), None if bias is None else bias.detach(),
                           item_cap=ops.bag_fwd_item_cap(batch.num_entries, batch.row_max))

    @staticmethod
    def backward(ctx, G):
        b, bag = ctx.batch, ctx.bag
        G = G.contiguous()
        db = G.sum(0) if ctx.has_bias else None
        if bag.grad == "fused":
            bag._pending = (b, G)
            return None, db, None, None
        N, H = bag.weight.shape
        if b.num_unique == 0:
            return torch.sparse_coo_tensor(torch.zeros((1, 0), dtype=torch.int64, device=G.device),
                                           torch.zeros((0, H), device=G.device), (N, H)), db, None, None
        vals = ops.bag_bwd(G, b.tptr, b.trow, b.num_unique, b.num_entries, item_cap=ops.bag_bwd_item_cap(b.num_entries, b.seg_max))
        return torch.sparse_coo_tensor(b.uniq.long()[None], vals, (N, H), is_coalesced=True), db, None, None


class AdjacencyBag(nn.Module):
    """AdjacencyBag(num_nodes, out_channels, bias=True, grad="fused"|"sparse"): weight [N, H] and bias [H], initialised as PyG's
    SparseLinear (uniform in +-1 / sqrt(N)).  forward(batch) takes a BagBatcher batch and returns [m, H].
    grad="sparse": weight.grad is a torch.sparse_coo_tensor (indices batch.uniq, coalesced), which torch.optim.SparseAdam takes.
    grad="fused": weight gets no gradient; the pair (batch, d out) is kept for BagAdam.step(), which forms the segment sums and
    applies the update in one pass."""

    def __init__(self, num_nodes: int, out_channels: int, bias: bool = True, grad: str = "fused"):
        super().__init__()
        if grad not in GRADS:
            raise ValueError(f"AdjacencyBag: grad={grad!r} is not built (built: fused, sparse)")
        if int(num_nodes) < 1 or not ops.gather_width_ok(int(out_channels)):
            raise ValueError(f"AdjacencyBag: {out_channels} columns is not a width the gathers are built for (any up to 256, multiples "
                             "of 4 up to 1024), and num_nodes is at least 1")
        self.num_nodes, self.out_channels, self.grad = int(num_nodes), int(out_channels), grad
        bound = 1.0 / float(self.num_nodes) ** 0.5
        self.weight = nn.Parameter(torch.empty(self.num_nodes, self.out_channels).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.empty(self.out_channels).uniform_(-bound, bound)) if bias else None
        self._pending = None

    def forward(self, batch):
        if batch.graph.num_nodes != self.num_nodes:
            raise ValueError("AdjacencyBag: the batch's graph has another number of nodes than the table")
        return _BagFn.apply(self.weight, self.bias, batch, self)

    def embed(self, graph, rows, item_cap=None):
        """The forward alone over rows of `graph`, no batch tables and no gradient (inference)."""
        return ops.bag_fwd(graph.rowptr, graph.col, graph.num_nodes, rows, self.weight.detach(),
                           None if self.bias is None else self.bias.detach(), item_cap=item_cap)


class BagAdam:
    """BagAdam(bag, lr, betas=(0.9, 0.999), eps=1e-8): torch.optim.SparseAdam's rule for the table of an AdjacencyBag(grad="fused"),
    applied by ops.bag_bwd_adam to the rows the pending batch touched — lazy semantics: a row outside the batch's columns is neither
    read nor written, its moments do not decay; the step count t advances on every step().  step() raises when no backward has left
    a pair since the last step()."""

    def __init__(self, bag: AdjacencyBag, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        if not isinstance(bag, AdjacencyBag) or bag.grad != "fused":
            raise ValueError("BagAdam: the layer is an AdjacencyBag(grad=\"fused\")")
        if not (lr >= 0.0 and eps >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("BagAdam: lr and eps are not negative and the betas lie inside [0, 1)")
        self.bag, self.lr, self.betas, self.eps, self.t = bag, float(lr), (float(betas[0]), float(betas[1])), float(eps), 0
        self.exp_avg = torch.zeros_like(bag.weight.data)
        self.exp_avg_sq = torch.zeros_like(bag.weight.data)

    def zero_grad(self):
        self.bag.weight.grad = None
        self.bag._pending = None

    def step(self):
        if self.bag._pending is None:
            raise RuntimeError("BagAdam.step: no backward pass is pending (nothing ran since the last step, or it was consumed)")
        (b, G), self.bag._pending = self.bag._pending, None
        self.t += 1
        if b.num_unique:
            ops.bag_bwd_adam(G, b.tptr, b.trow, b.uniq, b.num_unique, b.num_entries, self.bag.weight.data, self.exp_avg, self.exp_avg_sq,
                             self.lr, self.betas[0], self.betas[1], self.eps, self.t,
                             item_cap=ops.bag_bwd_item_cap(b.num_entries, b.seg_max))


class _MLP(nn.Module):
    """Linear - ReLU - dropout stacks `lins` over the widths dims; the last layer is plain."""

    def __init__(self, dims, dropout: float):
        super().__init__()
        self.lins = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))
        self.dropout = float(dropout)

    def forward(self, x):
        for i, lin in enumerate(self.lins):
            if i:
                x = nn.functional.dropout(torch.relu(x), self.dropout, self.training)
            x = lin(x)
        return x


class LINKX(nn.Module):
    """LINKX(num_nodes, in_features, hidden, num_classes, num_node_layers=1, num_final_layers=2, dropout=0., grad="fused"), PyG's
    forward with one edge layer:
        out = edge_lin(batch);  out = out + cat_lin1(out);  x = node_mlp(xb);  out = out + x + cat_lin2(x);  final_mlp(relu(out))
    forward(xb, batch): xb the gathered feature rows [m, F] of batch.rows.  Keys: edge_lin.weight / .bias, node_mlp.lins.*, cat_lin1.*,
    cat_lin2.*, final_mlp.lins.*.  As in PyG the node MLP runs without dropout and the final MLP with `dropout`.  Normalisation
    layers and num_edge_layers > 1 are not built."""

    def __init__(self, num_nodes: int, in_features: int, hidden: int, num_classes: int, num_node_layers: int = 1,
                 num_final_layers: int = 2, dropout: float = 0.0, grad: str = "fused", num_edge_layers: int = 1, norm=None):
        super().__init__()
        if int(num_edge_layers) != 1:
            raise NotImplementedError("LINKX: num_edge_layers > 1 is not built (one adjacency embedding, no edge MLP behind it)")
        if norm is not None and norm is not False:
            raise NotImplementedError("LINKX: normalisation layers (batch_norm / norm) are not built")
        if min(int(in_features), int(hidden), int(num_classes), int(num_node_layers), int(num_final_layers)) < 1:
            raise ValueError("LINKX: every width and layer count is at least 1")
        H = int(hidden)
        self.edge_lin = AdjacencyBag(num_nodes, H, grad=grad)
        self.node_mlp = _MLP([int(in_features)] + [H] * int(num_node_layers), 0.0)
        self.cat_lin1 = nn.Linear(H, H)
        self.cat_lin2 = nn.Linear(H, H)
        self.final_mlp = _MLP([H] * int(num_final_layers) + [int(num_classes)], dropout)
        self.out_channels = int(num_classes)

    def dense_parameters(self):
        """Every parameter but the table: what the trainer's torch optimiser holds."""
        return [p for n, p in self.named_parameters() if n != "edge_lin.weight"]

    def head(self, out, xb):
        out = out + self.cat_lin1(out)
        x = self.node_mlp(xb)
        out = out + x + self.cat_lin2(x)
        return self.final_mlp(torch.relu(out))

    def forward(self, xb, batch):
        return self.head(self.edge_lin(batch), xb)
