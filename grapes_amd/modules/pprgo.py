"""PPRGo [Bojchevski et al., KDD 2020 — recalled; the rules in include/grapes_hip.h are the contract] on the gfx950 kernels of
csrc/shadow_kernels.hip (ops.pprgo_topk) and csrc/pprgo_kernels.hip (ops.pprgo_batch, ops.pprgo_aggregate_fwd / _bwd): the decoupled
family — an MLP runs once per distinct node and a root's logits are the PPR-weighted sum of its k best nodes' rows,

    logits_b = sum_t weight[b, t] MLP(x)[nbr[b, t]].

There is no graph between a batch's nodes and no induced subgraph.

PPRGoSampler.sample(roots) returns a namespace: node_idx int32 [n] — the ascending union of the batch's nodes, whose feature rows
the trainer gathers; num_nodes = n; nbr int32 [m, K], score uint32 [m, K] (the fixed-point score in units of 2^-30) and cnt int32 [m] — the slot tables, K = k + 1,
slot 0 the root; weight fp32 [m, K]; loc int32 [m, K] — a slot's row among node_idx; tptr int32 [n + 1] and tslot int32 [E] — the
by-source inverted index the backward walks (num_slots = E; item_cap: the room its chunked form needs, 0 when no segment is long); targets = the roots, local_targets = arange(m): row b of the model's output is root b;
rounds, stop int32 [m] as ShaDowPPRSampler's.  Nothing is drawn: a batch is a function of the graph and the roots.

PPRGo is the model: an MLP of bias-free linear layers, then the aggregation.  PPRGo.propagate is the power-iteration inference.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence

import torch
from torch import nn

from .. import ops
from .._lib import GrapesHipError
from .sampling import _graph_of, as_targets, raise_on_status

NORMALIZATIONS = ("row", "sym", "col")


def _degrees(rowptr) -> torch.Tensor:
    """d_v = max(stored length of row v, 1) as fp32 (exact below 2^24)."""
    return (rowptr[1:] - rowptr[:-1]).clamp_(min=1).to(torch.float32)


class PPRGoSampler:
    """PPRGoSampler(data_or_graph, k=32, alpha=0.5, eps=1e-4, max_rounds=32, normalization="row").  alpha, eps, max_rounds and k as
    ShaDowPPRSampler takes them (alpha_q = round(alpha 2^16), thr = max(1, round(eps 2^30))); the push is that sampler's rule.
    normalization, with d_v = max(row length of v, 1) [PPRGo-recall for the names]:
        "row"   weight = float(score) 2^-30: the integer rounded once to fp32, the scaling exact
        "sym"   that times sqrt(d_b) / sqrt(d_v)
        "col"   that times d_b / d_v
    for root b and slot node v; a dead slot's weight is 0.  precompute(nodes) runs the push once and sample() then serves the roots
    it holds by row lookup — the scores depend on nothing that training changes."""

    def __init__(self, data_or_graph, k: int = 32, alpha: float = 0.5, eps: float = 1e-4, max_rounds: int = 32,
                 normalization: str = "row"):
        self.k, self.alpha, self.eps, self.max_rounds = int(k), float(alpha), float(eps), int(max_rounds)
        if not (self.alpha == self.alpha and self.eps == self.eps and 0.0 < self.alpha < 1.0 and 0.0 < self.eps <= 1.0):
            raise ValueError(f"PPRGoSampler: alpha = {alpha} must lie inside (0, 1) and eps = {eps} inside (0, 1]")
        if normalization not in NORMALIZATIONS:
            raise ValueError(f"PPRGoSampler: normalization={normalization!r} is not built (built: row, sym, col)")
        self.normalization = normalization
        self.alpha_q, self.thr = int(round(self.alpha * 2 ** 16)), max(1, int(round(self.eps * 2 ** 30)))
        self.K = ops.shadow_ppr_args(self.k, self.alpha_q, self.thr, self.max_rounds)
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("PPRGoSampler: a graph with 2^31 or more entries is not built")
        self.status = torch.zeros(1, dtype=torch.int32, device=g.device)
        self.symmetry = ops.csr_symmetric_check(g.rowptr, g.col, g.num_nodes)       # (bit 1: not symmetric, which the trainer refuses)
        if self.symmetry & 2:
            raise GrapesHipError("PPRGoSampler: a column id is outside [0, num_nodes)")
        self.deg = _degrees(g.rowptr)
        self._scratch = (g.bits, g.node_map)                         # (the graph's frontier bitmap is zero at rest, and left so)
        self._row = None                                             # node id -> row of the precomputed tables, -1 for none
        self._tables = None

    # ---------------------------------------------------------------------------------------------------------- the push
    def _topk(self, roots):
        g = self.graph
        return ops.pprgo_topk(g.rowptr, g.col, g.num_nodes, roots, self.k, self.alpha_q, self.thr, self.max_rounds, status=self.status)

    def precompute(self, nodes):
        """Runs the push for `nodes` (any integer tensor of distinct ids) in chunks of at most ops.PPRGO_MAX_ROOTS roots and keeps
        nbr / score / cnt / rounds / stop [len(nodes), ...] on the device; sample() then reads the rows of the roots found here."""
        g = self.graph
        nodes = as_targets(nodes, g.device, type(self).__name__)
        parts = [self._topk(nodes[i:i + ops.PPRGO_MAX_ROOTS]) for i in range(0, nodes.numel(), ops.PPRGO_MAX_ROOTS)]
        self.check()
        self._tables = tuple(torch.cat([p[j] for p in parts]) for j in range(5))
        self._row = torch.full((g.num_nodes,), -1, dtype=torch.int64, device=g.device)
        self._row[nodes.long()] = torch.arange(nodes.numel(), device=g.device)
        return self

    def _slots(self, roots):
        """The five slot tables of the roots: looked up where every root is precomputed, else pushed."""
        if self._row is not None:
            r = roots.long()
            rows = torch.where((r >= 0) & (r < self._row.numel()), self._row[r.clamp(0, self._row.numel() - 1)], -1)
            if bool((rows >= 0).all()):                              # (one host read)
                return tuple(t[rows].contiguous() for t in self._tables)
        return self._topk(roots)

    def _weight(self, roots, nbr, score, cnt):
        w = score.to(torch.float32) * (2.0 ** -30)
        if self.normalization != "row":
            K = nbr.shape[1]
            live = torch.arange(K, device=nbr.device)[None, :] < cnt[:, None]
            top = self.deg.numel() - 1                               # (a bad root has raised its status bit; its weights are 0)
            d_b = self.deg[roots.long().clamp(0, top)][:, None]
            d_v = self.deg[torch.where(live, nbr, roots[:, None]).long().clamp(0, top)]
            w = (w * torch.sqrt(d_b)) / torch.sqrt(d_v) if self.normalization == "sym" else (w * d_b) / d_v
        return w.contiguous()

    def sample(self, roots) -> SimpleNamespace:
        """roots: node ids (any integer tensor, at most ops.PPRGO_MAX_ROOTS, in the given order).  Returns the batch namespace of the
        module docstring.  One host read (n and E)."""
        g = self.graph
        roots = as_targets(roots, g.device, type(self).__name__)
        m = roots.numel()
        if m > ops.PPRGO_MAX_ROOTS:
            raise ValueError(f"PPRGoSampler.sample: at most {ops.PPRGO_MAX_ROOTS} roots per batch")
        nbr, score, cnt, rounds, stop = self._slots(roots)
        node_idx, loc, tptr, tslot, counts = ops.pprgo_batch(nbr, cnt, g.num_nodes, self._scratch, status=self.status)
        n, e, seg_max = counts.tolist()                              # the batch's rows, live slots and longest segment (the host read)
        return SimpleNamespace(node_idx=node_idx[:n], num_nodes=n, num_slots=e, item_cap=ops.pprgo_item_cap(e, seg_max), nbr=nbr,
                               score=_as_uint32(score), cnt=cnt,
                               weight=self._weight(roots, nbr, score, cnt), loc=loc, tptr=tptr[:n + 1], tslot=tslot[:e], targets=roots,
                               local_targets=torch.arange(m, dtype=torch.int32, device=g.device), rounds=rounds, stop=stop)

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError("PPRGo sampler: ...") on an overflow or a bad id, and clears it
        (the graph's bitmap is zeroed too: a truncated batch may have left marks)."""
        if int(self.status.item()):
            self.graph.bits.zero_()
        raise_on_status(self.status, "PPRGo sampler")


def _as_uint32(score):
    """The library's uint32 scores (held in int32 by ops: at most 2^30) under torch's uint32 dtype where this torch has one."""
    return score.view(torch.uint32) if hasattr(torch, "uint32") else score


class _PPRGoAggregateFn(torch.autograd.Function):
    """out[b] = sum_t weight[b, t] z[loc[b, t]] (ops.pprgo_aggregate_fwd); the backward walks the inverted index
    (ops.pprgo_aggregate_bwd).  The weights carry no gradient: scores are constants."""

    @staticmethod
    def forward(ctx, z, batch):
        ctx.batch = batch
        return ops.pprgo_aggregate_fwd(z.contiguous(), batch.weight, batch.loc, batch.cnt)

    @staticmethod
    def backward(ctx, g):
        b = ctx.batch
        return ops.pprgo_aggregate_bwd(g.contiguous(), b.weight, b.tptr, b.tslot, b.num_nodes, b.tslot.numel(),
                                       item_cap=getattr(b, "item_cap", None)), None


class PPRGo(nn.Module):
    """PPRGo(in_features, hidden_dims, dropout=0.): an MLP of nn.Linear(bias=False) layers `lins` with ReLU and dropout between them —
    the last entry of hidden_dims is the class count — then the PPR-weighted sum.  forward(xb, batch) takes the gathered feature rows
    [n, F] of batch.node_idx and a PPRGoSampler batch and returns logits [m, C], one row per root.  (Aggregating first where the
    hidden width is below the class count is not built: the MLP always runs over the n rows.)"""

    def __init__(self, in_features: int, hidden_dims: Sequence[int], dropout: float = 0.0):
        super().__init__()
        dims = [int(in_features)] + [int(d) for d in hidden_dims]
        if len(dims) < 2 or min(dims) < 1:
            raise ValueError("PPRGo: hidden_dims holds at least the class count, and every width is at least 1")
        if not ops.gather_width_ok(dims[-1]):
            raise ValueError(f"PPRGo: {dims[-1]} classes is not a width the gathers are built for (any up to 256, multiples of 4 up to 1024)")
        self.lins = nn.ModuleList(nn.Linear(a, b, bias=False) for a, b in zip(dims[:-1], dims[1:]))
        self.dropout = float(dropout)
        self.out_channels = dims[-1]

    def mlp(self, x):
        for i, lin in enumerate(self.lins):
            if i:
                x = nn.functional.dropout(torch.relu(x), self.dropout, self.training)
            x = lin(x)
        return x

    def forward(self, xb, batch):
        return _PPRGoAggregateFn.apply(self.mlp(xb), batch)

    @staticmethod
    def propagate(z, graph, alpha: float, nprop: int, normalization: str = "row"):
        """The power-iteration inference: Q_0 = Z, then Q <- (1 - alpha) S Q + alpha Z, nprop times, over the WHOLE graph.  S = D^-1 A
        ("row"), D^-1/2 A D^-1/2 ("sym") or A D^-1 ("col"), each as the mean aggregation ops.sage_aggregate_fwd(aggr="mean") over the
        full graph's preparation with its stored-self-loop counts (A as stored: loops and duplicates by multiplicity, as the push
        counts them; d = max(row length, 1)) between two ops.scale_rows by sqrt(d) or d.  graph: a symmetric DeviceGraph below 2^31
        entries.  Existing kernels only; z fp32 [N, C]; returns [N, C]."""
        if normalization not in NORMALIZATIONS:
            raise ValueError(f"PPRGo.propagate: normalization={normalization!r} is not built (built: row, sym, col)")
        if not 0.0 < float(alpha) < 1.0 or int(nprop) < 0:
            raise ValueError("PPRGo.propagate: alpha lies inside (0, 1) and nprop is at least 0")
        from .gcn import _gcn2_graph
        prep = _gcn2_graph(graph, graph.num_nodes)
        z = z.contiguous()
        post = pre = None
        C = z.shape[1]
        if normalization != "row":
            if C % 4:                                                # (ops.scale_rows takes float4 columns: zero columns up to a multiple of 4)
                z = torch.nn.functional.pad(z, (0, 4 - C % 4)).contiguous()
            d = _degrees(graph.rowptr)
            post = torch.sqrt(d) if normalization == "sym" else d
            pre = (1.0 / post).contiguous()
        q = z
        for _ in range(int(nprop)):
            s = ops.sage_aggregate_fwd(q if pre is None else ops.scale_rows(q, pre), prep, "mean")
            if post is not None:
                s = ops.scale_rows(s, post, out=s)
            q = s.mul_(1.0 - float(alpha)).add_(z, alpha=float(alpha))
        return q if q.shape[1] == C else q[:, :C].contiguous()
