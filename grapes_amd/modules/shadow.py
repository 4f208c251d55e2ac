"""ShaDow-GNN [Zeng et al., NeurIPS 2021; PyG-recall: ShaDowKHopSampler(data, depth, num_neighbors) over torch_sparse's
ego_k_hop_sample_adj, examples/shadow.py] on the gfx950 kernels of csrc/shadow_kernels.hip (ops.shadow_sample, ops.shadow_ppr_sample,
ops.segment_mean_fwd / _bwd).  The paper is recalled, not read: the rule written in include/grapes_hip.h is the contract.

The method decouples the model's depth from its scope.  Every root gets its OWN small sampled ego-net: `depth` hops from the root,
each expanding the nodes first reached at the hop before and keeping at most `num_neighbors` entries of an expanded row (Floyd's
algorithm on Philox words), then the subgraph induced on everything reached.  The batch is the disjoint union of the ego-nets, in root
order; a GNN of any number of layers runs on the union as on an ordinary edge list, and each root is read out of its own component.

A batch (ShaDowKHopSampler.sample) has
  node_idx       int32 [n]: the global id of every row, ascending within an ego-net (= PyG's n_id); a node reached from two roots has
                 two rows, so node_idx repeats ids across ego-nets;
  num_nodes      n;  targets = the roots as given;  local_targets = arange(B), the rows of the model's [B, C] logits;
  ptr            int32 [B + 1]: ego-net b holds the rows ptr[b] .. ptr[b + 1];  batch int32 [n]: the ego-net of each row;
  root_n_id      int32 [B]: the row of each root;
  edge_index     ONE int32 [2, e] tensor in row ids (row 0 the sources, the neighbours; row 1 the targets), ordered by ego-net, then
                 target row, then the CSR's order — one tensor, so that every layer of the model shares one cached preparation;
  e_id           int64 [e]: each entry's position in the graph's col.
sample() reads two counts on the host (n and e): this is the eager form.

ShaDowPPRSampler builds the same batch from the paper's other scope, the k best nodes of an approximate personalised PageRank from the
root (ops.shadow_ppr_sample: forward push in fixed point, no random numbers), and adds score, rounds and stop to the namespace.

ShaDow is the model: the project's SAGE or GCN as the body, the root's row (and the mean over its ego-net) as the readout, the
project's Linear as the head.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch
from torch import nn

from .. import ops
from .._lib import GrapesHipError
from ..target_batch import _GatherX
from .gcn import GCN, SAGE, Linear
from .sampling import _graph_of, as_targets, draw_seed, raise_on_status

_E_FLOOR = 1 << 14                  # the smallest edge buffer the sampler starts from
_E_CEIL = 2 ** 31 - 1


class ShaDowKHopSampler:
    """ShaDowKHopSampler(data_or_graph, depth, num_neighbors, seed=None, n_cap=None, e_cap=None).  data_or_graph: a DeviceGraph, or a
    data object as the GraphSAINT samplers take.  depth >= 1 hops; num_neighbors: 1 .. 64, one value for every hop (-1 is refused:
    the ego-net would be unbounded); 1 + k + ... + k^depth <= ops.SHADOW_MAX_NODES.  seed: the Philox key of the draws (None: from
    torch's generator); a call advances the stream offset by B * depth.  n_cap: the node buffer (default B * C, which cannot
    overflow).  e_cap: the edge buffer; by default it starts near the last batch's size and a batch that does not fit is drawn again
    — the same draw, the offset has not moved — into a buffer twice as large; a given e_cap is kept and an overflow raises at check()."""

    def __init__(self, data_or_graph, depth: int, num_neighbors: int, seed: Optional[int] = None, n_cap: Optional[int] = None,
                 e_cap: Optional[int] = None):
        self.depth, self.num_neighbors = int(depth), int(num_neighbors)
        self.cap = ops.shadow_cap(self.depth, self.num_neighbors)
        self.n_cap, self.e_cap = (None if n_cap is None else int(n_cap)), (None if e_cap is None else int(e_cap))
        if (self.n_cap is not None and self.n_cap < 1) or (self.e_cap is not None and self.e_cap < 1):
            raise ValueError("ShaDowKHopSampler: n_cap and e_cap are at least 1")
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("ego-net sampling over a graph with 2^31 or more entries is not built: an entry's position in a row is "
                             "drawn with a 32-bit word")
        self.seed, self.philox_offset = draw_seed(seed), 0
        self.status = torch.zeros(1, dtype=torch.int32, device=g.device)
        self._e_hint = _E_FLOOR
        if ops.csr_symmetric_check(g.rowptr, g.col, g.num_nodes) & 2:
            raise GrapesHipError("ShaDowKHopSampler: a column id is outside [0, num_nodes)")

    def sample(self, roots, words=None) -> SimpleNamespace:
        """roots: node ids (any integer tensor, at most ops.SHADOW_MAX_ROOTS; taken in the given order; a root listed twice gets two
        ego-nets).  words: int32 bit patterns [B, depth, num_neighbors] replacing the Philox words (tests).  Returns the batch
        namespace described in the module docstring."""
        g = self.graph
        roots = as_targets(roots, g.device, type(self).__name__)
        B = roots.numel()
        if B > ops.SHADOW_MAX_ROOTS:
            raise ValueError(f"ShaDowKHopSampler.sample: at most {ops.SHADOW_MAX_ROOTS} roots per batch")
        ec = self.e_cap if self.e_cap is not None else self._e_hint
        while True:
            n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e = ops.shadow_sample(
                g.rowptr, g.col, g.num_nodes, roots, self.depth, self.num_neighbors, n_cap=self.n_cap, e_cap=ec, words=words,
                philox_seed=self.seed, philox_offset=self.philox_offset, status=self.status)
            n, e = int(d_n.item()), int(d_e.item())                  # the batch's rows and entries (host reads)
            if self.e_cap is not None or e < ec or ec >= _E_CEIL or not int(self.status.item()) & 1:
                break
            self.status.bitwise_and_(~1)                             # the buffer was too small: the same draw into twice the room
            ec = min(2 * ec, _E_CEIL)
        if self.e_cap is None:
            self._e_hint = max(_E_FLOOR, min(e + e // 4, _E_CEIL))
        self.philox_offset += B * self.depth
        return SimpleNamespace(node_idx=n_id[:n], num_nodes=n, targets=roots,
                               local_targets=torch.arange(B, dtype=torch.int32, device=g.device), ptr=ptr, batch=batch[:n],
                               root_n_id=root_n_id, edge_index=ei[:, :e], e_id=e_id[:e])

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError("ego-net sampler: ...") on a node or edge overflow or a bad id,
        and clears it."""
        raise_on_status(self.status, "ego-net sampler", hints={1: " (give the sampler a larger e_cap)", 2: " (give it a larger n_cap)"})


class ShaDowPPRSampler:
    """ShaDowPPRSampler(data_or_graph, k, alpha=0.25, eps=2**-14, max_rounds=32, n_cap=None, e_cap=None): ShaDow's other scope.  The
    ego-net of a root is the root and the k best nodes of an approximate personalised PageRank from it — synchronous forward push in
    fixed point (the rule of grapes_shadow_ppr_sample in include/grapes_hip.h) — and the subgraph induced on them.  alpha: the teleport
    probability, taken as alpha_q = round(alpha 2^16) in 1 .. 65535; eps: the push threshold per stored entry (a node pushes while
    r_v >= eps deg(v)), taken as thr = max(1, round(eps 2^30)) in 1 .. 2^30; max_rounds: 1 .. 1024; k: 1 .. 1023.  Values outside
    are refused.  There is no seed and no offset: the scope is a function of the graph and the root.  n_cap / e_cap as
    ShaDowKHopSampler's (n_cap defaults to B (k + 1)).  A batch is ShaDowKHopSampler's namespace and additionally carries score fp32
    [n] (= the fixed-point score / 2^30: the integer rounded once to fp32, the division exact), rounds int32 [B] and stop int32 [B] (0: no node left to push, 1: max_rounds,
    2: the next round could overflow the ops.SHADOW_PPR_TOUCHED touched nodes)."""

    def __init__(self, data_or_graph, k: int, alpha: float = 0.25, eps: float = 2 ** -14, max_rounds: int = 32,
                 n_cap: Optional[int] = None, e_cap: Optional[int] = None):
        self.k, self.alpha, self.eps, self.max_rounds = int(k), float(alpha), float(eps), int(max_rounds)
        if not (self.alpha == self.alpha and self.eps == self.eps and 0.0 < self.alpha < 1.0 and 0.0 < self.eps <= 1.0):
            raise ValueError(f"ShaDowPPRSampler: alpha = {alpha} must lie inside (0, 1) and eps = {eps} inside (0, 1]")
        self.alpha_q, self.thr = int(round(self.alpha * 2 ** 16)), max(1, int(round(self.eps * 2 ** 30)))
        self.cap = ops.shadow_ppr_args(self.k, self.alpha_q, self.thr, self.max_rounds)
        self.n_cap, self.e_cap = (None if n_cap is None else int(n_cap)), (None if e_cap is None else int(e_cap))
        if (self.n_cap is not None and self.n_cap < 1) or (self.e_cap is not None and self.e_cap < 1):
            raise ValueError("ShaDowPPRSampler: n_cap and e_cap are at least 1")
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("ego-net sampling over a graph with 2^31 or more entries is not built")
        self.status = torch.zeros(1, dtype=torch.int32, device=g.device)
        self._e_hint = _E_FLOOR
        if ops.csr_symmetric_check(g.rowptr, g.col, g.num_nodes) & 2:
            raise GrapesHipError("ShaDowPPRSampler: a column id is outside [0, num_nodes)")

    def sample(self, roots) -> SimpleNamespace:
        """roots: node ids (any integer tensor, at most ops.SHADOW_MAX_ROOTS; taken in the given order; a root listed twice gets two
        identical ego-nets).  Returns the batch namespace described in the class docstring."""
        g = self.graph
        roots = as_targets(roots, g.device, type(self).__name__)
        B = roots.numel()
        if B > ops.SHADOW_MAX_ROOTS:
            raise ValueError(f"ShaDowPPRSampler.sample: at most {ops.SHADOW_MAX_ROOTS} roots per batch")
        ec = self.e_cap if self.e_cap is not None else self._e_hint
        while True:
            n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e, score, rounds, stop = ops.shadow_ppr_sample(
                g.rowptr, g.col, g.num_nodes, roots, self.k, self.alpha_q, self.thr, self.max_rounds, n_cap=self.n_cap, e_cap=ec,
                status=self.status)
            n, e = int(d_n.item()), int(d_e.item())                  # the batch's rows and entries (host reads)
            if self.e_cap is not None or e < ec or ec >= _E_CEIL or not int(self.status.item()) & 1:
                break
            self.status.bitwise_and_(~1)                             # the buffer was too small: the same scopes into twice the room
            ec = min(2 * ec, _E_CEIL)
        if self.e_cap is None:
            self._e_hint = max(_E_FLOOR, min(e + e // 4, _E_CEIL))
        return SimpleNamespace(node_idx=n_id[:n], num_nodes=n, targets=roots,
                               local_targets=torch.arange(B, dtype=torch.int32, device=g.device), ptr=ptr, batch=batch[:n],
                               root_n_id=root_n_id, edge_index=ei[:, :e], e_id=e_id[:e],
                               score=score[:n].to(torch.float32) * (2.0 ** -30), rounds=rounds, stop=stop)

    def check(self):
        """As ShaDowKHopSampler.check."""
        raise_on_status(self.status, "ego-net sampler", hints={1: " (give the sampler a larger e_cap)", 2: " (give it a larger n_cap)"})


class _SegmentMeanFn(torch.autograd.Function):
    """The mean of h over the row segments ptr (ops.segment_mean_fwd); the backward broadcasts g[b] / n_b to the segment's rows."""

    @staticmethod
    def forward(ctx, h, ptr):
        ctx.save_for_backward(ptr)
        ctx.n_rows = h.shape[0]
        return ops.segment_mean_fwd(h.contiguous(), ptr)

    @staticmethod
    def backward(ctx, g):
        (ptr,) = ctx.saved_tensors
        return ops.segment_mean_bwd(g.contiguous(), ptr, ctx.n_rows), None


class ShaDow(nn.Module):
    """ShaDow(in_features, hidden_dim, num_classes, num_layers, conv="sage" | "gcn", pool=True, dropout=0.).  The body is the project's
    SAGE (aggr="mean") or GCN with num_layers layers of hidden_dim columns — ReLU and dropout between them as those classes place them
    — in `body`; num_layers is independent of the sampler's depth.  The readout of root b is the body's row root_n_id[b], followed
    (pool=True) by the mean of the body's rows over ego-net b; `head` is the project's Linear over it.  forward(x, batch) takes the
    batch's gathered feature rows and a ShaDowKHopSampler batch and returns logits [B, num_classes], one row per root."""

    def __init__(self, in_features: int, hidden_dim: int, num_classes: int, num_layers: int, conv: str = "sage", pool: bool = True,
                 dropout: float = 0.):
        super().__init__()
        if conv not in ("sage", "gcn"):
            raise NotImplementedError(f"ShaDow: conv={conv!r} is not built (built: sage, gcn)")
        if int(num_layers) < 1 or int(hidden_dim) < 1:
            raise ValueError("ShaDow: num_layers and hidden_dim are at least 1")
        if not ops.gather_width_ok(int(hidden_dim)):
            raise ValueError(f"ShaDow: hidden_dim {hidden_dim} is not a width the gathers are built for (any up to 256, multiples of 4 "
                             "up to 1024)")
        self.conv, self.pool, self.num_layers = conv, bool(pool), int(num_layers)
        dims = [int(hidden_dim)] * self.num_layers
        self.body = SAGE(in_features, dims, dropout=dropout) if conv == "sage" else GCN(in_features, dims, dropout=dropout)
        self.head = Linear(int(hidden_dim) * (2 if self.pool else 1), num_classes)

    def forward(self, x, batch):
        h = self.body(x, batch.edge_index)
        if self.conv == "gcn":
            h = h[0]                                                 # (GCN.forward returns the allocated MiB beside its output)
        h = h.contiguous()
        out = _GatherX.apply(h, batch.root_n_id, None, None, False)
        if self.pool:
            out = torch.cat([out, _SegmentMeanFn.apply(h, batch.ptr)], dim=1)
        return self.head(out)
