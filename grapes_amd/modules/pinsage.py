"""PinSAGE [Ying et al., KDD 2018 — recalled; DGL-recall: RandomWalkNeighborSampler / PinSAGESampler, not read: the rule in
include/grapes_hip.h is the contract] on the gfx950 kernels of csrc/pinsage_kernels.hip (ops.pinsage_neighbors, ops.relu_l2norm_fwd /
_bwd) and csrc/pprgo_kernels.hip (ops.pprgo_batch, ops.pprgo_aggregate_fwd / _bwd, used as they are): importance neighbourhoods from
short random walks.  A node's neighbourhood is not its stored row but the T nodes that R restarting walks from it visit most often,
and the normalised visit counts are the aggregation weights — the Monte-Carlo counterpart of the PPR rows (ShaDowPPRSampler,
PPRGoSampler), at a cost per seed that no degree enters.

PinSAGESampler.sample(roots) returns a namespace: blocks — num_layers of them, block 0 next to the output; node_idx int32 [n] — the
deepest block's, whose feature rows the trainer gathers; num_nodes = n; targets = the roots, local_targets = arange(m).  Block d is
built on seeds_d (seeds_0 = the roots, seeds_{d + 1} = node_idx_d) and carries seeds, nbr / visits int32 [m_d, K] and cnt int32 [m_d]
(the slot tables, K = num_neighbors + 1, slot 0 the seed itself), weight fp32 [m_d, K] = visits / the row's total visits (0 where
there is none; slot 0 weighs 0: the seed has its own term in the layer), node_idx int32 [n_d] (the ascending union of the live
slots), num_nodes = n_d, loc int32 [m_d, K], self_loc int32 [m_d] = loc[:, 0], tptr, tslot, num_slots and item_cap as a PPRGoSampler
batch has them.  One host read per block.

PinSAGEConv is the layer, PinSAGE the model: the convs, deepest block first, then a linear head.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Sequence

import torch
from torch import nn

from .. import ops
from .._lib import GrapesHipError
from ..target_batch import _GatherX
from .pprgo import _PPRGoAggregateFn
from .sampling import _graph_of, as_targets, raise_on_status

EPS = 1e-12                         # the floor under a row's norm (torch.nn.functional.normalize's)


def visit_weights(visits):
    """weight[b, t] = float(visits[b, t]) / float(sum_t visits[b, t]) — both exact below 2^24, so one fp32 division — and 0 where the
    row has no visit."""
    v = visits.to(torch.float32)
    tot = v.sum(dim=1, keepdim=True)
    return torch.where(tot > 0, v / tot.clamp(min=1.0), torch.zeros_like(v)).contiguous()


class PinSAGESampler:
    """PinSAGESampler(data_or_graph, num_layers=2, num_neighbors=10, num_random_walks=10, walk_length=2, termination_prob=0.5, seed=0).
    num_neighbors: T, 1 .. ops.PINSAGE_MAX_NEIGHBORS; num_random_walks R and walk_length L at least 1 with R L <=
    ops.PINSAGE_MAX_VISITS; termination_prob in [0, 1): a walk ends before a step with this probability.  seed: the Philox key; the
    stream offset lives on the device (philox_offset, int64 [1]) and advances by ceil(L / 2) per block, so two calls draw different
    walks and a reset offset repeats them.  Returns to the root are not counted (DGL counts them); edge weights, metapaths and
    bipartite item - user graphs are not built."""

    def __init__(self, data_or_graph, num_layers: int = 2, num_neighbors: int = 10, num_random_walks: int = 10, walk_length: int = 2,
                 termination_prob: float = 0.5, seed: int = 0):
        self.num_layers, self.num_neighbors = int(num_layers), int(num_neighbors)
        self.num_random_walks, self.walk_length = int(num_random_walks), int(walk_length)
        self.termination_prob = float(termination_prob)
        if self.num_layers < 1:
            raise ValueError("PinSAGESampler: num_layers is at least 1")
        self.K = ops.pinsage_args(self.num_random_walks, self.walk_length, self.num_neighbors)
        self.term_q = ops.pinsage_term_q(self.termination_prob)
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("PinSAGESampler: a graph with 2^31 or more entries is not built")
        self.seed = int(seed)
        self.philox_offset = torch.zeros(1, dtype=torch.int64, device=g.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=g.device)
        if ops.csr_symmetric_check(g.rowptr, g.col, g.num_nodes) & 2:
            raise GrapesHipError("PinSAGESampler: a column id is outside [0, num_nodes)")
        self._scratch = (g.bits, g.node_map)                         # (the graph's frontier bitmap is zero at rest, and left so)

    def block(self, seeds) -> SimpleNamespace:
        """One block over `seeds` (int32, distinct, at most ops.PPRGO_MAX_ROOTS): the walks, then the batch structure of their tables."""
        g = self.graph
        if seeds.numel() > ops.PPRGO_MAX_ROOTS:
            raise ValueError(f"PinSAGESampler: a block of {seeds.numel()} seeds is not built (at most {ops.PPRGO_MAX_ROOTS} = "
                             "ops.PPRGO_MAX_ROOTS per block: fewer roots, neighbours or layers)")
        nbr, visits, cnt = ops.pinsage_neighbors(g.rowptr, g.col, g.num_nodes, seeds, self.num_random_walks, self.walk_length,
                                                 self.term_q, self.num_neighbors, philox_seed=self.seed,
                                                 d_philox_offset=self.philox_offset, status=self.status)
        node_idx, loc, tptr, tslot, counts = ops.pprgo_batch(nbr, cnt, g.num_nodes, self._scratch, status=self.status)
        n, e, seg_max = counts.tolist()                              # the block's rows, live slots and longest segment (the host read)
        if n < 1:
            self.check()
            raise GrapesHipError("PinSAGESampler: a block without a node")
        return SimpleNamespace(seeds=seeds, num_seeds=seeds.numel(), nbr=nbr, visits=visits, cnt=cnt, weight=visit_weights(visits),
                               node_idx=node_idx[:n], num_nodes=n, loc=loc, self_loc=loc[:, 0].contiguous(), tptr=tptr[:n + 1],
                               tslot=tslot[:e], num_slots=e, item_cap=ops.pprgo_item_cap(e, seg_max))

    def sample(self, roots) -> SimpleNamespace:
        """roots: DISTINCT node ids (any integer tensor, in the given order; a repeat is refused: the self term's backward scatters
        distinct rows).  Returns the batch namespace of the module docstring."""
        g = self.graph
        roots = as_targets(roots, g.device, type(self).__name__)
        m = roots.numel()
        if m > ops.PPRGO_MAX_ROOTS:
            raise ValueError(f"PinSAGESampler.sample: at most {ops.PPRGO_MAX_ROOTS} roots per batch")
        if torch.unique(roots).numel() != m:                         # (one host read)
            raise ValueError("PinSAGESampler.sample: the roots are distinct")
        blocks, seeds = [], roots
        for _ in range(self.num_layers):
            blocks.append(self.block(seeds))
            seeds = blocks[-1].node_idx
        return SimpleNamespace(blocks=blocks, node_idx=blocks[-1].node_idx, num_nodes=blocks[-1].num_nodes, targets=roots,
                               local_targets=torch.arange(m, dtype=torch.int32, device=g.device))

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError("PinSAGE sampler: ...") on an overflow or a bad id, and clears
        it (the graph's bitmap is zeroed too: a truncated batch may have left marks)."""
        if int(self.status.item()):
            self.graph.bits.zero_()
        raise_on_status(self.status, "PinSAGE sampler")


class _ReluL2NormFn(torch.autograd.Function):
    """out = relu(s) / max(|relu(s)|_2, eps) per row (ops.relu_l2norm_fwd); the backward is ops.relu_l2norm_bwd on the saved out, nrm
    and s."""

    @staticmethod
    def forward(ctx, s, eps):
        s = s.contiguous()
        out, nrm = ops.relu_l2norm_fwd(s, eps)
        ctx.save_for_backward(s, out, nrm)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, g):
        s, out, nrm = ctx.saved_tensors
        return ops.relu_l2norm_bwd(g.contiguous(), out, nrm, s, ctx.eps), None


def relu_l2norm(s, eps: float = EPS):
    """relu, then every row divided by max(its L2 norm, eps): one launch forward, one backward."""
    return _ReluL2NormFn.apply(s, float(eps))


class PinSAGEConv(nn.Module):
    """PinSAGEConv(in_features, hidden_features, out_features) over a PinSAGESampler block and the rows h [n, in] of its node_idx:

        n_b = sum_t weight[b, t] relu(Q h + q)[loc[b, t]]          (the importance pooling: ops.pprgo_aggregate_fwd)
        s_b = W [h[loc[b, 0]] ; n_b] + w
        out = relu(s) / max(|relu(s)|_2, eps) per row              (ops.relu_l2norm_fwd)

    one row per seed.  Q = nn.Linear(in, hidden), W = nn.Linear(in + hidden, out): the state dict holds Q.weight, Q.bias, W.weight,
    W.bias.  The self rows are the project's row gather (its backward the row scatter: the seeds are distinct).  hidden_features and
    out_features are widths of the row gathers."""

    def __init__(self, in_features: int, hidden_features: int, out_features: int, eps: float = EPS):
        super().__init__()
        for name, f in (("hidden_features", hidden_features), ("out_features", out_features)):
            if not ops.gather_width_ok(int(f)):
                raise ValueError(f"PinSAGEConv: {name} = {f} is not a width the gathers are built for (any up to 256, multiples of 4 "
                                 "up to 1024)")
        if int(in_features) < 1:
            raise ValueError("PinSAGEConv: in_features is at least 1")
        self.Q = nn.Linear(int(in_features), int(hidden_features))
        self.W = nn.Linear(int(in_features) + int(hidden_features), int(out_features))
        self.eps = float(eps)

    def forward(self, h, block):
        h = h.contiguous()
        n = _PPRGoAggregateFn.apply(torch.relu(self.Q(h)), block)
        own = _GatherX.apply(h, block.self_loc, None, None, False)
        return relu_l2norm(self.W(torch.cat([own, n], dim=1)), self.eps)


class PinSAGE(nn.Module):
    """PinSAGE(in_features, hidden_dims, num_classes, dropout=0.): one PinSAGEConv per entry of hidden_dims (in `convs`: conv i maps
    width d_i to d_{i + 1} with a pooling width of d_{i + 1}, d_0 = in_features) and the head `lin` = nn.Linear(d_last, num_classes).
    forward(xb, batch) takes the gathered feature rows of batch.node_idx and a PinSAGESampler batch of len(hidden_dims) blocks, runs
    the convs deepest block first with dropout in front of each, and returns logits [m, num_classes], one row per root."""

    def __init__(self, in_features: int, hidden_dims: Sequence[int], num_classes: int, dropout: float = 0.0):
        super().__init__()
        dims = [int(in_features)] + [int(d) for d in hidden_dims]
        if len(dims) < 2 or min(dims) < 1 or int(num_classes) < 1:
            raise ValueError("PinSAGE: hidden_dims holds at least one width, and every width is at least 1")
        self.convs = nn.ModuleList(PinSAGEConv(a, b, b) for a, b in zip(dims[:-1], dims[1:]))
        self.lin = nn.Linear(dims[-1], int(num_classes))
        self.dropout = float(dropout)
        self.out_channels = int(num_classes)

    def forward(self, xb, batch):
        if len(batch.blocks) != len(self.convs):
            raise ValueError(f"PinSAGE: {len(self.convs)} layers over a batch of {len(batch.blocks)} blocks")
        h = xb
        for conv, block in zip(self.convs, reversed(batch.blocks)):
            h = conv(nn.functional.dropout(h, self.dropout, self.training), block)
        return self.lin(h)
