"""Cluster-GCN's batches [Chiang et al., KDD 2019; PyG-recall: ClusterData(data, num_parts), ClusterLoader(cluster_data, batch_size)]
on the gfx950 kernels of csrc/cluster_kernels.hip (ops.cluster_batch).  The paper is recalled, not read: the rule written in
include/grapes_hip.h is the contract.

The graph is cut into `num_parts` clusters ONCE (ClusterData); a batch is the subgraph induced on the union of `batch_size` chosen
clusters, so the edges between the chosen clusters come back (ClusterLoader).  Nothing is drawn inside a batch: in cluster order
its node set is a handful of contiguous ranges, membership of a neighbour is one table lookup and its local id is arithmetic.

A batch (ClusterLoader.batch) has
  clusters       int32 [q]: the chosen clusters, in the given order;
  node_idx       int32 [n]: the global id of every row — cluster by cluster in that order, ascending id inside a cluster;
  num_nodes      n;  cptr int32 [q + 1]: chosen cluster k holds the rows cptr[k] .. cptr[k + 1];
  rowptr         int32 [n + 1]: the first edge of every row;
  edge_index     ONE int32 [2, e] tensor in row ids (row 0 the neighbours, row 1 the target rows), ordered by target row, then the
                 CSR's order — one tensor, so that every layer of the model shares one cached preparation;
  e_id           int64 [e]: each entry's position in the graph's col.
batch() reads two counts on the host (n and e): this is the eager form.

The partition.  "random" and "range" are the two graph-free cuts (make_partition).  method="lp" follows the graph: it refines a
balanced start — random or range, or a given `part=` — by size-constrained synchronous label propagation on the kernels of
csrc/partition_kernels.hip (refine_partition; the rule is in include/grapes_hip.h, integers only, bit-reproducible).  Every node
proposes the commonest label among its neighbours, a cluster admits the proposers with the largest gain up to `cap`, and the
assignment of the round with the smallest cut is kept, so the result is never worse than the start.  Its limit: once clusters sit
at `cap` the rule stalls — on a planted graph it stops at about twice the planted cut.  Not built: a partitioner of METIS quality
(multilevel coarsening), a swap or rebalancing phase that would get past that stall, edge or node weights; `part=` still takes an
assignment computed elsewhere.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from .. import ops
from .._lib import GrapesHipError
from .sampling import _graph_of, draw_seed, raise_on_status

_E_FLOOR = 1 << 14                  # the smallest edge buffer the loader starts from
_E_CEIL = 2 ** 31 - 1
METHODS = ("random", "range")


def make_partition(num_nodes: int, num_parts: int, method: str = "random", seed: Optional[int] = None) -> torch.Tensor:
    """The cluster of every node, int64 [N] on the host.  "range": node v goes to cluster v * P // N.  "random": the nodes in the
    order of torch.randperm under a generator seeded with `seed`, position i of that order going to cluster i * P // N — P pieces
    whose sizes differ by at most 1, the same for the same seed."""
    N, P = int(num_nodes), int(num_parts)
    if N < 1 or not 1 <= P <= N:
        raise ValueError(f"ClusterData: num_parts is 1 .. num_nodes ({N}), not {num_parts}")
    if method == "lp":
        raise ValueError("make_partition: method 'lp' refines an assignment over a graph: ClusterData(graph, num_parts, method='lp')")
    if method not in METHODS:
        raise ValueError(f"ClusterData: method {method!r} is not built (built: {', '.join(METHODS)}; part= takes any other assignment)")
    pos = torch.arange(N, dtype=torch.int64) * P // N
    if method == "range":
        return pos
    gen = torch.Generator()
    gen.manual_seed(draw_seed(seed))
    part = torch.empty(N, dtype=torch.int64)
    part[torch.randperm(N, generator=gen)] = pos
    return part


def partition_tables(part, num_parts: int):
    """(perm int32 [N], partptr int32 [P + 1], where int32 [N, 2]) of an assignment `part` (any integer tensor [N] in [0, P)), on its
    device: perm = the node ids in cluster order, ascending id inside a cluster (a stable sort by cluster); cluster c holds
    perm[partptr[c] : partptr[c + 1]]; where[v] = (cluster of v, position of v inside its cluster)."""
    P = int(num_parts)
    if part.dim() != 1 or part.numel() < 1 or part.is_floating_point() or part.dtype == torch.bool:
        raise ValueError("ClusterData: part is an integer tensor [N]")
    N = part.numel()
    if N >= 2 ** 31 or P < 1:
        raise ValueError("ClusterData: fewer than 2^31 nodes and at least one cluster")
    part = part.to(torch.int64)
    if int(part.min()) < 0 or int(part.max()) >= P:
        raise ValueError(f"ClusterData: part holds a cluster id outside [0, {P})")
    perm = torch.sort(part, stable=True)[1]
    counts = torch.bincount(part, minlength=P)
    partptr = torch.zeros(P + 1, dtype=torch.int64, device=part.device)
    partptr[1:] = torch.cumsum(counts, 0)
    where = torch.empty((N, 2), dtype=torch.int32, device=part.device)
    where[:, 0] = part.to(torch.int32)
    where[perm, 1] = (torch.arange(N, dtype=torch.int64, device=part.device) - partptr[part[perm]]).to(torch.int32)
    return perm.to(torch.int32).contiguous(), partptr.to(torch.int32).contiguous(), where.contiguous()


def default_cap(num_nodes: int, num_parts: int, imbalance: float = 0.1) -> int:
    """ceil(N / P) + floor(imbalance N / P), in integers: imbalance is taken as the nearest fraction with a denominator up to 10^6."""
    from fractions import Fraction
    N, P = int(num_nodes), int(num_parts)
    if not imbalance >= 0:
        raise ValueError("refine_partition: imbalance is at least 0")
    f = Fraction(imbalance).limit_denominator(10 ** 6)
    return -(-N // P) + (f.numerator * N) // (f.denominator * P)


def refine_partition(graph, part, num_parts: int, rounds: int = 30, imbalance: float = 0.1, cap: Optional[int] = None):
    """(part int32 [N] on the device, info): `part` refined over the DeviceGraph `graph` by at most `rounds` rounds of the
    size-constrained synchronous label propagation written in include/grapes_hip.h (ops.partition_propose / _admit / _cut).  cap: the
    largest size a cluster may reach — default ceil(N / P) + floor(imbalance N / P); one below the start's largest cluster is a
    ValueError.  The cut is evaluated for the start and after every round, and the assignment of the earliest round with the
    smallest cut is returned; a round that moves nothing ends the run.  One host read per round: the eager form of a one-time
    preprocessing step.  info: cuts (the start's first, then one per round that moved a node), moved (one per round run), round (the
    chosen one; 0 = the start), max_size (the largest cluster of the returned assignment) and cap."""
    g = graph
    N, P, dev = g.num_nodes, int(num_parts), g.device
    if not 1 <= P <= N:
        raise ValueError(f"refine_partition: num_parts is 1 .. num_nodes ({N}), not {num_parts}")
    if g.nnz >= 2 ** 31:
        raise ValueError("refine_partition: a graph with 2^31 or more entries is not built")
    if not torch.is_tensor(part) or part.numel() != N or part.is_floating_point() or part.dtype == torch.bool:
        raise ValueError("refine_partition: part is an integer tensor with one cluster id per node")
    if int(rounds) < 0:
        raise ValueError("refine_partition: rounds is at least 0")
    part64 = part.to(dev).reshape(-1).to(torch.int64)
    if int(part64.min()) < 0 or int(part64.max()) >= P:
        raise ValueError(f"refine_partition: part holds a cluster id outside [0, {P})")
    size = torch.bincount(part64, minlength=P).to(torch.int32)
    cap = default_cap(N, P, imbalance) if cap is None else int(cap)
    if cap < int(size.max()) or cap >= 2 ** 31:
        raise ValueError(f"refine_partition: cap {cap} is below the start's largest cluster ({int(size.max())}), or not below 2^31")
    cur = part64.to(torch.int32).contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    want, gain = torch.empty_like(cur), torch.empty_like(cur)
    moved, cut = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int64, device=dev)

    def cut_now() -> int:
        ops.partition_cut(g.rowptr, g.col, N, cur, P, status=status, out=cut)
        return int(cut.item())

    cuts, moves, best, best_round = [cut_now()], [], cur.clone(), 0
    raise_on_status(status, "refine_partition")
    for r in range(1, int(rounds) + 1):
        ops.partition_propose(g.rowptr, g.col, N, cur, P, status=status, out=(want, gain))
        ops.partition_admit(want, gain, cur, size, cap, status=status, moved=moved)
        moves.append(int(moved.item()))                              # (the round's host read)
        if moves[-1] == 0:
            break
        cuts.append(cut_now())
        if cuts[-1] < cuts[best_round]:
            best, best_round = cur.clone(), r
    raise_on_status(status, "refine_partition")
    info = dict(cuts=cuts, moved=moves, round=best_round, max_size=int(torch.bincount(best.to(torch.int64), minlength=P).max()), cap=cap)
    return best, info


class ClusterData:
    """ClusterData(data_or_graph, num_parts, part=None, method="random" | "range" | "lp", seed=None, lp_start="random", lp_rounds=30,
    lp_imbalance=0.1).  data_or_graph: a DeviceGraph, or a data object as the GraphSAINT samplers take.  part: the cluster of every
    node computed elsewhere (METIS offline, say) — it wins over method "random" / "range"; seed: "random"'s (None: from torch's
    generator).  method="lp": the start — make_partition(lp_start), or the given part — is refined by refine_partition(rounds =
    lp_rounds, imbalance = lp_imbalance) and its info kept as lp_info (None otherwise).  Built once with torch ops: perm, partptr,
    where (partition_tables), the clusters' sizes and their work-item counts (the sum over a cluster's rows of ceil(deg / 64), which
    bounds the items of any batch)."""

    def __init__(self, data_or_graph, num_parts: int, part=None, method: str = "random", seed: Optional[int] = None,
                 lp_start: str = "random", lp_rounds: int = 30, lp_imbalance: float = 0.1):
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("cluster batches over a graph with 2^31 or more entries are not built: the batch's edge offsets are 32-bit")
        N, self.num_parts = g.num_nodes, int(num_parts)
        lp = method == "lp"
        if part is None:
            part = make_partition(N, self.num_parts, lp_start if lp else method, seed)
        elif not torch.is_tensor(part) or part.numel() != N:
            raise ValueError("ClusterData: part holds one cluster id per node")
        if not 1 <= self.num_parts <= N:
            raise ValueError(f"ClusterData: num_parts is 1 .. num_nodes ({N}), not {num_parts}")
        if ops.csr_symmetric_check(g.rowptr, g.col, N) & 2:
            raise GrapesHipError("ClusterData: a column id is outside [0, num_nodes)")
        self.lp_info = None
        if lp:
            part, self.lp_info = refine_partition(g, part, self.num_parts, rounds=lp_rounds, imbalance=lp_imbalance)
        self.perm, self.partptr, self.where = partition_tables(part.to(g.device).reshape(-1), self.num_parts)
        self.part = self.where[:, 0].contiguous()
        self.sizes = (self.partptr[1:] - self.partptr[:-1]).to(torch.int64)
        chunks = (g.rowptr[1:] - g.rowptr[:-1] + (ops.CLUSTER_CHUNK - 1)) // ops.CLUSTER_CHUNK
        self.items = torch.zeros(self.num_parts, dtype=torch.int64, device=g.device).index_add_(0, self.part.to(torch.int64), chunks)

    def __len__(self) -> int:
        return self.num_parts


class ClusterLoader:
    """ClusterLoader(cluster_data, batch_size, seed=None, n_cap=None, e_cap=None): batches of batch_size clusters.  __iter__ walks a
    permutation of the P clusters (torch.randperm under a generator seeded with `seed`; None: from torch's generator) batch_size at a
    time; the last batch may be short.  n_cap: the node buffer (default: the batch_size largest clusters together, which cannot
    overflow).  e_cap: the edge buffer; by default it starts near the last batch's size and a batch that does not fit is built again
    — the same clusters — into a buffer twice as large; a given e_cap is kept and an overflow raises at check().  The loader owns the
    membership table and its serial: a call takes the next serial, and the table is zeroed before one would repeat."""

    def __init__(self, cluster_data: ClusterData, batch_size: int, seed: Optional[int] = None, n_cap: Optional[int] = None,
                 e_cap: Optional[int] = None):
        cd = self.cluster_data = cluster_data
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= min(cd.num_parts, ops.CLUSTER_MAX_BATCH_PARTS):
            raise ValueError(f"ClusterLoader: batch_size is 1 .. {min(cd.num_parts, ops.CLUSTER_MAX_BATCH_PARTS)} clusters")
        if (n_cap is not None and int(n_cap) < 1) or (e_cap is not None and int(e_cap) < 1):
            raise ValueError("ClusterLoader: n_cap and e_cap are at least 1")
        dev = cd.graph.device
        top = lambda t: int(torch.sort(t, descending=True)[0][:self.batch_size].sum().item())     # noqa: E731
        self.n_cap = max(1, top(cd.sizes)) if n_cap is None else int(n_cap)
        self.item_cap = min(max(1, top(cd.items)), ops.CLUSTER_ITEM_CAP_MAX)
        self.e_cap = None if e_cap is None else int(e_cap)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stamp = torch.zeros((cd.num_parts, 2), dtype=torch.int32, device=dev)
        self.serial = 0                                              # the last serial handed out
        self._e_hint = _E_FLOOR
        self._gen = torch.Generator()
        self._gen.manual_seed(draw_seed(seed))

    def __len__(self) -> int:
        return (self.cluster_data.num_parts + self.batch_size - 1) // self.batch_size

    def _next_serial(self) -> int:
        if self.serial >= ops.CLUSTER_MAX_SERIAL:
            self.stamp.zero_()                                       # every serial has been used: start over on a clean table
            self.serial = 0
        self.serial += 1
        return self.serial

    def batch(self, clusters) -> SimpleNamespace:
        """clusters: cluster ids (any integer tensor or list; taken in the given order, each at most once).  Returns the batch
        namespace described in the module docstring."""
        cd = self.cluster_data
        g = cd.graph
        clusters = torch.as_tensor(clusters).to(device=g.device, dtype=torch.int32).contiguous().reshape(-1)
        if not 1 <= clusters.numel() <= ops.CLUSTER_MAX_BATCH_PARTS:
            raise ValueError(f"ClusterLoader.batch: 1 .. {ops.CLUSTER_MAX_BATCH_PARTS} clusters")
        ec = self.e_cap if self.e_cap is not None else self._e_hint
        while True:
            cptr, node_idx, rowptr_l, ei, e_id, d_n, d_e = ops.cluster_batch(
                g.rowptr, g.col, g.num_nodes, cd.perm, cd.partptr, cd.where, clusters, self.stamp, self._next_serial(), self.n_cap, ec,
                item_cap=self.item_cap, status=self.status)
            n, e = int(d_n.item()), int(d_e.item())                  # the batch's rows and entries (host reads)
            if self.e_cap is not None or e < ec or ec >= _E_CEIL or not int(self.status.item()) & 1:
                break
            self.status.bitwise_and_(~1)                             # the buffer was too small: the same clusters into twice the room
            ec = min(2 * ec, _E_CEIL)
        if self.e_cap is None:
            self._e_hint = max(_E_FLOOR, min(e + e // 4, _E_CEIL))
        return SimpleNamespace(clusters=clusters, node_idx=node_idx[:n], num_nodes=n, cptr=cptr, rowptr=rowptr_l[:n + 1],
                               edge_index=ei[:, :e], e_id=e_id[:e])

    def __iter__(self):
        order = torch.randperm(self.cluster_data.num_parts, generator=self._gen)
        for i in range(0, order.numel(), self.batch_size):
            yield self.batch(order[i:i + self.batch_size])

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError("cluster loader: ...") on a node or edge overflow or a bad
        cluster id, and clears it."""
        raise_on_status(self.status, "cluster loader", hints={1: " (give the loader a larger e_cap)", 2: " (give it a larger n_cap)"})
