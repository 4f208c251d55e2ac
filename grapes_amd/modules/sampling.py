"""What the batch samplers (modules/saint.py, modules/ladies.py, modules/asgcn.py, modules/sage.py, modules/labor.py) share: the
graph they sample over, the Philox key, the status word, for the samplers that draw layers for a batch of target nodes the targets,
the union of id lists and the local edge lists, and — for the two neighbour samplers, which keep entries of every row of the layer
before — the inward loop itself (InwardSampler).  DeviceGraph.check_status and dist.GraphScratch.check_status keep their own
decoding: they name a fourth bit (8, the one-launch scan) and the first zeroes two more tables.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from .. import ops
from .._lib import GrapesHipError

_STATUS_BITS = ((1, "edge buffer overflow"), (2, "node buffer overflow"), (4, "index out of range"))
_UNION_MAX = 4096                   # ops.union_sorted's limit (ids in all its lists)


def _graph_of(data_or_graph):
    """(DeviceGraph, data or None) of a DeviceGraph, an object with .graph, or a data object (rowptr / col or edge_index, and
    num_nodes; host tensors are moved to the current device)."""
    from ..driver import open_graph
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
        g = open_graph(data_or_graph, dev)
    return g, data_or_graph


def draw_seed(seed) -> int:
    """The Philox key: `seed`, or one draw from torch's generator for None (so torch.manual_seed makes a run reproducible)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


def raise_on_status(status, who: str, *, graph=None, hints={}):
    """Reads the status word (synchronises).  If it is set: clears it, zeroes graph's two bitmaps (a truncated batch may have left
    marks behind), and raises GrapesHipError(`who: names of the set bits`).  hints: bit -> text appended to the bit's name; a bit
    mapped to None is not named."""
    s = int(status.item())
    if s:
        status.zero_()
        if graph is not None:
            graph.bits.zero_(); graph.prev_bits.zero_()
        named = [(n, hints.get(b, "")) for b, n in _STATUS_BITS if s & b]
        raise GrapesHipError(f"{who}: " + ", ".join(n + h for n, h in named if h is not None))


def as_targets(targets, device, who: str):
    """The targets as a flat contiguous int32 tensor on the device, in the given order; ValueError for none."""
    targets = targets.to(device=device, dtype=torch.int32).contiguous().reshape(-1)
    if targets.numel() < 1:
        raise ValueError(f"{who}.sample: no target")
    return targets


def union_of_lists(g, lists, status):
    """The ascending duplicate-free union of id lists (int32 tensors, exact lengths) over the DeviceGraph g: one union_sorted launch
    per four lists while they are small, else marks into the frontier bitmap and a compaction (which zeroes it again).
    node_map[id] = rank."""
    N = g.num_nodes
    lists = [t for t in lists if t.numel()]
    total = sum(t.numel() for t in lists)
    if total <= _UNION_MAX:
        acc = []
        while True:
            part, lists = acc + lists[:4 - len(acc)], lists[4 - len(acc):]
            cap = sum(t.numel() for t in part)
            out, counts = ops.union_sorted([(t, None) for t in part], N, cap, node_map=g.node_map, status=status)
            acc = [out[:int(counts[0].item())]]
            if not lists:
                return acc[0]
    for i in range(0, len(lists), 4):
        ops.bitmap_mark_lists(g.bits, None, [(t, None) for t in lists[i:i + 4]], N, status=status)
    out, _, _, counts = ops.frontier_compact(g.bits, None, None, N, min(total, N), node_map=g.node_map, status=status)
    return out[:int(counts[0].item())]


def local_edge_lists(g, layers, device):
    """Per layer the int32 [2, e] edge list in local ids (row 0 the sources): edge_src / edge_dst through g.node_map, which holds
    the ranks in the batch's node_idx."""
    return [torch.stack([ops.tensormap_map(g.node_map, L.edge_src.contiguous()),
                         ops.tensormap_map(g.node_map, L.edge_dst.contiguous())]) if L.edge_src.numel()
            else torch.zeros((2, 0), dtype=torch.int32, device=device) for L in layers]


def check_fanouts(fanouts: Sequence[int]) -> "list[int]":
    """The fanouts as a list of ints: each -1 (every neighbour) or 1 .. ops.SAGE_MAX_FANOUT; at least one layer."""
    out = [int(k) for k in fanouts]
    if not out:
        raise ValueError("NeighborSampler: at least one fanout")
    for k in out:
        if k != -1 and not 1 <= k <= ops.SAGE_MAX_FANOUT:
            raise ValueError(f"NeighborSampler: fanout {k} is not built (-1 for every neighbour, or 1 .. {ops.SAGE_MAX_FANOUT})")
    return out


class InwardSampler:
    """The loop modules.sage.NeighborSampler and modules.labor.LaborSampler share.  Layers are drawn from the targets inward: d = 0 is
    the layer next to the output, prev_0 = the targets as given; layer d keeps entries of the rows of prev_d (source = the neighbour,
    target = the row), prev_{d + 1} = the ascending union of prev_d and the kept sources.  Each layer reads two counts on the host
    (the rows' entry count, and the kept count where the layer's call returns one).  A sampler gives _KIND (its name in the error
    texts) and _layer, and may add to _empty_layer; its stream advance and its further batch fields are its own."""

    _KIND = ""
    _SLICED = ("edge_src", "edge_dst", "edge_pos", "edge_weight")       # a layer's fields that hold one value per kept entry

    def __init__(self, data_or_graph, fanouts: Sequence[int], seed: Optional[int] = None):
        self.fanouts = check_fanouts(fanouts)
        self.num_layers = len(self.fanouts)
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError(f"{self._KIND} sampling over a graph with 2^31 or more entries is not built: the layer's entry offsets "
                             "are 32-bit")
        self.seed, self.philox_offset = draw_seed(seed), 0
        self.status = torch.zeros(1, dtype=torch.int32, device=g.device)
        if ops.csr_symmetric_check(g.rowptr, g.col, g.num_nodes) & 2:
            raise GrapesHipError(f"{type(self).__name__}: a column id is outside [0, num_nodes)")

    def _layer(self, d: int, k: int, prev, eoff, deg_sum: int, keys):
        """Layer d (fanout k) over the rows prev, which hold deg_sum >= 1 entries at the offsets eoff; keys: the caller's words for
        this layer or None.  Returns (fields, count): the layer's fields by name — edge_src, edge_dst, edge_pos and the sampler's
        own — and the int32 [1] kept count the _SLICED fields are cut to, or None when they are exact."""
        raise NotImplementedError

    def _empty_layer(self, dev) -> dict:
        """The fields of a layer whose rows hold no entry."""
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        return dict(edge_src=empty, edge_dst=empty, edge_pos=torch.zeros(0, dtype=torch.int64, device=dev))

    def sample(self, targets, keys=None) -> SimpleNamespace:
        """targets: node ids (any integer tensor; taken in the given order).  keys: per layer one tensor of 32-bit words replacing the
        layer's Philox words (tests); None entries and layers past the list draw from the stream.  Returns the batch: node_idx = the
        ascending union of the targets and every layer's sources, num_nodes, targets, local_targets, edge_index = per layer a local
        int32 [2, e_d] list (row 0 the sources), layers (prev, after, fanout and the layer's fields, in global ids)."""
        g, who = self.graph, type(self).__name__
        dev = g.device
        targets = as_targets(targets, dev, who)
        keys = list(keys) if keys is not None else []
        prev, layers = targets, []
        for d, k in enumerate(self.fanouts):
            eoff, d_e = ops.frontier_offsets(g.rowptr, prev)
            deg_sum = int(d_e.item())                                    # the rows' entry count (host read)
            if deg_sum >= 2 ** 31:
                raise ValueError(f"{who}.sample: a layer's rows hold 2^31 or more entries")
            if deg_sum == 0:
                L = self._empty_layer(dev)
            else:
                L, d_l = self._layer(d, k, prev, eoff, deg_sum, keys[d] if d < len(keys) else None)
                if d_l is not None:
                    e = int(d_l.item())                                  # the layer's entry count (host read)
                    L.update({name: L[name][:e] for name in self._SLICED if L.get(name) is not None})
            src = L["edge_src"]
            after = union_of_lists(g, [prev, src], self.status) if src.numel() else union_of_lists(g, [prev], self.status)
            layers.append(SimpleNamespace(prev=prev, after=after, fanout=k, **L))
            prev = after
        node_idx = prev                                  # the last union holds every earlier layer, and left node_map[id] = rank
        return SimpleNamespace(node_idx=node_idx, num_nodes=node_idx.numel(), targets=targets,
                               local_targets=ops.tensormap_map(g.node_map, targets), edge_index=local_edge_lists(g, layers, dev),
                               layers=layers)

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError on an edge overflow or a bad id, and clears it (and, as
        DeviceGraph.check_status does, the bitmaps a truncated batch may have left marked)."""
        raise_on_status(self.status, f"{self._KIND} sampler", graph=self.graph)
