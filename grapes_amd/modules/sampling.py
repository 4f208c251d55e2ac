"""What the batch samplers (modules/saint.py, modules/ladies.py, modules/asgcn.py, modules/sage.py) share: the graph they sample
over, the Philox key, the status word, and — for the two samplers that draw layers for a batch of target nodes — the targets, the
union of id lists and the local edge lists.  DeviceGraph.check_status and dist.GraphScratch.check_status keep their own decoding:
they name a fourth bit (8, the one-launch scan) and the first zeroes two more tables.
"""
from __future__ import annotations

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
