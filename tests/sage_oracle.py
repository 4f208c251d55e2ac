"""TEST INFRASTRUCTURE — GraphSAGE restated on the host: the node-wise sampler's selection rule in integers over the Philox words of
tests/saint_samplers_oracle.py, the batch construction of modules/sage.py in numpy, and SAGEConv / SAGE in fp64 torch [Hamilton
et al., NeurIPS 2017; PyG-recall: torch_geometric 2.5.2 SAGEConv, NeighborLoader].

The selection rule (include/grapes_hip.h, grapes_sage_sample_layer): off_r = the exclusive prefix over the list rows r of
deg(rows[r]); entry t of list row r has stream position p = off_r + t and key keys[p], or raw Philox word p of (seed, offset); row r
keeps its min(deg, fanout) entries with the smallest (key << 32) | t, written for r ascending and within a row for t ascending.

SAGEConv: out_i = W_l aggr_{j -> i} x_j + W_r x_i + b over an edge list used as stored (duplicates by multiplicity, stored loops are
ordinary neighbours, a node without a neighbour aggregates 0), aggr = mean or sum — ONE form, the definition; both kernel forms are
compared with it.  Only tests import this module; it imports nothing of the product.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from tests.saint_samplers_oracle import philox_words

F32, F64 = np.float32, np.float64


# --------------------------------------------------------------------------------------------- the sampler
def stream_keys(seed, offset, total):
    """uint32 [total]: the raw words of the stream (seed, offset) the kernel reads at the positions 0 .. total - 1."""
    return philox_words(seed, offset, total).astype(np.uint32)


def offset_advance(deg_sum):
    return (int(deg_sum) + 3) // 4


def select_row(keys_row, fanout):
    """The kept positions t (ascending) of one row whose entries have the 32-bit keys keys_row: the min(deg, fanout) smallest
    composites (key << 32) | t, in Python integers."""
    deg = len(keys_row)
    if deg <= fanout:
        return np.arange(deg, dtype=np.int64)
    comp = sorted(((int(k) << 32) | t) for t, k in enumerate(keys_row))
    return np.array(sorted(c & 0xFFFFFFFF for c in comp[:fanout]), dtype=np.int64)


def sample_layer(indptr, indices, rows, fanout, keys=None, seed=0, offset=0, num_nodes=None):
    """(src, dst, pos int64, deg_sum) of one layer.  keys: uint32 words, one per stream position, replacing the Philox words.  A row
    id outside [0, num_nodes) is an empty row.  fanout -1: every entry of every row."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = len(indptr) - 1 if num_nodes is None else int(num_nodes)
    rows = np.asarray(rows, dtype=np.int64)
    degs = np.array([int(indptr[i + 1] - indptr[i]) if 0 <= i < n else 0 for i in rows], dtype=np.int64)
    total = int(degs.sum())
    if fanout == -1:
        words = None                                                     # every entry: no key is read
    else:
        words = np.asarray(keys).view(np.uint32)[:total] if keys is not None else stream_keys(seed, offset, total)
    src, dst, pos, p = [], [], [], 0
    for i, deg in zip(rows, degs):
        t = np.arange(deg, dtype=np.int64) if words is None else select_row(words[p:p + deg], fanout)
        p += int(deg)
        if len(t):
            a = int(indptr[i])
            src.append(np.asarray(indices[a + t], dtype=np.int64)); dst.append(np.full(len(t), i, np.int64)); pos.append(a + t)
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    return cat(src), cat(dst), cat(pos), total


def sample(indptr, indices, targets, fanouts, seed=0, keys=None):
    """One batch of modules.sage.NeighborSampler: layers from the targets inward, prev_{d + 1} = the ascending union of prev_d and
    the kept sources; fanout -1 keeps every neighbour and consumes no stream position; the stream offset starts at 0 and advances by
    ceil(deg_sum / 4) per drawn layer.  keys: per layer uint32 words or None."""
    targets = np.asarray(targets, dtype=np.int64)
    n = len(indptr) - 1
    prev, layers, off = targets, [], 0
    for d, k in enumerate(fanouts):
        kd = keys[d] if keys is not None and d < len(keys) else None
        if k == -1:
            src, dst, pos, total = sample_layer(indptr, indices, prev, -1)
        else:
            src, dst, pos, total = sample_layer(indptr, indices, prev, k, keys=kd, seed=seed, offset=off)
            off += offset_advance(total)
        after = np.union1d(prev, src)
        layers.append(SimpleNamespace(prev=prev, after=after, src=src, dst=dst, pos=pos, deg_sum=total))
        prev = after
    node_idx = np.unique(prev)                                           # (every after holds its prev, so the last one holds all)
    local = np.full(n, -1, np.int64)
    local[node_idx] = np.arange(len(node_idx))
    return SimpleNamespace(node_idx=node_idx, targets=targets, local_targets=local[targets], layers=layers, philox_offset=off,
                           edge_index=[np.stack([local[L.src], local[L.dst]]) for L in layers])


# --------------------------------------------------------------------------------------------- SAGEConv / SAGE in fp64
def aggregate64(x, ei, n, aggr):
    """aggr_{j -> i} x_j over the edge list ei ([2, e]: row 0 the sources) as stored; x fp64 torch [n, f]."""
    src, dst = torch.as_tensor(np.asarray(ei[0], dtype=np.int64)), torch.as_tensor(np.asarray(ei[1], dtype=np.int64))
    s = torch.zeros((n, x.shape[1]), dtype=torch.float64).index_add_(0, dst, x[src])
    if aggr == "sum":
        return s
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64))
    return s / deg.clamp(min=1.0)[:, None]


def sage_conv64(x, ei, w_l, b_l, w_r, aggr="mean", relu=False, gate=None):
    """act(aggr x W_lᵀ + x W_rᵀ + b); w_r / b_l may be None.  gate: a 0/1 array that replaces the ReLU."""
    out = aggregate64(x, ei, x.shape[0], aggr) @ w_l.T
    if w_r is not None:
        out = out + x @ w_r.T
    if b_l is not None:
        out = out + b_l
    if gate is not None:
        return out * torch.as_tensor(np.asarray(gate, dtype=F64))
    return out.clamp(min=0) if relu else out


def mean_sum_backward_closed_form(g, ei, n, aggr):
    """d L / d x of aggregate64 for the output gradient g, by the formula the kernels use: dx_j = sum_{i <- j} s_i g_i with
    s_i = 1 / deg_i (mean) or 1 (sum), every stored entry once."""
    src, dst = np.asarray(ei[0], dtype=np.int64), np.asarray(ei[1], dtype=np.int64)
    g = np.asarray(g, dtype=F64)
    s = np.ones(n)
    if aggr == "mean":
        s = 1.0 / np.maximum(np.bincount(dst, minlength=n), 1)
    dx = np.zeros_like(g)
    np.add.at(dx, src, s[dst][:, None] * g[dst])
    return dx


def sage_forward64(x, params, edge_index, aggr="mean", gates=None):
    """SAGE's routing (hidden layer i on edge_index[-i], the last on [0]; one edge list for every layer when edge_index is not a
    list), ReLU on the hidden layers.  params [(W_l, b_l, W_r), ...] fp64 torch."""
    L = len(params)
    listed = isinstance(edge_index, list)
    for i, (w_l, b_l, w_r) in enumerate(params):
        last = i == L - 1
        ei = (edge_index[0] if last else edge_index[-(i + 1)]) if listed else edge_index
        x = sage_conv64(x, ei, w_l, b_l, w_r, aggr, relu=not last, gate=None if (last or gates is None) else gates[i])
    return x


def loss64(logits, local_targets, labels):
    """Mean CrossEntropy (labels int [B]) or BCEWithLogits (labels float [B, C]) over the targets' rows."""
    z = logits[torch.as_tensor(np.asarray(local_targets, dtype=np.int64))]
    y = torch.as_tensor(np.asarray(labels))
    if y.dim() == 1:
        return torch.nn.functional.cross_entropy(z, y.long())
    return torch.nn.functional.binary_cross_entropy_with_logits(z, y.double())


def train_step64(x32, params32, edge_index, local_targets, labels, aggr="mean", gates=None):
    """(loss, [(dW_l, db_l, dW_r), ...], logits) in fp64 by autograd; params32 [(W_l, b_l, W_r), ...] numpy."""
    x = torch.as_tensor(np.asarray(x32, dtype=F64))
    params = [tuple(torch.as_tensor(np.asarray(p, dtype=F64)).requires_grad_(True) for p in layer) for layer in params32]
    logits = sage_forward64(x, params, edge_index, aggr, gates)
    loss = loss64(logits, local_targets, labels)
    loss.backward()
    grads = [tuple(p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape)) for p in layer) for layer in params]
    return float(loss.detach()), grads, logits.detach().numpy()


def adam_first_step64(p, g, lr=1e-3, eps=1e-8):
    """A parameter after torch.optim.Adam's FIRST step (betas cancel in the bias corrections): p - lr g / (|g| + eps)."""
    p, g = np.asarray(p, dtype=F64), np.asarray(g, dtype=F64)
    return p - lr * g / (np.abs(g) + eps)


def rel_err(a, ref):
    """The project's measure: max|a − ref| / max(1, max|ref|)."""
    a, ref = np.asarray(a, dtype=F64), np.asarray(ref, dtype=F64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


# --------------------------------------------------------------------------------------------- graphs
def csr_from_rows(rows):
    """(indptr int64, indices int32) of a list of per-row column lists, kept exactly as given (order and duplicates)."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = [c for r in rows for c in r]
    return indptr, np.asarray(flat, dtype=np.int32).reshape(-1)


def degree_graph(degrees, n, seed):
    """A graph of n nodes whose row r < len(degrees) has exactly degrees[r] distinct ascending columns (the other rows are empty);
    not symmetric — the sampler reads rows only."""
    rng = np.random.default_rng(seed)
    rows = [sorted(rng.choice(n, d, replace=False).tolist()) for d in degrees] + [[] for _ in range(n - len(degrees))]
    return csr_from_rows(rows)


def conv_graph(n, seed):
    """An edge list [2, e] (row 0 the sources) over n nodes for the aggregation tests.  n >= 8: node 0 has NO incoming entry (an
    empty row), node 3 is a hub with 200 incoming entries (duplicates among them once n < 200), (1, 4) is stored twice, the
    self-loop (5, 5) twice and (2, 2) once, and 3 n random entries go elsewhere.  n == 1: the single node's stored self-loop."""
    rng = np.random.default_rng(seed)
    if n == 1:
        return np.array([[0], [0]], dtype=np.int64)
    src, dst = [], []
    if n >= 8:
        hub = rng.integers(0, n, 200)
        src += hub.tolist(); dst += [3] * 200
        src += [1, 1, 5, 5, 2]; dst += [4, 4, 5, 5, 2]                   # a duplicate entry, a loop stored twice, another loop
    for _ in range(3 * n):
        a, b = int(rng.integers(0, n)), int(rng.integers(1, n))          # (never into node 0)
        src.append(a); dst.append(b)
    return np.array([src, dst], dtype=np.int64)
