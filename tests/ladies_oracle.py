"""TEST INFRASTRUCTURE — the two published layer-wise samplers restated on the host in numpy fp64 [LADIES-recall: acbull/LADIES
pytorch_ladies.py, ladies_sampler / fastgcn_sampler], and the weighted GCN they feed in fp64 torch.

A = the CSR (indptr, indices: columns ascending, duplicate-free, stored loops kept), V = A + I (v_ii = 1 + [(i, i) stored]),
P = D^-1 V with D_i = sum_j v_ij = (indptr[i + 1] - indptr[i]) + 1.  Layers from the targets inward, prev_0 = the targets as given.

LADIES per layer: candidates = ascending union of prev and its neighbours; pi_j = sum_{i in prev} P_ij^2; min(#candidates, samp_num)
of them drawn without replacement in proportion to pi; after = ascending union of the drawn nodes and the targets; entries
(i in prev, j in after, v_ij > 0) weigh (v_ij / pi_j) / sum_j' (v_ij' / pi_j'); prev <- after.  FastGCN: pi over ALL rows, once; every
layer draws min(N, samp_num) of all nodes; after = the ascending drawn set.

The draw is the project's: oracle.grapes_oracle.sample_neighborhoods_from_probs (portable_math.gumbel_keys + exact top-k) on fp32
logits l_j = log pi_j - C, C = 20 + log(float(|prev|)), and the uniforms given — so sets are bit-comparable with the device's when it
is fed the device's logits.  Only tests import this module; it imports nothing of the product.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from oracle import grapes_oracle as go

F32, F64 = np.float32, np.float64


def row_of_v(indptr, indices, i):
    """(columns ascending, v) of row i of V = A + I: the diagonal at its sorted place, a stored loop folded into it (v = 2)."""
    cols = np.asarray(indices[indptr[i]:indptr[i + 1]], dtype=np.int64)
    if (cols == i).any():
        return cols, np.where(cols == i, 2.0, 1.0)
    p = int(np.searchsorted(cols, i))
    return np.insert(cols, p, i), np.ones(len(cols) + 1)


def degree(indptr):
    return np.diff(np.asarray(indptr, dtype=np.int64)).astype(F64) + 1.0


def importance(indptr, indices, n, prev=None):
    """(pi fp64 [n], terms int64 [n]): pi_j = sum over i in prev (None: every row) of P_ij^2, and how many terms each sum has."""
    D = degree(indptr)
    pi, t = np.zeros(n), np.zeros(n, np.int64)
    for i in (range(n) if prev is None else np.asarray(prev, dtype=np.int64)):
        cols, v = row_of_v(indptr, indices, int(i))
        np.add.at(pi, cols, (v / D[i]) ** 2)
        np.add.at(t, cols, 1)
    return pi, t


def candidates(indptr, indices, prev):
    prev = np.asarray(prev, dtype=np.int64)
    nb = [np.asarray(indices[indptr[i]:indptr[i + 1]], dtype=np.int64) for i in prev]
    return np.unique(np.concatenate([prev] + nb))


def shift(m):
    """C = 20 + log(float(m))"""
    return 20.0 + np.log(F64(F32(m)))


def logits64(pi, m):
    return np.log(pi) - shift(m)


def draw(logit32, cand, k, uniforms):
    """The ascending ids of the min(len(cand), k) candidates the project's draw keeps on these fp32 logits and uniforms."""
    cand = np.asarray(cand, dtype=np.int64)
    if len(cand) <= k:
        return cand
    res = go.sample_neighborhoods_from_probs(np.asarray(logit32, dtype=F32), cand, k,
                                             uniforms=np.asarray(uniforms, dtype=F32)[:len(cand)])
    return np.asarray(res["kept"], dtype=np.int64)


def layer_entries(indptr, indices, n, prev, after, pi):
    """(src = j, dst = i, w fp64, terms) of one layer: rows in prev's order, ascending j within a row; terms[e] = the entries of
    e's row (the length of its normalising sum)."""
    keep = np.zeros(n, bool)
    keep[np.asarray(after, dtype=np.int64)] = True
    src, dst, w, terms = [], [], [], []
    for i in np.asarray(prev, dtype=np.int64):
        cols, v = row_of_v(indptr, indices, int(i))
        sel = keep[cols]
        if not sel.any():
            continue
        q = v[sel] / pi[cols[sel]]
        src.append(cols[sel]); dst.append(np.full(int(sel.sum()), i)); w.append(q / q.sum()); terms.append(np.full(int(sel.sum()), int(sel.sum())))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(src, np.int64), cat(dst, np.int64), cat(w, F64), cat(terms, np.int64)


def sample(indptr, indices, n, targets, samp_num, num_layers, kind="ladies", uniforms=None, logits=None):
    """One batch.  uniforms: per layer the fp32 uniforms of the draw; logits: per layer fp32 logits that replace the oracle's own
    fp32(log pi - C) (the device's, for bit-equal sets).  Returns node_idx, edge_index (local, [2, e] per layer), edge_weight and
    layers (prev, candidates, pi over the candidates, terms, logit64, sampled, after, src, dst, w, row_terms in global ids)."""
    targets = np.asarray(targets, dtype=np.int64)
    prev, layers = targets, []
    gpi = importance(indptr, indices, n) if kind == "fastgcn" else None
    for d in range(num_layers):
        if kind == "ladies":
            cand = candidates(indptr, indices, prev)
            pi_all, t_all = importance(indptr, indices, n, prev)
            m = len(prev)
        else:
            cand, (pi_all, t_all), m = np.arange(n), gpi, n
        l64 = logits64(pi_all[cand], m)
        l32 = np.asarray(logits[d], dtype=F32) if logits is not None else l64.astype(F32)
        sampled = draw(l32, cand, samp_num, None if uniforms is None else uniforms[d])
        after = np.union1d(sampled, targets) if kind == "ladies" else np.sort(sampled)
        src, dst, w, rt = layer_entries(indptr, indices, n, prev, after, pi_all)
        layers.append(SimpleNamespace(prev=prev, candidates=cand, pi=pi_all[cand], terms=t_all[cand], logit64=l64, sampled=sampled,
                                      after=after, src=src, dst=dst, w=w, row_terms=rt, pi_all=pi_all))
        prev = after
    node_idx = np.unique(np.concatenate([targets] + [L.after for L in layers]))
    local = np.full(n, -1, np.int64)
    local[node_idx] = np.arange(len(node_idx))
    return SimpleNamespace(node_idx=node_idx, targets=targets, local_targets=local[targets], layers=layers,
                           edge_index=[np.stack([local[L.src], local[L.dst]]) for L in layers], edge_weight=[L.w for L in layers])


# --------------------------------------------------------------------------------------------- the weighted GCN in fp64
def gcn_forward64(x, params, edge_index, edge_weight, gates=None):
    """GCN's routing over per-layer weighted edge lists (hidden layer i on [-i], the last on [0]), every layer
    out[c] = sum_{e: r -> c} w_e (x Wᵀ)[r] + b, ReLU on the hidden layers (gates: the 0/1 arrays that replace it, per hidden layer).
    x fp64 torch [n, F]; params [(W, b), ...] fp64 torch."""
    L = len(params)
    for i, (W, b) in enumerate(params):
        last = i == L - 1
        k = 0 if last else -(i + 1)
        ei, w = edge_index[k], torch.as_tensor(np.asarray(edge_weight[k], dtype=F64))
        H = x @ W.T
        out = torch.zeros_like(H).index_add_(0, torch.as_tensor(ei[1]), w[:, None] * H[torch.as_tensor(ei[0])]) + b
        if last:
            return out
        x = out * torch.as_tensor(np.asarray(gates[i], dtype=F64)) if gates is not None else out.clamp(min=0)


def loss64(logits, local_targets, labels):
    """Mean CrossEntropy (labels int [B]) or BCEWithLogits (labels float [B, C]) over the targets' rows."""
    z = logits[torch.as_tensor(np.asarray(local_targets, dtype=np.int64))]
    y = torch.as_tensor(np.asarray(labels))
    if y.dim() == 1:
        return torch.nn.functional.cross_entropy(z, y.long())
    return torch.nn.functional.binary_cross_entropy_with_logits(z, y.double())


def train_step64(x32, weights, biases, edge_index, edge_weight, local_targets, labels, gates=None):
    """(loss, [dW...], [db...], logits) in fp64 by autograd."""
    x = torch.as_tensor(np.asarray(x32, dtype=F64))
    params = [(torch.as_tensor(np.asarray(W, dtype=F64)).requires_grad_(True), torch.as_tensor(np.asarray(b, dtype=F64)).requires_grad_(True))
              for W, b in zip(weights, biases)]
    logits = gcn_forward64(x, params, edge_index, edge_weight, gates)
    loss = loss64(logits, local_targets, labels)
    loss.backward()
    return (float(loss.detach()), [p[0].grad.numpy() if p[0].grad is not None else np.zeros(tuple(p[0].shape)) for p in params],
            [p[1].grad.numpy() for p in params], logits.detach().numpy())


# --------------------------------------------------------------------------------------------- graphs
def csr_from_edges(src, dst, n):
    """(indptr int64, indices int32) of the entries (src[k], dst[k]): duplicates collapse, columns ascending."""
    key = np.unique(np.asarray(src, dtype=np.int64) * n + np.asarray(dst, dtype=np.int64))
    r, c = key // n, key % n
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64), c.astype(np.int32)


def random_symmetric(n, max_deg, seed, loops=0):
    """A symmetric graph of degree <= max_deg: n max_deg / 2 random pairs, one accepted while both ends have room; `loops` nodes
    also store (i, i), which does not count."""
    rng = np.random.default_rng(seed)
    deg, seen, s, d = np.zeros(n, np.int64), set(), [], []
    for a, b in rng.integers(0, n, (n * max(1, max_deg // 2), 2)):
        if a != b and deg[a] < max_deg and deg[b] < max_deg and (min(a, b), max(a, b)) not in seen:
            seen.add((min(a, b), max(a, b)))
            deg[a] += 1; deg[b] += 1
            s += [a, b]; d += [b, a]
    lp = rng.choice(n, loops, replace=False) if loops else np.zeros(0, np.int64)
    return csr_from_edges(np.concatenate([np.array(s, np.int64), lp]), np.concatenate([np.array(d, np.int64), lp]), n)


def hand_graph():
    """12 nodes, symmetric: a path 0-1-2-3, a triangle 4-5-6 joined to 3, a star 7 <- 8, 9, 10 joined to 6; node 2 stores a loop; node
    11 is isolated."""
    e = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (4, 6), (6, 7), (7, 8), (7, 9), (7, 10)]
    s = [a for a, b in e] + [b for a, b in e] + [2]
    d = [b for a, b in e] + [a for a, b in e] + [2]
    return csr_from_edges(s, d, 12) + (12,)


def dense_p(indptr, indices, n):
    """P = D^-1 (A + I) as a dense matrix: the brute force the oracle is checked against."""
    V = np.eye(n)
    for i in range(n):
        for j in indices[indptr[i]:indptr[i + 1]]:
            V[i, j] += 1.0
    return V / V.sum(1, keepdims=True)
