"""TEST INFRASTRUCTURE — PinSAGE's rules in numpy and Python integers, independent of the product: the walks and the selection of
grapes_pinsage_neighbors (include/grapes_hip.h is the contract) with dictionaries and a plain sort where the kernel sorts in LDS; the
weights; the block chain over tests/pprgo_oracle.py's batch structure; the exact expectation of the visit counts from a dense fp64
matrix power; relu + L2 normalisation, PinSAGEConv and the model in fp64.  Only tests import this module; it imports nothing of the
product."""
from types import SimpleNamespace

import numpy as np

from tests import pprgo_oracle as GO
from tests.shadow_oracle import philox4x32_10_wide

U = 2.0 ** -24                                                           # fp32's unit roundoff
TINY = 2.0 ** -149                                                       # the smallest subnormal
gamma = GO.gamma


def term_q(p):
    return min(2 ** 32 - 1, int(round(float(p) * 2 ** 32)))


# --------------------------------------------------------------------------------------------- the walks
def walk(indptr, indices, v, j, L, tq, seed, off):
    """(visits, bad): the visited nodes of walk j of root v in step order, returns to the root left out."""
    n, c, out = len(indptr) - 1, int(v), []
    words = None
    for t in range(L):
        if t % 2 == 0:
            words = philox4x32_10_wide(int(v) | (int(j) << 32), (int(off) + (t >> 1)) & (2 ** 64 - 1), seed)
        a, s = words[2 * (t & 1)], words[2 * (t & 1) + 1]
        beg, deg = int(indptr[c]), int(indptr[c + 1]) - int(indptr[c])
        if a < tq or deg == 0:
            break
        c = int(indices[beg + ((s * deg) >> 32)])
        if not 0 <= c < n:
            return out, True
        if c != v:
            out.append(c)
    return out, False


def counts_of(indptr, indices, v, R, L, tq, seed, off):
    """({node: visits over the root's R walks}, bad)."""
    cnt, bad = {}, False
    for j in range(R):
        vs, b = walk(indptr, indices, v, j, L, tq, seed, off)
        bad = bad or b
        for u in vs:
            cnt[u] = cnt.get(u, 0) + 1
    return cnt, bad


def select(cnt, V, T):
    """The kept (node, count) pairs: the min(T, distinct) smallest keys ((V - count) << 32) | node, in key order."""
    keys = sorted(((V - c) << 32) | u for u, c in cnt.items())[:T]
    return [(k & 0xFFFFFFFF, V - (k >> 32)) for k in keys]


def neighbors(indptr, indices, roots, R, L, tq, T, seed=0, off=0, live=None, memo=None):
    """nbr, visits [m, K], cnt [m] and bad_index of grapes_pinsage_neighbors; live: *d_m (default m).  memo: a dictionary the caller
    keeps per (graph, R, L, tq, seed, off) — a root's counts are computed once and shared among the T of a test."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n, K, V = len(indptr) - 1, T + 1, R * L
    roots = [int(x) for x in np.asarray(roots).reshape(-1)]
    m = len(roots)
    live = m if live is None else live
    nbr, vis, cnt, bad = np.zeros((m, K), dtype=np.int64), np.zeros((m, K), dtype=np.int64), np.zeros(m, dtype=np.int64), False
    for b, v in enumerate(roots):
        if b >= live or not 0 <= v < n:
            bad = bad or b < live
            nbr[b] = -1
            continue
        res = memo.get(v) if memo is not None else None
        if res is None:
            res = counts_of(indptr, indices, v, R, L, tq, seed, off)
            if memo is not None:
                memo[v] = res
        bad = bad or res[1]
        kept = select(res[0], V, T)
        nbr[b], cnt[b] = v, 1 + len(kept)
        for t, (u, c) in enumerate(kept):
            nbr[b, 1 + t], vis[b, 1 + t] = u, c
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return SimpleNamespace(nbr=i32(nbr), visits=i32(vis), cnt=i32(cnt), bad_index=bad)


def weights(visits):
    """weight fp32 [m, K]: visits / the row's total in ONE fp32 division, 0 where the row has no visit."""
    v = np.asarray(visits, dtype=np.float32)
    tot = v.sum(1, keepdims=True, dtype=np.float32)
    return np.where(tot > 0, v / np.maximum(tot, np.float32(1)), np.float32(0)).astype(np.float32)


def sample(indptr, indices, roots, num_layers, R, L, tq, T, seed=0, off=0):
    """The blocks of PinSAGESampler.sample: block d on seeds_d (seeds_0 = roots, seeds_{d + 1} = node_idx_d) at offset off + d
    ceil(L / 2)."""
    n, blocks, seeds = len(indptr) - 1, [], np.asarray(roots, dtype=np.int32)
    for d in range(num_layers):
        nb = neighbors(indptr, indices, seeds, R, L, tq, T, seed, off + d * ((L + 1) // 2))
        ob = GO.batch(nb.nbr, nb.cnt, n)
        blocks.append(SimpleNamespace(seeds=seeds, nbr=nb.nbr, visits=nb.visits, cnt=nb.cnt, weight=weights(nb.visits),
                                      node_idx=ob.node_idx, num_nodes=ob.n, loc=ob.loc, tptr=ob.tptr, tslot=ob.tslot, num_slots=ob.e))
        seeds = ob.node_idx
    return blocks


# --------------------------------------------------------------------------------------------- the expectation
def expected_visits(indptr, indices, r, R, L, p):
    """E[count[u]] = R sum_{t = 1 .. L} (1 - p)^t [P^t]_{r, u} for u != r, with dead ends absorbing (a walk that stops visits
    nothing more): P is the row-normalised adjacency by multiplicity, a row without an entry all zero.  fp64, dense."""
    A = GO.dense_adjacency(indptr, indices)
    d = A.sum(1)
    P = np.divide(A, d[:, None], out=np.zeros_like(A), where=d[:, None] > 0)
    e, Pt = np.zeros(len(d)), np.eye(len(d))
    for t in range(1, L + 1):
        Pt = Pt @ P
        e += (1.0 - p) ** t * Pt[r]
    e *= R
    e[r] = 0.0
    return e


# --------------------------------------------------------------------------------------------- relu + L2 normalisation, fp64
def relu_l2norm64(s, eps):
    """(out, nrm) in fp64."""
    z = np.maximum(np.asarray(s, dtype=np.float64), 0.0)
    nrm = np.sqrt((z * z).sum(1))
    return z / np.maximum(nrm, eps)[:, None], nrm


def relu_l2norm_bwd64(g, s, eps):
    """(ds, mag) in fp64: ds = [s > 0] (g - out <g, out> [nrm >= eps]) / max(nrm, eps) and mag = (|g| + |out| sum |g out|) /
    max(nrm, eps), the sum of the absolute terms."""
    g, s = np.asarray(g, dtype=np.float64), np.asarray(s, dtype=np.float64)
    out, nrm = relu_l2norm64(s, eps)
    d = np.maximum(nrm, eps)[:, None]
    dot = (g * out).sum(1, keepdims=True) * (nrm >= eps)[:, None]
    ds = (s > 0) * (g - out * dot) / d
    mag = (np.abs(g) + np.abs(out) * np.abs(g * out).sum(1, keepdims=True)) / d
    return ds, mag


def torch_relu_l2norm(s, eps):
    """The plain-torch restatement (any dtype, with autograd)."""
    import torch
    z = torch.relu(s)
    return z / z.pow(2).sum(1, keepdim=True).sqrt().clamp(min=eps)


def torch_conv(h, block, Qw, Qb, Ww, Wb, eps):
    """PinSAGEConv restated in plain torch over an oracle block (any dtype, with autograd)."""
    import torch
    K = block.nbr.shape[1]
    z = torch.relu(h @ Qw.T + Qb)
    live = torch.as_tensor((np.arange(K)[None, :] < np.asarray(block.cnt)[:, None])).to(h.dtype)
    w = torch.as_tensor(np.asarray(block.weight)).to(h.dtype) * live
    loc = torch.as_tensor(np.maximum(np.asarray(block.loc), 0).astype(np.int64))
    n = (w[:, :, None] * z[loc]).sum(1)
    s = torch.cat([h[loc[:, 0]], n], dim=1) @ Ww.T + Wb
    return torch_relu_l2norm(s, eps)


def torch_model(xb, blocks, convs, lin, eps):
    """PinSAGE restated: convs = [(Qw, Qb, Ww, Wb), ...] deepest block first, lin = (w, b)."""
    h = xb
    for prm, block in zip(convs, reversed(blocks)):
        h = torch_conv(h, block, *prm, eps)
    return h @ lin[0].T + lin[1]
