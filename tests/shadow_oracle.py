"""TEST INFRASTRUCTURE — ShaDow-GNN's per-root ego-net sampler restated on the host in NumPy and Python integers [Zeng et al., NeurIPS
2021; PyG-recall: ShaDowKHopSampler].  The rule of include/grapes_hip.h (grapes_shadow_sample) is the contract; this file states it a
second time, with DIFFERENT algorithms where the kernel's could be wrong:

  philox4x32_10_wide   Philox4x32-10 over the whole 128-bit counter, in Python integers (one call at a time, no vector arithmetic)
  row_words            w_s of a row: word s & 3 at the counter (low = v << 4 | s >> 2, high = off + b depth + h - 1)
  floyd                Floyd's rule over given words, with a Python set (the kernel: one position per lane and a ballot)
  ego_net              the hop recursion with Python sets (the kernel: an LDS hash, a node list and a bitonic sort)
  induced_edges        a plain double loop over the members and their rows with a dictionary of ranks (the kernel: binary searches
                       of the sorted set and ballots)
  sample               the batch: the ego-nets concatenated in root order, with every output of the device call
  segment_mean64 / segment_mean_bwd64   the readout's mean in fp64
Only tests import this module; it imports nothing of the product.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

_M32 = 0xFFFFFFFF
MAX_NODES, MAX_FANOUT = 1024, 64


def philox4x32_10_wide(lo, hi, seed):
    """The four 32-bit words of Philox4x32-10 at the 128-bit counter (lo = c0 | c1 << 32, hi = c2 | c3 << 32) under the 64-bit key."""
    lo, hi, seed = int(lo) & (2 ** 64 - 1), int(hi) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    c0, c1, c2, c3 = lo & _M32, lo >> 32, hi & _M32, hi >> 32
    k0, k1 = seed & _M32, seed >> 32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return [c0, c1, c2, c3]


def cap(depth, fanout):
    """C = 1 + k + ... + k^depth."""
    return sum(int(fanout) ** h for h in range(int(depth) + 1))


def row_words(seed, off, b, depth, h, v, fanout):
    """[w_0 .. w_{k-1}] of the row v expanded by root b at hop h (1-based)."""
    hi = int(off) + b * depth + (h - 1)
    calls = [philox4x32_10_wide((int(v) << 4) | q, hi, seed) for q in range((fanout + 3) // 4)]
    return [calls[s >> 2][s & 3] for s in range(fanout)]


def floyd(deg, fanout, words):
    """The chosen positions of a row of deg > fanout entries, as a set: for s = 0 .. k - 1, j = deg - k + s, t = (w_s (j + 1)) >> 32;
    t when it is absent, else j."""
    chosen = set()
    for s in range(fanout):
        j = deg - fanout + s
        t = (int(words[s]) * (j + 1)) >> 32
        assert 0 <= t <= j
        chosen.add(j if t in chosen else t)
    assert len(chosen) == fanout
    return chosen


def ego_net(indptr, indices, root, depth, fanout, words_of):
    """S_depth of one root as a Python set.  words_of(h, v) -> the k words of row v at hop h.  Columns outside [0, N) are dropped."""
    n = len(indptr) - 1
    seen, frontier = {int(root)}, {int(root)}
    for h in range(1, depth + 1):
        reached = set()
        for v in frontier:
            a, deg = int(indptr[v]), int(indptr[v + 1] - indptr[v])
            pos = range(deg) if deg <= fanout else floyd(deg, fanout, words_of(h, v))
            reached.update(int(indices[a + t]) for t in pos if 0 <= int(indices[a + t]) < n)
        frontier = reached - seen
        seen |= reached
    return seen


def induced_edges(indptr, indices, members):
    """(src local, dst local, position in col) of every stored entry with both ends among the ascending list `members`: rows ascending,
    within a row in the CSR's order; duplicates and loops stay."""
    rank = {int(m): r for r, m in enumerate(members)}
    assert len(rank) == len(members) and list(members) == sorted(members)
    src, dst, pos = [], [], []
    for i, u in enumerate(members):
        for p in range(int(indptr[u]), int(indptr[u + 1])):
            r = rank.get(int(indices[p]))
            if r is not None:
                src.append(r); dst.append(i); pos.append(p)
    return src, dst, pos


def sample(indptr, indices, roots, depth, fanout, seed=0, philox_offset=0, words=None):
    """The batch of grapes_shadow_sample for the roots in order.  words: uint32 [B, depth, k] replacing the Philox words.  A root
    outside [0, N) gives an empty ego-net and root_n_id -1 (bad_index set)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    C = cap(depth, fanout)
    assert depth >= 1 and 1 <= fanout <= MAX_FANOUT and C <= MAX_NODES
    roots = [int(r) for r in np.asarray(roots).reshape(-1)]
    if words is not None:
        words = np.asarray(words).view(np.uint32).reshape(len(roots), depth, fanout)
    n_id, ptr, batch, root_n_id, src, dst, e_id, bad = [], [0], [], [], [], [], [], False
    for b, root in enumerate(roots):
        if not 0 <= root < n:
            bad = True
            ptr.append(ptr[-1]); root_n_id.append(-1)
            continue
        if words is not None:
            words_of = lambda h, v, b=b: [int(w) for w in words[b, h - 1]]
        else:
            words_of = lambda h, v, b=b: row_words(seed, philox_offset, b, depth, h, v, fanout)
        members = sorted(ego_net(indptr, indices, root, depth, fanout, words_of))
        assert len(members) <= C
        base = ptr[-1]
        s, d, p = induced_edges(indptr, indices, members)
        n_id += members; batch += [b] * len(members); ptr.append(base + len(members)); root_n_id.append(base + members.index(root))
        src += [base + r for r in s]; dst += [base + r for r in d]; e_id += p
    i32 = lambda a: np.asarray(a, dtype=np.int32).reshape(-1)
    return SimpleNamespace(n_id=i32(n_id), ptr=i32(ptr), batch=i32(batch), root_n_id=i32(root_n_id),
                           edge_index=np.stack([i32(src), i32(dst)]), e_id=np.asarray(e_id, dtype=np.int64).reshape(-1),
                           n=len(n_id), e=len(src), bad_index=bad, philox_offset=int(philox_offset) + len(roots) * depth)


# --------------------------------------------------------------------------------------------- the segment mean in fp64
def segment_mean64(h, ptr):
    h = np.asarray(h, dtype=np.float64)
    out = np.zeros((len(ptr) - 1, h.shape[1]))
    for b in range(len(ptr) - 1):
        if ptr[b + 1] > ptr[b]:
            out[b] = h[ptr[b]:ptr[b + 1]].sum(0) / (ptr[b + 1] - ptr[b])
    return out


def segment_mean_bwd64(g, ptr, n_rows):
    g = np.asarray(g, dtype=np.float64)
    out = np.zeros((n_rows, g.shape[1]))
    for b in range(len(ptr) - 1):
        if ptr[b + 1] > ptr[b]:
            out[ptr[b]:ptr[b + 1]] = g[b] / (ptr[b + 1] - ptr[b])
    return out


# --------------------------------------------------------------------------------------------- graphs
def csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.asarray([c for r in rows for c in r], dtype=np.int32).reshape(-1)


def random_graph(n, degree, seed, hub=None, hub_degree=0):
    """Rows of about `degree` random columns (with replacement: duplicates occur, loops too); row `hub`, when given, holds hub_degree
    entries.  Not symmetric: the sampler reads rows only."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, n, int(rng.integers(max(degree - 3, 0), degree + 4))).tolist() for _ in range(n)]
    if hub is not None:
        rows[hub] = rng.integers(0, n, hub_degree).tolist()
    return csr(rows)
