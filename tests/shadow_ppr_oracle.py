"""TEST INFRASTRUCTURE — ShaDow-GNN's PPR scope restated on the host in Python integers [Zeng et al., NeurIPS 2021 for the scope;
Andersen, Chung, Lang, FOCS 2006 for the forward push — both recalled].  The rule of include/grapes_hip.h (grapes_shadow_ppr_sample) is
the contract; this file states it a second time, with DIFFERENT algorithms where the kernel's could be wrong:

  push       the synchronous fixed-point rounds over Python dictionaries (the kernel: an LDS hash, integer atomics, a workgroup scan
             and a flat walk of the frontier's entries), with the three stops in the rule's order
  members    the root and the k best of a FULL sort by (-score, id) (the kernel: a bitonic sort of 64-bit keys)
  sample     the batch: the ego-nets concatenated in root order with every output of the device call, the induced entries by
             shadow_oracle.induced_edges
  exact_ppr  pi = alpha (I - (1 - alpha) P^T)^-1 e_root in fp64, P = D^-1 A
  planted_graph   the symmetric planted graph the estimate is judged on
Only tests import this module; it imports nothing of the product.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests import shadow_oracle as SO

ONE = 1 << 30
T = 4096
MAX_K, MAX_ROUNDS = 1023, 1024


def fixed(alpha, eps):
    """(alpha_q, thr) as the sampler derives them."""
    return int(round(alpha * 2 ** 16)), max(1, int(round(eps * 2 ** 30)))


def push(indptr, indices, root, alpha_q, thr, max_rounds, after_round=None):
    """The rounds of one root -> p, r, score (dictionaries over the touched set S), rounds, stop, bad (a column outside [0, N) was
    met).  after_round(r, p) is called behind every round that ran."""
    assert 1 <= alpha_q <= 65535 and 1 <= thr <= ONE and 1 <= max_rounds <= MAX_ROUNDS
    n = len(indptr) - 1
    root = int(root)
    deg = lambda v: int(indptr[v + 1] - indptr[v])
    r, p = {root: ONE}, {root: 0}
    rounds, bad = 0, False
    while True:
        front = [v for v in r if r[v] > 0 and r[v] >= thr * deg(v)]
        if not front:
            stop = 0
            break
        if rounds == max_rounds:
            stop = 1
            break
        if len(r) + sum(deg(v) for v in front) > T:
            stop = 2
            break
        snap = [(v, r[v]) for v in front]
        for v, _ in snap:
            r[v] = 0
        for v, rv in snap:
            d = deg(v)
            if d == 0:
                p[v] += rv
                continue
            keep = (rv * alpha_q) >> 16
            p[v] += keep
            share = (rv - keep) // d
            for u in indices[int(indptr[v]):int(indptr[v + 1])]:
                u = int(u)
                if not 0 <= u < n:
                    bad = True
                    continue
                if u not in r:
                    r[u], p[u] = 0, 0
                r[u] += share
        rounds += 1
        assert len(r) <= T and sum(r.values()) + sum(p.values()) <= ONE
        if after_round is not None:
            after_round(r, p)
    score = {v: p[v] + ((r[v] * alpha_q) >> 16) for v in r}
    return SimpleNamespace(p=p, r=r, score=score, rounds=rounds, stop=stop, bad=bad, root=root)


def members(res, k):
    """The root, then the k best nodes with a positive score: score descending, id ascending (a full sort)."""
    rest = sorted((v for v in res.score if v != res.root and res.score[v] > 0), key=lambda v: (-res.score[v], v))
    return [res.root] + rest[:k]


def sample(indptr, indices, roots, k, alpha_q, thr, max_rounds):
    """The batch of grapes_shadow_ppr_sample for the roots in order; `pushes` holds push()'s result per root (None for a bad root)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    assert 1 <= k <= MAX_K
    roots = [int(x) for x in np.asarray(roots).reshape(-1)]
    n_id, ptr, batch, root_n_id, src, dst, e_id, score, rounds, stop, pushes, bad = [], [0], [], [], [], [], [], [], [], [], [], False
    for b, root in enumerate(roots):
        if not 0 <= root < n:
            bad = True
            ptr.append(ptr[-1]); root_n_id.append(-1); rounds.append(0); stop.append(0); pushes.append(None)
            continue
        res = push(indptr, indices, root, alpha_q, thr, max_rounds)
        mem = sorted(members(res, k))
        assert len(mem) == len(set(mem)) <= k + 1
        bad = bad or res.bad or any(not 0 <= int(c) < n for u in mem for c in indices[indptr[u]:indptr[u + 1]])
        base = ptr[-1]
        s, d, pos = SO.induced_edges(indptr, indices, mem)
        n_id += mem; batch += [b] * len(mem); ptr.append(base + len(mem)); root_n_id.append(base + mem.index(root))
        score += [res.score[v] for v in mem]
        src += [base + x for x in s]; dst += [base + x for x in d]; e_id += pos
        rounds.append(res.rounds); stop.append(res.stop); pushes.append(res)
    i32 = lambda a: np.asarray(a, dtype=np.int32).reshape(-1)
    return SimpleNamespace(n_id=i32(n_id), ptr=i32(ptr), batch=i32(batch), root_n_id=i32(root_n_id),
                           edge_index=np.stack([i32(src), i32(dst)]), e_id=np.asarray(e_id, dtype=np.int64).reshape(-1),
                           score=i32(score), rounds=i32(rounds), stop=i32(stop), n=len(n_id), e=len(src), bad_index=bad, pushes=pushes)


# --------------------------------------------------------------------------------------------- exact PPR and its graph
def exact_ppr(indptr, indices, root, alpha):
    """pi = alpha (I - (1 - alpha) P^T)^-1 e_root in fp64; P = D^-1 A with A's multiplicities (every row must hold an entry)."""
    n = len(indptr) - 1
    A = np.zeros((n, n))
    for v in range(n):
        for u in indices[indptr[v]:indptr[v + 1]]:
            A[v, int(u)] += 1.0
    P = A / A.sum(1, keepdims=True)
    e = np.zeros(n)
    e[int(root)] = 1.0
    return alpha * np.linalg.solve(np.eye(n) - (1.0 - alpha) * P.T, e)


def planted_graph(n=600, groups=6, seed=0):
    """A symmetric planted graph: n nodes in `groups` equal groups; every node has 4 partners inside its group (the union of two random
    Hamiltonian cycles of the group) and 1 outside (a random perfect matching that joins no two nodes of one group); every edge is
    stored both ways, so every row holds exactly 5 entries (a pair joined by both cycles is stored with its multiplicity)."""
    rng = np.random.default_rng(seed)
    size = n // groups
    assert size * groups == n and n % 2 == 0
    rows = [[] for _ in range(n)]
    for g in range(groups):
        for _ in range(2):
            cyc = g * size + rng.permutation(size)
            for a, b in zip(cyc, np.roll(cyc, -1)):
                rows[int(a)].append(int(b)); rows[int(b)].append(int(a))
    perm = rng.permutation(n)
    left, right = perm[0::2].copy(), perm[1::2].copy()
    for _ in range(10000):
        clash = np.nonzero(left // size == right // size)[0]
        if len(clash) == 0:
            break
        j, l = int(clash[0]), int(rng.integers(0, len(left)))
        right[j], right[l] = right[l], right[j]
    assert (left // size != right // size).all()
    for a, b in zip(left, right):
        rows[int(a)].append(int(b)); rows[int(b)].append(int(a))
    assert all(len(r) == 5 for r in rows)
    return SO.csr([sorted(r) for r in rows])
