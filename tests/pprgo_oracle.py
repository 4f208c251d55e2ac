"""PPRGo's rules in numpy, independent of the product: the slot tables of grapes_pprgo_topk from the push and the member order of
tests/shadow_ppr_oracle.py; the batch structure of grapes_pprgo_batch by np.unique and a stable sort; the weights, the forward and
backward of the weighted gather and the power iteration in fp64."""
from types import SimpleNamespace

import numpy as np

from tests import shadow_ppr_oracle as PO

U = 2.0 ** -24                                                           # fp32's unit roundoff


def gamma(n):
    """gamma_n = n u / (1 - n u): the bound on a sum of n roundings in any order, with or without fma."""
    return n * U / (1.0 - n * U)


# --------------------------------------------------------------------------------------------- the slot tables
def topk(indptr, indices, roots, k, alpha_q, thr, max_rounds, live=None, pushes=None):
    """nbr, score [m, K], cnt, rounds, stop [m] and bad (the status bit) of grapes_pprgo_topk; live: *d_m (default m).  pushes: a
    dictionary the caller keeps per graph and settings — a root's push is run once and shared among the k of a test."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n, K = len(indptr) - 1, k + 1
    roots = [int(x) for x in np.asarray(roots).reshape(-1)]
    m = len(roots)
    live = m if live is None else live
    nbr, score = np.zeros((m, K), dtype=np.int64), np.zeros((m, K), dtype=np.int64)
    cnt, rounds, stop, bad = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), False
    for b, root in enumerate(roots):
        if b >= live or not 0 <= root < n:
            bad = bad or b < live
            nbr[b] = -1
            continue
        res = pushes.get(root) if pushes is not None else None
        if res is None:
            res = PO.push(indptr, indices, root, alpha_q, thr, max_rounds)
            if pushes is not None:
                pushes[root] = res
        mem = PO.members(res, k)
        bad = bad or res.bad
        nbr[b], cnt[b], rounds[b], stop[b] = root, len(mem), res.rounds, res.stop
        nbr[b, :len(mem)] = mem
        score[b, :len(mem)] = [res.score[v] for v in mem]
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return SimpleNamespace(nbr=i32(nbr), score=i32(score), cnt=i32(cnt), rounds=i32(rounds), stop=i32(stop), bad_index=bad)


# --------------------------------------------------------------------------------------------- the batch structure
def batch(nbr, cnt, num_nodes):
    """node_idx, n, loc [m, K], tptr [n + 1], tslot [E], E and bad of grapes_pprgo_batch (capacities that hold everything)."""
    nbr, cnt = np.asarray(nbr, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    m, K = nbr.shape
    c = np.clip(cnt, 0, K)
    live = np.arange(K)[None, :] < c[:, None]
    ok = live & (nbr >= 0) & (nbr < num_nodes)
    node_idx = np.unique(nbr[ok])                                        # ascending, duplicate-free
    n = len(node_idx)
    rank = lambda ids: np.searchsorted(node_idx, ids) if n else np.zeros_like(ids)
    loc = np.full((m, K), -1, dtype=np.int64)
    loc[ok] = rank(nbr[ok])
    for b in range(m):                                                   # a dead slot repeats slot 0's value
        loc[b, c[b]:] = loc[b, 0] if c[b] > 0 else -1
    flat = np.nonzero(ok.reshape(-1))[0]                                 # ascending flat slot indices
    src = loc.reshape(-1)[flat]
    order = np.argsort(src, kind="stable")                               # by source, ascending slots inside a source
    tslot = flat[order]
    tptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=tptr[1:])
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return SimpleNamespace(node_idx=i32(node_idx), n=n, loc=i32(loc), tptr=i32(tptr), tslot=i32(tslot), e=len(tslot),
                           bad_index=bool((live & ~ok).any()))


# --------------------------------------------------------------------------------------------- weights and the gathers, fp64
def degrees(indptr):
    return np.maximum(np.diff(np.asarray(indptr, dtype=np.int64)), 1).astype(np.float64)


def weights(indptr, roots, nbr, score, cnt, normalization="row"):
    """weight [m, K] in fp64: score / 2^30, times sqrt(d_b / d_v) ("sym") or d_b / d_v ("col"); 0 in dead slots."""
    d = degrees(indptr)
    nbr, roots = np.asarray(nbr, dtype=np.int64), np.asarray(roots, dtype=np.int64)
    live = np.arange(nbr.shape[1])[None, :] < np.asarray(cnt)[:, None]
    w = np.asarray(score, dtype=np.float64) / 2.0 ** 30
    v = np.where(live, nbr, roots[:, None])
    if normalization == "sym":
        w = w * np.sqrt(d[roots])[:, None] / np.sqrt(d[v])
    elif normalization == "col":
        w = w * d[roots][:, None] / d[v]
    else:
        assert normalization == "row"
    return np.where(live, w, 0.0)


def aggregate_fwd(z, w, loc, cnt):
    """(out, mag) fp64 [m, F]: out[b] = sum_{t < cnt[b]} w[b, t] z[loc[b, t]] and mag the same sum of absolute values."""
    z, w = np.asarray(z, dtype=np.float64), np.asarray(w, dtype=np.float64)
    m = len(cnt)
    out, mag = np.zeros((m, z.shape[1])), np.zeros((m, z.shape[1]))
    for b in range(m):
        c = int(cnt[b])
        if c:
            wb, zb = w[b, :c, None], z[np.asarray(loc[b, :c], dtype=np.int64)]
            out[b], mag[b] = (wb * zb).sum(0), np.abs(wb * zb).sum(0)
    return out, mag


def aggregate_bwd(g, w, tptr, tslot, K):
    """(dz, mag) fp64 [n, F]: dz[u] = sum over s in tslot[tptr[u] : tptr[u + 1]] of w[s] g[s // K]."""
    g, wf = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64).reshape(-1)
    n = len(tptr) - 1
    dz, mag = np.zeros((n, g.shape[1])), np.zeros((n, g.shape[1]))
    for u in range(n):
        s = np.asarray(tslot[tptr[u]:tptr[u + 1]], dtype=np.int64)
        if len(s):
            t = wf[s, None] * g[s // K]
            dz[u], mag[u] = t.sum(0), np.abs(t).sum(0)
    return dz, mag


# --------------------------------------------------------------------------------------------- power iteration, dense fp64
def dense_adjacency(indptr, indices, drop_loops=False):
    n = len(indptr) - 1
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), np.diff(indptr)), np.asarray(indices, dtype=np.int64)), 1.0)
    if drop_loops:
        A[np.arange(n), np.arange(n)] = 0.0
    return A


def transition(A, normalization="row"):
    """S = D^-1 A, D^-1/2 A D^-1/2 or A D^-1 with d = max(row sum, 1)."""
    d = np.maximum(A.sum(1), 1.0)
    if normalization == "row":
        return A / d[:, None]
    if normalization == "sym":
        return A / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]
    assert normalization == "col"
    return A / d[None, :]


def power_iteration(S, Z, alpha, nprop):
    """Q_0 = Z, then Q <- (1 - alpha) S Q + alpha Z, nprop times."""
    Q = np.array(Z, dtype=np.float64)
    for _ in range(nprop):
        Q = (1.0 - alpha) * (S @ Q) + alpha * Z
    return Q
