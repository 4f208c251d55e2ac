"""Host oracle of LINKX's adjacency embedding bag (include/grapes_hip.h: grapes_bag_batch / _fwd / _bwd / _bwd_adam), numpy and torch
on the CPU.  Integers are reproduced exactly; floats are fp64 (or, for adam_rows, whatever dtype the caller hands in)."""
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24


def gamma(d):
    d = np.asarray(d, dtype=np.float64)
    return d * U / (1.0 - d * U)


def csr(rows_of, n):
    """(rowptr int64 [n + 1], col int32) of a list of lists, entries as given (duplicates, loops and any order kept)."""
    ip = np.zeros(n + 1, dtype=np.int64)
    for i, r in enumerate(rows_of):
        ip[i + 1] = ip[i] + len(r)
    ix = np.array([c for r in rows_of for c in r], dtype=np.int32)
    return ip, ix


def batch(ip, ix, rows):
    """The tables of grapes_bag_batch for valid rows (an id outside [0, N) is an empty row) and valid columns."""
    N = len(ip) - 1
    rows = np.asarray(rows, dtype=np.int64)
    ok = (rows >= 0) & (rows < N)
    deg = np.where(ok, ip[np.clip(rows, 0, N - 1) + 1] - ip[np.clip(rows, 0, N - 1)], 0)
    bptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ent = [ix[ip[r]:ip[r + 1]] if k else ix[:0] for r, k in zip(np.clip(rows, 0, N - 1), ok)]
    cols = np.concatenate(ent) if len(ent) else ix[:0]
    brow = np.repeat(np.arange(len(rows)), deg)
    keep = (cols >= 0) & (cols < N)
    cols, brow = cols[keep].astype(np.int64), brow[keep]
    uniq = np.unique(cols).astype(np.int32)
    order = np.lexsort((brow, cols))                                   # by column, then by batch row: duplicates stay adjacent
    trow = brow[order].astype(np.int32)
    cnt = np.bincount(np.searchsorted(uniq, cols), minlength=len(uniq)) if len(uniq) else np.zeros(0, dtype=np.int64)
    tptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    return SimpleNamespace(bptr=bptr, uniq=uniq, tptr=tptr, trow=trow, n_u=len(uniq), e=int(bptr[-1]),
                           seg_max=int(cnt.max()) if len(cnt) else 0, row_max=int(deg.max()) if len(deg) else 0)


def count_matrix(ip, ix, rows):
    """A[rows] as a dense count matrix [m, N] (fp64): entry (b, j) = how often row rows[b] stores column j."""
    N = len(ip) - 1
    A = np.zeros((len(rows), N))
    for b, r in enumerate(rows):
        if 0 <= r < N:
            np.add.at(A[b], ix[ip[r]:ip[r + 1]], 1.0)
    return A


def fwd(ip, ix, rows, W, bias=None):
    """(out fp64 [m, H], mag): out[b] = bias + sum W[col[t]] and mag = |bias| + sum |W[col[t]]|."""
    N = len(ip) - 1
    W = np.asarray(W, dtype=np.float64)
    out = np.zeros((len(rows), W.shape[1]))
    mag = np.zeros_like(out)
    if bias is not None:
        out += np.asarray(bias, dtype=np.float64)
        mag += np.abs(np.asarray(bias, dtype=np.float64))
    for b, r in enumerate(rows):
        if 0 <= r < N:
            c = ix[ip[r]:ip[r + 1]]
            out[b] += W[c].sum(0)
            mag[b] += np.abs(W[c]).sum(0)
    return out, mag


def grad_rows(bt, G):
    """(values fp64 [n_u, H], mag) of the row-sparse gradient: values[s] = sum of G[trow[q]] over segment s."""
    G = np.asarray(G, dtype=np.float64)
    vals = np.zeros((bt.n_u, G.shape[1]))
    mag = np.zeros_like(vals)
    for s in range(bt.n_u):
        r = bt.trow[bt.tptr[s]:bt.tptr[s + 1]]
        vals[s] = G[r].sum(0)
        mag[s] = np.abs(G[r]).sum(0)
    return vals, mag


class _BagFn(torch.autograd.Function):
    """The oracle's layer under autograd: a sparse COO gradient over bt.uniq for W."""

    @staticmethod
    def forward(ctx, W, bias, A, bt):
        ctx.A, ctx.bt, ctx.shape = A, bt, W.shape
        return A @ W + bias

    @staticmethod
    def backward(ctx, G):
        vals, _ = grad_rows(ctx.bt, G.numpy())
        idx = torch.as_tensor(ctx.bt.uniq.astype(np.int64))[None]
        return torch.sparse_coo_tensor(idx, torch.as_tensor(vals, dtype=G.dtype), ctx.shape), G.sum(0), None, None


def bag(W, bias, ip, ix, rows):
    bt = batch(ip, ix, rows)
    return _BagFn.apply(W, bias, torch.as_tensor(count_matrix(ip, ix, rows), dtype=W.dtype), bt)


def adam_rows(p, m, v, uniq, g, lr, beta1, beta2, eps, t):
    """The rule of grapes_bag_bwd_adam on rows uniq of p, m, v (numpy arrays, updated in place, in their own dtype): every
    operation rounded once in that dtype; step_size formed in double."""
    dt = p.dtype.type
    ss = dt(lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
    o1, o2, ep = dt(1.0 - beta1), dt(1.0 - beta2), dt(eps)
    g = g.astype(p.dtype)
    mo, vo = m[uniq], v[uniq]
    mn = mo + o1 * (g - mo)
    vn = vo + o2 * (g * g - vo)
    p[uniq] = p[uniq] - ss * (mn / (np.sqrt(vn) + ep))
    m[uniq], v[uniq] = mn, vn


def linkx_forward(sd, A, xb):
    """The five lines of LINKX's forward, literally, on a state dict of tensors, A = the count matrix of the batch rows [m, N] and
    xb [m, F]; ReLU between the layers of an MLP, none behind its last."""
    def mlp(prefix, h):
        k = 0
        while f"{prefix}.lins.{k}.weight" in sd:
            if k:
                h = torch.relu(h)
            h = h @ sd[f"{prefix}.lins.{k}.weight"].T + sd[f"{prefix}.lins.{k}.bias"]
            k += 1
        return h
    out = A @ sd["edge_lin.weight"] + sd["edge_lin.bias"]
    out = out + (out @ sd["cat_lin1.weight"].T + sd["cat_lin1.bias"])
    x = mlp("node_mlp", xb)
    out = out + x + (x @ sd["cat_lin2.weight"].T + sd["cat_lin2.bias"])
    return mlp("final_mlp", torch.relu(out))


def random_graph(n, mean_deg, seed, dup=0.1, loops=True, empty=(3,)):
    """A directed multigraph: rows of Poisson length, some entries repeated, some loops, the rows in `empty` empty, order as drawn."""
    rng = np.random.default_rng(seed)
    rows_of = []
    for i in range(n):
        d = 0 if i in empty else int(rng.poisson(mean_deg))
        r = rng.integers(0, n, d).tolist()
        if r and rng.random() < dup:
            r.append(r[0]); r.append(r[-2])
        if loops and i % 7 == 0 and i not in empty:
            r.append(i)
        rows_of.append(r)
    return csr(rows_of, n)
