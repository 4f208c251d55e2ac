"""TEST INFRASTRUCTURE — VR-GCN restated on the host in fp64 numpy [Chen, Zhu and Song, "Stochastic Training of Graph Convolutional
Networks with Variance Reduction", ICML 2018]: the control-variate estimator from explicit kept-entry lists, its gradient, the
history update, and an L-layer training step that carries its own histories from step to step.

Everything is over a loop-free CSR (loop_free): d_u = the stored entries of row u (duplicates count once each), deg_u = d_u + 1,
dinv_u = deg_u^-1/2, P = D^-1/2 (A + I) D^-1/2.  For a row u with the kept sources kept_u (k_u of its d_u entries; any list):

    A[u] = dinv_u^2 H[u] + (d_u / k_u) sum_{v in kept_u} dinv_u dinv_v (H[v] - Hbar[v]) + sum_{v in row u} dinv_u dinv_v Hbar[v]

H and Hbar are [N, f] arrays on GLOBAL ids here (the rows of H outside the batch are never read).  Hbar is a constant: the
gradient reaches H through the kept entries and the self term only.  Only tests import this module; it imports nothing of the
product.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

F64 = np.float64


def loop_free(indptr, indices):
    """(indptr, indices) without the stored (u, u) entries."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    row = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    keep = row != indices
    return np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=len(indptr) - 1))]).astype(np.int64), indices[keep]


def dinv(indptr):
    return 1.0 / np.sqrt(np.diff(np.asarray(indptr, dtype=np.int64)).astype(F64) + 1.0)


def dense_p(indptr, indices, n):
    """P = D^-1/2 (A + I) D^-1/2 as a dense matrix, every stored entry once."""
    V = np.eye(n)
    for i in range(n):
        for j in indices[indptr[i]:indptr[i + 1]]:
            V[i, j] += 1.0
    di = dinv(indptr)
    return di[:, None] * V * di[None, :]


def aggregate(indptr, indices, rows, kept, H, Hbar):
    """A [m, f] for the listed rows; kept[r] = the global ids of row rows[r]'s kept sources."""
    di = dinv(indptr)
    H, Hbar = np.asarray(H, dtype=F64), np.asarray(Hbar, dtype=F64)
    out = np.zeros((len(rows), H.shape[1]))
    for r, u in enumerate(np.asarray(rows, dtype=np.int64)):
        cols = np.asarray(indices[indptr[u]:indptr[u + 1]], dtype=np.int64)
        kv = np.asarray(kept[r], dtype=np.int64)
        a = di[u] * di[u] * H[u]
        if len(kv):
            a = a + (len(cols) / len(kv)) * di[u] * (di[kv][:, None] * (H[kv] - Hbar[kv])).sum(0)
        if len(cols):
            a = a + di[u] * (di[cols][:, None] * Hbar[cols]).sum(0)
        out[r] = a
    return out


def aggregate_grad(indptr, rows, kept, dA, n):
    """d L / d H [n, f] for d L / d A = dA [m, f]: (d_u / k_u) dinv_u dinv_v dA[u] per kept (u, v), dinv_u^2 dA[u] to u itself."""
    di = dinv(indptr)
    dA = np.asarray(dA, dtype=F64)
    dH = np.zeros((n, dA.shape[1]))
    for r, u in enumerate(np.asarray(rows, dtype=np.int64)):
        d = int(indptr[u + 1] - indptr[u])
        kv = np.asarray(kept[r], dtype=np.int64)
        dH[u] += di[u] * di[u] * dA[r]
        if len(kv):
            np.add.at(dH, kv, (d / len(kv)) * di[u] * di[kv][:, None] * dA[r][None, :])
    return dH


def history_update(Hbar, rows, values):
    """A copy of Hbar with Hbar[rows[r]] = values[r]."""
    out = np.array(Hbar, dtype=F64, copy=True)
    out[np.asarray(rows, dtype=np.int64)] = np.asarray(values, dtype=F64)
    return out


def kept_lists(prev, src, dst):
    """Per row of prev the kept sources, from a layer's flat lists written for the rows in prev's order (prev duplicate-free)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    out, p = [], 0
    for u in np.asarray(prev, dtype=np.int64):
        q = p
        while q < len(dst) and dst[q] == u:
            q += 1
        out.append(src[p:q])
        p = q
    assert p == len(dst), "the layer's entries are not grouped by row in the rows' order"
    return out


def loss_and_grad(z, labels):
    """(mean CrossEntropy for int labels [B] or mean BCEWithLogits for float labels [B, C], d loss / d z)."""
    z, y = np.asarray(z, dtype=F64), np.asarray(labels)
    if y.ndim == 1:
        s = z - z.max(1, keepdims=True)
        logp = s - np.log(np.exp(s).sum(1, keepdims=True))
        B = len(y)
        g = np.exp(logp)
        g[np.arange(B), y] -= 1.0
        return float(-logp[np.arange(B), y].mean()), g / B
    y = y.astype(F64)
    loss = np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))
    return float(loss.mean()), (1.0 / (1.0 + np.exp(-z)) - y) / z.size


class Trainer64:
    """The L-layer estimator with its own histories.  weights[i] [out_i, in_i], biases[i] [out_i] (numpy); px = P X [N, F] fp64.
    layers: per d (0 next to the output) a namespace with prev (the rows level L - d needs, global ids) and kept (kept_lists)."""

    def __init__(self, indptr, indices, x, hidden_widths):
        self.indptr, self.indices = loop_free(indptr, indices)
        self.n = len(self.indptr) - 1
        self.px = dense_p(self.indptr, self.indices, self.n) @ np.asarray(x, dtype=F64)
        self.hbar = [np.zeros((self.n, w)) for w in hidden_widths]          # hbar[l - 1] = the history of level l

    def step(self, weights, biases, layers, labels, gates=None):
        """One step from the given parameters: SimpleNamespace(loss, logits, dW, db, acts = [(rows, H^(l)) per level], a_in = the
        aggregate each layer multiplied); the histories are updated AFTER the forward.  gates: per hidden level a 0/1 array [m_l,
        width] that replaces the ReLU."""
        W = [np.asarray(w, dtype=F64) for w in weights]
        b = [np.asarray(v, dtype=F64) for v in biases]
        L = len(W)
        assert L == len(layers) and len(self.hbar) == L - 1
        rows = [np.asarray(layers[L - 1 - i].prev, dtype=np.int64) for i in range(L)]       # rows[i]: what layer i (0-based) produces
        a_in, z, g01, Hg = [], [], [], []
        a = self.px[rows[0]]
        for i in range(L):
            if i > 0:
                a = aggregate(self.indptr, self.indices, rows[i], layers[L - 1 - i].kept, Hg[i - 1], self.hbar[i - 1])
            a_in.append(a)
            zi = a @ W[i].T + b[i]
            z.append(zi)
            if i < L - 1:
                gate = (zi > 0).astype(F64) if gates is None else np.asarray(gates[i], dtype=F64)
                g01.append(gate)
                full = np.zeros((self.n, zi.shape[1]))
                full[rows[i]] = zi * gate
                Hg.append(full)
        loss, dz = loss_and_grad(z[-1], labels)
        dW, db = [None] * L, [None] * L
        for i in range(L - 1, -1, -1):
            dW[i], db[i] = dz.T @ a_in[i], dz.sum(0)
            if i > 0:
                dH = aggregate_grad(self.indptr, rows[i], layers[L - 1 - i].kept, dz @ W[i], self.n)
                dz = dH[rows[i - 1]] * g01[i - 1]
        acts = [(rows[i], Hg[i][rows[i]]) for i in range(L - 1)]
        for i, (r, h) in enumerate(acts):
            self.hbar[i] = history_update(self.hbar[i], r, h)
        return SimpleNamespace(loss=loss, logits=z[-1], dW=dW, db=db, acts=acts, a_in=a_in)


def batch_layers(sampled):
    """The layers of a tests.sage_oracle.sample batch as Trainer64.step takes them."""
    return [SimpleNamespace(prev=L.prev, kept=kept_lists(L.prev, L.src, L.dst)) for L in sampled.layers]
