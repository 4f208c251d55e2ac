"""TEST INFRASTRUCTURE — GCNConv's constructor arguments restated on the host (PyG 2.5 GCNConv / gcn_norm as recalled: improved,
add_self_loops, normalize; flow='source_to_target').  With w the per-entry weights (all 1 without edge_weight), entries r -> c:

  1. normalize, add_self_loops:      add_remaining_self_loops(fill): node i gets one loop of weight lw[i] = fill (2 if improved else 1),
                                     or the weight of its LAST stored (i, i); deg[c] = lw[c] + the non-loop weights into c;
                                     out[c] = s_c sum_{e: r -> c, r != c} w_e s_r H[r] + s_c^2 lw_c H[c] + b,  s = deg^-1/2 (inf -> 0);
  2. normalize, no added loops:      stored loops are ordinary entries: deg[c] = sum_{e -> c} w_e, out[c] = s_c sum_e w_e s_r H[r] + b;
  3. not normalize:                  out[c] = sum_{e: r -> c} w_e H[r] + b.

`forward64` is exactly that in fp64 torch with index_add, so autograd gives dx, dW, db and d edge_weight.  `ModeProblem` extends
tests/wgcn_oracle.py's Problem (graphs, magnitudes, host fp32 baseline) by the rule for the loop weights: in the kernels' language
rules 2 and 3 are lw[i] = the weights of all stored (i, i) added in input order, and rule 3 has s = 1 everywhere.  Only tests import
this module.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import accuracy as acc
from tests import wgcn_oracle as O

F32, F64 = np.float32, np.float64

# (improved, add_self_loops, normalize) of the four modes the tests run
MODES = {"default": (False, True, True), "improved": (True, True, True), "no_loops": (False, False, True),
         "plain": (False, False, False)}


def rule(improved=False, add_self_loops=None, normalize=True):
    """("fill" | "sum" | "plain", fill): which of the three rules the constructor arguments select."""
    if add_self_loops is None:
        add_self_loops = normalize
    if add_self_loops and not normalize:
        raise ValueError("add_self_loops=True needs normalize=True")
    if not normalize:
        return "plain", 1.0
    if not add_self_loops:
        return "sum", 1.0
    return "fill", 2.0 if improved else 1.0


def _inv_sqrt(deg):
    zero = deg == 0
    return torch.where(zero, torch.zeros_like(deg), torch.where(zero, torch.ones_like(deg), deg).pow(-0.5))


def forward64(x, W, b, src, dst, w, n, improved=False, add_self_loops=None, normalize=True, gate=None, relu=False):
    """The layer in fp64 torch (x [n, fi], W [fo, fi] or None for the bare aggregation, b [fo] or None, w [e] fp64).  gate: a 0/1
    array the pre-activation is multiplied with instead of the ReLU (the device's gates)."""
    kind, fill = rule(improved, add_self_loops, normalize)
    s_all, d_all = torch.as_tensor(np.asarray(src, dtype=np.int64)), torch.as_tensor(np.asarray(dst, dtype=np.int64))
    inr = (s_all >= 0) & (s_all < n) & (d_all >= 0) & (d_all < n)
    H = x if W is None else x @ W.T
    if kind == "fill":
        keep = inr & (s_all != d_all)
        ls = torch.as_tensor(O.loop_sources(src, dst, n))
        lw = torch.where(ls >= 0, w[ls.clamp(min=0)], torch.full((n,), fill, dtype=torch.float64))
        s = _inv_sqrt(lw.index_add(0, d_all[keep], w[keep]))
        r, c = s_all[keep], d_all[keep]
        out = torch.zeros_like(H).index_add_(0, c, (w[keep] * s[r] * s[c])[:, None] * H[r]) + (s * s * lw)[:, None] * H
    else:
        r, c, wk = s_all[inr], d_all[inr], w[inr]
        if kind == "sum":
            s = _inv_sqrt(torch.zeros(n, dtype=torch.float64).index_add(0, c, wk))
            wk = wk * s[r] * s[c]
        out = torch.zeros_like(H).index_add_(0, c, wk[:, None] * H[r])
    if b is not None:
        out = out + b
    if gate is not None:
        return out * torch.as_tensor(np.asarray(gate, dtype=F64))
    return out.clamp(min=0) if relu else out


def dense_forward(x, W, b, src, dst, w, n, improved=False, add_self_loops=None, normalize=True):
    """D^-1/2 (A_w [+ diag(lw)]) D^-1/2 X Wᵀ + b (or A_w X Wᵀ + b) with a dense adjacency, numpy fp64."""
    kind, fill = rule(improved, add_self_loops, normalize)
    w = np.asarray(w, dtype=F64)
    A, lw = np.zeros((n, n)), np.full(n, fill)
    for i, (r, c) in enumerate(zip(np.asarray(src), np.asarray(dst))):
        if not (0 <= r < n and 0 <= c < n):
            continue
        if r == c and kind == "fill":
            lw[r] = w[i]                     # (in input order: the last one stays)
        else:
            A[c, r] += w[i]
    if kind == "fill":
        A = A + np.diag(lw)
    if kind != "plain":
        deg = A.sum(1)
        with np.errstate(divide="ignore"):
            dinv = np.where(deg == 0, 0.0, 1.0 / np.sqrt(np.where(deg == 0, 1.0, deg)))
        A = dinv[:, None] * A * dinv[None, :]
    out = A @ (np.asarray(x, dtype=F64) @ np.asarray(W, dtype=F64).T)
    return out if b is None else out + np.asarray(b, dtype=F64)


class ModeProblem(O.Problem):
    """wgcn_oracle.Problem under one of the three rules: lw, deg and dinv (fp64 and fp32) by the rule, `loops` = the input indices
    of the stored loops (ascending: every node's in input order).  aggregate_sums / aggregate / chain_* are inherited: they read
    lw and dinv, and the plain rule is dinv = 1 (multiplications by 1 are exact, so the fp32 baseline is the plain weighted sum)."""

    def __init__(self, src, dst, w, n, improved=False, add_self_loops=None, normalize=True):
        super().__init__(src, dst, w, n)
        self.args = dict(improved=improved, add_self_loops=add_self_loops, normalize=normalize)
        self.kind, self.fill = rule(improved, add_self_loops, normalize)
        inr = (self.src >= 0) & (self.src < n) & (self.dst >= 0) & (self.dst < n)
        self.loops = np.nonzero(inr & (self.src == self.dst))[0]
        if self.kind == "fill":
            has = self.loop_src >= 0
            self.lw = np.where(has, self.w[np.maximum(self.loop_src, 0)], self.fill)
            self.lw32 = self.lw.astype(F32)
            self.loop_entries = self.loop_src[has]                # the loops that enter the result
        else:
            self.lw, self.lw32 = np.zeros(n), np.zeros(n, F32)
            for i in self.loops:                                  # input order, one fp32 addition per loop
                self.lw[self.src[i]] += self.w[i]
                self.lw32[self.src[i]] = F32(self.lw32[self.src[i]] + self.w32[i])
            self.loop_entries = self.loops
        ot = self.order_t
        d64, _, d32 = O._seg_sum(self.dst[ot], self.w[ot, None], np.abs(self.w[ot, None]), self.w32[ot, None], n)
        if self.kind == "plain":
            self.deg, self.deg32 = np.ones(n), np.ones(n, F32)
            self.dinv, self.dinv32 = np.ones(n), np.ones(n, F32)
            return
        self.deg = self.lw + d64[:, 0]
        self.deg32 = (self.lw32 + d32[:, 0]).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.dinv = np.where(self.deg == 0, 0.0, 1.0 / np.sqrt(np.where(self.deg == 0, 1.0, self.deg)))
            s32 = (F32(1) / np.sqrt(self.deg32, dtype=F32)).astype(F32)
        self.dinv32 = np.where(np.isinf(s32), F32(0), s32).astype(F32)

    def weight_grad(self, G, H, Gabs=None, Habs=None, G32=None, H32=None):
        """d edge_weight of sum(G * (Â H)) in closed form: (ref, mag, base) [e].  fill: wgcn_oracle's (the loop that set lw).  sum:
        the same q with lw the loop sum, and EVERY stored loop of i gets s_i^2 (G[i] . H[i]) + q_i.  plain: p_e, a loop G[i] . H[i]."""
        if self.kind == "fill":
            return super().weight_grad(G, H, Gabs, Habs, G32, H32)
        G, H = np.asarray(G, dtype=F64), np.asarray(H, dtype=F64)
        Gabs = np.abs(G) if Gabs is None else np.asarray(Gabs, dtype=F64)
        Habs = np.abs(H) if Habs is None else np.asarray(Habs, dtype=F64)
        G32 = G.astype(F32) if G32 is None else np.asarray(G32, dtype=F32)
        H32 = H.astype(F32) if H32 is None else np.asarray(H32, dtype=F32)
        n, s, s32, k, li = self.n, self.dinv, self.dinv32, self.keep, self.loops
        p = np.zeros(self.e); pa = np.zeros(self.e); p32 = np.zeros(self.e, F32)
        p[k] = (G[self.dst[k]] * H[self.src[k]]).sum(1)
        pa[k] = (Gabs[self.dst[k]] * Habs[self.src[k]]).sum(1)
        p32[k] = O._dot32(G32[self.dst[k]], H32[self.src[k]])
        gh, gha, gh32 = (G[:n] * H[:n]).sum(1), (Gabs[:n] * Habs[:n]).sum(1), O._dot32(G32[:n], H32[:n])
        ln = self.src[li]
        if self.kind == "plain":
            ref, mag, base = p, pa, p32
            ref[li], mag[li], base[li] = gh[ln], gha[ln], gh32[ln]
            return torch.from_numpy(ref), torch.from_numpy(mag), torch.from_numpy(base)

        def side(order, rows, other):
            c64 = self.w[order] * s[other[order]]
            c32 = (self.w32[order] * s32[other[order]]).astype(F32)
            return O._seg_sum(rows[order], (c64 * p[order])[:, None], (np.abs(c64) * pa[order])[:, None],
                              (c32 * p32[order]).astype(F32)[:, None], n)

        dt, dta, dt32 = side(self.order_t, self.dst, self.src)
        st, sta, st32 = side(self.order_s, self.src, self.dst)
        t = dt[:, 0] + st[:, 0] + 2 * s * self.lw * gh
        ta = dta[:, 0] + sta[:, 0] + 2 * s * np.abs(self.lw) * gha
        t32 = ((dt32[:, 0] + st32[:, 0]).astype(F32) + ((F32(2) * s32 * self.lw32).astype(F32) * gh32).astype(F32)).astype(F32)
        q = np.where(s == 0, 0.0, -0.5 * s ** 3 * t)
        qa = np.where(s == 0, 0.0, 0.5 * np.abs(s) ** 3 * ta)
        q32 = np.where(s32 == 0, F32(0), (F32(-0.5) * s32 * s32 * s32 * t32).astype(F32)).astype(F32)
        ref, mag, base = np.zeros(self.e), np.zeros(self.e), np.zeros(self.e, F32)
        r, c = self.src[k], self.dst[k]
        ref[k] = s[r] * s[c] * p[k] + q[c]
        mag[k] = np.abs(s[r] * s[c]) * pa[k] + qa[c]
        base[k] = ((s32[r] * s32[c]).astype(F32) * p32[k] + q32[c]).astype(F32)
        ref[li] = s[ln] ** 2 * gh[ln] + q[ln]
        mag[li] = s[ln] ** 2 * gha[ln] + qa[ln]
        base[li] = ((s32[ln] * s32[ln]).astype(F32) * gh32[ln] + q32[ln]).astype(F32)
        return torch.from_numpy(ref), torch.from_numpy(mag), torch.from_numpy(base)

    def layer(self, x, W, b, relu, dout, gate=None):
        """wgcn_oracle.Problem.layer under this problem's rule; b may be None (bias=False: no "db").  The references are autograd
        on this module's forward64."""
        n = self.n
        x32, W32, d32 = (np.ascontiguousarray(v, dtype=F32) for v in (x, W, dout))
        b32 = None if b is None else np.ascontiguousarray(b, dtype=F32)
        xt = torch.from_numpy(x32.astype(F64)).requires_grad_(True)
        Wt = torch.from_numpy(W32.astype(F64)).requires_grad_(True)
        bt = None if b32 is None else torch.from_numpy(b32.astype(F64)).requires_grad_(True)
        wt = torch.from_numpy(self.w.copy()).requires_grad_(True)
        Href, Hmag, Hbase = acc.matmul_reference(x32, W32.T.copy())
        sums = self.aggregate_sums(Href.numpy(), Hmag.numpy(), Hbase.numpy())
        out = acc.aggregate_finish(sums, b32, relu)
        if gate is None:
            gate = (out[0].numpy() > 0) if relu else np.ones_like(d32)
        gate = np.asarray(gate, dtype=F64)
        o = forward64(xt, Wt, bt, self.src, self.dst, wt, n, gate=gate, **self.args)
        o.backward(torch.from_numpy(d32.astype(F64)))
        G32 = (d32 * gate.astype(F32)).astype(F32)
        G = G32.astype(F64)
        dh = self.aggregate_sums(G, transpose=True)
        dh_ref, dh_mag, dh_base = dh[0].numpy(), dh[1].numpy(), dh[2]
        res = {"out": out, "out64": o.detach()}
        if b32 is not None:
            res["db"] = acc.colsum_reference(G32)
            res["db64"] = bt.grad
        res["dW"] = (Wt.grad, torch.from_numpy(dh_mag.T @ np.abs(x32.astype(F64))), acc.fp32_contract(dh_base, x32))
        res["dx"] = (xt.grad, torch.from_numpy(dh_mag @ np.abs(W32.astype(F64))),
                     acc.fp32_contract(np.ascontiguousarray(dh_base.T), W32))
        dw = self.weight_grad(G, Href.numpy(), Habs=Hmag.numpy(), G32=G32, H32=Hbase.numpy())
        res["dw"] = (wt.grad, dw[1], dw[2])
        res["dw_closed"] = dw[0]
        return res
