"""TEST INFRASTRUCTURE — GCNConv with edge weights restated on the host (PyG 2.5 gcn_norm with edge_weight, add_self_loops=True,
improved=False, flow='source_to_target'):

  1. add_remaining_self_loops(fill_value=1): non-loop entries keep their weights; node i gets one loop of weight lw[i] = 1, or the
     weight of its LAST stored entry (i, i) in input order;
  2. deg[c] = lw[c] + sum of w_e over the non-loop entries into c; dinv = deg^-1/2, inf -> 0;
  3. out[c] = dinv[c] sum_{e: r -> c} w_e dinv[r] H[r] + dinv[c]^2 lw[c] H[c] + b, then ReLU where the layer fuses it.

`forward64` is that in fp64 torch with index_add_, so autograd gives dx, dW, db and d edge_weight.  `Problem` adds what
oracle/accuracy.py's criterion needs beside a reference: per output the magnitude (the same sums over absolute values) and a
host fp32 baseline that adds the same terms in by-target (or, for the transpose, by-source) row order, and the closed form of
the edge-weight gradient.  Only tests import this module.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import accuracy as acc

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------ fp64 + autograd
def loop_sources(src, dst, n):
    """int64[n]: the input index of the stored loop that sets lw (the last (i, i) in input order), or -1."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    out = np.full(n, -1, np.int64)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n) & (src == dst)
    idx = np.nonzero(ok)[0]
    out[src[idx]] = idx                      # (ascending idx: numpy assigns in order, the last one stays)
    for i in idx:                            # (spelled out: the rule must not rest on an assignment order)
        out[src[i]] = max(out[src[i]], i)
    return out


def norm64(src, dst, w, n):
    """(lw, dinv, keep) in fp64 torch, differentiable in w; keep = the in-range non-loop entries."""
    src_t, dst_t = torch.as_tensor(np.asarray(src, dtype=np.int64)), torch.as_tensor(np.asarray(dst, dtype=np.int64))
    inr = (src_t >= 0) & (src_t < n) & (dst_t >= 0) & (dst_t < n)
    keep = inr & (src_t != dst_t)
    ls = torch.as_tensor(loop_sources(src, dst, n))
    lw = torch.where(ls >= 0, w[ls.clamp(min=0)], torch.ones(n, dtype=torch.float64))
    deg = lw.index_add(0, dst_t[keep], w[keep])
    zero = deg == 0
    dinv = torch.where(zero, torch.zeros_like(deg), torch.where(zero, torch.ones_like(deg), deg).pow(-0.5))
    return lw, dinv, keep


def forward64(x, W, b, src, dst, w, n, gate=None, relu=False):
    """The layer in fp64 torch (x [n, fi], W [fo, fi] or None for the bare aggregation of x, b [fo] or None, w [e]).  gate: a 0/1
    array the pre-activation is multiplied with instead of the ReLU (the device's gates, so that an output within rounding of
    zero does not decide the gradient)."""
    lw, dinv, keep = norm64(src, dst, w, n)
    r = torch.as_tensor(np.asarray(src, dtype=np.int64))[keep]
    c = torch.as_tensor(np.asarray(dst, dtype=np.int64))[keep]
    H = x if W is None else x @ W.T
    coef = w[keep] * dinv[r] * dinv[c]
    out = torch.zeros_like(H).index_add_(0, c, coef[:, None] * H[r]) + (dinv * dinv * lw)[:, None] * H
    if b is not None:
        out = out + b
    if gate is not None:
        return out * torch.as_tensor(np.asarray(gate, dtype=F64))
    return out.clamp(min=0) if relu else out


def dense_forward(x, W, b, src, dst, w, n):
    """D^-1/2 (A_w + diag(lw)) D^-1/2 X Wᵀ + b with a dense adjacency, numpy fp64 (the hand graph's second opinion)."""
    src, dst, w = np.asarray(src), np.asarray(dst), np.asarray(w, dtype=F64)
    A = np.zeros((n, n))
    lw = np.ones(n)
    for i, (r, c) in enumerate(zip(src, dst)):
        if not (0 <= r < n and 0 <= c < n):
            continue
        if r == c:
            lw[r] = w[i]                     # (in input order: the last one stays)
        else:
            A[c, r] += w[i]
    deg = A.sum(1) + lw
    with np.errstate(divide="ignore"):
        dinv = np.where(deg == 0, 0.0, 1.0 / np.sqrt(np.where(deg == 0, 1.0, deg)))
    Ah = dinv[:, None] * (A + np.diag(lw)) * dinv[None, :]
    return Ah @ (np.asarray(x, dtype=F64) @ np.asarray(W, dtype=F64).T) + np.asarray(b, dtype=F64)


# ------------------------------------------------------------------------------------------------------------ the criterion's parts
def _seg_sum(rows, t64, tabs, t32, n):
    """Per segment (rows ascending, one segment per value) the sums of the entries' term vectors: (ref fp64, mag fp64, base fp32
    with a segment's terms added one after the other in the order given)."""
    f = t64.shape[1]
    ref, mag = np.zeros((n, f)), np.zeros((n, f))
    np.add.at(ref, rows, t64)
    np.add.at(mag, rows, tabs)
    base = np.zeros((n, f), F32)
    lens = np.bincount(rows, minlength=n)
    start = np.concatenate([[0], np.cumsum(lens)])[:-1]
    for j in range(int(lens.max()) if len(rows) else 0):
        rr = np.nonzero(lens > j)[0]
        base[rr] += t32[start[rr] + j]
    return ref, mag, base


def _dot32(a, b):
    """Row-wise fp32 dot products, the columns added one after the other."""
    if a.shape[0] == 0:
        return np.zeros(0, F32)
    return np.add.accumulate((a * b).astype(F32), axis=1, dtype=F32)[:, -1]


class Problem:
    """One weighted graph: the normalisation in fp64 and in fp32, the two row orders, and (ref, mag, base) of everything the
    kernels compute.  src / dst int [e] (anything outside [0, n) is dropped), w fp32 [e]."""

    def __init__(self, src, dst, w, n):
        self.src, self.dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        self.w32 = np.asarray(w, dtype=F32)
        self.w = self.w32.astype(F64)
        self.n, self.e = n, len(self.src)
        inr = (self.src >= 0) & (self.src < n) & (self.dst >= 0) & (self.dst < n)
        self.keep = np.nonzero(inr & (self.src != self.dst))[0]
        self.loop_src = loop_sources(self.src, self.dst, n)
        has = self.loop_src >= 0
        self.lw = np.where(has, self.w[np.maximum(self.loop_src, 0)], 1.0)
        self.lw32 = self.lw.astype(F32)
        k = self.keep
        # by-target order: (target, source, input index); by-source: (source, target, input index) — the CSR rows are ascending
        # and duplicates sit in input order
        self.order_t = k[np.lexsort((k, self.src[k], self.dst[k]))]
        self.order_s = k[np.lexsort((k, self.dst[k], self.src[k]))]
        self.lens_t = np.bincount(self.dst[k], minlength=n)
        self.lens_s = np.bincount(self.src[k], minlength=n)
        ot = self.order_t
        d64, _, d32 = _seg_sum(self.dst[ot], self.w[ot, None], np.abs(self.w[ot, None]), self.w32[ot, None], n)
        self.deg = self.lw + d64[:, 0]
        self.deg32 = (self.lw32 + d32[:, 0]).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.dinv = np.where(self.deg == 0, 0.0, 1.0 / np.sqrt(np.where(self.deg == 0, 1.0, self.deg)))
            s32 = (F32(1) / np.sqrt(self.deg32, dtype=F32)).astype(F32)
        self.dinv32 = np.where(np.isinf(s32), F32(0), s32).astype(F32)
        self.slot_t = np.full(self.e, -1, np.int64); self.slot_t[self.order_t] = np.arange(len(k))
        self.slot_s = np.full(self.e, -1, np.int64); self.slot_s[self.order_s] = np.arange(len(k))

    def coef(self, idx):
        """w_e dinv[r] dinv[c] of the entries idx: (fp64, fp32)."""
        r, c = self.src[idx], self.dst[idx]
        return self.w[idx] * self.dinv[r] * self.dinv[c], ((self.w32[idx] * self.dinv32[c]).astype(F32) * self.dinv32[r]).astype(F32)

    def aggregate_sums(self, M, Mabs=None, M32=None, transpose=False):
        """Â_w M before bias and ReLU (transpose: Â_wᵀ M, the backward): (ref, mag, base).  M fp64 [n, f]; Mabs its magnitude
        (default |M|); M32 the fp32 operand (default M rounded)."""
        M = np.asarray(M, dtype=F64)
        Mabs = np.abs(M) if Mabs is None else np.asarray(Mabs, dtype=F64)
        M32 = M.astype(F32) if M32 is None else np.asarray(M32, dtype=F32)
        idx = self.order_s if transpose else self.order_t
        rows, cols = (self.src[idx], self.dst[idx]) if transpose else (self.dst[idx], self.src[idx])
        c64, c32 = self.coef(idx)
        ref, mag, base = _seg_sum(rows, c64[:, None] * M[cols], np.abs(c64)[:, None] * Mabs[cols],
                                  (c32[:, None] * M32[cols]).astype(F32), self.n)
        n = self.n
        cs = self.dinv * self.dinv * self.lw
        cs32 = ((self.dinv32 * self.dinv32).astype(F32) * self.lw32).astype(F32)
        ref = ref + cs[:, None] * M[:n]
        mag = mag + np.abs(cs)[:, None] * Mabs[:n]
        base = (base + (cs32[:, None] * M32[:n]).astype(F32)).astype(F32)
        return torch.from_numpy(ref), torch.from_numpy(mag), base

    def aggregate(self, M, bias=None, relu=False, transpose=False):
        return acc.aggregate_finish(self.aggregate_sums(M, transpose=transpose), bias, relu)

    def weight_grad(self, G, H, Gabs=None, Habs=None, G32=None, H32=None):
        """d edge_weight of sum(G * (Â_w H)) in closed form: (ref, mag, base) [e].  mag is the absolute sum of the two terms
        (s_r s_c |p_e| and |q_c|, each over absolute values), so cancellation between them is judged fairly."""
        G, H = np.asarray(G, dtype=F64), np.asarray(H, dtype=F64)
        Gabs = np.abs(G) if Gabs is None else np.asarray(Gabs, dtype=F64)
        Habs = np.abs(H) if Habs is None else np.asarray(Habs, dtype=F64)
        G32 = G.astype(F32) if G32 is None else np.asarray(G32, dtype=F32)
        H32 = H.astype(F32) if H32 is None else np.asarray(H32, dtype=F32)
        n, s, s32 = self.n, self.dinv, self.dinv32
        ot, os_ = self.order_t, self.order_s
        p = np.zeros(self.e); pa = np.zeros(self.e); p32 = np.zeros(self.e, F32)
        k = self.keep
        p[k] = (G[self.dst[k]] * H[self.src[k]]).sum(1)
        pa[k] = (Gabs[self.dst[k]] * Habs[self.src[k]]).sum(1)
        p32[k] = _dot32(G32[self.dst[k]], H32[self.src[k]])
        gh, gha, gh32 = (G[:n] * H[:n]).sum(1), (Gabs[:n] * Habs[:n]).sum(1), _dot32(G32[:n], H32[:n])

        def side(order, rows, other):
            c64 = self.w[order] * s[other[order]]
            c32 = (self.w32[order] * s32[other[order]]).astype(F32)
            return _seg_sum(rows[order], (c64 * p[order])[:, None], (np.abs(c64) * pa[order])[:, None],
                            (c32 * p32[order]).astype(F32)[:, None], n)

        dt, dta, dt32 = side(ot, self.dst, self.src)
        st, sta, st32 = side(os_, self.src, self.dst)
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
        li = np.nonzero(self.loop_src >= 0)[0]
        ls = self.loop_src[li]
        ref[ls] = s[li] ** 2 * gh[li] + q[li]
        mag[ls] = s[li] ** 2 * gha[li] + qa[li]
        base[ls] = ((s32[li] * s32[li]).astype(F32) * gh32[li] + q32[li]).astype(F32)
        return torch.from_numpy(ref), torch.from_numpy(mag), torch.from_numpy(base)

    # ---- layers in a chain: every operand is a triple (ref fp64, mag fp64, base fp32) of numpy arrays, so that the reference, the
    # magnitude and the fp32 baseline of a later layer carry what the earlier ones did to them
    def chain_forward(self, x3, W, b, gate=None):
        """gate ⊙ (Â_w (x Wᵀ) + b) (gate: a 0/1 array, the device's ReLU gates, or None) -> (ref, mag, base) numpy."""
        xr, xm, xb = x3
        W32, b32 = np.ascontiguousarray(W, dtype=F32), np.asarray(b, dtype=F32)
        W64 = W32.astype(F64)
        Hb = acc.fp32_contract(np.ascontiguousarray(np.asarray(xb, dtype=F32).T), W32.T.copy()).numpy()
        ref, mag, base = self.aggregate_sums(xr @ W64.T, xm @ np.abs(W64).T, Hb)
        ref, mag, base = ref.numpy() + b32.astype(F64), mag.numpy() + np.abs(b32.astype(F64)), (base + b32).astype(F32)
        if gate is not None:
            g = np.asarray(gate, dtype=F64)
            ref, mag, base = ref * g, mag * g, (base * g.astype(F32)).astype(F32)
        return ref, mag, base

    def chain_backward(self, G3, x3, W):
        """The gradients of out = Â_w (x Wᵀ) + b against G (already gated): {"dW" | "db" | "dx": (ref, mag, base)} numpy."""
        (Gr, Gm, Gb), (xr, xm, xb) = G3, x3
        W32 = np.ascontiguousarray(W, dtype=F32)
        W64 = W32.astype(F64)
        dh = self.aggregate_sums(Gr, Gm, Gb, transpose=True)
        dr, dm, db_ = dh[0].numpy(), dh[1].numpy(), dh[2]
        xb = np.ascontiguousarray(xb, dtype=F32)
        return {"dW": (dr.T @ xr, dm.T @ xm, acc.fp32_contract(db_, xb).numpy()),
                "dx": (dr @ W64, dm @ np.abs(W64), acc.fp32_contract(np.ascontiguousarray(db_.T), W32).numpy()),
                "db": (Gr.sum(0), Gm.sum(0), acc._seq_sum_f32(np.ascontiguousarray(Gb, dtype=F32)))}

    def layer(self, x, W, b, relu, dout, gate=None):
        """The layer out = act(Â_w (x Wᵀ) + b) and its gradients against dout: {"out" | "dx" | "dW" | "db" | "dw": (ref, mag, base)}.
        The references come from autograd on forward64 (dw's closed form is checked against it in the CPU tests); magnitudes and
        baselines chain the parts: the GEMMs through accuracy.matmul_reference's fixed-order fp32 sum.  gate: the device's ReLU
        gates (0/1, [n, fo]); default the reference's own."""
        n = self.n
        x32, W32, b32, d32 = (np.ascontiguousarray(v, dtype=F32) for v in (x, W, b, dout))
        xt = torch.from_numpy(x32.astype(F64)).requires_grad_(True)
        Wt = torch.from_numpy(W32.astype(F64)).requires_grad_(True)
        bt = torch.from_numpy(b32.astype(F64)).requires_grad_(True)
        wt = torch.from_numpy(self.w.copy()).requires_grad_(True)
        Href, Hmag, Hbase = acc.matmul_reference(x32, W32.T.copy())
        sums = self.aggregate_sums(Href.numpy(), Hmag.numpy(), Hbase.numpy())
        out = acc.aggregate_finish(sums, b32, relu)
        if gate is None:
            gate = (out[0].numpy() > 0) if relu else np.ones_like(d32)
        gate = np.asarray(gate, dtype=F64)
        o = forward64(xt, Wt, bt, self.src, self.dst, wt, n, gate=gate)
        o.backward(torch.from_numpy(d32.astype(F64)))
        G32 = (d32 * gate.astype(F32)).astype(F32)
        G = G32.astype(F64)
        dh = self.aggregate_sums(G, transpose=True)
        dh_ref, dh_mag, dh_base = dh[0].numpy(), dh[1].numpy(), dh[2]
        res = {"out": out, "db": acc.colsum_reference(G32)}
        res["dW"] = (Wt.grad, torch.from_numpy(dh_mag.T @ np.abs(x32.astype(F64))), acc.fp32_contract(dh_base, x32))
        res["dx"] = (xt.grad, torch.from_numpy(dh_mag @ np.abs(W32.astype(F64))),
                     acc.fp32_contract(np.ascontiguousarray(dh_base.T), W32))
        dw = self.weight_grad(G, Href.numpy(), Habs=Hmag.numpy(), G32=G32, H32=Hbase.numpy())
        res["dw"] = (wt.grad, dw[1], dw[2])
        res["dw_closed"] = dw[0]
        res["dh"] = (torch.from_numpy(dh_ref), torch.from_numpy(dh_mag), torch.from_numpy(dh_base))
        return res


# ------------------------------------------------------------------------------------------------------------ graphs
def hand_graph():
    """6 nodes: node 5 isolated; node 0 a pure source; node 1 with a stored loop of weight 2.5; node 2 with two stored loops
    (0.75 then 1.5: the last wins); the directed pair 3 <-> 4; a zero-weight entry 0 -> 3; the entry 0 -> 1 stored twice."""
    src = [0, 1, 0, 2, 3, 2, 4, 0, 0, 1]
    dst = [1, 1, 1, 2, 4, 2, 3, 3, 2, 2]
    w = [0.5, 2.5, 1.25, 0.75, 2.0, 1.5, 0.25, 0.0, 1.0, 3.0]
    return np.array(src), np.array(dst), np.array(w, F32), 6


def random_graph(n, e, seed, dup=0.05, loops=0.03):
    """A directed multigraph: e entries, about dup of them repeats of an earlier entry and loops of them stored loops (some
    nodes get two)."""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    nd = int(e * dup)
    j = rng.integers(0, e, nd); i = rng.integers(0, e, nd)
    src[i], dst[i] = src[j], dst[j]
    nl = int(e * loops)
    li = rng.integers(0, e, nl)
    dst[li] = src[li]
    src[li[: nl // 4]] = dst[li[: nl // 4]] = src[li[0]] if nl else 0
    return src, dst


def long_graph(seed=3):
    """n = 2304 (> 2048: long rows become work items), e ~ 12k: node 7 has ~700 incoming entries and node 11 ~700 outgoing ones
    (chunk + combine in both directions), node 20 exactly 64 incoming and node 21 exactly 65; duplicates and stored loops."""
    n = 2304
    rng = np.random.default_rng(seed)
    src, dst = random_graph(n, 10400, seed)
    clean = ~np.isin(dst, (20, 21)) & ~np.isin(src, (20, 21))
    src, dst = src[clean], dst[clean]
    hub_in = rng.integers(30, n, 700)
    hub_out = rng.integers(30, n, 700)
    s64 = rng.permutation(np.arange(30, n))[:64]; s65 = rng.permutation(np.arange(30, n))[:65]
    src = np.concatenate([src, hub_in, np.full(700, 11), s64, s65, [7, 7, 11]])
    dst = np.concatenate([dst, np.full(700, 7), hub_out, np.full(64, 20), np.full(65, 21), [7, 7, 11]])
    o = rng.permutation(len(src))
    return src[o], dst[o], n


def weights(kind, e, seed):
    rng = np.random.default_rng(seed + 100)
    if kind == "uniform":
        return rng.uniform(0.0, 2.0, e).astype(F32)
    if kind == "mixed":
        return (2.0 ** rng.uniform(-10, 10, e)).astype(F32)
    if kind == "ones":
        return np.ones(e, F32)
    raise ValueError(kind)
