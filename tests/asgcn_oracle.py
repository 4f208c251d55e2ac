"""TEST INFRASTRUCTURE — the AS-GCN adaptive layer-wise sampler and its loss, as grapes_amd/modules/asgcn.py and grapes_amd/asgcn.py
define them, restated on the host in numpy / torch fp64 [AS-GCN-recall: Huang et al., NeurIPS 2018, the layer-wise sampler with the
self-dependent g(x(u_j))].  Graphs, candidates, the draw and the entries are tests/ladies_oracle.py's.

Per layer (prev the rows): c_j = sum_{i in prev} P_ij, a_j = <x_j, w_g> + b_g, g_j = max(a_j, 0) + 1, q_j = c_j g_j, logq = log q,
logit = (logq - max logq) - 20; the draw in proportion to q; w_ij = (v_ij / q_j) / sum_{j' kept} v_ij' / q_j'.
L = L_c + lambda L_var, L_var = mean_i V_i over the rows of the layer that writes the logits, with H that layer's transformed input
held constant, mu_i = sum_j w_ij H_j, s_i = the row's entries: V_i = (1 / s_i) sum_j |s_i w_ij H_j - mu_i|^2
= s_i sum_j w_ij^2 |H_j|^2 - |mu_i|^2, d L_var / d w_ij = (2 / m)(s_i w_ij |H_j|^2 - <mu_i, H_j>).
With G = d L / d w: Gbar_i = sum_j G_ij w_ij, T_j = sum_i w_ij (G_ij - Gbar_i), d L / d logq_j = -T_j,
d L / d a_j = -[a_j > 0] / g_j sum_layers T_j.

Triples are (reference fp64, magnitude fp64, fp32 baseline) as oracle/accuracy.py judges them; a baseline adds its terms one after
the other in the order given.  Only tests import this module; it imports nothing of the product."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from tests import ladies_oracle as LO

F32, F64 = np.float32, np.float64


# --------------------------------------------------------------------------------------------- the sampler
def column_mass(indptr, indices, n, prev):
    """(c fp64 [n], terms int64 [n]): c_j = sum over i in prev of P_ij, and how many terms each sum has."""
    D = LO.degree(indptr)
    c, t = np.zeros(n), np.zeros(n, np.int64)
    for i in np.asarray(prev, dtype=np.int64):
        cols, v = LO.row_of_v(indptr, indices, int(i))
        np.add.at(c, cols, v / D[i])
        np.add.at(t, cols, 1)
    return c, t


def importance(indptr, indices, n, prev, x, w_g, b_g):
    """Over ALL nodes (only candidates have c > 0): namespace of c, terms, a, g, q, logq (fp64; logq = -inf where c = 0) and a_mag =
    sum_f |x_jf w_f| + |b_g|."""
    x64, w64, b64 = np.asarray(x, dtype=F64), np.asarray(w_g, dtype=F64).reshape(-1), float(np.asarray(b_g, dtype=F64).reshape(-1)[0])
    c, t = column_mass(indptr, indices, n, prev)
    a = x64 @ w64 + b64
    g = np.maximum(a, 0.0) + 1.0
    q = c * g
    with np.errstate(divide="ignore"):
        logq = np.log(q)
    return SimpleNamespace(c=c, terms=t, a=a, g=g, q=q, logq=logq, a_mag=np.abs(x64) @ np.abs(w64) + abs(b64))


def shifted_logits32(logq32):
    """(logq - max logq) - 20 in fp32, those two roundings, from fp32 logq."""
    l = np.asarray(logq32, dtype=F32)
    return ((l - l.max()).astype(F32) - F32(20.0)).astype(F32)


def sample(indptr, indices, n, targets, samp_num, num_layers, x, w_g, b_g, uniforms=None, logits=None, q_tables=None):
    """One batch, as ladies_oracle.sample.  logits: per layer fp32 logits over the candidates that replace the oracle's own (the
    device's, for bit-equal sets); q_tables: per layer a q over all nodes that replaces the oracle's in the weights (the device's)."""
    targets = np.asarray(targets, dtype=np.int64)
    prev, layers = targets, []
    for d in range(num_layers):
        cand = LO.candidates(indptr, indices, prev)
        imp = importance(indptr, indices, n, prev, x, w_g, b_g)
        l32 = np.asarray(logits[d], dtype=F32) if logits is not None else shifted_logits32(imp.logq[cand].astype(F32))
        sampled = LO.draw(l32, cand, samp_num, None if uniforms is None else uniforms[d])
        after = np.union1d(sampled, targets)
        q_all = imp.q if q_tables is None else np.asarray(q_tables[d], dtype=F64)
        src, dst, w, rt = LO.layer_entries(indptr, indices, n, prev, after, np.where(q_all > 0, q_all, 1.0))
        layers.append(SimpleNamespace(prev=prev, candidates=cand, imp=imp, sampled=sampled, after=after, src=src, dst=dst, w=w,
                                      row_terms=rt))
        prev = after
    node_idx = np.unique(np.concatenate([targets] + [L.after for L in layers]))
    local = np.full(n, -1, np.int64)
    local[node_idx] = np.arange(len(node_idx))
    return SimpleNamespace(node_idx=node_idx, targets=targets, local_targets=local[targets], layers=layers,
                           edge_index=[np.stack([local[L.src], local[L.dst]]) for L in layers], edge_weight=[L.w for L in layers],
                           local_prev=[local[L.prev] for L in layers])


# --------------------------------------------------------------------------------------------- the variance term
def _seq(v, dt):
    """The sum of v's rows one after the other in dtype dt."""
    v = np.asarray(v, dtype=dt)
    if v.shape[0] == 0:
        return np.zeros(v.shape[1:], dt)
    return np.add.accumulate(v, axis=0, dtype=dt)[-1]


def _rows_of(dst, rows):
    """Per row of `rows` the entry positions (the list is row-contiguous, rows in this order; a row may have none)."""
    dst = np.asarray(dst, dtype=np.int64)
    return [np.nonzero(dst == r)[0] for r in np.asarray(rows, dtype=np.int64)]


def variance(src, dst, w, rows, H, H32=None):
    """-> namespace: V, V_dev (the sum of squared deviations form), dw as triples' parts: V (ref [m]), V_mag, V32, L_var, dw, dw_mag,
    dw32.  Magnitudes: V: s sum w^2 |H|^2 + |mu|^2; dw: (2 / m)(s w |H|^2 + sum_c |mu_c| |H_jc|).  w is taken in fp32 (the
    sampler's weights as given); H is the reference's (fp64 as given), H32 the baseline's (default: H rounded)."""
    src, w32, H64 = np.asarray(src, dtype=np.int64), np.asarray(w, dtype=F32), np.asarray(H, dtype=F64)
    H32 = H64.astype(F32) if H32 is None else np.asarray(H32, dtype=F32)
    w64 = w32.astype(F64)
    segs, m, e = _rows_of(dst, rows), len(rows), len(src)
    V, Vd, Vm, V32 = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m, F32)
    dw, dwm, dw32 = np.zeros(e), np.zeros(e), np.zeros(e, F32)
    for r, idx in enumerate(segs):
        s = len(idx)
        if s == 0:
            continue
        Hj, wj = H64[src[idx]], w64[idx]
        mu = (wj[:, None] * Hj).sum(0)
        hh = (Hj * Hj).sum(1)
        V[r] = s * (wj * wj * hh).sum() - (mu * mu).sum()
        Vd[r] = ((s * wj[:, None] * Hj - mu) ** 2).sum() / s
        Vm[r] = s * (wj * wj * hh).sum() + (mu * mu).sum()
        dw[idx] = (2.0 / m) * (s * wj * hh - Hj @ mu)
        dwm[idx] = (2.0 / m) * (s * wj * hh + np.abs(Hj) @ np.abs(mu))
        Hj3, wj3 = H32[src[idx]], w32[idx]
        mu3 = _seq((wj3[:, None] * Hj3).astype(F32), F32)
        hh3 = _seq((Hj3 * Hj3).astype(F32).T, F32)
        mh3 = _seq((Hj3 * mu3).astype(F32).T, F32)
        acc3 = _seq(((wj3 * wj3).astype(F32) * hh3).astype(F32), F32)
        V32[r] = F32(F32(s) * acc3) - _seq((mu3 * mu3).astype(F32), F32)
        dw32[idx] = (F32(2.0) / F32(m)) * ((F32(s) * wj3).astype(F32) * hh3 - mh3).astype(F32)
    return SimpleNamespace(V=V, V_dev=Vd, V_mag=Vm, V32=V32, L_var=V.sum() / m, dw=dw, dw_mag=dwm, dw32=dw32)


# --------------------------------------------------------------------------------------------- d L / d logq
def logq_bwd(src, dst, w, G3, rows, n_local):
    """T[j] = sum_i w_ij (G_ij - Gbar_i), Gbar_i = sum_j G_ij w_ij, as a triple over n_local nodes; G3 = (G, |G| magnitude, G fp32).
    -> (T, T_mag, T32, abs_terms) with abs_terms = sum over the entries of w (|G| + Gbar_mag)."""
    src, w32 = np.asarray(src, dtype=np.int64), np.asarray(w, dtype=F32)
    w64 = w32.astype(F64)
    G, Gm, G32 = np.asarray(G3[0], dtype=F64), np.asarray(G3[1], dtype=F64), np.asarray(G3[2], dtype=F32)
    T, Tm, T32 = np.zeros(n_local), np.zeros(n_local), np.zeros(n_local, F32)
    for idx in _rows_of(dst, rows):                                       # rows in the list's order: the column sums' order
        if len(idx) == 0:
            continue
        gb, gbm = (G[idx] * w64[idx]).sum(), (Gm[idx] * w64[idx]).sum()
        gb32 = _seq((G32[idx] * w32[idx]).astype(F32), F32)
        T[src[idx]] += w64[idx] * (G[idx] - gb)
        Tm[src[idx]] += w64[idx] * (Gm[idx] + gbm)
        T32[src[idx]] = (T32[src[idx]] + (w32[idx] * (G32[idx] - gb32).astype(F32)).astype(F32)).astype(F32)
    return T, Tm, T32, float(Tm.sum())


def sampler_grads(T3_layers, a32, xb32):
    """From the per-layer T triples, the kernel's a over the batch rows (fp32, taken as given: its sign is the mask) and the gathered
    features: {"da" | "dw_g" | "db_g": (ref, mag, base)}, d L / d a_j = -[a_j > 0] / g_j sum_d T_j."""
    a32, xb32 = np.asarray(a32, dtype=F32), np.asarray(xb32, dtype=F32)
    mask = (a32 > 0).astype(F64)
    g64 = np.maximum(a32.astype(F64), 0.0) + 1.0
    g32 = (np.maximum(a32, F32(0)) + F32(1)).astype(F32)
    T = sum(t[0] for t in T3_layers); Tm = sum(t[1] for t in T3_layers)
    T32 = np.zeros(len(a32), F32)
    for t in T3_layers:
        T32 = (T32 + t[2]).astype(F32)
    da, dam = -mask / g64 * T, mask / g64 * Tm
    da32 = ((-mask.astype(F32) / g32).astype(F32) * T32).astype(F32)
    x64 = xb32.astype(F64)
    return {"da": (da, dam, da32),
            "dw_g": (da @ x64, dam @ np.abs(x64), _seq((da32[:, None] * xb32).astype(F32), F32)),
            "db_g": (np.array([da.sum()]), np.array([dam.sum()]), np.array([_seq(da32, F32)], F32))}


# --------------------------------------------------------------------------------------------- the whole step in fp64
def _weights_t(a, c_local, v, src, dst, n_local, mask):
    """A layer's weights as a torch fp64 function of a (the batch rows' pre-activations): q = c (mask a + 1),
    w = (v / q_src) / the row's sum of them.  mask: the 0/1 array that replaces [a > 0] (None: a's own sign)."""
    mk = torch.as_tensor(np.asarray(mask, dtype=F64)) if mask is not None else (a.detach() > 0).double()
    q = torch.as_tensor(np.asarray(c_local, dtype=F64)) * (a * mk + 1.0)
    src_t, dst_t = torch.as_tensor(np.asarray(src, dtype=np.int64)), torch.as_tensor(np.asarray(dst, dtype=np.int64))
    r = torch.as_tensor(np.asarray(v, dtype=F64)) / q[src_t]
    return r / torch.zeros(n_local, dtype=torch.float64).index_add_(0, dst_t, r)[dst_t]


def train_step64(x32, weights, biases, w_g, b_g, edge_index, c_local, v, local_prev, local_targets, labels, var_coef,
                 gates=None, mask=None, H_const=None):
    """The full step on a fixed batch in fp64 by autograd through the sampler's weights.  x32 [n_local, F] the gathered features;
    weights / biases the GCN's; edge_index per layer [2, e] local; c_local per layer the column mass over the batch rows (any
    positive value where a node is no column of the layer); v per layer v_ij of the entries; local_prev per layer the rows.
    H_const: the value H takes in L_var instead of this evaluation's own (H is a constant of the term: a finite difference of the loss
    must hold it at the base point's value, or it would also see H move with the hidden layer's weights).
    -> namespace: L_c, L_var, loss, dW, db (lists), dw_g, db_g, a, and per layer w (fp64), G = d loss / d w, T (by the closed form
    from G) and da_T = -[a > 0] / g sum T — the form the device computes, to be compared with autograd's da."""
    x = torch.as_tensor(np.asarray(x32, dtype=F64))
    n_local = x.shape[0]
    params = [(torch.as_tensor(np.asarray(W, dtype=F64)).requires_grad_(True), torch.as_tensor(np.asarray(b, dtype=F64)).requires_grad_(True))
              for W, b in zip(weights, biases)]
    wg = torch.as_tensor(np.asarray(w_g, dtype=F64).reshape(-1)).requires_grad_(True)
    bg = torch.as_tensor(np.asarray(b_g, dtype=F64).reshape(-1)).requires_grad_(True)
    a = x @ wg + bg
    a.retain_grad()
    ws = [_weights_t(a, c_local[d], v[d], edge_index[d][0], edge_index[d][1], n_local, mask) for d in range(len(edge_index))]
    for w in ws:
        w.retain_grad()
    L = len(params)
    h = x
    for i, (W, b) in enumerate(params):
        last = i == L - 1
        k = 0 if last else -(i + 1)
        src_t, dst_t = torch.as_tensor(np.asarray(edge_index[k][0], dtype=np.int64)), torch.as_tensor(np.asarray(edge_index[k][1], dtype=np.int64))
        Hh = h @ W.T
        if last:
            H0 = Hh.detach() if H_const is None else torch.as_tensor(np.asarray(H_const, dtype=F64))
        out = torch.zeros_like(Hh).index_add_(0, dst_t, ws[k][:, None] * Hh[src_t]) + b
        if not last:
            h = out * torch.as_tensor(np.asarray(gates[i], dtype=F64)) if gates is not None else out.clamp(min=0)
    L_c = LO.loss64(out, local_targets, labels)
    src0, dst0 = torch.as_tensor(np.asarray(edge_index[0][0], dtype=np.int64)), torch.as_tensor(np.asarray(edge_index[0][1], dtype=np.int64))
    rows0 = torch.as_tensor(np.asarray(local_prev[0], dtype=np.int64))
    m = len(rows0)
    s = torch.zeros(n_local, dtype=torch.float64).index_add_(0, dst0, torch.ones(len(dst0), dtype=torch.float64))
    mu = torch.zeros_like(H0).index_add_(0, dst0, ws[0][:, None] * H0[src0])
    sq = torch.zeros(n_local, dtype=torch.float64).index_add_(0, dst0, ws[0] ** 2 * (H0[src0] ** 2).sum(1))
    L_var = (s[rows0] * sq[rows0] - (mu[rows0] ** 2).sum(1)).sum() / m
    loss = L_c + var_coef * L_var
    loss.backward()
    a64 = a.detach().numpy()
    mk = np.asarray(mask, dtype=F64) if mask is not None else (a64 > 0).astype(F64)
    G = [w.grad.numpy().copy() if w.grad is not None else np.zeros(len(w)) for w in ws]
    T = []                                                               # (logq_bwd takes fp32 weights: here they stay fp64)
    for d in range(len(ws)):
        w64, src, t = ws[d].detach().numpy(), np.asarray(edge_index[d][0], dtype=np.int64), np.zeros(n_local)
        for idx in _rows_of(edge_index[d][1], local_prev[d]):
            if len(idx):
                t[src[idx]] += w64[idx] * (G[d][idx] - (G[d][idx] * w64[idx]).sum())
        T.append(t)
    da_T = -mk / (a64 * mk + 1.0) * sum(T)
    zero = lambda p: p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape))
    return SimpleNamespace(L_c=float(L_c.detach()), L_var=float(L_var.detach()), loss=float(loss.detach()),
                           dW=[zero(p[0]) for p in params], db=[zero(p[1]) for p in params], dw_g=zero(wg), db_g=zero(bg), a=a64,
                           da=a.grad.numpy() if a.grad is not None else np.zeros(n_local), w=[w.detach().numpy() for w in ws], G=G, T=T,
                           da_T=da_T, logits=out.detach().numpy(), H0=H0.numpy())


def entry_v(indptr, indices, src, dst):
    """v_ij of the entries (global ids): 2 on a stored loop's diagonal, else 1."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    stored = np.array([i in indices[indptr[i]:indptr[i + 1]] for i in dst], dtype=bool) if len(dst) else np.zeros(0, bool)
    return np.where((src == dst) & stored, 2.0, 1.0)
