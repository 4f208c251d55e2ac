"""The GNNAutoScale rule of include/grapes_hip.h in numpy / torch fp64: the resolve as plain loops, the aggregation over
(local row | history row) codes with its backward over the batch's induced entries, and a whole training step.  The graph is a
loop-free CSR (rowptr, col as numpy integer arrays), d_u = row u's stored entries, dinv_u = (d_u + 1)^-1/2,
P = D^-1/2 (A + I) D^-1/2, duplicates counting once each."""
import numpy as np
import torch

BAD_CODE = 2 ** 31 - 1


def dinv(rowptr):
    """(d + 1)^-1/2 as torch fp64 [N]."""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    return torch.from_numpy(1.0 / np.sqrt(deg.astype(np.float64) + 1.0))


def batch_nodes(part, clusters):
    """node_idx of the union of `clusters` under the assignment `part` [N]: cluster by cluster in the given order, ascending id
    inside a cluster."""
    part = np.asarray(part)
    return np.concatenate([np.nonzero(part == int(c))[0] for c in clusters]).astype(np.int64)


def resolve(rowptr, col, node_idx):
    """(rowptr_h int32 [n + 1], code int32 [total], counts int64 [2]): for every batch row i, u = node_idx[i], and every stored
    entry v of row u in the CSR's order: the local row of v when v is in the batch, else -1 - v."""
    loc = {int(v): i for i, v in enumerate(node_idx)}
    rowptr_h, code, n_in, n_out = [0], [], 0, 0
    for u in node_idx:
        for t in range(int(rowptr[u]), int(rowptr[u + 1])):
            v = int(col[t])
            if v in loc:
                code.append(loc[v]); n_in += 1
            else:
                code.append(-1 - v); n_out += 1
        rowptr_h.append(len(code))
    return np.asarray(rowptr_h, dtype=np.int32), np.asarray(code, dtype=np.int32), np.asarray([n_in, n_out], dtype=np.int64)


def induced_edges(rowptr_h, code):
    """(src, dst) local ids of the batch's induced entries, by target row then the CSR's order: ClusterLoader's edge_index."""
    dst = np.repeat(np.arange(len(rowptr_h) - 1), np.diff(rowptr_h))
    keep = code >= 0
    return code[keep].astype(np.int64), dst[keep].astype(np.int64)


def aggregate(h, hbar, dv, node_idx, rowptr_h, code):
    """A [n, f] (fp64): A[i] = dinv_u (dinv_u h[i] + sum_t dinv_{v_t} (code_t >= 0 ? h[code_t] : hbar[-1 - code_t]))."""
    h, hbar = h.double(), hbar.double()
    idx = torch.from_numpy(np.asarray(node_idx, dtype=np.int64))
    c = torch.from_numpy(np.asarray(code, dtype=np.int64))
    dst = torch.from_numpy(np.repeat(np.arange(len(rowptr_h) - 1), np.diff(rowptr_h)).astype(np.int64))
    inb = c >= 0
    acc = dv[idx][:, None] * h
    acc = acc.index_add(0, dst[inb], dv[idx[c[inb]]][:, None] * h[c[inb]])
    g = -1 - c[~inb]
    acc = acc.index_add(0, dst[~inb], dv[g][:, None] * hbar[g])
    return dv[idx][:, None] * acc


def aggregate_bwd(da, dv, node_idx, src, dst):
    """dh [n, f]: dh[j] = dinv_{v_j} (dinv_{v_j} da[j] + sum over the induced entries (src = j, dst = i) of dinv_{u_i} da[i])."""
    da = da.double()
    idx = torch.from_numpy(np.asarray(node_idx, dtype=np.int64))
    s, d = torch.from_numpy(np.asarray(src, dtype=np.int64)), torch.from_numpy(np.asarray(dst, dtype=np.int64))
    acc = dv[idx][:, None] * da
    acc = acc.index_add(0, s, dv[idx[d]][:, None] * da[d])
    return dv[idx][:, None] * acc


class _Agg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, hbar, dv, node_idx, rowptr_h, code):
        ctx.args = (dv, node_idx) + induced_edges(rowptr_h, code)
        return aggregate(h, hbar, dv, node_idx, rowptr_h, code)

    @staticmethod
    def backward(ctx, da):
        return aggregate_bwd(da, *ctx.args), None, None, None, None, None


def propagate(rowptr, col, x):
    """P x for every node (fp64)."""
    x, dv = x.double(), dinv(rowptr)
    N = len(rowptr) - 1
    row = torch.from_numpy(np.repeat(np.arange(N), np.diff(rowptr)).astype(np.int64))
    c = torch.from_numpy(np.asarray(col, dtype=np.int64))
    acc = (dv[:, None] * x).index_add(0, row, dv[c][:, None] * x[c])
    return dv[:, None] * acc


def full_forward(rowptr, col, x, weights):
    """The exact full-graph GCN: the list [H^(1), ..., H^(L - 1), logits] (fp64); weights = [(W, b), ...]."""
    h, outs = x.double(), []
    for i, (w, b) in enumerate(weights):
        z = propagate(rowptr, col, h) @ w.double().T + b.double()
        h = torch.relu(z) if i < len(weights) - 1 else z
        outs.append(h)
    return outs


def forward(rowptr, col, px, weights, histories, node_idx, rowptr_h, code, gates=None):
    """(logits [n, C], [H^(1), ..., H^(L - 1)] on the batch's rows) of the GAS forward; px = P X (fp64), histories = [Hbar^(1), ...].
    gates: per level a bool array [n, hidden_l] that stands in for z > 0 (a device's own gates, so that a pre-activation within
    fp32 rounding of 0 cannot flip a whole gradient row)."""
    dv = dinv(rowptr)
    idx = torch.from_numpy(np.asarray(node_idx, dtype=np.int64))
    L = len(weights)
    z = px[idx] @ weights[0][0].T + weights[0][1]
    acts = []
    for i in range(1, L):
        h = torch.relu(z) if gates is None else z * torch.as_tensor(gates[i - 1]).to(z.dtype)
        acts.append(h)
        a = _Agg.apply(h, histories[i - 1].double(), dv, node_idx, rowptr_h, code)
        z = a @ weights[i][0].T + weights[i][1]
    return z, acts


def step(rowptr, col, x, y, train_mask, weights, histories, node_idx, gates=None):
    """One step on the batch `node_idx`: (loss, [dW], [db], the histories after the push), all fp64.  weights = [(W, b), ...] and
    histories = [Hbar^(1), ...] are not modified.  The loss is the mean cross entropy over the batch's training rows."""
    ws = [(w.detach().double().clone().requires_grad_(True), b.detach().double().clone().requires_grad_(True)) for w, b in weights]
    rowptr_h, code, _ = resolve(rowptr, col, node_idx)
    logits, acts = forward(rowptr, col, propagate(rowptr, col, x), ws, histories, node_idx, rowptr_h, code, gates)
    idx = torch.from_numpy(np.asarray(node_idx, dtype=np.int64))
    m = train_mask[idx]
    loss = torch.nn.functional.cross_entropy(logits[m], y[idx][m])
    loss.backward()
    new = [hb.double().clone() for hb in histories]
    for hb, h in zip(new, acts):
        hb[idx] = h.detach()
    return float(loss.detach()), [w.grad for w, _ in ws], [b.grad for _, b in ws], new


def random_graph(n, avg_deg, seed, dup=None):
    """A symmetric loop-free CSR (rowptr int64, col int32) of about n avg_deg / 2 undirected edges.  dup = (u, v): entry (u, v)
    is stored TWICE while (v, u) stays once — the stored multiset is then not its own transpose."""
    rng = np.random.default_rng(seed)
    m = max(1, int(n * avg_deg / 2))
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = a != b
    pairs = {(min(int(p), int(q)), max(int(p), int(q))) for p, q in zip(a[keep], b[keep])}
    if dup is not None:
        pairs.add((min(dup), max(dup)))
    src = [p for p, q in pairs] + [q for p, q in pairs]
    dst = [q for p, q in pairs] + [p for p, q in pairs]
    if dup is not None:
        src.append(dup[0]); dst.append(dup[1])
    return csr_from_edges(n, np.asarray(src), np.asarray(dst))


def csr_from_edges(n, row, col):
    order = np.lexsort((col, row))
    row, col = np.asarray(row)[order], np.asarray(col)[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
    return rowptr, col.astype(np.int32)
