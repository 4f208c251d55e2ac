"""numpy restatement of GraphSAINT's normalisation (grapes_amd/modules/saint.py: estimate_norm; csrc/saint_kernels.hip) [PyG-recall:
PyG 2.5 GraphSAINTSampler._compute_norm / __collate__, examples/graph_saint.py]: the coverage counts as integers, the two norm
vectors by their fp32 rules, the weighted loss with its gradient in fp64 (and, for the accuracy criterion, in fp32 by the kernel's
formula), and the normalised two-layer step on a dense weighted adjacency.  No GPU."""
import numpy as np
import torch

F32 = np.float32


def entry_rows(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def coverage_counts(rowptr, col, node_sets):
    """(node_count int64 [N], edge_count int64 [nnz], total): node_count[v] += 1 for v in each set (duplicates of a set removed),
    edge_count[j] += 1 for every stored entry j whose row and column are both in it, total += |set|."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    row = entry_rows(rowptr)
    node_count, edge_count, total = np.zeros(n, np.int64), np.zeros(len(col), np.int64), 0
    for ns in node_sets:
        ns = np.unique(np.asarray(ns, np.int64))
        member = np.zeros(n, bool)
        member[ns] = True
        node_count[ns] += 1
        edge_count += (member[row] & member[col]).astype(np.int64)
        total += len(ns)
    return node_count, edge_count, total


def norms(rowptr, node_count, edge_count, num_samples):
    """(edge_norm fp32 [nnz], node_norm fp32 [N]): every operation in fp32, in the order the issue states."""
    n = len(rowptr) - 1
    nc, ec = np.asarray(node_count), np.asarray(edge_count)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = nc[entry_rows(rowptr)].astype(F32) / ec.astype(F32)
    nan = np.isnan(q)
    q = np.minimum(np.maximum(q, F32(0)), F32(1e4))
    q[nan] = F32(0.1)
    c = nc.astype(F32)
    c[nc == 0] = F32(0.1)
    node_norm = (F32(num_samples) / c) / F32(n)
    return q.astype(F32), node_norm.astype(F32)


def weighted_loss(z, y, w, train, dtype=np.float64):
    """(loss, g, loss_mag, g_mag) of the normalised step's loss over the rows i with train[i]: loss = sum_i w_i rowloss_i.
    y 1-D: rowloss = lse - z[y], g = w (softmax - onehot).  y 2-D: rowloss = mean_c (max(z, 0) - z y + log1p(exp(-|z|))),
    g = w (sigmoid - y) / C.  Rows that do not train have g = 0.  dtype float32 evaluates the kernel's formulas in fp32 (the rows
    added one after the other in fp32; the cross-entropy rows shift first, lsm = (z - max) - log(se), so that a common offset of a
    row costs the baseline nothing): the baseline of oracle/accuracy.py's criterion.  *_mag: the sums of the absolute values of
    the terms each output adds up (fp64 only meaningful)."""
    z = np.asarray(z).astype(dtype)
    w = np.asarray(w).astype(dtype)
    train = np.asarray(train, bool)
    y = np.asarray(y)
    n, C = z.shape
    g = np.zeros((n, C), dtype)
    gm = np.zeros((n, C), dtype)
    rows = np.nonzero(train)[0]
    zt, wt = z[rows], w[rows]
    if y.ndim == 1:
        yt = y[rows].astype(np.int64)
        mx = zt.max(1)
        se = np.exp(zt - mx[:, None]).sum(1, dtype=dtype)
        lse = mx + np.log(se)
        zy = zt[np.arange(len(rows)), yt]
        if dtype == np.float64:
            p = np.exp(zt - lse[:, None])
            rl = lse - zy
        else:       # the fp32 baseline shifts first, as the kernels and torch's log_softmax do: no rounding at the size of mx
            lsm = (zt - mx[:, None]) - np.log(se)[:, None]
            p = np.exp(lsm)
            rl = -lsm[np.arange(len(rows)), yt]
        one = np.zeros_like(p)
        one[np.arange(len(rows)), yt] = 1
        rl_mag = np.abs(lse) + np.abs(zy)
        g[rows] = (p - one) * wt[:, None]
        gm[rows] = (p + one) * np.abs(wt)[:, None]
    else:
        yt = y[rows].astype(dtype)
        el = np.maximum(zt, 0) - zt * yt + np.log1p(np.exp(-np.abs(zt)))
        rl = el.sum(1, dtype=dtype) / dtype(C)
        rl_mag = (np.maximum(zt, 0) + np.abs(zt * yt) + np.log1p(np.exp(-np.abs(zt)))).sum(1) / C
        sig = dtype(1) / (dtype(1) + np.exp(-zt))
        wc = wt / dtype(C)
        g[rows] = (sig - yt) * wc[:, None]
        gm[rows] = (sig + np.abs(yt)) * np.abs(wc)[:, None]
    terms = (wt * rl).astype(dtype)
    loss = np.add.accumulate(terms, dtype=dtype)[-1] if len(terms) else dtype(0)
    return loss, g, float((np.abs(wt) * rl_mag).sum()), gm


def wgcn_dense(src, dst, w, n):
    """PyG gcn_norm with edge weights as a dense fp64 matrix P (out = P @ h): A[d, s] += w over the non-loop edges s -> d; the
    loop weight lw[i] = 1, or the weight of the LAST stored loop (i, i); deg = A.sum(1) + lw; P = D^-1/2 (A + diag(lw)) D^-1/2."""
    A = np.zeros((n, n))
    lw = np.ones(n)
    for s, d, x in zip(np.asarray(src), np.asarray(dst), np.asarray(w, np.float64)):
        if s == d:
            lw[s] = x
        else:
            A[d, s] += x
    deg = A.sum(1) + lw
    with np.errstate(divide="ignore"):
        dinv = np.where(deg > 0, deg ** -0.5, 0.0)
    return dinv[:, None] * (A + np.diag(lw)) * dinv[None, :]


def normalised_step(x_rows, P, weights, y_rows, w_rows, train, mm=None, dtype=np.float64):
    """The normalised step on a dense adjacency: z = P relu(P (x W1ᵀ) + b1) W2ᵀ + b2, loss = weighted_loss(z), and the gradients
    written out by hand so that every contraction goes through mm(a, b) = a @ b: fp64 by default; the fp32 baseline passes a
    fixed-order fp32 product.  Returns (loss, [dW1, db1, dW2, db2], [mag of each]) — mag: for dW = dHᵀ X the sum |dH|ᵀ |X| of the
    absolute terms of that last contraction, for db the column sums of |dZ|, both from this pass's own values."""
    cast = lambda a: np.asarray(a).astype(dtype)
    if mm is None:
        mm = lambda a, b: a @ b
    x, P = cast(x_rows), cast(P)
    W1, b1, W2, b2 = [cast(t) for t in weights]
    h1 = mm(x, W1.T)
    a1 = np.maximum(mm(P, h1) + b1, 0).astype(dtype)
    h2 = mm(a1, W2.T)
    z = (mm(P, h2) + b2).astype(dtype)
    loss, gz, _, _ = weighted_loss(z, y_rows, w_rows, train, dtype)
    dh2 = mm(P.T, gz)
    dW2 = mm(dh2.T, a1)
    da1 = mm(dh2, W2) * (a1 > 0)
    dh1 = mm(P.T, da1)
    dW1 = mm(dh1.T, x)
    grads = [dW1, da1.sum(0, dtype=dtype), dW2, gz.sum(0, dtype=dtype)]
    mags = [np.abs(dh1).T @ np.abs(x), np.abs(da1).sum(0), np.abs(dh2).T @ np.abs(a1), np.abs(gz).sum(0)]
    return loss, grads, mags


def torch_weighted_ce(z, y, w, train):
    """(loss, d loss / d z) by torch in fp64: (F.cross_entropy(z, y, reduction='none') * w)[train].sum() and its autograd gradient."""
    zt = torch.tensor(np.asarray(z, np.float64), requires_grad=True)
    loss = (torch.nn.functional.cross_entropy(zt, torch.as_tensor(np.asarray(y, np.int64)), reduction="none") *
            torch.as_tensor(np.asarray(w, np.float64)))[torch.as_tensor(np.asarray(train, bool))].sum()
    loss.backward()
    return float(loss.detach()), zt.grad.numpy()
