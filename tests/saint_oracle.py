"""CPU restatement (numpy / fp64 torch) of GraphSAINT random-walk sampling and one training step, for the tests of
grapes_amd.saint.  The package never imports this module.

Contract (PyG 2.5 GraphSAINTRandomWalkSampler with num_steps 1, sample_coverage 0; torch_cluster random_walk, p = q = 1):
a node without neighbours stays; otherwise next = col[rowptr[v] + int64(fp32(u) * fp32(deg))], clamped to deg - 1;
node_idx = unique(walks); the induced subgraph in CSR order, relabelled to positions in node_idx; stored self-loops stay.
"""
import numpy as np
import torch


def walk(rowptr, col, roots, uniforms, L):
    """walks int64 [B, L + 1]; uniforms fp32 [B, L]."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    roots = np.asarray(roots, dtype=np.int64)
    u = np.asarray(uniforms, dtype=np.float32).reshape(len(roots), L)
    out = np.empty((len(roots), L + 1), dtype=np.int64)
    for b, v in enumerate(roots):
        out[b, 0] = v
        for t in range(L):
            a, deg = rowptr[v], rowptr[v + 1] - rowptr[v]
            if deg > 0:
                k = min(int(np.float32(u[b, t]) * np.float32(deg)), int(deg) - 1)
                v = int(col[a + k])
            out[b, t + 1] = v
    return out


def node_set(walks):
    return np.unique(np.asarray(walks).reshape(-1))


def induced_subgraph(rowptr, col, node_idx):
    """(src, dst) local int64 arrays in CSR order."""
    pos = {int(v): i for i, v in enumerate(node_idx)}
    src, dst = [], []
    for i, v in enumerate(node_idx):
        for c in col[rowptr[v]:rowptr[v + 1]]:
            j = pos.get(int(c))
            if j is not None:
                src.append(i); dst.append(j)
    return np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)


def gcn_norm_dense(src, dst, n):
    """PyG GCNConv's propagation matrix (fp64): out = P @ h, P[d, s] = dinv[s] dinv[d] for every edge s -> d without the
    stored self-loops, plus the unit self-loop; deg = in-degree + 1."""
    src, dst = np.asarray(src), np.asarray(dst)
    keep = src != dst
    s, d = src[keep], dst[keep]
    A = np.zeros((n, n))
    np.add.at(A, (d, s), 1.0)
    A += np.eye(n)
    dinv = 1.0 / np.sqrt(A.sum(1))
    return torch.from_numpy(dinv[:, None] * A * dinv[None, :])


def step_fp64(x_rows, src, dst, n, weights, train_rows, y_rows):
    """loss and gradients (W1, b1, W2, b2, x_rows) of graphsaint.py:31-36 in fp64.  weights: [W1, b1, W2, b2] (PyG layout)."""
    P = gcn_norm_dense(src, dst, n)
    W1, b1, W2, b2 = [torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True) for w in weights]
    x = torch.tensor(np.asarray(x_rows, dtype=np.float64), requires_grad=True)
    h = torch.relu(P @ (x @ W1.T) + b1)
    z = P @ (h @ W2.T) + b2
    tr = torch.as_tensor(np.asarray(train_rows, dtype=np.int64))
    yy = torch.as_tensor(np.asarray(y_rows))
    if yy.dim() == 1:
        loss = torch.nn.functional.cross_entropy(z[tr], yy[tr].long())
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(z[tr], yy[tr].double())
    loss.backward()
    return float(loss.detach()), [t.grad.numpy() for t in (W1, b1, W2, b2, x)]
