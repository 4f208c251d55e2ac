"""Cluster-GCN on a CPU (numpy int64 / torch fp64): the partition tables, the cluster-union batch by the rule written in
include/grapes_hip.h — overflow and bad-id outcomes included — and ClusterGCNConv forward and backward.  Nothing here imports the
product."""
from types import SimpleNamespace

import numpy as np
import torch

F64 = np.float64
EDGE, NODE, BAD = 1, 2, 4                                                # the status bits
CHUNK = 64                                                               # the entries of one work item


def csr(rows):
    """(indptr int64, indices int32) of per-row column lists, kept exactly as given (order, duplicates, loops)."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.asarray([c for r in rows for c in r], dtype=np.int32).reshape(-1)


def random_graph(n, deg, seed, hub=None, hub_degree=0):
    """About `deg` random columns per row (duplicates and loops possible, stored order random); row `hub` gets hub_degree."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, n, int(rng.integers(max(deg - 3, 0), deg + 4))).tolist() for _ in range(n)]
    if hub is not None:
        rows[hub] = rng.integers(0, n, hub_degree).tolist()
    return csr(rows)


def partition_tables(part, P):
    """(perm, partptr, where [N, 2]): node ids in cluster order, ascending id inside a cluster; (cluster, position inside it)."""
    part = np.asarray(part, dtype=np.int64)
    N = len(part)
    assert part.min() >= 0 and part.max() < P
    perm = np.argsort(part, kind="stable")
    partptr = np.concatenate([[0], np.cumsum(np.bincount(part, minlength=P))]).astype(np.int64)
    where = np.zeros((N, 2), dtype=np.int64)
    where[:, 0] = part
    for c in range(P):
        where[perm[partptr[c]:partptr[c + 1]], 1] = np.arange(partptr[c + 1] - partptr[c])
    return perm, partptr, where


def range_partition(N, P):
    return np.arange(N, dtype=np.int64) * P // N


def batch(indptr, indices, part, P, clusters, n_cap=None, e_cap=None, item_cap=None):
    """The batch of the chosen clusters, in the given order -> namespace(status, n, e, e_total, cptr, node_idx, rowptr, rowptr_full,
    edge_index [2, e], e_id, rows, walked).  n_cap / e_cap None: room for everything.  rowptr_full holds n_cap + 1 values, e from n
    on.  rows / walked: the batch's rows and the entries its rows hold."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N, q = len(indptr) - 1, len(clusters)
    perm, partptr, where = partition_tables(part, P)
    clusters = [int(c) for c in clusters]
    status = 0
    refused = any(not 0 <= c < P for c in clusters) or len(set(clusters)) != len(clusters)
    cptr = np.zeros(q + 1, dtype=np.int64)
    if refused:
        status |= BAD
    else:
        cptr[1:] = np.cumsum([partptr[c + 1] - partptr[c] for c in clusters])
        if n_cap is not None and cptr[q] > n_cap:
            status |= NODE
            refused = True
            cptr[:] = 0
    n = int(cptr[q])
    nc = n if n_cap is None else n_cap
    node_idx = np.zeros(n, dtype=np.int64)
    base = {}
    if not refused:
        for k, c in enumerate(clusters):
            node_idx[cptr[k]:cptr[k + 1]] = perm[partptr[c]:partptr[c + 1]]
            base[c] = int(cptr[k])
    src, dst, eid, rowptr = [], [], [], [0]
    items, walked = 0, 0
    for i in range(n):
        v = int(node_idx[i])
        deg = int(indptr[v + 1] - indptr[v])
        walked += deg
        for t, j in enumerate(range(int(indptr[v]), int(indptr[v + 1]))):
            if item_cap is not None and items + t // CHUNK >= item_cap:
                status |= EDGE
                break
            u = int(indices[j])
            if not 0 <= u < N:
                status |= BAD
                continue
            if int(where[u, 0]) in base:
                src.append(base[int(where[u, 0])] + int(where[u, 1])); dst.append(i); eid.append(j)
        items += (deg + CHUNK - 1) // CHUNK
        rowptr.append(len(src))
    e_total = len(src)
    e = e_total if e_cap is None else min(e_total, e_cap)
    if e_total > e:
        status |= EDGE
    rowptr = np.minimum(np.asarray(rowptr, dtype=np.int64), e)
    full = np.full(nc + 1, e, dtype=np.int64)
    full[:n + 1] = rowptr
    return SimpleNamespace(status=status, n=n, e=e, e_total=e_total, cptr=cptr, node_idx=node_idx, rowptr=rowptr, rowptr_full=full,
                           edge_index=np.array([src[:e], dst[:e]], dtype=np.int64).reshape(2, e), e_id=np.asarray(eid[:e], dtype=np.int64),
                           rows=n, walked=walked)


def dense_batch(indptr, indices, part, clusters):
    """The same batch by brute force: a dense membership mask over the nodes, node_idx by concatenation, every stored entry tested."""
    indptr, indices, part = np.asarray(indptr), np.asarray(indices), np.asarray(part)
    node_idx = np.concatenate([np.nonzero(part == c)[0] for c in clusters] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    local = np.full(len(part), -1, dtype=np.int64)
    local[node_idx] = np.arange(len(node_idx))
    src, dst, eid = [], [], []
    for i, v in enumerate(node_idx):
        for j in range(int(indptr[v]), int(indptr[v + 1])):
            if local[indices[j]] >= 0:
                src.append(int(local[indices[j]])); dst.append(i); eid.append(j)
    return node_idx, np.array([src, dst], dtype=np.int64).reshape(2, len(src)), np.asarray(eid, dtype=np.int64)


# --------------------------------------------------------------------------------------------- ClusterGCNConv in fp64
def _noloop(ei):
    src, dst = np.asarray(ei[0], dtype=np.int64), np.asarray(ei[1], dtype=np.int64)
    keep = src != dst
    return src[keep], dst[keep]


def degrees(ei, n):
    """d_i = 1 + the stored entries into i that are not loops (duplicates by multiplicity)."""
    _, dst = _noloop(ei)
    return 1.0 + np.bincount(dst, minlength=n).astype(F64)


def propagate64(x, ei, n, lam):
    """(A^ x)_i = (sum_{j -> i, j != i} x_j + (1 + lam) x_i) / d_i; x fp64 torch [n, f]."""
    src, dst = (torch.as_tensor(a) for a in _noloop(ei))
    s = torch.zeros((n, x.shape[1]), dtype=torch.float64).index_add_(0, dst, x[src])
    return (s + (1.0 + lam) * x) / torch.as_tensor(degrees(ei, n))[:, None]


def conv64(x, ei, w_out, b, w_root, lam=0.0, relu=False, gate=None):
    """act(A^ x W_outᵀ + b + x W_rootᵀ); b may be None.  gate: a 0/1 array that replaces the ReLU."""
    out = propagate64(x, ei, x.shape[0], lam) @ w_out.T + x @ w_root.T
    if b is not None:
        out = out + b
    if gate is not None:
        return out * torch.as_tensor(np.asarray(gate, dtype=F64))
    return out.clamp(min=0) if relu else out


def conv_backward64(x, ei, w_out, w_root, lam, g):
    """(dx, dW_out, db, dW_root) of conv64 (no activation) for the output gradient g, by the closed form the kernels use:
    d(A^ x) = g W_out; dx_j = sum_{i <- j} s_i (g W_out)_i + (1 + lam) s_j (g W_out)_j + (g W_root)_j."""
    x, w_out, w_root, g = (np.asarray(a, dtype=F64) for a in (x, w_out, w_root, g))
    n = x.shape[0]
    s = 1.0 / degrees(ei, n)
    src, dst = _noloop(ei)
    da = g @ w_out
    dx = (1.0 + lam) * s[:, None] * da + g @ w_root
    np.add.at(dx, src, s[dst][:, None] * da[dst])
    ax = propagate64(torch.as_tensor(x), ei, n, lam).numpy()
    return dx, g.T @ ax, g.sum(0), g.T @ x


def dense_conv64(x, ei, w_out, b, w_root, lam):
    """The dense closed form under torch: A^ = D⁻¹(A_noloop + I) + lam diag(D⁻¹); out = A^ x W_outᵀ + b + x W_rootᵀ."""
    n = x.shape[0]
    src, dst = _noloop(ei)
    A = torch.zeros((n, n), dtype=torch.float64)
    A.index_put_((torch.as_tensor(dst), torch.as_tensor(src)), torch.ones(len(src), dtype=torch.float64), accumulate=True)
    dinv = 1.0 / (A.sum(1) + 1.0)
    Ahat = dinv[:, None] * (A + torch.eye(n, dtype=torch.float64)) + lam * torch.diag(dinv)
    return Ahat @ x @ w_out.T + b + x @ w_root.T


def forward64(x, params, ei, lam=0.0, gates=None):
    """ClusterGCN over ONE edge list: ReLU on the hidden layers.  params [(W_out, b, W_root), ...] fp64 torch."""
    L = len(params)
    for i, (w_out, b, w_root) in enumerate(params):
        last = i == L - 1
        x = conv64(x, ei, w_out, b, w_root, lam, relu=not last, gate=None if (last or gates is None) else gates[i])
    return x


def masked_loss64(logits, rows, labels):
    """Mean CrossEntropy over the given rows of the logits; labels: one per given row."""
    z = logits[torch.as_tensor(np.asarray(rows, dtype=np.int64))]
    return torch.nn.functional.cross_entropy(z, torch.as_tensor(np.asarray(labels)).long())


def train_step64(x32, params32, ei, rows, labels, lam=0.0, gates=None):
    """(loss, [(dW_out, db, dW_root), ...], logits) in fp64 by autograd; params32 [(W_out, b, W_root), ...] numpy."""
    x = torch.as_tensor(np.asarray(x32, dtype=F64))
    params = [tuple(torch.as_tensor(np.asarray(p, dtype=F64)).requires_grad_(True) for p in layer) for layer in params32]
    logits = forward64(x, params, ei, lam, gates)
    loss = masked_loss64(logits, rows, labels)
    loss.backward()
    return float(loss.detach()), [tuple(p.grad.numpy() for p in layer) for layer in params], logits.detach().numpy()
