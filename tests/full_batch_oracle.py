"""TEST INFRASTRUCTURE — plain numpy / torch restatements of the kernels under the row-blocked full-batch trainer
(grapes_amd/full_graph.py train_step; include/grapes_hip.h "full-batch training over the same graphs"): the row-list transpose, the
transposed gather, the row dropout's mask and the row-list loss with its gradient, fp64 by default, each with the magnitude of
every output (the sum of the absolute values of the terms it adds up) for oracle/accuracy.py's criterion; the host fp32 baselines
of that criterion; the problems the CPU and the GPU test share.  No GPU.

The fp32 baseline of the loss (rowlist_loss_base) is torch's own cross_entropy / binary_cross_entropy_with_logits with fp32 autograd
on the CPU, NOT a restatement of the kernel's formulas: a baseline written in the kernel's order of operations inherits the kernel's
weakness and cannot show it.  ce_rows_f32 emulates the two orders a cross-entropy row can be written in; only
tests/test_full_batch_kernels_cpu.py uses it, to show that the criterion separates them on the "shifted" logits."""
import numpy as np
import torch

from oracle import accuracy as acc
from oracle import portable_math as pm

F32 = np.float32
N_LOSS = 2000                   # nodes of every loss problem
LOSS_KINDS = ("normal", "wide", "shifted", "bce-extreme")


# ------------------------------------------------------------------------------------------------------------ graphs
def kernel_graph(n=700, seed=0, hub=13, hub_rows=320, long_rows=((100, 65), (200, 130), (301, 300))):
    """A by-target CSR (rowptr int64 [n + 1], col int32, a row's columns ascending and distinct) over n nodes with
      * rows with no entries: i % 7 == 3 and i % 5 != 0;
      * rows whose only entry is a stored self-loop: i % 7 == 3 and i % 5 == 0;
      * a stored self-loop on every fifth node;
      * the source `hub` stored in hub_rows rows;
      * long_rows = ((row, entries), ...): rows longer than a 64-entry chunk.
    The other rows hold 1 .. 17 sources.  -> (rowptr, col, info) with info = {"empty", "loop_only", "hub", "hub_rows", "long"}."""
    rng = np.random.default_rng(seed)
    lens_cycle = (1, 2, 3, 5, 8, 15, 16, 17)
    special = np.arange(n) % 7 == 3
    special[hub] = False
    for r, _ in long_rows:
        special[r] = False
    rows = [np.zeros(0, np.int64) for _ in range(n)]
    plain = np.nonzero(~special)[0]
    for k, r in enumerate(plain):
        others = np.delete(np.arange(n), r)
        rows[r] = rng.choice(others, lens_cycle[k % len(lens_cycle)], replace=False)
    for r, L in long_rows:
        others = np.delete(np.arange(n), [min(r, hub), max(r, hub)]) if r != hub else np.delete(np.arange(n), r)
        rows[r] = rng.choice(others, L, replace=False)
    with_hub = rng.choice(plain[plain != hub], hub_rows, replace=False)
    for r in with_hub:
        rows[r] = np.append(rows[r], hub)
    for r in range(0, n, 5):
        rows[r] = np.append(rows[r], r)
    rows = [np.unique(v) for v in rows]
    rowptr = np.concatenate([[0], np.cumsum([len(v) for v in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    empty = np.nonzero(special & (np.arange(n) % 5 != 0))[0]
    loop_only = np.nonzero(special & (np.arange(n) % 5 == 0))[0]
    hub_rows_ = np.array(sorted(r for r in range(n) if hub in rows[r] and r != hub), np.int64)
    return rowptr, col, {"empty": empty, "loop_only": loop_only, "hub": hub, "hub_rows": hub_rows_,
                         "long": np.array([r for r, _ in long_rows], np.int64)}


def host_dinv(rowptr, col):
    """fp32 (1 + entries of the row other than the row itself)^-1/2: gcn_norm with PyG's self-loop replacement."""
    rowptr = np.asarray(rowptr, np.int64)
    n = len(rowptr) - 1
    r = np.repeat(np.arange(n), np.diff(rowptr))
    deg = np.bincount(r[np.asarray(col)[:rowptr[-1]] != r], minlength=n)
    return (1.0 / np.sqrt(deg + 1.0)).astype(F32)


def without_loops(rowptr, col):
    """(rowptr, col int64, lens) of the CSR with its stored self-loops removed: what oracle.accuracy.aggregate_reference takes."""
    rowptr = np.asarray(rowptr, np.int64)
    n = len(rowptr) - 1
    col = np.asarray(col, np.int64)[:rowptr[-1]]
    r = np.repeat(np.arange(n), np.diff(rowptr))
    keep = col != r
    rt = np.concatenate([[0], np.cumsum(np.bincount(r[keep], minlength=n))]).astype(np.int64)
    return rt, col[keep], np.diff(rt)


def dense_adjacency(rowptr, col, dinv):
    """Â as a dense fp64 matrix: Â[r, s] = dinv[r] dinv[s] for every stored s != r of row r, Â[r, r] = dinv[r]^2."""
    rowptr = np.asarray(rowptr, np.int64)
    n = len(rowptr) - 1
    d = np.asarray(dinv, np.float64)
    A = np.zeros((n, n))
    for r in range(n):
        for s in np.asarray(col)[rowptr[r]:rowptr[r + 1]]:
            if s != r:
                A[r, s] += d[r] * d[s]
        A[r, r] = d[r] * d[r]
    return A


# ------------------------------------------------------------------------------------------------- row-list transpose
def rowlist_transpose_ref(rowptr_t, col_t, n, rows):
    """(srcs int32 [n_src], src_off int64 [n_src + 1], pos int32 [entries]) by the header's definition: for rows[p] = r every
    stored s != r of row r gives the entry (s, p), one (r, p) is added per row; sources ascend, positions ascend within a source."""
    rowptr_t, col_t, rows = np.asarray(rowptr_t, np.int64), np.asarray(col_t, np.int64), np.asarray(rows, np.int64)
    ss, pp = [], []
    for p, r in enumerate(rows):
        s = col_t[rowptr_t[r]:rowptr_t[r + 1]]
        s = np.append(s[s != r], r)
        ss.append(s); pp.append(np.full(len(s), p, np.int64))
    ss = np.concatenate(ss) if ss else np.zeros(0, np.int64)
    pp = np.concatenate(pp) if pp else np.zeros(0, np.int64)
    assert ss.size == 0 or (ss.min() >= 0 and ss.max() < n)
    o = np.lexsort((pp, ss))
    ss, pp = ss[o], pp[o]
    srcs, counts = np.unique(ss, return_counts=True)
    src_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return srcs.astype(np.int32), src_off, pp.astype(np.int32)


def gather_t_ref(g, srcs, src_off, pos, dinv, dtype=np.float64):
    """(out, mag): out[j] = dinv[srcs[j]] * sum_k g[pos[k]] over k in [src_off[j], src_off[j + 1]), mag = dinv[srcs[j]] * sum |g[pos[k]]|.
    dtype float32: the host baseline, a source's entries added one after the other in position order in fp32, then the product."""
    g = np.asarray(g).astype(dtype)
    d = np.asarray(dinv).astype(dtype)[np.asarray(srcs, np.int64)]
    src_off, pos = np.asarray(src_off, np.int64), np.asarray(pos, np.int64)
    out = np.zeros((len(srcs), g.shape[1]), dtype)
    mag = np.zeros((len(srcs), g.shape[1]), dtype)
    for j in range(len(srcs)):
        t = np.ascontiguousarray(g[pos[src_off[j]:src_off[j + 1]]])
        if dtype == np.float32:
            out[j] = acc._seq_sum_f32(t)
            mag[j] = acc._seq_sum_f32(np.abs(t))
        else:
            out[j] = t.sum(0)
            mag[j] = np.abs(t).sum(0)
    return (d[:, None] * out).astype(dtype), (d[:, None] * mag).astype(dtype)


def value_rows(kind, m, f, seed):
    """fp32 [m, f] operand rows of acc.KINDS: normal N(0, 1); mixed, row r at 10^a_r with a in [-12, 12]; zeros, N(0, 1) with whole
    zero rows, single zero entries and a zero column."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, f))
    if kind == "mixed":
        x *= 10.0 ** rng.uniform(-12, 12, m)[:, None]
    elif kind == "zeros":
        x[rng.integers(0, m, max(1, m // 50))] = 0.0
        x[rng.integers(0, m, m), rng.integers(0, f, m)] = 0.0
        x[:, f // 2] = 0.0
    elif kind not in acc.KINDS:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=F32)


GATHER_ENTRIES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)     # entries per hand-built source: both sides of chunk / 4, chunk, 2 chunks
GATHER_M = 400


def gather_structure(seed=0, n_nodes=50):
    """A hand-built (srcs, src_off, pos, dinv): source j has exactly GATHER_ENTRIES[j] ascending distinct positions in [0, GATHER_M)."""
    rng = np.random.default_rng(seed)
    srcs = np.sort(rng.choice(n_nodes, len(GATHER_ENTRIES), replace=False)).astype(np.int32)
    pos = [np.sort(rng.choice(GATHER_M, L, replace=False)) for L in GATHER_ENTRIES]
    src_off = np.concatenate([[0], np.cumsum(GATHER_ENTRIES)]).astype(np.int64)
    dinv = (1.0 / np.sqrt(rng.integers(1, 40, n_nodes))).astype(F32)
    return srcs, src_off, np.concatenate(pos).astype(np.int32), dinv


# ------------------------------------------------------------------------------------------------------------ dropout
def dropout_mask(N, width, p, seed, offset):
    """bool [N, width]: element (r, c) is kept iff uniform r * width + c of the Philox stream (seed, offset) is >= fp32(p)."""
    return pm.philox_uniform(seed, offset, N * width).reshape(N, width) >= F32(p)


def dropout_scale(p):
    """fp32 1 / (1 - p) as the kernels form it (0 at p = 1: everything is dropped)."""
    return F32(1) / (F32(1) - F32(p)) if p < 1.0 else F32(0)


# --------------------------------------------------------------------------------------------------------------- loss
def loss_problem(kind, M, C, multi, seed, cols=None):
    """One row-list loss over N_LOSS nodes: z fp32 [M, cols] (cols = ceil4(C) by default; columns C.. hold NaN, which a kernel that
    reads them carries into its loss), rows int32 [M] ascending, labels (int64 [N] or fp32 [N, C]), dinv fp32 [N] > 0.  kind:
      normal        N(0, 1);
      wide          N(0, 8^2): the softmax saturates;
      shifted       N(0, 1) plus a common offset per row drawn from {-1000, +1000};
      bce-extreme   every entry -90 or +90 (BCE only)."""
    if kind not in LOSS_KINDS or (kind == "bce-extreme" and not multi):
        raise ValueError(kind)
    rng = np.random.default_rng(seed)
    N = N_LOSS
    cols = (C + 3) // 4 * 4 if cols is None else cols
    rows = np.sort(rng.choice(N, M, replace=False)).astype(np.int32)
    z = np.full((M, cols), np.nan)
    v = rng.standard_normal((M, C))
    if kind == "wide":
        v *= 8.0
    elif kind == "shifted":
        v += rng.choice([-1000.0, 1000.0], M)[:, None]
    elif kind == "bce-extreme":
        v = rng.choice([-90.0, 90.0], (M, C))
    z[:, :C] = v
    labels = (rng.random((N, C)) < 0.3).astype(F32) if multi else rng.integers(0, C, N).astype(np.int64)
    dinv = (rng.random(N) * 2 + 0.05).astype(F32)
    return np.ascontiguousarray(z, dtype=F32), rows, labels, dinv


def _dropped(z, C, rows, p, mask, dtype):
    """(zd, keep [M, C], sc): the dropped logits where(keep, z * sc, 0) with the fp32 scale taken as given (as dinv is)."""
    z = np.asarray(z)[:, :C]
    keep = np.ones(z.shape, bool) if mask is None or p == 0 else np.asarray(mask, bool)[np.asarray(rows, np.int64)]
    sc = dropout_scale(p) if p > 0 else F32(1)
    zd = np.where(keep, z.astype(dtype) * dtype(sc), dtype(0)).astype(dtype)
    return zd, keep, sc


def rowlist_loss_ref(z, C, rows, labels, dinv, p=0.0, mask=None):
    """fp64 {"loss", "g" [M, C], "dcol" [C], "loss_mag", "g_mag", "dcol_mag"} of grapes_rowlist_loss: Zd = where(mask[rows], z / (1 - p), 0),
    loss = mean CrossEntropy (labels 1-D) or mean BCEWithLogits (labels [N, C]) over the M rows, dZ = d loss / d z,
    g = dinv[rows] ⊙ dZ, dcol = column sums of dZ.  mask: the keep mask of the whole N x C logits (dropout_mask), None = keep all.
    Magnitudes: of the CE gradient dinv sc inv (p + onehot); of a CE row loss |z_y - m| + |log se| (the shift-invariant terms); of
    the BCE terms max(z, 0) + |z y| + log1p(exp(-|z|)) and dinv sc inv (sigmoid + |y|); of dcol sum |dZ|."""
    rows = np.asarray(rows, np.int64)
    zd, keep, sc = _dropped(z, C, rows, p, mask, np.float64)
    M = zd.shape[0]
    d = np.asarray(dinv, np.float64)[rows][:, None]
    scale = float(sc) * keep
    labels = np.asarray(labels)
    if labels.ndim == 1:
        y = labels[rows].astype(np.int64)
        inv = 1.0 / M
        m = zd.max(1, keepdims=True)
        se = np.exp(zd - m).sum(1, keepdims=True)
        lsm = (zd - m) - np.log(se)
        prob = np.exp(lsm)
        one = np.zeros_like(prob)
        one[np.arange(M), y] = 1.0
        rl = -lsm[np.arange(M), y]
        rl_mag = np.abs((zd - m)[np.arange(M), y]) + np.abs(np.log(se))[:, 0]
        dz = (prob - one) * inv * scale
        dz_mag = (prob + one) * inv * scale
        loss, loss_mag = rl.sum() * inv, rl_mag.sum() * inv
    else:
        y = labels[rows].astype(np.float64)
        inv = 1.0 / (M * C)
        soft = np.log1p(np.exp(-np.abs(zd)))
        el = np.maximum(zd, 0) - zd * y + soft
        el_mag = np.maximum(zd, 0) + np.abs(zd * y) + soft
        with np.errstate(over="ignore"):                                   # exp(1000) = inf: sigmoid = 0, as it should be
            sig = 1.0 / (1.0 + np.exp(-zd))
        dz = (sig - y) * inv * scale
        dz_mag = (sig + np.abs(y)) * inv * scale
        loss, loss_mag = el.sum() * inv, el_mag.sum() * inv
    return {"loss": float(loss), "loss_mag": float(loss_mag), "g": d * dz, "g_mag": d * dz_mag,
            "dcol": dz.sum(0), "dcol_mag": np.abs(dz).sum(0), "keep": keep}


def _torch_loss(zd, labels_rows, multi):
    zt = torch.tensor(zd, requires_grad=True)
    if multi:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(zt, torch.as_tensor(labels_rows).to(zt.dtype))
    else:
        loss = torch.nn.functional.cross_entropy(zt, torch.as_tensor(labels_rows, dtype=torch.int64))
    loss.backward()
    return loss.detach().numpy(), zt.grad.numpy()


def rowlist_loss_base(z, C, rows, labels, dinv, p=0.0, mask=None):
    """The host fp32 baseline {"loss", "g", "dcol"}: torch's cross_entropy / binary_cross_entropy_with_logits on the dropped logits
    (fp32: fl(z sc) where kept) with fp32 autograd on the CPU, dZ = fl(grad sc) where kept, g = fl(dinv dZ), dcol the rows of dZ added
    one after the other in fp32."""
    rows = np.asarray(rows, np.int64)
    zd, keep, sc = _dropped(z, C, rows, p, mask, np.float32)
    labels = np.asarray(labels)
    loss, grad = _torch_loss(np.ascontiguousarray(zd, F32), labels[rows], labels.ndim == 2)
    dz = np.where(keep, grad.astype(F32) * F32(sc), F32(0)).astype(F32)
    g = (np.asarray(dinv, F32)[rows][:, None] * dz).astype(F32)
    return {"loss": float(loss), "g": g, "dcol": acc._seq_sum_f32(np.ascontiguousarray(dz))}


def torch_loss_fp64(z, C, rows, labels, dinv, p=0.0, mask=None):
    """(loss, g, dcol) by torch autograd in fp64 THROUGH the masked scaling (the check of rowlist_loss_ref itself)."""
    rows = np.asarray(rows, np.int64)
    _, keep, sc = _dropped(z, C, rows, p, mask, np.float64)
    zt = torch.tensor(np.asarray(z)[:, :C].astype(np.float64), requires_grad=True)
    zd = torch.where(torch.as_tensor(keep), zt * float(sc), torch.zeros_like(zt))
    labels = np.asarray(labels)
    if labels.ndim == 2:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(zd, torch.as_tensor(labels[rows].astype(np.float64)))
    else:
        loss = torch.nn.functional.cross_entropy(zd, torch.as_tensor(labels[rows], dtype=torch.int64))
    loss.backward()
    dz = zt.grad.numpy()
    return float(loss.detach()), np.asarray(dinv, np.float64)[rows][:, None] * dz, dz.sum(0)


def ce_rows_f32(zd, y, order):
    """The gradient rows (softmax - onehot) / M and the row losses of a cross-entropy written in fp32 numpy in one of two orders:
      "shift_first"   lsm = (x - m) - log(se), p = exp(lsm), loss = -lsm[y]
      "add_back"      lse = m + log(se), p = exp(x - lse), loss = lse - x[y]     (the row maximum added back before the subtraction:
                      the result depends on a common offset of the row)
    se is summed column by column in fp32.  For the CPU test of the criterion only."""
    zd = np.ascontiguousarray(zd, F32)
    M, C = zd.shape
    y = np.asarray(y, np.int64)
    m = zd.max(1, keepdims=True)
    se = acc._seq_sum_f32(np.ascontiguousarray(np.exp(zd - m, dtype=F32).T))[:, None]
    one = np.zeros((M, C), F32)
    one[np.arange(M), y] = 1
    if order == "shift_first":
        lsm = ((zd - m) - np.log(se, dtype=F32)).astype(F32)
        prob = np.exp(lsm, dtype=F32)
        rl = -lsm[np.arange(M), y]
    elif order == "add_back":
        lse = (m + np.log(se, dtype=F32)).astype(F32)
        prob = np.exp((zd - lse).astype(F32), dtype=F32)
        rl = (lse[:, 0] - zd[np.arange(M), y]).astype(F32)
    else:
        raise ValueError(order)
    return ((prob - one) * (F32(1) / F32(M))).astype(F32), rl.astype(F32)
