"""fp64 CPU oracle of GATv2Conv / GATv2 (PyG 2.5.2 GATv2Conv, [PyG-recall]; not in the reference tree):

    x_l = x W_lᵀ + b_l     x_r = x W_rᵀ + b_r     viewed as [n, H, C]   (share_weights: W_r = W_l, b_r = b_l)
    edges: stored self-loops dropped, one unit self-loop (i, i) per node, duplicate edges kept (gat_oracle.edge_set)
    z_ij = x_l[j] + x_r[i]     e_ij[h] = Σ_c att[h, c] LeakyReLU(z_ij[h, c], slope)     α_ij[h] = softmax over the incoming edges of i
    agg_i[h] = Σ_j α_ij[h] x_l[j, h]     out_i = concat_h agg_i[h] + b   or   mean_h agg_i[h] + b

Test infrastructure (like tests/gat_oracle.py): the sparse form, its analytic gradients — the formulas the kernels implement —
and a dense closed form (mask A_noloop + I with multiplicities, row softmax per head) to check the sparse form against.
Everything is torch-CPU float64 and differentiable, so torch.autograd can check the analytic gradients."""
import numpy as np
import torch

from tests.gat_oracle import F64, _f64, edge_set, random_graph, rel_err  # noqa: F401  (random_graph, rel_err: for the tests)

SLOPE = 0.2


def _leaky(z, slope):
    return torch.where(z > 0, z, slope * z)


def gatv2_conv(x, W_l, b_l, W_r, b_r, att, b, edge_index, heads, concat=True, slope=SLOPE, relu=False, full=False):
    """out [n, H C] (concat) or [n, C]; differentiable in every fp64 tensor argument.  W_r = b_r = None: shared weights.
    b may be None.  full=True: also the intermediates."""
    n = x.shape[0]
    H = heads
    src, dst = edge_set(edge_index, n)
    x_l = (x @ W_l.t() + b_l).reshape(n, H, -1)
    x_r = x_l if W_r is None else (x @ W_r.t() + b_r).reshape(n, H, -1)
    a = att.reshape(H, -1)
    z = x_l[src] + x_r[dst]                                              # [e, H, C]
    e = (a.unsqueeze(0) * _leaky(z, slope)).sum(-1)                      # [e, H]
    m = torch.full((n, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, dst.unsqueeze(1).expand(-1, H), e.detach(), "amax",
                                                                        include_self=True)
    p = torch.exp(e - m[dst])
    denom = torch.zeros((n, H), dtype=e.dtype).index_add(0, dst, p)
    alpha = p / denom[dst]
    agg = torch.zeros_like(x_l).index_add(0, dst, alpha.unsqueeze(-1) * x_l[src])     # [n, H, C]
    pre = agg.reshape(n, -1) if concat else agg.mean(1)
    if b is not None:
        pre = pre + b
    out = torch.relu(pre) if relu else pre
    if full:
        return dict(out=out, pre=pre, agg=agg, x_l=x_l, x_r=x_r, z=z, e=e, alpha=alpha, src=src, dst=dst)
    return out


def gatv2_conv_grads(x, W_l, b_l, W_r, b_r, att, b, edge_index, G, heads, concat=True, slope=SLOPE, relu=False):
    """The analytic backward the kernels implement: dict(dX, dW_l, db_l, dW_r, db_r, datt, db, dx_l, dx_r) for d loss / d out = G
    (shared weights: dW_l, db_l hold the sum of both contributions and dW_r, db_r are None)."""
    with torch.no_grad():
        r = gatv2_conv(x, W_l, b_l, W_r, b_r, att, b, edge_index, heads, concat, slope, relu, full=True)
        x_l, agg, z, alpha, src, dst = r["x_l"], r["agg"], r["z"], r["alpha"], r["src"], r["dst"]
        n, H = x.shape[0], heads
        a = att.reshape(H, -1)
        G = G * (r["out"] > 0) if relu else G
        Gh = G.reshape(n, H, -1) if concat else (G / H).unsqueeze(1).expand(-1, H, -1)          # each head receives G / H
        c = (Gh * agg).sum(-1)                                                                  # [n, H]
        de = alpha * ((Gh[dst] * x_l[src]).sum(-1) - c[dst])                                    # [e, H]
        dz = de.unsqueeze(-1) * a.unsqueeze(0) * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
        dx_l = torch.zeros_like(x_l).index_add(0, src, alpha.unsqueeze(-1) * Gh[dst] + dz).reshape(n, -1)
        dx_r = torch.zeros_like(x_l).index_add(0, dst, dz).reshape(n, -1)
        datt = (de.unsqueeze(-1) * _leaky(z, slope)).sum(0)
        out = dict(datt=datt.reshape(att.shape), db=G.sum(0), dx_l=dx_l, dx_r=dx_r)
        if W_r is None:
            d = dx_l + dx_r
            out.update(dX=d @ W_l, dW_l=d.t() @ x, db_l=d.sum(0), dW_r=None, db_r=None)
        else:
            out.update(dX=dx_l @ W_l + dx_r @ W_r, dW_l=dx_l.t() @ x, db_l=dx_l.sum(0), dW_r=dx_r.t() @ x, db_r=dx_r.sum(0))
        return out


def gatv2_conv_dense(x, W_l, b_l, W_r, b_r, att, b, edge_index, heads, concat=True, slope=SLOPE, relu=False):
    """Closed form: count matrix M[i, j] = multiplicity of j -> i (no self-loops) + I, α[h] = M ⊙ exp(e[h]) row-normalised."""
    n, H = x.shape[0], heads
    ei = torch.as_tensor(np.asarray(edge_index)).long().reshape(2, -1)
    M = torch.zeros((n, n), dtype=F64)
    for j, i in zip(ei[0].tolist(), ei[1].tolist()):
        if i != j:
            M[i, j] += 1.0
    M += torch.eye(n, dtype=F64)
    x_l = (x @ W_l.t() + b_l).reshape(n, H, -1)
    x_r = x_l if W_r is None else (x @ W_r.t() + b_r).reshape(n, H, -1)
    a = att.reshape(H, -1)
    heads_out = []
    for h in range(H):
        z = x_r[:, h].unsqueeze(1) + x_l[:, h].unsqueeze(0)                                     # [i, j, C]
        e = (_leaky(z, slope) * a[h]).sum(-1).masked_fill(M == 0, -float("inf"))
        w = M * torch.exp(e - e.max(dim=1, keepdim=True).values)
        heads_out.append((w / w.sum(1, keepdim=True)) @ x_l[:, h])
    out = torch.cat(heads_out, 1) if concat else torch.stack(heads_out, 0).mean(0)
    if b is not None:
        out = out + b
    return torch.relu(out) if relu else out


def layer_params(conv):
    """fp64 CPU copies (W_l, b_l, W_r, b_r, att, b) of a grapes_amd GATv2Conv's parameters (W_r = b_r = None: shared weights)."""
    shared = conv.share_weights
    return (_f64(conv.lin_l.weight), _f64(conv.lin_l.bias), None if shared else _f64(conv.lin_r.weight),
            None if shared else _f64(conv.lin_r.bias), _f64(conv.att), None if conv.bias is None else _f64(conv.bias))


def gatv2_forward(x, params, edge_index, heads, slope=SLOPE, full=False):
    """GATv2.forward over a list of per-layer parameter tuples, with GAT's routing (gat_oracle.gat_forward): layer i (1-based, all
    but the last) concatenates its heads, uses edge_index[-i] when a list is given and is followed by ReLU; the last layer averages
    its heads over edge_index[0].  full=True: (logits, the hidden layers' intermediates)."""
    layerwise = isinstance(edge_index, list)
    hidden = []
    for i, p in enumerate(params[:-1], start=1):
        r = gatv2_conv(x, *p, edge_index[-i] if layerwise else edge_index, heads, True, slope, relu=True, full=True)
        hidden.append(r)
        x = r["out"]
    last = gatv2_conv(x, *params[-1], edge_index[0] if layerwise else edge_index, heads, False, slope, full=True)
    return (last["out"], hidden, last) if full else last["out"]


def quantised_layer(n, fi, heads, c, seed, share=False):
    """(x [n, fi], (W_l, b_l, W_r, b_r)) in float32 with NO z = x_l[j] + x_r[i] on LeakyReLU's kink, by construction: x and the
    weights are multiples of 1/8 (|x| <= 3), b_l a multiple of 1/64 and b_r a multiple of 1/64 plus 1/128 (shared weights: the one
    bias an odd multiple of 1/256, which z holds twice), so every z is an odd multiple of 1/128 — exact in fp32, |z| >= 1/128."""
    g = torch.Generator().manual_seed(seed)
    f = heads * c
    x = (torch.randn(n, fi, generator=g) * 8).round().clamp(-24, 24) / 8
    W_l = torch.randint(-4, 5, (f, fi), generator=g).float() / 8
    W_r = torch.randint(-4, 5, (f, fi), generator=g).float() / 8
    b_l = torch.randint(-32, 33, (f,), generator=g).float() / 64
    b_r = torch.randint(-32, 33, (f,), generator=g).float() / 64 + 1.0 / 128
    if share:
        return x, (W_l, (2 * torch.randint(-64, 64, (f,), generator=g).float() + 1) / 256, None, None)
    return x, (W_l, b_l, W_r, b_r)
