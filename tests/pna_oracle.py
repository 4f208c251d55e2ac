"""fp64 CPU oracle of PNAConv / PNA (reference modules/gcn.py:120-149; PyG 2.5.2 PNAConv(in_channels, out_channels, aggregators,
scalers, deg) with every other argument at its default, [PyG-recall]):

    m_ij = pre_nn([x_i | x_j])  for every stored edge (j → i): every occurrence counts, a stored (i, i) like any edge, no loop added
    per row i with in-degree d_i, per feature:  mean = Σ m / max(d, 1);  min, max (0 when d = 0);
        var = relu(mean(m²) − mean(m)²);  std = sqrt(var + 1e-5);  sum = Σ m
    scalers: identity 1, amplification log(d + 1) / avg_log, attenuation avg_log / log(max(d, 1) + 1), linear d / avg_lin,
        inverse_linear avg_lin / max(d, 1);   avg_log, avg_lin from the in-degree histogram `deg`
    out = lin(post_nn([x_i | scaler_1(aggs) | scaler_2(aggs) | ...]))

Test infrastructure (like tests/gcn2_oracle.py): the literal per-edge form, a dense closed form for hand-sized graphs, the analytic
gradients the kernels implement, an fp32 evaluation of the kernels' formulas (centred or uncentred variance), the model, the inputs
of the GPU tests and the kink mask.  Everything is torch-CPU; fp64 unless a function says fp32."""
import math

import numpy as np
import torch

from tests.gat_oracle import random_graph, rel_err          # noqa: F401  (the GPU tests' graph generator and error measure)
from tests.gcn2_oracle import edges, f64, graph_properties, gpu_graph, HUB, N          # noqa: F401

F64 = torch.float64
KINK = 1e-5
STD_EPS = 1e-5
AGGREGATORS = ["mean", "min", "max", "std"]
SCALERS = ["identity", "amplification", "attenuation"]


def degree_histogram(edge_index, n):
    """deg[d] = number of nodes of in-degree d (int64)."""
    _, dst = edges(edge_index)
    return torch.bincount(torch.bincount(dst, minlength=n))


def degree_averages(deg):
    deg = torch.as_tensor(deg).to(F64)
    bins = torch.arange(deg.numel(), dtype=F64)
    return float(((bins + 1).log() * deg).sum() / deg.sum()), float((bins * deg).sum() / deg.sum())


def scaler_values(d, scalers, avg_log, avg_lin):
    """[n, |scalers|] (the dtype of d)."""
    d1 = d.clamp(min=1)
    table = {"identity": torch.ones_like(d), "amplification": (d + 1).log() / avg_log, "attenuation": avg_log / (d1 + 1).log(),
             "linear": d / avg_lin, "inverse_linear": avg_lin / d1}
    return torch.stack([table[s] for s in scalers], 1)


def _reduce(m, dst, n, how):
    idx = dst[:, None].expand_as(m)
    return torch.zeros((n, m.shape[1]), dtype=m.dtype).scatter_reduce(0, idx, m, how, include_self=False)


def aggregate(m, dst, n, aggregators):
    """dict name -> [n, F] of the messages m [e, F] by target; rows without a message give 0, 0, 0, sqrt(eps)."""
    d = torch.bincount(dst, minlength=n).to(m.dtype)
    d1 = d.clamp(min=1)[:, None]
    total = torch.zeros((n, m.shape[1]), dtype=m.dtype).index_add(0, dst, m)
    mean = total / d1
    var = torch.relu(torch.zeros_like(total).index_add(0, dst, m * m) / d1 - mean * mean)         # PyG's literal form
    out = {"sum": total, "mean": mean, "var": var, "std": (var + STD_EPS).sqrt()}
    if "min" in aggregators:
        out["min"] = _reduce(m, dst, n, "amin")
    if "max" in aggregators:
        out["max"] = _reduce(m, dst, n, "amax")
    return out, d


def messages(x, Wpre, bpre, edge_index):
    src, dst = edges(edge_index)
    return torch.cat([x[dst], x[src]], 1) @ Wpre.t() + bpre, src, dst


def pna_conv(x, P, edge_index, aggregators, scalers, avg_log, avg_lin, relu=False, full=False):
    """out [n, C], differentiable in x and the six parameters P = (Wpre, bpre, Wpost, bpost, Wlin, blin): the literal per-edge
    form (cat, Linear, index-reduce, scalers, post_nn, lin).  full=True: also the intermediates."""
    Wpre, bpre, Wpost, bpost, Wlin, blin = P
    n = x.shape[0]
    m, src, dst = messages(x, Wpre, bpre, edge_index)
    agg, d = aggregate(m, dst, n, aggregators)
    sc = scaler_values(d, scalers, avg_log, avg_lin)
    A = torch.cat([agg[a] for a in aggregators], 1)
    z = torch.cat([x] + [A * sc[:, k:k + 1] for k in range(len(scalers))], 1)
    pre = (z @ Wpost.t() + bpost) @ Wlin.t() + blin
    out = torch.relu(pre) if relu else pre
    return dict(out=out, pre=pre, z=z, m=m, agg=agg, d=d, src=src, dst=dst) if full else out


def pna_aggregate_ab(x, a, b, edge_index, aggregators, scalers, avg_log, avg_lin):
    """The aggregation alone from given a, b (messages a_i + b_j formed in the dtype of a): dict(z, agg, d, m, src, dst),
    differentiable in a and b — the oracle of the aggregation entry point."""
    src, dst = edges(edge_index)
    n = x.shape[0]
    m = a[dst] + b[src]
    agg, d = aggregate(m, dst, n, aggregators)
    sc = scaler_values(d, scalers, avg_log, avg_lin)
    A = torch.cat([agg[k] for k in aggregators], 1)
    z = torch.cat([x] + [A * sc[:, k:k + 1] for k in range(len(scalers))], 1)
    return dict(z=z, agg=agg, d=d, m=m, src=src, dst=dst)


def pna_conv_decomposed(x, P, edge_index, aggregators, scalers, avg_log, avg_lin, centred=True, fma=False):
    """The kernels' form in the dtype of x: a = x W_iᵀ + bias, b = x W_jᵀ, mean / min / max = a_i + the statistic of b_j; the
    variance CENTRED (Σ (b_j − mean_i)² / d: what Welford / Chan compute) or, centred=False, from raw moments of b — with fma=True
    the subtraction E[b²] − E[b]·E[b] keeps the product exact, which is what a compiler contracting it into one fused multiply-add
    computes.  Returns z (post_nn's operand) and the unscaled dict."""
    Wpre, bpre = P[0], P[1]
    n, F = x.shape
    src, dst = edges(edge_index)
    a, b = x @ Wpre[:, :F].t() + bpre, x @ Wpre[:, F:].t()
    bj = b[src]
    d = torch.bincount(dst, minlength=n).to(x.dtype)
    d1, has = d.clamp(min=1)[:, None], (d > 0)[:, None].to(x.dtype)
    mean_b = torch.zeros_like(b).index_add(0, dst, bj) / d1
    if centred:
        var = torch.zeros_like(b).index_add(0, dst, (bj - mean_b[dst]) ** 2) / d1
    else:
        msq = torch.zeros_like(b).index_add(0, dst, bj * bj) / d1
        if fma:
            var = torch.relu((msq.double() - mean_b.double() * mean_b.double()).to(x.dtype))
        else:
            var = torch.relu(msq - mean_b * mean_b)
    agg = {"mean": (a + mean_b) * has, "var": var, "std": (var + STD_EPS).sqrt()}
    agg["sum"] = agg["mean"] * d[:, None]
    agg["min"] = (a + _reduce(bj, dst, n, "amin")) * has
    agg["max"] = (a + _reduce(bj, dst, n, "amax")) * has
    sc = scaler_values(d, scalers, avg_log, avg_lin)
    A = torch.cat([agg[k] for k in aggregators], 1)
    return torch.cat([x] + [A * sc[:, k:k + 1] for k in range(len(scalers))], 1), agg


def pna_conv_dense(x, P, edge_index, aggregators, scalers, avg_log, avg_lin, relu=False):
    """Closed form for hand-sized graphs from the dense count matrix A[i, j] = multiplicity of j → i: row i's messages are listed one
    by one as a_i + b_j and reduced with plain tensor methods."""
    Wpre, bpre, Wpost, bpost, Wlin, blin = P
    n, F = x.shape
    A = torch.zeros((n, n), dtype=torch.long)
    src, dst = edges(edge_index)
    for j, i in zip(src.tolist(), dst.tolist()):
        A[i, j] += 1
    a, b = x @ Wpre[:, :F].t() + bpre, x @ Wpre[:, F:].t()
    rows = []
    for i in range(n):
        ms = [a[i] + b[j] for j in range(n) for _ in range(int(A[i, j]))]
        d = len(ms)
        if d:
            M = torch.stack(ms)
            var = torch.relu((M * M).mean(0) - M.mean(0) ** 2)
            st = {"mean": M.mean(0), "min": M.min(0).values, "max": M.max(0).values, "var": var, "std": (var + STD_EPS).sqrt(),
                  "sum": M.sum(0)}
        else:
            zero = torch.zeros(F, dtype=x.dtype)
            st = {"mean": zero, "min": zero, "max": zero, "var": zero, "std": zero + math.sqrt(STD_EPS), "sum": zero}
        sv = {"identity": 1.0, "amplification": math.log(d + 1) / avg_log, "attenuation": avg_log / math.log(max(d, 1) + 1),
              "linear": d / avg_lin, "inverse_linear": avg_lin / max(d, 1)}
        rows.append(torch.cat([x[i]] + [st[k] * sv[s] for s in scalers for k in aggregators]))
    out = (torch.stack(rows) @ Wpost.t() + bpost) @ Wlin.t() + blin
    return torch.relu(out) if relu else out


def pna_conv_grads(x, P, edge_index, aggregators, scalers, avg_log, avg_lin, G, relu=False):
    """The analytic backward the kernels implement: dict(dx, dWpre, dbpre, dWpost, dbpost, dWlin, dblin) for d loss / d out = G.
    Bit-equal extremes of a row share its gradient evenly."""
    with torch.no_grad():
        Wpre, bpre, Wpost, bpost, Wlin, blin = P
        n, F = x.shape
        r = pna_conv(x, P, edge_index, aggregators, scalers, avg_log, avg_lin, relu, full=True)
        src, dst, d, m, agg = r["src"], r["dst"], r["d"], r["m"], r["agg"]
        G = G * (r["pre"] > 0) if relu else G
        h = r["z"] @ Wpost.t() + bpost
        dWlin, dblin = G.t() @ h, G.sum(0)
        dh = G @ Wlin
        dWpost, dbpost = dh.t() @ r["z"], dh.sum(0)
        dz = dh @ Wpost
        sc = scaler_values(d, scalers, avg_log, avg_lin)
        K = len(aggregators)
        g = {k: torch.zeros((n, F), dtype=x.dtype) for k in ("mean", "min", "max", "var")}
        for s in range(len(scalers)):
            for k, name in enumerate(aggregators):
                blk = dz[:, (1 + s * K + k) * F:(2 + s * K + k) * F] * sc[:, s:s + 1]
                if name == "sum":
                    g["mean"] += blk * d[:, None]
                elif name == "std":
                    g["var"] += blk * 0.5 / agg["std"]
                else:
                    g[name] += blk
        has = (d > 0)[:, None].to(x.dtype)
        g["var"] = g["var"] * (agg["var"] > 0)
        d1 = d.clamp(min=1)[:, None]
        mx = agg["max"] if "max" in agg else _reduce(m, dst, n, "amax")
        mn = agg["min"] if "min" in agg else _reduce(m, dst, n, "amin")
        is_max, is_min = (m == mx[dst]).to(x.dtype), (m == mn[dst]).to(x.dtype)
        t_max = torch.zeros((n, F), dtype=x.dtype).index_add(0, dst, is_max).clamp(min=1)
        t_min = torch.zeros((n, F), dtype=x.dtype).index_add(0, dst, is_min).clamp(min=1)
        dm = ((g["mean"] / d1)[dst] + (2 * g["var"] / d1)[dst] * (m - agg["mean"][dst]) + (g["max"] / t_max)[dst] * is_max +
              (g["min"] / t_min)[dst] * is_min)
        cat = torch.cat([x[dst], x[src]], 1)
        dWpre, dbpre = dm.t() @ cat, dm.sum(0)
        dcat = dm @ Wpre
        dx = dz[:, :F] + torch.zeros_like(x).index_add(0, dst, dcat[:, :F]).index_add(0, src, dcat[:, F:])
        assert bool(((g["mean"] + g["min"] + g["max"]) * (1 - has) == (g["mean"] + g["min"] + g["max"]) * (1 - has)).all())
        return dict(dx=dx, dWpre=dWpre, dbpre=dbpre, dWpost=dWpost, dbpost=dbpost, dWlin=dWlin, dblin=dblin)


GRAD_NAMES = ("dx", "dWpre", "dbpre", "dWpost", "dbpost", "dWlin", "dblin")


# ------------------------------------------------------------------------------------------- kinks
def _second_extreme_gap(m, src, dst, n, largest):
    """[n, F]: the gap between the row's extreme message and the most extreme message of ANOTHER edge — another source node: the
    occurrences of a duplicated edge (j → i) carry the bit-same message a_i + b_j in any arithmetic, so no rounding can reorder
    them (and both the kernels and autograd split their gradient evenly).  inf for rows whose messages all come from one source."""
    how = "amax" if largest else "amin"
    fill = -math.inf if largest else math.inf
    ext = _reduce(m, dst, n, how)
    e = m.shape[0]
    ids = torch.arange(e)[:, None].expand_as(m)
    idx = dst[:, None].expand_as(m)
    hit = m == ext[dst]
    first = torch.full((n, m.shape[1]), e, dtype=torch.long).scatter_reduce(0, idx, torch.where(hit, ids, torch.full_like(ids, e)), "amin")
    src_first = src[first.clamp(max=e - 1)]
    rest = torch.where(src[:, None] == src_first[dst], torch.full_like(m, fill), m)
    second = torch.full((n, m.shape[1]), fill, dtype=m.dtype).scatter_reduce(0, idx, rest, how)
    gap = (ext - second).abs()
    return torch.where(torch.isfinite(second), gap, torch.full_like(gap, math.inf)), ext


def aggregate_kinks(r, n):
    """bool [n, F] per kind on the ORACLE's values (r = pna_conv(..., full=True)): the (row, feature) entries whose two largest /
    two smallest messages come from different edges and differ by less than KINK · max(1, |m|), and those with 0 < var < KINK."""
    gap_hi, hi = _second_extreme_gap(r["m"].detach(), r["src"], r["dst"], n, True)
    gap_lo, lo = _second_extreme_gap(r["m"].detach(), r["src"], r["dst"], n, False)
    var = r["agg"]["var"].detach()
    return dict(max=gap_hi < KINK * hi.abs().clamp(min=1), min=gap_lo < KINK * lo.abs().clamp(min=1), var=(var > 0) & (var < KINK))


def kink_free_gradient(G, r, n, relu):
    """(G', ReLU pre-activations within KINK of zero, kinked aggregate entries, rows cut): no upstream gradient rides on a kink fp32
    rounding could flip, judged on the oracle's values (r = pna_conv(..., full=True)).  A ReLU entry near zero loses its own
    gradient.  An aggregate entry (row, feature) has no upstream gradient of its own at the layer's output — post_nn mixes the whole
    row — so a row that owns a kinked entry loses its whole row of G: a choice of input.  (The aggregation entry point is tested
    entry by entry, hub row included, in the tests that call it directly.)"""
    near = r["pre"].detach().abs() < KINK if relu else torch.zeros_like(r["pre"], dtype=torch.bool)
    k = aggregate_kinks(r, n)
    bad = k["max"] | k["min"] | k["var"]
    rows = bad.any(1)
    G = torch.where(near, torch.zeros_like(G), G)
    G = torch.where(rows[:, None], torch.zeros_like(G), G)
    return G, int(near.sum()), int(bad.sum()), int(rows.sum())


# ------------------------------------------------------------------------------------------- the model
def model_params(model, dtype=F64):
    """CPU copies of a grapes_amd PNA's conv parameters: [(Wpre, bpre, Wpost, bpost, Wlin, blin), ...] and its configuration."""
    cp = lambda t: torch.as_tensor(np.asarray(t.detach().cpu())).to(dtype)
    convs = [tuple(cp(t) for t in (c.pre_nn.weight, c.pre_nn.bias, c.post_nn.weight, c.post_nn.bias, c.lin.weight, c.lin.bias))
             for c in model.conv]
    c0 = model.conv[0]
    return dict(convs=convs, aggregators=list(c0.aggregators), scalers=list(c0.scalers), avg_log=c0.avg_deg["log"],
                avg_lin=c0.avg_deg["lin"])


def param_leaves(params):
    """The conv parameters as autograd leaves in state_dict order (conv.i.pre_nn.weight, .bias, post_nn, lin)."""
    convs = [tuple(t.clone().requires_grad_(True) for t in c) for c in params["convs"]]
    return dict(params, convs=convs), [t for c in convs for t in c]


def pna_forward(x, params, edge_index, masks=None, drop_input=True, full=False):
    """PNA.forward as grapes_amd builds it.  masks: None, or the dropout masks (scaled by 1 / (1 − p)) in the order the model
    draws them: the input (drop_input), then one behind every hidden conv.  full=True: (logits, [hidden full results])."""
    layerwise = isinstance(edge_index, list)
    drop = iter(masks) if masks is not None else None
    dr = (lambda t: t * next(drop)) if drop is not None else (lambda t: t)
    kw = dict(aggregators=params["aggregators"], scalers=params["scalers"], avg_log=params["avg_log"], avg_lin=params["avg_lin"])
    hidden = []
    if drop_input:
        x = dr(x)
    L = len(params["convs"])
    for i in range(1, L):
        e = edge_index[-i] if layerwise else edge_index
        r = pna_conv(x, params["convs"][i - 1], e, relu=True, full=True, **kw)
        hidden.append(r)
        x = dr(r["out"])
    e = edge_index[0] if layerwise else edge_index
    logits = pna_conv(x, params["convs"][L - 1], e, **kw)
    return (logits, hidden) if full else logits


# ------------------------------------------------------------------------------------------- the GPU tests' inputs
# (input width F, output width C, ReLU): scalar columns (7: one partial tile; 1433: Cora's width, 23 column tiles of a wavefront),
# float4 columns on half a wavefront (100: products) and on a whole one (256: hidden layers); C small for the wide inputs so the
# oracle's post_nn stays cheap.
CONV_CASES = [(7, 16, True), (7, 5, False), (100, 47, True), (100, 32, False), (256, 64, True), (256, 47, False), (1433, 8, False),
              (602, 12, True)]


def linear_init(out_f, in_f, g):
    """PyG Linear's reset as modules.gcn.Linear does it: kaiming-uniform(a = sqrt 5) = U(±1/sqrt(in)), bias U(±1/sqrt(in))."""
    bound = 1.0 / math.sqrt(in_f)
    return (torch.rand(out_f, in_f, generator=g) * 2 - 1) * bound, (torch.rand(out_f, generator=g) * 2 - 1) * bound


def conv_case(F, C, seed, aggregators=AGGREGATORS, scalers=SCALERS):
    """fp32 inputs of one single-conv GPU test: (edge list, x, P, G, avg_log, avg_lin).  x is N(0, 1)."""
    ei = gpu_graph(seed)
    g = torch.Generator().manual_seed(seed + 200)
    x = torch.randn(N, F, generator=g)
    Wpre, bpre = linear_init(F, 2 * F, g)
    Wpost, bpost = linear_init(C, (len(aggregators) * len(scalers) + 1) * F, g)
    Wlin, blin = linear_init(C, C, g)
    G = torch.randn(N, C, generator=g)
    avg_log, avg_lin = degree_averages(degree_histogram(ei, N))
    return ei, x, (Wpre, bpre, Wpost, bpost, Wlin, blin), G, avg_log, avg_lin
