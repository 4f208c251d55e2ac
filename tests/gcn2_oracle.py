"""fp64 CPU oracle of GCN2Conv / GCN2 (reference modules/gcn.py:76-117; PyG 2.5.2 GCN2Conv(channels, alpha, theta, layer,
shared_weights, normalize=False) and Linear, [PyG-recall]):

    P_i = Σ over the stored edges (j → i) of x_j      every occurrence counts: duplicates by multiplicity, a stored (i, i) like any
                                                      edge, no loop is added, an isolated row gives 0
    S = (1 − α) P + α x_0          β = log(θ / layer + 1)   (1 when θ and layer are None)
    shared weights:  out = (1 − β) S + β S W1
    otherwise:       out = (1 − β)(1 − α) P + β (1 − α) P W1 + (1 − β) α x_0 + β α x_0 W2

Test infrastructure (like tests/gat_oracle.py): the edge-list form, a dense closed form (A[i, j] = multiplicity of j → i, loops
included), the analytic gradients the kernels implement, the model, and the inputs of the GPU tests (so that the CPU suite can
show an fp32 evaluation of the same formulas to be inside the tolerances before a GPU sees them).  Everything is torch-CPU and
differentiable; fp64 unless a test passes fp32 tensors on purpose."""
import math

import numpy as np
import torch

from tests.gat_oracle import random_graph, rel_err          # noqa: F401  (the GPU tests' graph generator and error measure)

F64 = torch.float64
KINK = 1e-5


def f64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)).to(F64)


def beta_of(theta, layer):
    return 1.0 if (theta is None or layer is None) else math.log(theta / layer + 1)


def edges(edge_index):
    ei = torch.as_tensor(np.asarray(edge_index.cpu() if torch.is_tensor(edge_index) else edge_index)).long().reshape(2, -1)
    return ei[0], ei[1]


def propagate(x, edge_index):
    """P = A x from the edge list: every stored edge once per occurrence."""
    src, dst = edges(edge_index)
    return torch.zeros_like(x).index_add(0, dst, x[src])


def gcn2_conv(x, x0, W1, W2, edge_index, alpha, beta, relu=False, full=False):
    """out [n, C] (differentiable in x, x0, W1, W2); W2 None = shared weights.  full=True: also the intermediates."""
    P = propagate(x, edge_index)
    S = (1 - alpha) * P + alpha * x0
    if W2 is None:
        pre = (1 - beta) * S + beta * (S @ W1)
    else:
        pre = ((1 - beta) * (1 - alpha)) * P + (beta * (1 - alpha)) * (P @ W1) + ((1 - beta) * alpha) * x0 + (beta * alpha) * (x0 @ W2)
    out = torch.relu(pre) if relu else pre
    return dict(out=out, pre=pre, P=P, S=S) if full else out


def dense_adjacency(edge_index, n):
    A = torch.zeros((n, n), dtype=F64)
    src, dst = edges(edge_index)
    for j, i in zip(src.tolist(), dst.tolist()):
        A[i, j] += 1.0
    return A


def gcn2_conv_dense(x, x0, W1, W2, edge_index, alpha, beta, relu=False):
    """Closed form with the dense count matrix A[i, j] = multiplicity of j → i (loops included, nothing added)."""
    P = dense_adjacency(edge_index, x.shape[0]) @ x
    eye = torch.eye(x.shape[1], dtype=x.dtype)
    if W2 is None:
        out = ((1 - alpha) * P + alpha * x0) @ ((1 - beta) * eye + beta * W1)
    else:
        out = (1 - alpha) * P @ ((1 - beta) * eye + beta * W1) + alpha * x0 @ ((1 - beta) * eye + beta * W2)
    return torch.relu(out) if relu else out


def gcn2_conv_grads(x, x0, W1, W2, edge_index, alpha, beta, G, relu=False):
    """The analytic backward the kernels implement: dict(dx, dx0, dW1, dW2) for d loss / d out = G."""
    with torch.no_grad():
        r = gcn2_conv(x, x0, W1, W2, edge_index, alpha, beta, relu, full=True)
        src, dst = edges(edge_index)
        G = G * (r["pre"] > 0) if relu else G
        if W2 is None:
            dS = (1 - beta) * G + beta * (G @ W1.t())
            dP, dx0 = (1 - alpha) * dS, alpha * dS
            dW1, dW2 = beta * (r["S"].t() @ G), None
        else:
            dP = (1 - alpha) * ((1 - beta) * G + beta * (G @ W1.t()))
            dx0 = alpha * ((1 - beta) * G + beta * (G @ W2.t()))
            dW1, dW2 = (beta * (1 - alpha)) * (r["P"].t() @ G), (beta * alpha) * (x0.t() @ G)
        dx = torch.zeros_like(x).index_add(0, src, dP[dst])           # Aᵀ dP
        return dict(dx=dx, dx0=dx0, dW1=dW1, dW2=dW2)


def model_params(model, dtype=F64):
    """CPU copies of a grapes_amd GCN2's parameters: dict(lin0=(W, b), lin1=(W, b), convs=[(W1, W2 or None), ...], betas=[...])."""
    cp = lambda t: None if t is None else torch.as_tensor(np.asarray(t.detach().cpu())).to(dtype)
    return dict(lin0=(cp(model.lins[0].weight), cp(model.lins[0].bias)), lin1=(cp(model.lins[1].weight), cp(model.lins[1].bias)),
                convs=[(cp(c.weight1), cp(c.weight2)) for c in model.conv], betas=[c.beta for c in model.conv],
                alpha=model.conv[0].alpha)


def param_leaves(params):
    """The parameters as autograd leaves, in state_dict order (lins.0.weight, lins.0.bias, lins.1.weight, lins.1.bias, then per conv
    weight1 [, weight2]); returns (params with the leaves in place, the flat list)."""
    leaf = lambda t: t.clone().requires_grad_(True)
    l0, l1 = tuple(leaf(t) for t in params["lin0"]), tuple(leaf(t) for t in params["lin1"])
    convs = [(leaf(w1), None if w2 is None else leaf(w2)) for w1, w2 in params["convs"]]
    flat = list(l0) + list(l1) + [t for c in convs for t in c if t is not None]
    return dict(params, lin0=l0, lin1=l1, convs=convs), flat


def gcn2_forward(x, params, edge_index, masks=None, full=False):
    """modules/gcn.py:97-117.  masks: None, or the L + 1 dropout masks (already scaled by 1 / (1 − p)) in the order the model
    draws them: the input, then one in front of every conv.  full=True: (logits, [hidden pre-activations: lins[0], convs[:-1]])."""
    layerwise = isinstance(edge_index, list)
    alpha = params["alpha"]
    drop = iter(masks) if masks is not None else None
    dr = (lambda t: t * next(drop)) if drop is not None else (lambda t: t)
    pres = []
    h = dr(x) @ params["lin0"][0].t() + params["lin0"][1]
    pres.append(h)
    x = x0 = torch.relu(h)
    L = len(params["convs"])
    for i in range(1, L):
        e = edge_index[-i] if layerwise else edge_index
        r = gcn2_conv(dr(x), x0, *params["convs"][i - 1], e, alpha, params["betas"][i - 1], relu=True, full=True)
        pres.append(r["pre"])
        x = r["out"]
    e = edge_index[0] if layerwise else edge_index
    x = gcn2_conv(dr(x), x0, *params["convs"][L - 1], e, alpha, params["betas"][L - 1])
    logits = x @ params["lin1"][0].t() + params["lin1"][1]
    return (logits, pres) if full else logits


# ------------------------------------------------------------------------------------------- the GPU tests' inputs
N = 3000
HUB, HUB_DEG = 17, 2100
# (width, shared weights, ReLU, alpha): the float4 form (256, 128, 100, 64), the scalar form (47, 30), more than one column slab
# per lane (320: float4, 4 slabs; 330: scalar, 16 slabs), both weight forms, ReLU on / off and alpha in {0, 0.1, 0.5}.  (alpha = 0
# goes with ReLU off: rows without an incoming edge are then exactly 0, about 1 % of the pre-activations on their own.)
CONV_CASES = [
    (256, True, True, 0.1), (256, False, False, 0.5), (128, True, False, 0.5), (128, False, True, 0.1), (100, True, False, 0.0),
    (100, False, True, 0.1), (64, True, True, 0.1), (64, False, False, 0.0), (47, True, True, 0.5), (47, False, False, 0.0),
    (30, True, False, 0.0), (30, False, True, 0.5), (320, True, True, 0.1), (320, False, False, 0.1), (330, True, True, 0.5),
]
THETA = 0.5


def gpu_graph(seed, n=N):
    return random_graph(n, seed=seed, mean_deg=6, hub=HUB, hub_deg=HUB_DEG, n_dup=60, n_loops=40, n_isolated=25, directed_block=30)


def graph_properties(ei, n=N):
    """(hub in-degree, duplicated edge occurrences, stored loops, isolated rows) of an edge list."""
    src, dst = np.asarray(ei[0]), np.asarray(ei[1])
    key = src.astype(np.int64) * n + dst
    _, cnt = np.unique(key, return_counts=True)
    touched = np.zeros(n, bool); touched[src] = True; touched[dst] = True
    return int((dst == HUB).sum()), int((cnt - 1).sum()), int((src == dst).sum()), int((~touched).sum())


def conv_case(c, shared, seed, layer=2):
    """fp32 inputs of one single-conv GPU test: (edge list, x, x0, W1, W2 or None, G, beta).  x plays a hidden activation (ReLU of a
    normal), x0 the first layer's output; W1 / W2 are glorot draws as GCN2Conv.reset_parameters makes them."""
    ei = gpu_graph(seed)
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.relu(torch.randn(N, c, generator=g))
    x0 = torch.relu(torch.randn(N, c, generator=g))
    a = math.sqrt(6.0 / (2 * c))
    W1 = (torch.rand(c, c, generator=g) * 2 - 1) * a
    W2 = None if shared else (torch.rand(c, c, generator=g) * 2 - 1) * a
    G = torch.randn(N, c, generator=g)
    return ei, x, x0, W1, W2, G, beta_of(THETA, layer)


def kink_free_gradient(G, pre):
    """(G with the entries whose oracle pre-activation lies within KINK of zero set to 0, the number of such entries): no upstream
    gradient rides on a ReLU gate that fp32 rounding could flip."""
    near = pre.detach().abs() < KINK
    return torch.where(near, torch.zeros_like(G), G), int(near.sum())
