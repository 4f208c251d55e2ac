"""The GCN2 classifier (reference modules/gcn.py:76-117) on the MI355X against the fp64 oracle of tests/gcn2_oracle.py.

Tolerances are the project's: activations max|a − ref| / max(1, max|ref|) <= 1e-5, gradients the same measure at 1e-4; the
single-conv inputs are those tests/test_gcn2_cpu.py shows to be reachable by an fp32 CPU evaluation of the same formulas.
ReLU kinks: every test with a ReLU asserts on the ORACLE's values that at most 1 % of the pre-activations lie within 1e-5 of zero.
The single-conv tests then carry no upstream gradient on those entries (gcn2_oracle.kink_free_gradient: a choice of input);
the two-layer test leaves the hidden units that own one out of the upstream gradient comparison, nothing else."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gcn2_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_TOL, GRAD_TOL = 1e-5, 1e-4
N = O.N


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _conv(c, shared, alpha, W1, W2, layer=2):
    from grapes_amd.modules.gcn import GCN2Conv
    conv = GCN2Conv(c, alpha, O.THETA, layer, shared_weights=shared)
    with torch.no_grad():
        conv.weight1.copy_(W1)
        if not shared:
            conv.weight2.copy_(W2)
    return conv.cuda()


def _run(conv, x, x0, edges, G, relu):
    """One forward and backward on the device: (out, dx, dx0, dW1[, dW2])."""
    xd, x0d = x.detach().clone().requires_grad_(True), x0.detach().clone().requires_grad_(True)
    out = conv(xd, x0d, edges, relu=relu)
    ws = [conv.weight1] + ([conv.weight2] if conv.weight2 is not None else [])
    grads = torch.autograd.grad(out, [xd, x0d] + ws, G)
    return (out.detach(),) + tuple(g.detach() for g in grads)


def _oracle(ei, x, x0, W1, W2, G, alpha, beta, relu):
    d = lambda t: None if t is None else t.double()
    ref = O.gcn2_conv(d(x), d(x0), d(W1), d(W2), ei, alpha, beta, relu=relu, full=True)
    near = 0
    if relu:
        G, near = O.kink_free_gradient(G, ref["pre"])
        assert near <= 0.01 * ref["pre"].numel()                       # the cap, on the oracle's values
    return ref, O.gcn2_conv_grads(d(x), d(x0), d(W1), d(W2), ei, alpha, beta, d(G), relu=relu), G, near


def _compare(got, ref, gr, shared):
    names = ("dx", "dx0", "dW1") + (() if shared else ("dW2",))
    errs = {"out": O.rel_err(got[0].cpu(), ref["out"])}
    for k, t in zip(names, got[1:]):
        errs[k] = O.rel_err(t.cpu(), gr[k])
    print("errors vs fp64 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(torch.isfinite(t).all() for t in got)
    assert errs["out"] <= ACT_TOL, errs
    for k in names:
        assert errs[k] <= GRAD_TOL, errs
    return errs


@pytest.mark.parametrize("case", range(len(O.CONV_CASES)))
def test_gcn2conv_forward_backward_match_oracle(case):
    _need_gpu()
    c, shared, relu, alpha = O.CONV_CASES[case]
    ei, x, x0, W1, W2, G, beta = O.conv_case(c, shared, seed=case + 1)
    hub, dup, loops, isolated = O.graph_properties(ei)
    assert hub > 2000 and dup >= 60 and loops >= 40 and isolated >= 25
    ref, gr, G, near = _oracle(ei, x, x0, W1, W2, G, alpha, beta, relu)
    print(f"width {c} shared {shared} relu {relu} alpha {alpha}: edges {ei.shape[1]}, hub in-degree {hub}, duplicates {dup}, "
          f"stored loops {loops}, isolated {isolated}, pre-activations within 1e-5 of zero {near}")
    conv = _conv(c, shared, alpha, W1, W2)
    assert abs(conv.beta - beta) < 1e-15
    got = _run(conv, x.cuda(), x0.cuda(), torch.from_numpy(ei).cuda(), G.cuda(), relu)
    _compare(got, ref, gr, shared)


def test_loop_counts_match_the_edge_list():
    _need_gpu()
    from grapes_amd import ops
    from grapes_amd.graph import DeviceGraph
    ei = O.gpu_graph(61)
    want = np.bincount(ei[0][ei[0] == ei[1]], minlength=N)
    src, dst = (torch.from_numpy(ei[k]).int().cuda().contiguous() for k in (0, 1))
    assert np.array_equal(ops.gcn2_loop_counts(src, dst, N).cpu().numpy(), want)
    d_e = torch.tensor([1000], dtype=torch.int32, device="cuda")              # device counts: only the first 1000 edges, 2000 rows
    d_n = torch.tensor([2000], dtype=torch.int32, device="cuda")
    head = ei[:, :1000]
    w2 = np.bincount(head[0][(head[0] == head[1]) & (head[0] < 2000)], minlength=N)[:2000]
    assert np.array_equal(ops.gcn2_loop_counts(src, dst, N, d_n=d_n, d_e=d_e).cpu().numpy()[:2000], w2)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).int()   # a relabelling table (global -> local)
    got = ops.gcn2_loop_counts(src, dst, N, node_map=perm.cuda()).cpu().numpy()
    assert np.array_equal(got[perm.numpy()], want)
    g = DeviceGraph.from_edge_index(torch.from_numpy(ei).cuda(), N)             # de-duplicated CSR: 0 or 1 per node
    assert np.array_equal(ops.gcn2_loop_counts_csr(g.rowptr, g.col, N).cpu().numpy(), np.minimum(want, 1))


def test_prepared_graph_without_loop_counts_is_refused():
    _need_gpu()
    from grapes_amd import ops
    from grapes_amd._lib import GrapesHipError
    ei = O.gpu_graph(62)
    prep = ops.PreparedGraph(torch.from_numpy(ei[0]).int().cuda().contiguous(), torch.from_numpy(ei[1]).int().cuda().contiguous(), N)
    x = torch.randn(N, 8, device="cuda")
    with pytest.raises(GrapesHipError, match="self-loop"):
        ops.gcn2_propagate_fwd(x, x, prep, 0.1)


def test_two_runs_are_bit_identical():
    _need_gpu()
    for case in (0, 3):                                                   # shared + ReLU at 256, unshared + ReLU at 128
        c, shared, relu, alpha = O.CONV_CASES[case]
        ei, x, x0, W1, W2, G, _ = O.conv_case(c, shared, seed=31 + case)
        conv = _conv(c, shared, alpha, W1, W2)
        xd, x0d, Gd, eid = x.cuda(), x0.cuda(), G.cuda(), torch.from_numpy(ei).cuda()
        a = _run(conv, xd, x0d, eid, Gd, True)
        b = _run(conv, xd, x0d, eid, Gd, True)
        for s, t in zip(a, b):
            assert torch.equal(s, t)


def test_captured_forward_backward_replays_bit_identically():
    _need_gpu()
    from grapes_amd.modules.gcn import _gcn2_graph
    c, shared, relu, alpha = O.CONV_CASES[6]                               # 64 wide, shared, ReLU
    ei, x, x0, W1, W2, G, _ = O.conv_case(c, shared, seed=41)
    conv = _conv(c, shared, alpha, W1, W2)
    xd, x0d, Gd = x.cuda(), x0.cuda(), G.cuda()
    prep = _gcn2_graph(torch.from_numpy(ei).cuda(), N)                     # (the graph build and the loop count are outside the capture)
    eager = [t.clone() for t in _run(conv, xd, x0d, prep, Gd, True)]
    again = _run(conv, xd, x0d, prep, Gd, True)
    for s, t in zip(eager, again):
        assert torch.equal(s, t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _run(conv, xd, x0d, prep, Gd, True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _run(conv, xd, x0d, prep, Gd, True)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for s, t in zip(eager, captured):
        assert torch.equal(s, t)


@pytest.mark.parametrize("c", [64, 47])
def test_long_rows_on_both_csrs_and_device_row_count(c):
    """A hub as target AND as source on a graph large enough for the work-item path (n > 2048): rows longer than GRAPES_LONG_ROW on
    both CSRs; then the same launches with d_n below the allocated rows leave the rows past it untouched."""
    _need_gpu()
    from grapes_amd import ops
    n, hub = 2600, 5
    rng = np.random.default_rng(71)
    base = O.random_graph(n, seed=72, mean_deg=4, hub=hub, hub_deg=900, n_dup=20, n_loops=30, n_isolated=10)
    out_edges = np.stack([np.full(700, hub), rng.integers(0, n - 10, 700)])          # the hub as source
    ei = np.concatenate([base, out_edges, np.array([[hub, hub], [hub, hub]]).T.reshape(2, -1)], axis=1).astype(np.int64)
    indeg, outdeg = np.bincount(ei[1][ei[0] != ei[1]], minlength=n), np.bincount(ei[0][ei[0] != ei[1]], minlength=n)
    assert indeg[hub] > 64 * 8 and outdeg[hub] > 64 * 8
    g = torch.Generator().manual_seed(73)
    x, x0, ds = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    src, dst = (torch.from_numpy(ei[k]).int().cuda().contiguous() for k in (0, 1))
    prep = ops.gcn2_attach_loops(ops.PreparedGraph(src, dst, n), src, dst)
    assert int(prep.n_items_t.item()) > 8 and int(prep.n_items_s.item()) > 8
    alpha = 0.3
    s, p = ops.gcn2_propagate_fwd(x.cuda(), x0.cuda(), prep, alpha, want_p=True)
    P = O.propagate(x.double(), ei)
    assert O.rel_err(p.cpu(), (1 - alpha) * P) <= ACT_TOL and O.rel_err(s.cpu(), (1 - alpha) * P + alpha * x0.double()) <= ACT_TOL
    dx, dx0 = ops.gcn2_propagate_bwd(ds.cuda(), prep, alpha)
    s_, d_ = O.edges(ei)
    want_dx = (1 - alpha) * torch.zeros(n, c, dtype=O.F64).index_add(0, s_, ds.double()[d_])
    assert O.rel_err(dx.cpu(), want_dx) <= GRAD_TOL and O.rel_err(dx0.cpu(), alpha * ds.double()) <= GRAD_TOL
    acc = torch.ones(n, c, device="cuda")
    _, dx0b = ops.gcn2_propagate_bwd(ds.cuda(), prep, alpha, dx0=acc)               # the accumulate flag
    assert O.rel_err(dx0b.cpu(), 1.0 + alpha * ds.double()) <= GRAD_TOL
    # d_n < allocated rows: a graph over the first m nodes, buffers of n rows pre-filled with a mark
    m = 2100
    keep = (ei[0] < m) & (ei[1] < m)
    em = ei[:, keep]
    d_n = torch.tensor([m], dtype=torch.int32, device="cuda")
    srcm, dstm = (torch.from_numpy(em[k]).int().cuda().contiguous() for k in (0, 1))
    prepm = ops.gcn2_attach_loops(ops.PreparedGraph(srcm, dstm, n, d_n=d_n), srcm, dstm)
    L = ops.lib()
    mark = 12345.0
    so, po, dxo, dx0o, mo, g0, g1 = (torch.full((n, c), mark, device="cuda") for _ in range(7))
    ws = ops._ws(L.grapes_gcn2_propagate_workspace_bytes(n, prepm.item_cap, c), "cuda")
    P_ = ops._p
    xd, x0d, dsd = x.cuda(), x0.cuda(), ds.cuda()
    assert L.grapes_gcn2_propagate_fwd(P_(xd), P_(x0d), P_(prepm.loops), P_(prepm.rowptr_t), P_(prepm.csr_src), alpha, P_(so), P_(po), n,
                                       P_(d_n), c, P_(prepm.items_t), P_(prepm.n_items_t), prepm.item_cap, P_(ws), None,
                                       ops._stream()) == 0
    assert L.grapes_gcn2_propagate_bwd(P_(dsd), None, 0, None, P_(prepm.loops), P_(prepm.rowptr_s), P_(prepm.csr_dst), alpha, P_(dxo),
                                       P_(dx0o), 0, n, P_(d_n), c, P_(prepm.items_s), P_(prepm.n_items_s), prepm.item_cap, P_(ws), None,
                                       ops._stream()) == 0
    assert L.grapes_gcn2_mix_fwd(P_(xd), P_(x0d), None, 0.5, 0.5, 0.0, 1, P_(mo), n, P_(d_n), c, ops._stream()) == 0
    assert L.grapes_gcn2_mix_bwd(P_(dsd), P_(mo), 1, 0.25, 0.75, 0.0, P_(g0), P_(g1), None, n, P_(d_n), c, ops._stream()) == 0
    torch.cuda.synchronize()
    Pm = O.propagate(x.double()[:m], em)
    assert O.rel_err(so[:m].cpu(), (1 - alpha) * Pm + alpha * x0.double()[:m]) <= ACT_TOL and O.rel_err(po[:m].cpu(), (1 - alpha) * Pm) <= ACT_TOL
    sm, dm = O.edges(em)
    assert O.rel_err(dxo[:m].cpu(), (1 - alpha) * torch.zeros(m, c, dtype=O.F64).index_add(0, sm, ds.double()[:m][dm])) <= GRAD_TOL
    assert O.rel_err(dx0o[:m].cpu(), alpha * ds.double()[:m]) <= GRAD_TOL
    want_mix = torch.relu(0.5 * x.double()[:m] + 0.5 * x0.double()[:m])
    assert O.rel_err(mo[:m].cpu(), want_mix) <= ACT_TOL
    assert O.rel_err(g1[:m].cpu(), 0.75 * ds.double()[:m] * (mo[:m].cpu() > 0)) <= ACT_TOL
    for t in (so, po, dxo, dx0o, mo, g0, g1):
        assert bool((t[m:] == mark).all())                               # rows past d_n are untouched


def _masks_from(draws, p):
    """The dropout masks the model drew, regenerated from the Philox stream at the recorded (seed, offset): kept iff u >= p."""
    from grapes_amd import ops
    out = []
    for shape, seed, off in draws:
        u = ops.philox_uniform(int(np.prod(shape)), seed, off, "cuda").cpu().double().reshape(shape)
        out.append((u >= p).double() / (1.0 - p))
    return out


@pytest.mark.parametrize("dropout", [0.0, 0.3])
def test_two_layer_gcn2_on_layerwise_graphs_matches_oracle(dropout):
    _need_gpu()
    from grapes_amd import ops
    from grapes_amd.modules.gcn import GCN2
    e0, e1 = O.gpu_graph(51), O.gpu_graph(52)
    x = torch.randn(N, 48, generator=torch.Generator().manual_seed(53))
    y = torch.randint(0, 7, (N,), generator=torch.Generator().manual_seed(55))
    torch.manual_seed(54)
    model = GCN2(48, [64, 7], alpha=0.1, theta=0.5, dropout=dropout)
    params = O.model_params(model)
    model = model.cuda()
    draws, counter = [], [1000]
    if dropout:
        def hook(n_elements):                                            # the trainer's hook: hands out Philox counters
            off = counter[0]
            counter[0] += (int(n_elements) + 3) // 4
            draws.append([None, 77, off])
            return 77, off
        model.philox_dropout = hook
    preps = []
    for e in (e0, e1):
        s, d = (torch.from_numpy(e[k]).int().cuda().contiguous() for k in (0, 1))
        preps.append(ops.gcn2_attach_loops(ops.PreparedGraph(s, d, N), s, d))
    logits = model(x.cuda(), preps)
    assert torch.is_tensor(logits)                                       # gcn.py:117: logits only
    masks = None
    if dropout:
        assert len(draws) == 3                                           # the input and one in front of each conv
        for dr, shape in zip(draws, [(N, 48), (N, 64), (N, 64)]):
            dr[0] = shape
        masks = _masks_from(draws, dropout)
    leaves, flat = O.param_leaves(params)
    ref, pres = O.gcn2_forward(x.double(), leaves, [e0, e1], masks=masks, full=True)
    near = [(p.detach().abs() < O.KINK) for p in pres]
    for p, nr in zip(pres, near):
        print(f"hidden pre-activations within 1e-5 of zero: {int(nr.sum())} of {nr.numel()} ({int(nr.any(0).sum())} units)")
        assert int(nr.sum()) <= 0.01 * nr.numel()                        # the cap: at most 1 % of the hidden values
    err = O.rel_err(logits.detach().cpu(), ref.detach())
    print(f"logits rel err {err:.2e}")
    assert err <= ACT_TOL
    rg = torch.autograd.grad(torch.nn.functional.cross_entropy(ref, y), flat)
    torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
    keep0, keep1 = ~near[0].any(0), ~near[1].any(0)                      # units of lins[0] / of the first conv next to a kink
    got = [model.lins[0].weight, model.lins[0].bias, model.lins[1].weight, model.lins[1].bias, model.conv[0].weight1, model.conv[1].weight1]
    names = ["lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias", "conv.0.weight1", "conv.1.weight1"]
    for name, t, want in zip(names, got, rg):
        g = t.grad.detach().cpu().double()
        if name.startswith("lins.0"):                                    # upstream of lins[0]'s ReLU: its own units
            g, want = g[keep0], want[keep0]
        elif name == "conv.0.weight1":                                   # upstream of the first conv's ReLU: its output units
            g, want = g[:, keep1], want[:, keep1]
        e = float((g - want).abs().max()) / max(1.0, float(want.abs().max()))
        print(f"{name}: grad rel err {e:.2e}")
        assert e <= GRAD_TOL, name


def _cora_like(seed=3):
    from grapes_amd import synth
    n, F, C = 2708, 32, 7
    indptr, indices = synth.synth_csr_numpy(n, 4.0, 170, seed=seed)
    rng = np.random.default_rng(seed + 1)
    X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, C, n))
    return n, F, C, indptr, indices, X, y, rng


def test_grapes_trainer_with_gcn2_classifier_matches_oracle():
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN, GCN2
    from grapes_amd.step import GrapesTrainer
    n, F, C, indptr, indices, X, y, rng = _cora_like()
    hops, K, B, H = 2, 16, 64, 64
    torch.manual_seed(0)
    gf0, z0 = GCN(F + hops + 1, [H, 1]), GCN(F, [H, 1])
    kept = {}
    for kind in ("gcn2", "gcn"):
        torch.manual_seed(1)
        c = (GCN2(F, [H, C], alpha=0.1, theta=0.5) if kind == "gcn2" else GCN(F, [H, C])).cuda()
        gf, z = GCN(F + hops + 1, [H, 1]).cuda(), GCN(F, [H, 1]).cuda()
        gf.load_state_dict(gf0.state_dict()); z.load_state_dict(z0.state_dict())
        opt_c = torch.optim.Adam(c.parameters(), lr=1e-2)
        tr = GrapesTrainer(DeviceGraph.from_csr(indptr, indices), X.cuda(), y.cuda(), c, gf, z, sampling_hops=hops, num_samples=K,
                           loss_coef=10.0, optimizer_c=opt_c, optimizer_gf=None, philox_seed=7)
        kept[kind] = []
        targets_rng = np.random.default_rng(5)
        for step in range(3):
            targets = torch.from_numpy(targets_rng.permutation(n)[:B].astype(np.int64))
            params = O.model_params(c) if kind == "gcn2" else None
            out = tr.step(targets, trace=True)
            kept[kind].append([h["kept"].cpu().numpy().astype(np.int64) for h in out["hops"]])
            if kind != "gcn2":
                continue
            all_nodes = out["all_nodes"].cpu().long()
            edges = [e.cpu().numpy().astype(np.int64) for e in out["edge_indices"]]
            ref = O.gcn2_forward(X[all_nodes].double(), params, edges)
            lt = out["local_target_ids"].cpu().long()
            ref_loss = float(torch.nn.functional.cross_entropy(ref[lt], y[targets]))
            err = O.rel_err(out["logits"].cpu(), ref)
            print(f"step {step}: {all_nodes.numel()} nodes, logits rel err {err:.2e}, loss_c {float(out['loss_c']):.6f} vs {ref_loss:.6f}")
            assert err <= ACT_TOL
            assert abs(float(out["loss_c"]) - ref_loss) <= ACT_TOL * max(1.0, abs(ref_loss))
    for a, b in zip(kept["gcn2"], kept["gcn"]):                          # the sampler does not see the classifier
        for ka, kb in zip(a, b):
            assert np.array_equal(ka, kb)


def test_trainer_step_gradients_match_oracle():
    """One TRAINING step (backward inside the trainer, no optimiser): every parameter's gradient against the oracle on the sampled
    graphs the step reports."""
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN, GCN2
    from grapes_amd.step import GrapesTrainer
    n, F, C, indptr, indices, X, y, rng = _cora_like(seed=13)
    hops, K, B, H = 2, 16, 64, 64
    torch.manual_seed(2)
    c = GCN2(F, [H, C], alpha=0.1, theta=0.5, shared_weights=False).cuda()
    gf, z = GCN(F + hops + 1, [H, 1]).cuda(), GCN(F, [H, 1]).cuda()
    tr = GrapesTrainer(DeviceGraph.from_csr(indptr, indices), X.cuda(), y.cuda(), c, gf, z, sampling_hops=hops, num_samples=K,
                       loss_coef=10.0, optimizer_c=None, optimizer_gf=None, philox_seed=9)
    params = O.model_params(c)
    targets = torch.from_numpy(rng.permutation(n)[:B].astype(np.int64))
    out = tr.step(targets, trace=True)
    all_nodes = out["all_nodes"].cpu().long()
    edges = [e.cpu().numpy().astype(np.int64) for e in out["edge_indices"]]
    leaves, flat = O.param_leaves(params)
    ref = O.gcn2_forward(X[all_nodes].double(), leaves, edges)
    ref_loss = torch.nn.functional.cross_entropy(ref[out["local_target_ids"].cpu().long()], y[targets])
    assert O.rel_err(out["logits"].cpu(), ref.detach()) <= ACT_TOL
    assert abs(float(out["loss_c"]) - float(ref_loss)) <= ACT_TOL * max(1.0, abs(float(ref_loss)))
    rg = torch.autograd.grad(ref_loss, flat)
    names = [k for k, _ in c.named_parameters()]
    assert names == ["lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias", "conv.0.weight1", "conv.0.weight2",
                     "conv.1.weight1", "conv.1.weight2"]
    for (name, p_), want in zip(c.named_parameters(), rg):
        e = O.rel_err(p_.grad.cpu(), want)
        print(f"{name}: grad rel err {e:.2e}")
        assert e <= GRAD_TOL, name


def test_graphed_trainer_refuses_a_gcn2_classifier():
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN, GCN2
    from grapes_amd.step_graph import GraphedTrainer
    n, F, C, indptr, indices, X, y, _ = _cora_like()
    with pytest.raises(NotImplementedError, match="GCN classifier"):
        GraphedTrainer(DeviceGraph.from_csr(indptr, indices), X.cuda(), y.cuda(), GCN2(F, [16, C], alpha=0.1, theta=0.5).cuda(),
                       GCN(F + 3, [16, 1]).cuda(), GCN(F, [16, 1]).cuda(), batch_size=32)


def _with_loops(indptr, indices, n, rng, k=50):
    """The CSR with k stored self-loops added (a DeviceGraph keeps them: main.py:134-136)."""
    rows = np.repeat(np.arange(n), np.diff(indptr))
    v = rng.permutation(n)[:k]
    key = np.unique(np.concatenate([rows * np.int64(n) + np.asarray(indices, dtype=np.int64), v * np.int64(n) + v]))
    r, c = key // n, (key % n).astype(np.int32)
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ip[1:])
    return ip, c


@pytest.mark.parametrize("full_batch", [True, False])
def test_evaluate_with_gcn2_classifier_matches_oracle(full_batch, monkeypatch):
    _need_gpu()
    from types import SimpleNamespace
    from grapes_amd import eval as E, step_graph
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN, GCN2
    n, F, C, indptr, indices, X, y, rng = _cora_like(seed=9)
    indptr, indices = _with_loops(indptr, indices, n, rng)
    hops, K, H = 2, 100000, 32
    torch.manual_seed(3)
    c, gf = GCN2(F, [H, C], alpha=0.1, theta=0.5).cuda(), GCN(F + hops + 1, [H, 1]).cuda()
    g = DeviceGraph.from_csr(indptr, indices)
    mask = torch.zeros(n, dtype=torch.bool); mask[rng.permutation(n)[:640]] = True
    idx = mask.nonzero().squeeze(1)
    args = SimpleNamespace(sampling_hops=hops, num_samples=K, use_indicators=True)
    data = SimpleNamespace(x=X.cuda(), y=y.cuda())

    def no_capture(*a, **k):
        raise AssertionError("evaluate built a GraphedTrainer for a GCN2 classifier")
    monkeypatch.setattr(step_graph, "GraphedTrainer", no_capture)
    loader = [(idx[o:o + 128],) for o in range(0, idx.numel(), 128)]        # five full batches: a GCN would be captured
    acc, f1, pred = E.evaluate(c, gf, data, args, g, mask=mask.cuda(), loader=loader, full_batch=full_batch, return_predictions=True)
    assert acc == f1 and pred.numel() == idx.numel()
    params = O.model_params(c)
    if full_batch:
        rows = np.repeat(np.arange(n), np.diff(indptr))
        ref = O.gcn2_forward(X.double(), params, np.stack([rows, np.asarray(indices, dtype=np.int64)]))[idx]
    else:
        # num_samples exceeds every neighbourhood, so the greedy sampler keeps all candidates and the batch graphs are the exact
        # 2-hop neighbourhoods: the oracle rebuilds them (eval.py:92-150) from the CSR, stored loops included
        adj = [np.asarray(indices[indptr[v]:indptr[v + 1]], dtype=np.int64) for v in range(n)]
        want = []
        for (tb,) in loader:
            t = tb.numpy()
            previous, kept_all, slices = t, [], []
            for _ in range(hops):
                inprev = np.zeros(n, bool); inprev[previous] = True
                nb = np.unique(np.concatenate([adj[u] for u in previous]))
                kept = nb[~inprev[nb]]
                nxt = np.concatenate([t, kept])
                innext = np.zeros(n, bool); innext[nxt] = True
                slices.append([(u, v) for u in previous for v in adj[u] if innext[v]])
                kept_all.append(kept)
                previous = nxt
            all_nodes = np.unique(np.concatenate([t] + kept_all))
            loc = -np.ones(n, np.int64); loc[all_nodes] = np.arange(all_nodes.size)
            edges = [loc[np.array(sl, dtype=np.int64).reshape(-1, 2).T] for sl in slices]
            want.append(O.gcn2_forward(X[all_nodes].double(), params, edges)[loc[t]])
        ref = torch.cat(want)
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-4                               # (an argmax between two near-equal logits is not a mismatch)
    assert int(sure.sum()) >= 0.99 * idx.numel()
    assert torch.equal(pred.cpu()[sure], ref.argmax(1)[sure])
    assert abs(acc - float((pred.cpu() == y[idx]).float().mean())) < 1e-6


def test_device_graph_on_the_large_path_is_refused():
    _need_gpu()
    from grapes_amd import full_graph
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN2
    n, F, C, indptr, indices, X, y, _ = _cora_like()
    g = DeviceGraph.from_csr(indptr, indices)
    old = full_graph.LARGE_NNZ
    full_graph.LARGE_NNZ = 1                          # (every graph then counts as one of 2^31 or more entries)
    try:
        with pytest.raises(ValueError, match="2\\^31"):
            GCN2(F, [8, C], alpha=0.1, theta=0.5).cuda()(X.cuda(), g)
    finally:
        full_graph.LARGE_NNZ = old


def test_cli_trains_a_gcn2_classifier():
    _need_gpu()
    r = subprocess.run([sys.executable, "-m", "grapes_amd.main", "--dataset", "cora", "--classifier", "gcn2", "--max_epochs", "2",
                        "--runs", "1", "--eval_frequency", "1", "--dropout", "0.1"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    losses = [(float(a), float(b)) for a, b in re.findall(r"loss_gfn=([-\w.+]+), loss_c=([-\w.+]+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(v) for p in losses for v in p)
    assert "valid_accuracy=" in r.stdout and "test_accuracy=" in r.stdout and "Acc: " in r.stdout


def test_full_batch_cli_trains_a_gcn2_classifier():
    _need_gpu()
    r = subprocess.run([sys.executable, "-m", "grapes_amd.full_batch", "--dataset", "cora", "--classifier", "gcn2", "--max_epochs", "3",
                        "--runs", "1", "--eval_frequency", "2", "--hidden_dim", "32", "--seed", "1", "--lr_gc", "0.01",
                        "--gcn2_shared_weights", "false"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    losses = [float(v) for v in re.findall(r"epoch \d+: loss_c=([-\w.+]+)", r.stdout)]
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert "valid_f1=" in r.stdout and "test_accuracy=" in r.stdout and "Acc: " in r.stdout
