"""The GAT classifier (reference modules/gcn.py:45-72) on the MI355X against the fp64 oracle of tests/gat_oracle.py.

Tolerances are the project's: activations max|a − ref| / max(1, max|ref|) <= 1e-5, gradients the same measure at 1e-4.
LeakyReLU / ReLU kinks are avoided by the choice of inputs, which every gradient test asserts on the ORACLE's values before it
compares (min |s_src[j] + s_dst[i]| over the edges > 1e-5; in the two-layer test at most 1 % of the hidden pre-activations lie
within 1e-5 of zero, and the hidden units that own one are left out of the first layer's gradient comparison)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gat_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_TOL, GRAD_TOL = 1e-5, 1e-4
N = 3000
HUB, HUB_DEG = 17, 2100


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _graph(seed, n=N):
    return O.random_graph(n, seed=seed, mean_deg=6, hub=HUB, hub_deg=HUB_DEG, n_dup=60, n_loops=40, n_isolated=25,
                          directed_block=30)


def _conv(fi, c, seed):
    from grapes_amd.modules.gcn import GATConv
    torch.manual_seed(seed)
    conv = GATConv(fi, c)
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)              # (PyG initialises it to zero; a non-zero one exercises c_i = G_i·(out_i − b))
    return conv


def _inputs(fi, c, seed, att_scale=None):
    ei = _graph(seed)
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(N, fi, generator=g)
    G = torch.randn(N, c, generator=g)
    conv = _conv(fi, c, seed + 200)
    if att_scale is not None:
        W, a_s, a_d, b = O.layer_params(conv)
        r = O.gat_conv(x.double(), W, a_s, a_d, b, ei, full=True)
        e = torch.where(r["raw"] > 0, r["raw"], O.SLOPE * r["raw"])
        k = att_scale / float(e.abs().max())
        with torch.no_grad():
            conv.att_src.mul_(k); conv.att_dst.mul_(k)
    return ei, x, G, conv


def _run(conv, x, ei_dev, G, relu=False):
    """One forward and backward on the device: (out, dX, dW, da_src, da_dst, db)."""
    xd = x.detach().clone().requires_grad_(True)
    out = conv(xd, ei_dev, relu=relu)
    grads = torch.autograd.grad(out, [xd, conv.lin.weight, conv.att_src, conv.att_dst, conv.bias], G)
    return (out.detach(),) + tuple(g.detach() for g in grads)


def _compare(got, x, G, conv, ei, relu=False):
    W, a_s, a_d, b = O.layer_params(conv)
    ref = O.gat_conv(x.double(), W, a_s, a_d, b, ei, relu=relu)
    gr = O.gat_conv_grads(x.double(), W, a_s, a_d, b, ei, G.double(), relu=relu)
    errs = {"out": O.rel_err(got[0].cpu(), ref)}
    for k, t in zip(("dX", "dW", "da_src", "da_dst", "db"), got[1:]):
        errs[k] = O.rel_err(t.cpu().reshape(gr[k].shape), gr[k])
    print("errors vs fp64 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert torch.isfinite(got[0]).all()
    assert errs["out"] <= ACT_TOL, errs
    for k in ("dX", "dW", "da_src", "da_dst", "db"):
        assert errs[k] <= GRAD_TOL, errs
    return errs


def _min_raw(x, conv, ei):
    r = O.gat_conv(x.double(), *O.layer_params(conv), ei, full=True)
    return float(r["raw"].abs().min()), r


@pytest.mark.parametrize("fi,c,seed", [(48, 64, 1), (100, 256, 2), (256, 47, 3), (64, 7, 4), (64, 1, 5), (32, 41, 6), (24, 40, 7)])
def test_gatconv_forward_backward_match_oracle(fi, c, seed):
    _need_gpu()
    ei, x, G, conv = _inputs(fi, c, seed)
    m, r = _min_raw(x, conv, ei)
    indeg = torch.bincount(r["dst"], minlength=N)
    print(f"edges {r['src'].numel()}, hub in-degree {int(indeg[HUB])}, isolated {int((indeg == 1).sum())}, min|raw| {m:.2e}")
    assert int(indeg[HUB]) > 2000 and m > 1e-5           # no edge sits on LeakyReLU's kink in the oracle
    conv = conv.cuda()
    got = _run(conv, x.cuda(), torch.from_numpy(ei).cuda(), G.cuda())
    _compare(got, x, G, conv, ei)


def test_softmax_is_stable_at_large_scores():
    _need_gpu()
    ei, x, G, conv = _inputs(48, 64, 21, att_scale=80.0)
    m, r = _min_raw(x, conv, ei)
    e = torch.where(r["raw"] > 0, r["raw"], O.SLOPE * r["raw"])
    print(f"max|e| {float(e.abs().max()):.1f}, min|raw| {m:.2e}")
    assert float(e.abs().max()) >= 79.0 and m > 1e-5
    conv = conv.cuda()
    got = _run(conv, x.cuda(), torch.from_numpy(ei).cuda(), G.cuda())
    for t in got:
        assert torch.isfinite(t).all()
    _compare(got, x, G, conv, ei)


def test_two_runs_are_bit_identical():
    _need_gpu()
    ei, x, G, conv = _inputs(100, 256, 31)
    conv = conv.cuda()
    xd, Gd, eid = x.cuda(), G.cuda(), torch.from_numpy(ei).cuda()
    a = _run(conv, xd, eid, Gd, relu=True)
    b = _run(conv, xd, eid, Gd, relu=True)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_captured_forward_backward_replays_bit_identically():
    _need_gpu()
    from grapes_amd.modules.gcn import prepare_edges
    ei, x, G, conv = _inputs(48, 64, 41)
    conv = conv.cuda()
    xd, Gd = x.cuda(), G.cuda()
    prep = prepare_edges(torch.from_numpy(ei).cuda(), N)            # (the graph build is outside the capture)
    eager = [t.clone() for t in _run(conv, xd, prep, Gd)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _run(conv, xd, prep, Gd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _run(conv, xd, prep, Gd)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for s, t in zip(eager, captured):
        assert torch.equal(s, t)
    assert int(prep.status.item()) == 0 if prep.status is not None else True


@pytest.mark.parametrize("c", [64, 47])
def test_long_rows_on_both_csrs_and_device_row_count(c):
    """A hub as target AND as source on a graph large enough for the work-item path (n > 2048): rows longer than GRAPES_LONG_ROW on
    both CSRs, so the by-source chunk and combine kernels run as well; the hub row is measured on its own and with all rows.  Then
    the same launches with d_n below the allocated rows leave the rows past it untouched."""
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
    h, G = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    a_s, a_d = (torch.rand(c, generator=g) * 2 - 1) * 0.3, (torch.rand(c, generator=g) * 2 - 1) * 0.3
    b = (torch.rand(c, generator=g) * 2 - 1) * 0.1
    eye = torch.eye(c, dtype=O.F64)                                                    # (W = I: the oracle's H is h itself)

    def oracle(m, edges):
        args = (h[:m].double(), eye, a_s.double(), a_d.double(), b.double(), edges)
        r = O.gat_conv(*args, full=True)
        raw = float(r["raw"].abs().min())
        print(f"c {c} rows {m}: edges {r['src'].numel()}, min|raw| {raw:.2e}")
        assert raw > 1e-5                                                             # no edge sits on LeakyReLU's kink in the oracle
        return r["out"], O.gat_conv_grads(*args, G[:m].double())

    def check(name, rows, got, ref, gr):
        out, dh, da_src, da_dst, db = (t.cpu() for t in got)
        errs = {"out": O.rel_err(out[rows], ref[rows]), "dh": O.rel_err(dh[rows], gr["dH"][rows])}
        if name[:3] != "hub":                                                         # (the parameter gradients are sums over all rows)
            errs.update(da_src=O.rel_err(da_src, gr["da_src"]), da_dst=O.rel_err(da_dst, gr["da_dst"]), db=O.rel_err(db, gr["db"]))
        print(f"c {c} rows {name}:", {k: f"{v:.2e}" for k, v in errs.items()})
        assert errs.pop("out") <= ACT_TOL
        assert all(v <= GRAD_TOL for v in errs.values()), errs

    ref, gr = oracle(n, ei)
    src, dst = (torch.from_numpy(ei[k]).int().cuda().contiguous() for k in (0, 1))
    prep = ops.PreparedGraph(src, dst, n)
    assert int(prep.n_items_t.item()) > 8 and int(prep.n_items_s.item()) > 8
    hd, Gd, asd, add, bd = h.cuda(), G.cuda(), a_s.cuda(), a_d.cuda(), b.cuda()
    s_src, s_dst = ops.gat_scores(hd, asd, add)
    out, row_ms = ops.gat_aggregate_fwd(hd, s_src, s_dst, prep, bd)
    got = (out,) + tuple(ops.gat_aggregate_bwd(Gd, out, hd, s_src, s_dst, row_ms, asd, add, prep, bd))
    for rows, name in ((torch.arange(n) == hub, "hub"), (torch.ones(n, dtype=torch.bool), "all")):
        check(name, rows, got, ref, gr)
    # d_n < allocated rows: a graph over the first m nodes, buffers of n rows pre-filled with a mark
    m = 2100
    em = ei[:, (ei[0] < m) & (ei[1] < m)]
    refm, grm = oracle(m, em)
    d_n = torch.tensor([m], dtype=torch.int32, device="cuda")
    srcm, dstm = (torch.from_numpy(em[k]).int().cuda().contiguous() for k in (0, 1))
    prepm = ops.PreparedGraph(srcm, dstm, n, d_n=d_n)
    assert int(prepm.n_items_t.item()) > 8 and int(prepm.n_items_s.item()) > 8
    L, P_, mark = ops.lib(), ops._p, 12345.0
    oo, dho = torch.full((n, c), mark, device="cuda"), torch.full((n, c), mark, device="cuda")
    sso, sdo = torch.full((n,), mark, device="cuda"), torch.full((n,), mark, device="cuda")
    rmo = torch.full((n, 2), mark, device="cuda")
    dpar = [torch.empty(c, device="cuda") for _ in range(3)]
    ws = ops._ws(max(L.grapes_gat_aggregate_workspace_bytes(prepm.item_cap, c),
                     L.grapes_gat_aggregate_bwd_workspace_bytes(n, prepm.item_cap, c)), "cuda")
    assert L.grapes_gat_scores(P_(hd), P_(asd), P_(add), P_(sso), P_(sdo), n, P_(d_n), c, ops._stream()) == 0
    assert L.grapes_gat_aggregate_fwd(P_(hd), P_(sso), P_(sdo), P_(prepm.rowptr_t), P_(prepm.csr_src), P_(bd), P_(oo), P_(rmo), n,
                                      P_(d_n), c, 0, P_(prepm.items_t), P_(prepm.n_items_t), prepm.item_cap, P_(ws), None,
                                      ops._stream()) == 0
    assert L.grapes_gat_aggregate_bwd(P_(Gd), P_(oo), P_(bd), 0, P_(hd), P_(sso), P_(sdo), P_(rmo), P_(asd), P_(add),
                                      P_(prepm.rowptr_t), P_(prepm.csr_src), P_(prepm.rowptr_s), P_(prepm.csr_dst), P_(dho),
                                      P_(dpar[0]), P_(dpar[1]), P_(dpar[2]), n, P_(d_n), c, P_(prepm.items_t), P_(prepm.n_items_t),
                                      P_(prepm.items_s), P_(prepm.n_items_s), prepm.item_cap, P_(ws), None, ops._stream()) == 0
    torch.cuda.synchronize()
    gotm = (oo[:m], dho[:m], dpar[0], dpar[1], dpar[2])
    for rows, name in ((torch.arange(m) == hub, "hub"), (torch.ones(m, dtype=torch.bool), "all")):
        check(name + " (d_n)", rows, gotm, refm, grm)
    for t in (oo, dho, sso, sdo, rmo):
        assert bool((t[m:] == mark).all())                               # rows past d_n are untouched


def test_two_layer_gat_on_prepared_graphs_matches_oracle():
    _need_gpu()
    from grapes_amd import ops
    from grapes_amd.modules.gcn import GAT
    e0, e1 = _graph(51), _graph(52)
    g = torch.Generator().manual_seed(53)
    x = torch.randn(N, 48, generator=g)
    y = torch.randint(0, 7, (N,), generator=g)
    torch.manual_seed(54)
    model = GAT(48, [64, 7])
    params = [O.layer_params(l) for l in model.gat_layers]
    leaves = [[t.clone().requires_grad_(True) for t in p] for p in params]
    ref, pres = O.gat_forward(x.double(), leaves, [e0, e1], full=True)
    near = (pres[0].detach().abs() < 1e-5)
    units = near.any(0)
    print(f"hidden pre-activations within 1e-5 of zero: {int(near.sum())} of {near.numel()} ({int(units.sum())} of {units.numel()} units)")
    assert int(near.sum()) <= 0.01 * near.numel()                  # the cap: at most 1 % of the hidden values
    loss = torch.nn.functional.cross_entropy(ref, y)
    rg = torch.autograd.grad(loss, [t for p in leaves for t in p])
    model = model.cuda()
    preps = [ops.PreparedGraph(torch.from_numpy(e[0]).int().cuda().contiguous(), torch.from_numpy(e[1]).int().cuda().contiguous(), N)
             for e in (e0, e1)]
    logits = model(x.cuda(), preps)
    assert torch.is_tensor(logits)                                   # gcn.py:72: logits only, no (logits, memory) pair
    err = O.rel_err(logits.detach().cpu(), ref.detach())
    print(f"logits rel err {err:.2e}")
    assert err <= ACT_TOL
    torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
    keep = ~units
    for li, layer in enumerate(model.gat_layers):
        for k, t in enumerate((layer.lin.weight, layer.att_src, layer.att_dst, layer.bias)):
            got, want = t.grad.detach().cpu().double().reshape(rg[4 * li + k].shape), rg[4 * li + k]
            if li == 0:                                              # units next to the ReLU kink are left out (see the module docstring)
                got, want = got[keep], want[keep]
            e = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
            print(f"layer {li} grad {k}: rel err {e:.2e}")
            assert e <= GRAD_TOL


def _cora_like(seed=3):
    from grapes_amd import synth
    n, F, C = 2708, 32, 7
    indptr, indices = synth.synth_csr_numpy(n, 4.0, 170, seed=seed)
    rng = np.random.default_rng(seed + 1)
    X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, C, n))
    return n, F, C, indptr, indices, X, y, rng


def test_grapes_trainer_with_gat_classifier_matches_oracle():
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GAT, GCN
    from grapes_amd.step import GrapesTrainer
    n, F, C, indptr, indices, X, y, rng = _cora_like()
    hops, K, B, H = 2, 16, 64, 64
    torch.manual_seed(0)
    gf0, z0 = GCN(F + hops + 1, [H, 1]), GCN(F, [H, 1])
    kept = {}
    for kind in ("gat", "gcn"):
        torch.manual_seed(1)
        c = (GAT(F, [H, C]) if kind == "gat" else GCN(F, [H, C])).cuda()
        gf, z = GCN(F + hops + 1, [H, 1]).cuda(), GCN(F, [H, 1]).cuda()
        gf.load_state_dict(gf0.state_dict()); z.load_state_dict(z0.state_dict())
        opt_c = torch.optim.Adam(c.parameters(), lr=1e-2)
        tr = GrapesTrainer(DeviceGraph.from_csr(indptr, indices), X.cuda(), y.cuda(), c, gf, z, sampling_hops=hops, num_samples=K,
                           loss_coef=10.0, optimizer_c=opt_c, optimizer_gf=None, philox_seed=7)
        kept[kind] = []
        targets_rng = np.random.default_rng(5)
        for step in range(3):
            targets = torch.from_numpy(targets_rng.permutation(n)[:B].astype(np.int64))
            params = [O.layer_params(l) for l in c.gat_layers] if kind == "gat" else None
            out = tr.step(targets, trace=True)
            kept[kind].append([h["kept"].cpu().numpy().astype(np.int64) for h in out["hops"]])
            if kind != "gat":
                continue
            all_nodes = out["all_nodes"].cpu().long()
            edges = [e.cpu().numpy().astype(np.int64) for e in out["edge_indices"]]
            ref = O.gat_forward(X[all_nodes].double(), params, edges)
            lt = out["local_target_ids"].cpu().long()
            ref_loss = float(torch.nn.functional.cross_entropy(ref[lt], y[targets]))
            err = O.rel_err(out["logits"].cpu(), ref)
            print(f"step {step}: {all_nodes.numel()} nodes, logits rel err {err:.2e}, loss_c {float(out['loss_c']):.6f} vs {ref_loss:.6f}")
            assert err <= ACT_TOL
            assert abs(float(out["loss_c"]) - ref_loss) <= ACT_TOL * max(1.0, abs(ref_loss))
    for a, b in zip(kept["gat"], kept["gcn"]):                       # the sampler does not see the classifier
        for ka, kb in zip(a, b):
            assert np.array_equal(ka, kb)


def test_graphed_trainer_refuses_a_gat_classifier():
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GAT, GCN
    from grapes_amd.step_graph import GraphedTrainer
    n, F, C, indptr, indices, X, y, _ = _cora_like()
    with pytest.raises(NotImplementedError):
        GraphedTrainer(DeviceGraph.from_csr(indptr, indices), X.cuda(), y.cuda(), GAT(F, [16, C]).cuda(), GCN(F + 3, [16, 1]).cuda(),
                       GCN(F, [16, 1]).cuda(), batch_size=32)


@pytest.mark.parametrize("full_batch", [True, False])
def test_evaluate_with_gat_classifier_matches_oracle(full_batch, monkeypatch):
    _need_gpu()
    from types import SimpleNamespace
    from grapes_amd import eval as E, step_graph
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GAT, GCN
    n, F, C, indptr, indices, X, y, rng = _cora_like(seed=9)
    hops, K, H = 2, 100000, 32
    torch.manual_seed(3)
    c, gf = GAT(F, [H, C]).cuda(), GCN(F + hops + 1, [H, 1]).cuda()
    g = DeviceGraph.from_csr(indptr, indices)
    mask = torch.zeros(n, dtype=torch.bool); mask[rng.permutation(n)[:640]] = True
    idx = mask.nonzero().squeeze(1)
    args = SimpleNamespace(sampling_hops=hops, num_samples=K, use_indicators=True)
    data = SimpleNamespace(x=X.cuda(), y=y.cuda())

    def no_capture(*a, **k):
        raise AssertionError("evaluate built a GraphedTrainer for a GAT classifier")
    monkeypatch.setattr(step_graph, "GraphedTrainer", no_capture)
    loader = [(idx[o:o + 128],) for o in range(0, idx.numel(), 128)]        # five full batches: a GCN would be captured
    acc, f1, pred = E.evaluate(c, gf, data, args, g, mask=mask.cuda(), loader=loader, full_batch=full_batch, return_predictions=True)
    assert acc == f1 and pred.numel() == idx.numel()
    params = [O.layer_params(l) for l in c.gat_layers]
    if full_batch:
        rows = np.repeat(np.arange(n), np.diff(indptr))
        ref = O.gat_forward(X.double(), params, np.stack([rows, np.asarray(indices, dtype=np.int64)]))[idx]
        top2 = ref.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) > 1e-4                           # (an argmax between two near-equal logits is not a mismatch)
        assert int(sure.sum()) >= 0.99 * idx.numel()
        assert torch.equal(pred.cpu()[sure], ref.argmax(1)[sure])
        assert abs(acc - float((pred.cpu() == y[idx]).float().mean())) < 1e-6
    else:
        # num_samples exceeds every neighbourhood, so the greedy sampler keeps all candidates and the batch graphs are the exact
        # 2-hop neighbourhoods: the oracle rebuilds them (eval.py:92-150) from the CSR
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
            ref = O.gat_forward(X[all_nodes].double(), params, edges)[loc[t]]
            want.append(ref)
        ref = torch.cat(want)
        top2 = ref.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) > 1e-4
        assert int(sure.sum()) >= 0.99 * idx.numel()
        assert torch.equal(pred.cpu()[sure], ref.argmax(1)[sure])
        assert abs(acc - float((pred.cpu() == y[idx]).float().mean())) < 1e-6


def test_device_graph_on_the_large_path_is_refused():
    _need_gpu()
    from grapes_amd import full_graph
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GAT
    n, F, C, indptr, indices, X, y, _ = _cora_like()
    g = DeviceGraph.from_csr(indptr, indices)
    old = full_graph.LARGE_NNZ
    full_graph.LARGE_NNZ = 1                          # (every graph then counts as one of 2^31 or more entries)
    try:
        with pytest.raises(ValueError, match="2\\^31"):
            GAT(F, [8, C]).cuda()(X.cuda(), g)
    finally:
        full_graph.LARGE_NNZ = old


def test_cli_trains_a_gat_classifier():
    _need_gpu()
    import re
    r = subprocess.run([sys.executable, "-m", "grapes_amd.main", "--dataset", "cora", "--classifier", "gat", "--max_epochs", "2",
                        "--runs", "1", "--eval_frequency", "1"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    losses = [(float(a), float(b)) for a, b in re.findall(r"loss_gfn=([-\w.+]+), loss_c=([-\w.+]+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(v) for p in losses for v in p)
    assert losses[1][1] < losses[0][1]
    assert "test_accuracy=" in r.stdout


def test_full_batch_cli_trains_a_gat_classifier(capsys):
    _need_gpu()
    import re
    from grapes_amd import full_batch
    f1 = full_batch.main(["--dataset", "cora", "--classifier", "gat", "--max_epochs", "3", "--runs", "1", "--eval_frequency", "2",
                          "--hidden_dim", "32", "--seed", "1", "--lr_gc", "0.01"])
    out = capsys.readouterr().out
    losses = [float(v) for v in re.findall(r"epoch \d+: loss_c=([-\w.+]+)", out)]
    assert 0.0 <= f1 <= 1.0 and len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0]
