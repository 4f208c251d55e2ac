"""The GATv2 classifier (PyG's GATv2Conv: multi-head dynamic attention) on the MI355X against the fp64 oracle of tests/gatv2_oracle.py.

Tolerances are the project's: activations max|a − ref| / max(1, max|ref|) <= 1e-5, gradients the same measure at 1e-4.
GATv2 has one LeakyReLU kink per edge AND channel, so the single-layer tests keep every z = x_l[j] + x_r[i] off it by
construction (gatv2_oracle.quantised_layer: every z is an odd multiple of 1/128, exact in fp32), and each test asserts
min|z| >= 1/128 on the ORACLE before it compares; with a fused ReLU it also asserts that no pre-activation of the oracle lies
within 1e-5 of zero.  The graph has 400 nodes, a hub target of in-degree >= 700 (11 or more work items of 64 entries) and a hub
source of out-degree >= 300, so the long-row chunk and combine kernels run on both CSRs in every test."""
import numpy as np
import pytest
import torch

from tests import gatv2_oracle as O

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4
N, HUB_T, HUB_S = 400, 17, 23
GRAD_NAMES = ("dX", "dW_l", "db_l", "dW_r", "db_r", "datt", "db")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _graph(seed, n=N, hub_in=720, hub_out=330):
    base = O.random_graph(n, seed=seed, mean_deg=6, hub=HUB_T, hub_deg=hub_in, n_dup=40, n_loops=25, n_isolated=8)
    rng = np.random.default_rng(seed + 1000)
    out_edges = np.stack([np.full(hub_out, HUB_S), rng.integers(0, n - 8, hub_out)])          # the hub as source
    return np.concatenate([base, out_edges], axis=1).astype(np.int64)


def _degrees(ei, n=N):
    keep = ei[0] != ei[1]
    return np.bincount(ei[1][keep], minlength=n), np.bincount(ei[0][keep], minlength=n)


def _conv(fi, H, C, concat, share, seed, slope=0.2):
    """A GATv2Conv with the quantised transform of gatv2_oracle.quantised_layer, its own att and a non-zero output bias, and the
    matching quantised input x."""
    from grapes_amd.modules.gcn import GATv2Conv
    torch.manual_seed(seed)
    conv = GATv2Conv(fi, C, heads=H, concat=concat, share_weights=share, negative_slope=slope)
    x, (W_l, b_l, W_r, b_r) = O.quantised_layer(N, fi, H, C, seed=seed + 1, share=share)
    with torch.no_grad():
        conv.lin_l.weight.copy_(W_l); conv.lin_l.bias.copy_(b_l)
        if not share:
            conv.lin_r.weight.copy_(W_r); conv.lin_r.bias.copy_(b_r)
        conv.bias.uniform_(-0.1, 0.1)              # (PyG initialises it to zero; a non-zero one exercises c = G . (out - b))
    return conv, x


def _inputs(fi, H, C, concat, share, seed, slope=0.2):
    ei = _graph(seed)
    conv, x = _conv(fi, H, C, concat, share, seed + 200, slope)
    G = torch.randn(N, H * C if concat else C, generator=torch.Generator().manual_seed(seed + 100))
    return ei, x, G, conv


def _leaves(conv):
    return [conv.lin_l.weight, conv.lin_l.bias] + ([] if conv.share_weights else [conv.lin_r.weight, conv.lin_r.bias]) + \
           [conv.att, conv.bias]


def _run(conv, x, ei_dev, G, relu=False):
    """One forward and backward on the device: dict(out, dX, dW_l, db_l, [dW_r, db_r,] datt, db)."""
    xd = x.detach().clone().requires_grad_(True)
    out = conv(xd, ei_dev, relu=relu)
    grads = torch.autograd.grad(out, [xd] + _leaves(conv), G)
    names = [k for k in GRAD_NAMES if not (conv.share_weights and k in ("dW_r", "db_r"))]
    got = dict(zip(names, (g.detach() for g in grads)))
    got["out"] = out.detach()
    return got


def _oracle(conv, x, ei, relu=False):
    return O.gatv2_conv(x.double(), *O.layer_params(conv), ei, conv.heads, conv.concat, conv.negative_slope, relu=relu, full=True)


def _compare(got, x, G, conv, ei, relu=False):
    r = _oracle(conv, x, ei, relu)
    gr = O.gatv2_conv_grads(x.double(), *O.layer_params(conv), ei, G.double(), conv.heads, conv.concat, conv.negative_slope, relu=relu)
    errs = {"out": O.rel_err(got["out"].cpu(), r["out"])}
    for k in GRAD_NAMES:
        if gr[k] is not None:
            errs[k] = O.rel_err(got[k].cpu().reshape(gr[k].shape), gr[k])
    print(f"relu {relu}: errors vs fp64 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    for t in got.values():
        assert torch.isfinite(t).all()
    assert errs["out"] <= ACT_TOL, errs
    for k, v in errs.items():
        assert k == "out" or v <= GRAD_TOL, errs
    return errs


def _check_off_kinks(conv, x, ei, relu_too=True):
    """The oracle's own values: the hub degrees, min|z| >= 1/128 and (for the fused ReLU) no pre-activation within 1e-5 of zero."""
    r = _oracle(conv, x, ei)
    indeg, outdeg = _degrees(ei)
    zmin, pmin = float(r["z"].abs().min()), float(r["pre"].abs().min())
    print(f"edges {r['src'].numel()}, hub in-degree {int(indeg[HUB_T])}, hub out-degree {int(outdeg[HUB_S])}, isolated "
          f"{int(((indeg == 0) & (outdeg == 0)).sum())}, min|z| {zmin}, min|pre| {pmin:.2e}, max|e| {float(r['e'].abs().max()):.1f}")
    assert int(indeg[HUB_T]) >= 700 and int(outdeg[HUB_S]) >= 300
    assert zmin >= 1.0 / 128
    if relu_too:
        assert pmin > 1e-5
    return r


# (in, H, C, concat, share, seed) — the seeds are chosen on the CPU so that the oracle's pre-activations clear the ReLU's kink:
# scalar path; scalar, odd C, head mean; two float4 lanes per head, H not a power of two; shared
# weights; F = 256 <4, 64, 1>; head mean at F = 256; F = 512 <4, 64, 4>; one float4 per head
_CASES = [(16, 1, 5, True, False, 1), (12, 3, 7, False, False, 2), (24, 6, 8, True, False, 3), (24, 4, 16, True, True, 4),
          (20, 8, 32, True, False, 9), (32, 2, 128, False, False, 6), (32, 8, 64, True, False, 11), (16, 16, 4, True, False, 10)]


@pytest.mark.parametrize("fi,H,C,concat,share,seed", _CASES)
def test_gatv2conv_forward_backward_match_oracle(fi, H, C, concat, share, seed):
    _need_gpu()
    from grapes_amd.modules.gcn import prepare_edges
    ei, x, G, conv = _inputs(fi, H, C, concat, share, seed)
    _check_off_kinks(conv, x, ei)
    conv = conv.cuda()
    prep = prepare_edges(torch.from_numpy(ei).cuda(), N)
    assert int(prep.n_items_t.item()) >= 11 and int(prep.n_items_s.item()) >= 5          # the long-row kernels have work
    for relu in (False, True):
        _compare(_run(conv, x.cuda(), prep, G.cuda(), relu=relu), x, G, conv, ei, relu=relu)
    assert prep.status is None or int(prep.status.item()) == 0


def test_softmax_is_stable_at_large_scores():
    _need_gpu()
    ei, x, G, conv = _inputs(24, 4, 16, True, False, 21)
    r = _oracle(conv, x, ei)
    with torch.no_grad():
        conv.att.mul_(80.0 / float(r["e"].abs().max()))
    r = _check_off_kinks(conv, x, ei, relu_too=False)
    assert float(r["e"].abs().max()) >= 79.0
    conv = conv.cuda()
    _compare(_run(conv, x.cuda(), torch.from_numpy(ei).cuda(), G.cuda()), x, G, conv, ei)


@pytest.mark.parametrize("H,C,concat", [(6, 8, True), (3, 7, False)])
def test_negative_slope_is_a_runtime_argument(H, C, concat):
    _need_gpu()
    ei, x, G, conv = _inputs(24, H, C, concat, False, 31, slope=0.05)
    assert conv.negative_slope == 0.05
    _check_off_kinks(conv, x, ei, relu_too=False)
    at_default = O.gatv2_conv(x.double(), *O.layer_params(conv), ei, H, concat, 0.2)
    assert O.rel_err(_oracle(conv, x, ei)["out"], at_default) > 1e-3          # (the slope matters at these inputs)
    conv = conv.cuda()
    _compare(_run(conv, x.cuda(), torch.from_numpy(ei).cuda(), G.cuda()), x, G, conv, ei)


@pytest.mark.parametrize("fi,H,C,concat,share", [(20, 8, 32, True, False), (12, 3, 7, False, True)])
def test_two_runs_and_a_captured_replay_are_bit_identical(fi, H, C, concat, share):
    _need_gpu()
    from grapes_amd.modules.gcn import prepare_edges
    ei, x, G, conv = _inputs(fi, H, C, concat, share, 41)
    conv = conv.cuda()
    xd, Gd = x.cuda(), G.cuda()
    prep = prepare_edges(torch.from_numpy(ei).cuda(), N)            # (the graph build is outside the capture)
    a = _run(conv, xd, prep, Gd, relu=True)
    b = _run(conv, xd, prep, Gd, relu=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    eager = {k: t.clone() for k, t in a.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _run(conv, xd, prep, Gd, relu=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _run(conv, xd, prep, Gd, relu=True)
    for t in captured.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], captured[k]), k
    assert prep.status is None or int(prep.status.item()) == 0


@pytest.mark.parametrize("H,C,concat", [(4, 16, True), (3, 7, False)])
def test_device_row_count_below_the_allocated_rows(H, C, concat):
    """The entry points themselves with d_n = m < n: x = [x_l | x_r] and one-hot weights make the oracle's x_l, x_r the kernels'
    operands, so dx_l and dx_r are compared directly; rows past d_n of every output keep their mark."""
    _need_gpu()
    from grapes_amd import ops
    n, m, F = N, 330, H * C
    W = F if concat else C
    ei = _graph(51)
    em = ei[:, (ei[0] < m) & (ei[1] < m)]
    indeg, outdeg = _degrees(em, m)
    assert indeg[HUB_T] > 64 * 8 and outdeg[HUB_S] > 64 * 3
    g = torch.Generator().manual_seed(52)
    x_l = torch.randint(-128, 129, (n, F), generator=g).float() / 64
    x_r = torch.randint(-128, 129, (n, F), generator=g).float() / 64 + 1.0 / 128
    att = (torch.rand(F, generator=g) * 2 - 1) * 0.4
    b = (torch.rand(W, generator=g) * 2 - 1) * 0.1
    G = torch.randn(n, W, generator=g)
    eye, zero = torch.eye(F, dtype=O.F64), torch.zeros(F, F, dtype=O.F64)
    args = (torch.cat([x_l, x_r], 1)[:m].double(), torch.cat([eye, zero], 1), torch.zeros(F, dtype=O.F64), torch.cat([zero, eye], 1),
            torch.zeros(F, dtype=O.F64), att.double(), b.double(), em)
    ref = O.gatv2_conv(*args, H, concat, full=True)
    gr = O.gatv2_conv_grads(*args, G[:m].double(), H, concat)
    assert float(ref["z"].abs().min()) >= 1.0 / 128
    d_n = torch.tensor([m], dtype=torch.int32, device="cuda")
    srcm, dstm = (torch.from_numpy(em[k]).int().cuda().contiguous() for k in (0, 1))
    prep = ops.PreparedGraph(srcm, dstm, n, d_n=d_n)
    assert int(prep.n_items_t.item()) > 8 and int(prep.n_items_s.item()) > 3
    L, P_, mark = ops.lib(), ops._p, 12345.0
    xl_d, xr_d, att_d, b_d, G_d = x_l.cuda(), x_r.cuda(), att.cuda(), b.cuda(), G.cuda()
    out, agg = torch.full((n, W), mark, device="cuda"), torch.full((n, F), mark, device="cuda")
    row_ms = torch.full((n, H, 2), mark, device="cuda")
    dxl, dxr = torch.full((n, F), mark, device="cuda"), torch.full((n, F), mark, device="cuda")
    datt, db = torch.empty(F, device="cuda"), torch.empty(W, device="cuda")
    ws = ops._ws(max(L.grapes_gatv2_aggregate_workspace_bytes(prep.item_cap, F, H),
                     L.grapes_gatv2_aggregate_bwd_workspace_bytes(n, prep.item_cap, F, H)), "cuda")
    cc = 1 if concat else 0
    assert L.grapes_gatv2_aggregate_fwd(P_(xl_d), P_(xr_d), P_(att_d), P_(prep.rowptr_t), P_(prep.csr_src), P_(b_d), P_(out),
                                        None if concat else P_(agg), P_(row_ms), n, P_(d_n), H, C, cc, 0.2, 0, P_(prep.items_t),
                                        P_(prep.n_items_t), prep.item_cap, P_(ws), None, ops._stream()) == 0
    assert L.grapes_gatv2_aggregate_bwd(P_(G_d), P_(out), None if concat else P_(agg), P_(b_d), 0, P_(xl_d), P_(xr_d), P_(att_d),
                                        P_(row_ms), P_(prep.rowptr_t), P_(prep.csr_src), P_(prep.rowptr_s), P_(prep.csr_dst),
                                        P_(dxl), P_(dxr), P_(datt), P_(db), n, P_(d_n), H, C, cc, 0.2, P_(prep.items_t),
                                        P_(prep.n_items_t), P_(prep.items_s), P_(prep.n_items_s), prep.item_cap, P_(ws), None,
                                        ops._stream()) == 0
    torch.cuda.synchronize()
    errs = {"out": O.rel_err(out[:m].cpu(), ref["out"]), "dx_l": O.rel_err(dxl[:m].cpu(), gr["dx_l"]),
            "dx_r": O.rel_err(dxr[:m].cpu(), gr["dx_r"]), "datt": O.rel_err(datt.cpu(), gr["datt"].reshape(-1)),
            "db": O.rel_err(db.cpu(), gr["db"])}
    hub = {"out": O.rel_err(out[HUB_T].cpu(), ref["out"][HUB_T]), "dx_r": O.rel_err(dxr[HUB_T].cpu(), gr["dx_r"][HUB_T]),
           "dx_l": O.rel_err(dxl[HUB_S].cpu(), gr["dx_l"][HUB_S])}
    print("d_n rows:", {k: f"{v:.2e}" for k, v in errs.items()}, "hub rows:", {k: f"{v:.2e}" for k, v in hub.items()})
    assert errs.pop("out") <= ACT_TOL and hub.pop("out") <= ACT_TOL
    assert all(v <= GRAD_TOL for v in errs.values()) and all(v <= GRAD_TOL for v in hub.values()), (errs, hub)
    for t in (out, row_ms, dxl, dxr) + (() if concat else (agg,)):
        assert bool((t[m:] == mark).all())                               # rows past d_n are untouched


def _two_layer(seed=61, n=200, fi=24, C=7, heads=4):
    """(model, x, y, [e0, e1]): GATv2(fi, [16, C], heads) with a quantised first transform, over a layer-wise edge list."""
    from grapes_amd.modules.gcn import GATv2
    e0 = O.random_graph(n, seed=seed, mean_deg=5, hub=3, hub_deg=150, n_dup=20, n_loops=10, n_isolated=5)
    e1 = O.random_graph(n, seed=seed + 1, mean_deg=5, hub=9, hub_deg=90, n_dup=20, n_loops=10, n_isolated=5)
    torch.manual_seed(seed + 2)
    model = GATv2(fi, [16, C], heads=heads)
    x, (W_l, b_l, W_r, b_r) = O.quantised_layer(n, fi, heads, 16, seed=seed + 3)
    first = model.gat_layers[0]
    with torch.no_grad():
        first.lin_l.weight.copy_(W_l); first.lin_l.bias.copy_(b_l); first.lin_r.weight.copy_(W_r); first.lin_r.bias.copy_(b_r)
        for layer in model.gat_layers:
            layer.bias.uniform_(-0.1, 0.1)
        model.gat_layers[1].lin_l.bias.uniform_(-0.1, 0.1); model.gat_layers[1].lin_r.bias.uniform_(-0.1, 0.1)
    y = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(seed + 4))
    return model, x, y, [e0, e1]


def test_two_layer_gatv2_on_prepared_graphs_matches_oracle():
    _need_gpu()
    from grapes_amd import ops
    heads, n = 4, 200
    model, x, y, edges = _two_layer()
    params = [O.layer_params(l) for l in model.gat_layers]
    leaves = [[t.clone().requires_grad_(True) for t in p] for p in params]
    ref, hidden, last = O.gatv2_forward(x.double(), leaves, edges, heads, full=True)
    near = hidden[0]["pre"].detach().abs() < 1e-5
    units = near.any(0)
    z1, z2 = float(hidden[0]["z"].detach().abs().min()), float(last["z"].detach().abs().min())
    print(f"hidden pre-activations within 1e-5 of zero: {int(near.sum())} of {near.numel()} ({int(units.sum())} of {units.numel()} "
          f"units); min|z| layer 1 {z1}, layer 2 {z2:.2e} over {last['z'].numel()} values")
    assert int(near.sum()) <= 0.01 * near.numel()                  # the cap: at most 1 % of the hidden values
    assert z1 >= 1.0 / 128 and z2 > 1e-5                           # layer 1 by construction, layer 2 for the committed seed
    loss = torch.nn.functional.cross_entropy(ref, y)
    rg = torch.autograd.grad(loss, [t for p in leaves for t in p])
    model = model.cuda()
    preps = [ops.PreparedGraph(torch.from_numpy(e[0]).int().cuda().contiguous(), torch.from_numpy(e[1]).int().cuda().contiguous(), n)
             for e in edges]
    logits = model(x.cuda(), preps)
    assert torch.is_tensor(logits) and logits.shape == (n, 7)       # logits only, no (logits, memory) pair
    err = O.rel_err(logits.detach().cpu(), ref.detach())
    print(f"logits rel err {err:.2e}")
    assert err <= ACT_TOL
    torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
    keep = ~units
    for li, layer in enumerate(model.gat_layers):
        for k, t in enumerate((layer.lin_l.weight, layer.lin_l.bias, layer.lin_r.weight, layer.lin_r.bias, layer.att, layer.bias)):
            got, want = t.grad.detach().cpu().double(), rg[6 * li + k]
            if li == 0:                                              # units next to the ReLU kink are left out (see the module docstring)
                got, want = got.reshape(units.numel(), -1)[keep], want.reshape(units.numel(), -1)[keep]
            e = float((got.reshape(want.shape) - want).abs().max()) / max(1.0, float(want.abs().max()))
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


def test_grapes_trainer_steps_a_gatv2_classifier():
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GATv2, GCN
    from grapes_amd.step import GrapesTrainer
    n, F, C, indptr, indices, X, y, rng = _cora_like()
    hops, K, B, H, heads = 2, 16, 64, 16, 4
    torch.manual_seed(1)
    c, gf, z = GATv2(F, [H, C], heads=heads).cuda(), GCN(F + hops + 1, [H, 1]).cuda(), GCN(F, [H, 1]).cuda()
    tr = GrapesTrainer(DeviceGraph.from_csr(indptr, indices), X.cuda(), y.cuda(), c, gf, z, sampling_hops=hops, num_samples=K,
                       loss_coef=10.0, optimizer_c=torch.optim.Adam(c.parameters(), lr=1e-2), optimizer_gf=None, philox_seed=7)
    targets = torch.from_numpy(np.random.default_rng(5).permutation(n)[:B].astype(np.int64))
    params = [O.layer_params(l) for l in c.gat_layers]
    out = tr.step(targets, trace=True)
    assert np.isfinite(float(out["loss_c"]))
    for p in c.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0
    all_nodes = out["all_nodes"].cpu().long()
    edges = [e.cpu().numpy().astype(np.int64) for e in out["edge_indices"]]
    ref = O.gatv2_forward(X[all_nodes].double(), params, edges, heads)
    err = O.rel_err(out["logits"].cpu(), ref)
    ref_loss = float(torch.nn.functional.cross_entropy(ref[out["local_target_ids"].cpu().long()], y[targets]))
    print(f"{all_nodes.numel()} nodes, logits rel err {err:.2e}, loss_c {float(out['loss_c']):.6f} vs {ref_loss:.6f}")
    assert err <= ACT_TOL and abs(float(out["loss_c"]) - ref_loss) <= ACT_TOL * max(1.0, abs(ref_loss))


def test_graphed_trainer_refuses_a_gatv2_classifier():
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GATv2, GCN
    from grapes_amd.step_graph import GraphedTrainer
    n, F, C, indptr, indices, X, y, _ = _cora_like()
    with pytest.raises(NotImplementedError, match="GCN classifier"):
        GraphedTrainer(DeviceGraph.from_csr(indptr, indices), X.cuda(), y.cuda(), GATv2(F, [16, C], heads=2).cuda(),
                       GCN(F + 3, [16, 1]).cuda(), GCN(F, [16, 1]).cuda(), batch_size=32)


@pytest.mark.parametrize("full_batch", [True, False])
def test_evaluate_with_gatv2_classifier_matches_oracle(full_batch, monkeypatch):
    _need_gpu()
    from types import SimpleNamespace
    from grapes_amd import eval as E, step_graph
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GATv2, GCN
    n, F, C, indptr, indices, X, y, rng = _cora_like(seed=9)
    hops, K, H, heads = 2, 100000, 16, 2
    torch.manual_seed(3)
    c, gf = GATv2(F, [H, C], heads=heads).cuda(), GCN(F + hops + 1, [H, 1]).cuda()
    g = DeviceGraph.from_csr(indptr, indices)
    mask = torch.zeros(n, dtype=torch.bool); mask[rng.permutation(n)[:256]] = True
    idx = mask.nonzero().squeeze(1)
    args = SimpleNamespace(sampling_hops=hops, num_samples=K, use_indicators=True)
    data = SimpleNamespace(x=X.cuda(), y=y.cuda())

    def no_capture(*a, **k):
        raise AssertionError("evaluate built a GraphedTrainer for a GATv2 classifier")
    monkeypatch.setattr(step_graph, "GraphedTrainer", no_capture)
    loader = [(idx[o:o + 64],) for o in range(0, idx.numel(), 64)]          # four full batches: a GCN would be captured
    acc, f1, pred = E.evaluate(c, gf, data, args, g, mask=mask.cuda(), loader=loader, full_batch=full_batch, return_predictions=True)
    assert acc == f1 and pred.numel() == idx.numel()
    params = [O.layer_params(l) for l in c.gat_layers]
    if full_batch:
        rows = np.repeat(np.arange(n), np.diff(indptr))
        ref = O.gatv2_forward(X.double(), params, np.stack([rows, np.asarray(indices, dtype=np.int64)]), heads)[idx]
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
            want.append(O.gatv2_forward(X[all_nodes].double(), params, edges, heads)[loc[t]])
        ref = torch.cat(want)
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-4                           # (an argmax between two near-equal logits is not a mismatch)
    assert int(sure.sum()) >= 0.99 * idx.numel()
    assert torch.equal(pred.cpu()[sure], ref.argmax(1)[sure])
    assert abs(acc - float((pred.cpu() == y[idx]).float().mean())) < 1e-6


def test_full_batch_cli_trains_a_gatv2_classifier(capsys):
    _need_gpu()
    import re
    from grapes_amd import full_batch
    f1 = full_batch.main(["--dataset", "cora", "--classifier", "gatv2", "--gat_heads", "4", "--max_epochs", "3", "--runs", "1",
                          "--eval_frequency", "2", "--hidden_dim", "16", "--seed", "1", "--lr_gc", "0.01"])
    out = capsys.readouterr().out
    losses = [float(v) for v in re.findall(r"epoch \d+: loss_c=([-\w.+]+)", out)]
    assert 0.0 <= f1 <= 1.0 and len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0]
