"""The PNA classifier (reference modules/gcn.py:120-149) on the MI355X against the fp64 oracle of tests/pna_oracle.py.

Tolerances are the project's: activations max|a − ref| / max(1, max|ref|) <= 1e-5, gradients the same measure at 1e-4; the
single-conv inputs are those tests/test_pna_cpu.py shows to be reachable by an fp32 CPU evaluation of the same formulas.
Kinks (all judged on the ORACLE's values, each capped at 1 % of the entries): ReLU pre-activations within 1e-5 of zero; (row, feature)
entries whose two most extreme messages come from different source nodes and differ by less than 1e-5 max(1, |m|); entries with
0 < var < 1e-5.  The single-conv tests carry no upstream gradient on a ReLU kink or on a row that owns an aggregation kink
(pna_oracle.kink_free_gradient: a choice of input); the tests of the aggregation entry point cut the gradient entry by entry, so
the hub row's backward is checked there."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pna_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_TOL, GRAD_TOL = 1e-5, 1e-4
N = O.N
AGG, SCAL = O.AGGREGATORS, O.SCALERS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _conv(F, C, P, deg, aggregators=AGG, scalers=SCAL):
    from grapes_amd.modules.gcn import PNAConv
    conv = PNAConv(F, C, aggregators, scalers, deg)
    with torch.no_grad():
        for t, v in zip((conv.pre_nn.weight, conv.pre_nn.bias, conv.post_nn.weight, conv.post_nn.bias, conv.lin.weight, conv.lin.bias), P):
            t.copy_(v)
    return conv.cuda()


def _params(conv):
    return [conv.pre_nn.weight, conv.pre_nn.bias, conv.post_nn.weight, conv.post_nn.bias, conv.lin.weight, conv.lin.bias]


def _run(conv, x, edges, G, relu):
    """One forward and backward on the device: (out, dx, dWpre, dbpre, dWpost, dbpost, dWlin, dblin)."""
    xd = x.detach().clone().requires_grad_(True)
    out = conv(xd, edges, relu=relu)
    grads = torch.autograd.grad(out, [xd] + _params(conv), G)
    return (out.detach(),) + tuple(g.detach() for g in grads)


def _oracle(ei, x, P, G, avg_log, avg_lin, relu, aggregators=AGG, scalers=SCAL):
    Pd = tuple(t.double() for t in P)
    ref = O.pna_conv(x.double(), Pd, ei, aggregators, scalers, avg_log, avg_lin, relu=relu, full=True)
    G, near, bad, rows = O.kink_free_gradient(G, ref, x.shape[0], relu)
    assert near <= 0.01 * ref["pre"].numel() and bad <= 0.01 * x.numel()          # the caps, on the oracle's values
    gr = O.pna_conv_grads(x.double(), Pd, ei, aggregators, scalers, avg_log, avg_lin, G.double(), relu=relu)
    return ref, gr, G, (near, bad, rows)


def _compare(got, ref, gr):
    errs = {"out": O.rel_err(got[0].cpu(), ref["out"])}
    for k, t in zip(O.GRAD_NAMES, got[1:]):
        errs[k] = O.rel_err(t.cpu(), gr[k])
    print("errors vs fp64 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(torch.isfinite(t).all() for t in got)
    assert errs["out"] <= ACT_TOL, errs
    for k in O.GRAD_NAMES:
        assert errs[k] <= GRAD_TOL, errs
    return errs


@pytest.mark.parametrize("case", range(len(O.CONV_CASES)))
def test_pnaconv_forward_backward_match_oracle(case):
    _need_gpu()
    F, C, relu = O.CONV_CASES[case]
    ei, x, P, G, avg_log, avg_lin = O.conv_case(F, C, seed=case + 1)
    hub, dup, loops, isolated = O.graph_properties(ei)
    assert hub > 2000 and dup >= 60 and loops >= 40 and isolated >= 25
    ref, gr, G, (near, bad, rows) = _oracle(ei, x, P, G, avg_log, avg_lin, relu)
    print(f"F {F} C {C} relu {relu}: edges {ei.shape[1]}, hub in-degree {hub}, duplicates {dup}, stored loops {loops}, isolated "
          f"{isolated}; pre-activations within 1e-5 of zero {near}, kinked aggregate entries {bad} in {rows} rows")
    conv = _conv(F, C, P, O.degree_histogram(ei, N))
    assert abs(conv.avg_deg["log"] - avg_log) < 1e-12
    got = _run(conv, x.cuda(), torch.from_numpy(ei).cuda(), G.cuda(), relu)
    _compare(got, ref, gr)


def test_every_aggregator_and_scaler_matches_oracle():
    _need_gpu()
    aggregators, scalers = ["sum", "var", "max", "mean", "std", "min"], ["inverse_linear", "linear", "identity", "attenuation", "amplification"]
    F, C = 20, 9
    ei, x, P, G, avg_log, avg_lin = O.conv_case(F, C, seed=91, aggregators=aggregators, scalers=scalers)
    ref, gr, G, _ = _oracle(ei, x, P, G, avg_log, avg_lin, True, aggregators, scalers)
    conv = _conv(F, C, P, O.degree_histogram(ei, N), aggregators, scalers)
    _compare(_run(conv, x.cuda(), torch.from_numpy(ei).cuda(), G.cuda(), True), ref, gr)


def _prep(ei, n, d_n=None):
    from grapes_amd import ops
    src, dst = (torch.from_numpy(ei[k]).int().cuda().contiguous() for k in (0, 1))
    return ops.gcn2_attach_loops(ops.PreparedGraph(src, dst, n, d_n=d_n), src, dst)


def _aggregation_case(ei, n, F, seed):
    """fp32 x, [a | b], dz and the fp64 oracle of the aggregation alone with dz cut entry by entry at the kinks."""
    g = torch.Generator().manual_seed(seed)
    x, ab = torch.randn(n, F, generator=g), torch.randn(n, 2 * F, generator=g)
    avg_log, avg_lin = O.degree_averages(O.degree_histogram(ei, n))
    a, b = (ab[:, :F].double().requires_grad_(True), ab[:, F:].double().requires_grad_(True))
    r = O.pna_aggregate_ab(x.double(), a, b, ei, AGG, SCAL, avg_log, avg_lin)
    kinks = O.aggregate_kinks(dict(r, agg={k: v for k, v in r["agg"].items()}), n)
    bad = sum(int(v.sum()) for v in kinks.values())
    assert bad <= 0.01 * n * F
    K = len(AGG)
    dz = torch.randn(n, (1 + K * len(SCAL)) * F, generator=g)
    for s in range(len(SCAL)):
        for k, name in enumerate(AGG):
            kind = {"max": "max", "min": "min", "std": "var", "var": "var"}.get(name)
            if kind is not None:
                blk = dz[:, (1 + s * K + k) * F:(2 + s * K + k) * F]
                blk[kinks[kind]] = 0.0
    da, db = torch.autograd.grad(r["z"], [a, b], dz.double())
    return x, ab, dz, r, da, db, (avg_log, avg_lin), bad


@pytest.mark.parametrize("F", [5, 64, 100])
def test_aggregation_alone_element_wise_on_short_rows_and_the_hub(F):
    """grapes_pna_aggregate_fwd / _bwd against the oracle on the rows of in-degree 0, 1 and 2 and on the hub row, each group
    measured on its own (the hub's scale does not hide a short row's error); the saved statistics of b as well."""
    _need_gpu()
    from grapes_amd import ops
    ei = O.gpu_graph(81)
    x, ab, dz, r, da, db, (avg_log, avg_lin), bad = _aggregation_case(ei, N, F, seed=82)
    cfg = ops.PNAConfig(AGG, SCAL, avg_log, avg_lin)
    prep = _prep(ei, N)
    z, stats = ops.pna_aggregate_fwd(x.cuda(), ab.cuda(), prep, cfg)
    dab = ops.pna_aggregate_bwd(dz.cuda(), ab.cuda(), stats, prep, cfg)
    d = r["d"]
    assert int(d[O.HUB]) > 2000
    groups = {"d=0": d == 0, "d=1": d == 1, "d=2": d == 2, "hub": torch.arange(N) == O.HUB, "all": torch.ones(N, dtype=torch.bool)}
    zc, dabc, st = z.cpu(), dab.cpu(), stats.cpu()
    for name, rows in groups.items():
        assert int(rows.sum()) > 0, name
        ez = O.rel_err(zc[rows], r["z"].detach()[rows])
        eda, edb = O.rel_err(dabc[rows, :F], da[rows]), O.rel_err(dabc[rows, F:], db[rows])
        print(f"F {F} rows {name} ({int(rows.sum())}): z {ez:.2e}, da {eda:.2e}, db {edb:.2e}")
        assert ez <= ACT_TOL and eda <= GRAD_TOL and edb <= GRAD_TOL, name
    empty = d == 0
    k0 = zc[empty][:, F:].reshape(int(empty.sum()), len(SCAL), len(AGG), F)
    assert bool((k0[:, :, :3] == 0).all())                                        # mean, min, max of an empty row: exactly 0
    want_std = np.sqrt(np.float32(1e-5)) * O.scaler_values(d[empty].float(), SCAL, avg_log, avg_lin)
    assert O.rel_err(k0[:, :, 3], want_std[:, :, None].expand(-1, -1, F)) <= 1e-7
    one = d == 1
    assert bool((st[one][:, 3] == 0).all())                                       # the variance of one message: exactly 0
    has = d > 0
    b64 = ab[:, F:].double()
    mean_b = torch.zeros(N, F, dtype=O.F64).index_add(0, r["dst"], b64[r["src"]]) / d.clamp(min=1)[:, None]
    assert O.rel_err(st[has][:, 0], mean_b[has]) <= ACT_TOL
    assert O.rel_err(st[has][:, 3], r["agg"]["var"].detach()[has]) <= ACT_TOL
    assert bool((zc[:, :F] == x).all())                                           # the copy of x


@pytest.mark.parametrize("F", [64, 47])
def test_long_rows_on_both_csrs_and_device_row_count(F):
    """A hub as target AND as source on a graph large enough for the work-item path (n > 2048): rows longer than GRAPES_LONG_ROW on
    both CSRs (Chan's merge forward, chunk-ordered sums backward); then the same launches with d_n below the allocated rows leave the
    rows past it untouched."""
    _need_gpu()
    from grapes_amd import ops
    n, hub = 2600, 5
    rng = np.random.default_rng(71)
    base = O.random_graph(n, seed=72, mean_deg=4, hub=hub, hub_deg=900, n_dup=20, n_loops=30, n_isolated=10)
    out_edges = np.stack([np.full(700, hub), rng.integers(0, n - 10, 700)])          # the hub as source
    ei = np.concatenate([base, out_edges, np.array([[hub, hub], [hub, hub]]).T.reshape(2, -1)], axis=1).astype(np.int64)
    indeg, outdeg = np.bincount(ei[1][ei[0] != ei[1]], minlength=n), np.bincount(ei[0][ei[0] != ei[1]], minlength=n)
    assert indeg[hub] > 64 * 8 and outdeg[hub] > 64 * 8
    x, ab, dz, r, da, db, (avg_log, avg_lin), bad = _aggregation_case(ei, n, F, seed=73)
    cfg = ops.PNAConfig(AGG, SCAL, avg_log, avg_lin)
    prep = _prep(ei, n)
    assert int(prep.n_items_t.item()) > 8 and int(prep.n_items_s.item()) > 8
    z, stats = ops.pna_aggregate_fwd(x.cuda(), ab.cuda(), prep, cfg)
    dab = ops.pna_aggregate_bwd(dz.cuda(), ab.cuda(), stats, prep, cfg)
    for rows, name in ((torch.arange(n) == hub, "hub"), (torch.ones(n, dtype=torch.bool), "all")):
        ez = O.rel_err(z.cpu()[rows], r["z"].detach()[rows])
        eda, edb = O.rel_err(dab.cpu()[rows, :F], da[rows]), O.rel_err(dab.cpu()[rows, F:], db[rows])
        print(f"F {F} rows {name}: z {ez:.2e}, da {eda:.2e}, db {edb:.2e}")
        assert ez <= ACT_TOL and eda <= GRAD_TOL and edb <= GRAD_TOL
    # d_n < allocated rows: a graph over the first m nodes, buffers of n rows pre-filled with a mark
    m = 2100
    em = ei[:, (ei[0] < m) & (ei[1] < m)]
    d_n = torch.tensor([m], dtype=torch.int32, device="cuda")
    prepm = _prep(em, n, d_n=d_n)
    xm, abm, dzm, rm, dam, dbm, (al, ali), _ = _aggregation_case(em, m, F, seed=74)
    pad = lambda t: torch.cat([t, torch.zeros(n - m, t.shape[1])]).cuda()
    cfgm = ops.PNAConfig(AGG, SCAL, al, ali)
    L, P_, mark = ops.lib(), ops._p, 12345.0
    xd, abd, dzd = pad(xm), pad(abm), pad(dzm)
    zo = torch.full((n, cfgm.blocks * F), mark, device="cuda")
    so = torch.full((n, 6, F), mark, device="cuda")
    dabo = torch.full((n, 2 * F), mark, device="cuda")
    ws = ops._ws(max(L.grapes_pna_aggregate_fwd_workspace_bytes(prepm.item_cap, F), L.grapes_pna_aggregate_bwd_workspace_bytes(n, prepm.item_cap, F)), "cuda")
    assert L.grapes_pna_aggregate_fwd(P_(xd), P_(abd), abd.data_ptr() + 4 * F, 2 * F, P_(prepm.loops), P_(prepm.rowptr_t), P_(prepm.csr_src),
                                      cfgm.n_agg, cfgm.agg_code, cfgm.n_scal, cfgm.scal_code, cfgm.avg_log, cfgm.avg_lin, P_(zo), P_(so), n,
                                      P_(d_n), F, P_(prepm.items_t), P_(prepm.n_items_t), prepm.item_cap, P_(ws), None, ops._stream()) == 0
    assert L.grapes_pna_aggregate_bwd(P_(dzd), abd.data_ptr() + 4 * F, 2 * F, P_(so), P_(prepm.loops), P_(prepm.rowptr_t), P_(prepm.rowptr_s),
                                      P_(prepm.csr_dst), cfgm.n_agg, cfgm.agg_code, cfgm.n_scal, cfgm.scal_code, cfgm.avg_log, cfgm.avg_lin,
                                      P_(dabo), dabo.data_ptr() + 4 * F, 2 * F, n, P_(d_n), F, P_(prepm.items_s), P_(prepm.n_items_s),
                                      prepm.item_cap, P_(ws), None, ops._stream()) == 0
    dxo = torch.full((n, F), 1.0, device="cuda")
    assert L.grapes_pna_add_input_grad(P_(dxo), P_(dzd), cfgm.blocks * F, n, P_(d_n), F, ops._stream()) == 0
    torch.cuda.synchronize()
    assert O.rel_err(zo[:m].cpu(), rm["z"].detach()) <= ACT_TOL
    assert O.rel_err(dabo[:m, :F].cpu(), dam) <= GRAD_TOL and O.rel_err(dabo[:m, F:].cpu(), dbm) <= GRAD_TOL
    assert O.rel_err(dxo[:m].cpu(), 1.0 + dzm[:, :F].double()) <= ACT_TOL
    for t in (zo, so, dabo):
        assert bool((t[m:] == mark).all())                               # rows past d_n are untouched
    assert bool((dxo[m:] == 1.0).all())


def test_prepared_graph_without_loop_counts_is_refused():
    _need_gpu()
    from grapes_amd import ops
    from grapes_amd._lib import GrapesHipError
    ei = O.gpu_graph(62)
    prep = ops.PreparedGraph(torch.from_numpy(ei[0]).int().cuda().contiguous(), torch.from_numpy(ei[1]).int().cuda().contiguous(), N)
    x = torch.randn(N, 8, device="cuda")
    with pytest.raises(GrapesHipError, match="self-loop"):
        ops.pna_aggregate_fwd(x, torch.randn(N, 16, device="cuda"), prep, ops.PNAConfig(AGG, SCAL, 1.0, 1.0))


def test_two_runs_are_bit_identical():
    _need_gpu()
    for case in (2, 0):                                                   # float4 columns at 100, scalar columns at 7; both with ReLU
        F, C, relu = O.CONV_CASES[case]
        ei, x, P, G, _, _ = O.conv_case(F, C, seed=31 + case)
        conv = _conv(F, C, P, O.degree_histogram(ei, N))
        xd, Gd, eid = x.cuda(), G.cuda(), torch.from_numpy(ei).cuda()
        a = _run(conv, xd, eid, Gd, True)
        b = _run(conv, xd, eid, Gd, True)
        for s, t in zip(a, b):
            assert torch.equal(s, t)


def test_captured_forward_backward_replays_bit_identically():
    _need_gpu()
    from grapes_amd.modules.gcn import _layer_graph
    F, C, relu = O.CONV_CASES[4]                                           # 256 wide, ReLU
    ei, x, P, G, _, _ = O.conv_case(F, C, seed=41)
    conv = _conv(F, C, P, O.degree_histogram(ei, N))
    xd, Gd = x.cuda(), G.cuda()
    prep = _layer_graph(torch.from_numpy(ei).cuda(), N, "PNA", loops=True)    # (the graph build and the loop count are outside the capture)
    eager = [t.clone() for t in _run(conv, xd, prep, Gd, True)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _run(conv, xd, prep, Gd, True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _run(conv, xd, prep, Gd, True)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for s, t in zip(eager, captured):
        assert torch.equal(s, t)


def _masks_from(draws, p):
    """The dropout masks the model drew, regenerated from the Philox stream at the recorded (seed, offset): kept iff u >= p."""
    from grapes_amd import ops
    out = []
    for shape, seed, off in draws:
        u = ops.philox_uniform(int(np.prod(shape)), seed, off, "cuda").cpu().double().reshape(shape)
        out.append((u >= p).double() / (1.0 - p))
    return out


def _kink_report(hidden, logits_r, n):
    """The caps on the oracle's values of a model run: hidden ReLU pre-activations near zero and aggregation kinks of every conv."""
    for r in hidden:
        near = r["pre"].detach().abs() < O.KINK
        assert int(near.sum()) <= 0.01 * near.numel()
    for r in hidden + [logits_r]:
        k = O.aggregate_kinks(r, n)
        bad = int((k["max"] | k["min"] | k["var"]).sum())
        print(f"kinked aggregate entries {bad} of {k['max'].numel()}")
        assert bad <= 0.01 * k["max"].numel()


@pytest.mark.parametrize("dropout", [0.0, 0.3])
def test_two_layer_pna_on_layerwise_graphs_matches_oracle(dropout):
    _need_gpu()
    from grapes_amd.modules.gcn import PNA
    e0, e1 = O.gpu_graph(51), O.gpu_graph(52)
    Fin, H, C = 24, 32, 7
    x = torch.randn(N, Fin, generator=torch.Generator().manual_seed(53))
    torch.manual_seed(54)
    model = PNA(Fin, [H, C], AGG, SCAL, O.degree_histogram(e0, N), dropout=dropout)
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
    preps = [_prep(e, N) for e in (e0, e1)]
    logits = model(x.cuda(), preps)
    assert torch.is_tensor(logits) and tuple(logits.shape) == (N, C)     # logits only
    masks = None
    if dropout:
        assert len(draws) == 2                                           # the input and behind the hidden conv
        for dr, shape in zip(draws, [(N, Fin), (N, H)]):
            dr[0] = shape
        masks = _masks_from(draws, dropout)
    leaves, flat = O.param_leaves(params)
    ref, hidden = O.pna_forward(x.double(), leaves, [e0, e1], masks=masks, full=True)
    err = O.rel_err(logits.detach().cpu(), ref.detach())
    print(f"logits rel err {err:.2e}")
    assert err <= ACT_TOL
    # the upstream gradient: random, cut on the rows of the LAST conv that own an aggregation kink (its output is the logits)
    kw = dict(aggregators=AGG, scalers=SCAL, avg_log=params["avg_log"], avg_lin=params["avg_lin"])
    xin = hidden[0]["out"].detach() * (masks[1] if masks else 1.0)
    last = O.pna_conv(xin, params["convs"][1], e0, full=True, **kw)
    _kink_report(hidden, last, N)
    G = torch.randn(N, C, generator=torch.Generator().manual_seed(55)).double()
    G, _, _, _ = O.kink_free_gradient(G, last, N, False)
    rg = torch.autograd.grad(ref, flat, G)
    logits.backward(G.float().cuda())
    names = [k for k, _ in model.named_parameters() if k.startswith("conv.")]
    got = [p for k, p in model.named_parameters() if k.startswith("conv.")]
    assert names == [f"conv.{i}.{m}.{w}" for i in (0, 1) for m in ("pre_nn", "post_nn", "lin") for w in ("weight", "bias")]
    assert model.lins.weight.grad is None                                # lins is kept for the state dict, not applied
    for name, t, want in zip(names, got, rg):
        e = O.rel_err(t.grad.cpu(), want)
        print(f"{name}: grad rel err {e:.2e}")
        assert e <= GRAD_TOL, name
    # (conv.0's gradients pass the hidden conv's own kinks, which cannot be cut from the logits' side: _kink_report caps them, and a
    # flip needs a gap at the fp32 spacing, a hundredth of the kink width)


def _cora_like(seed=3):
    from grapes_amd import synth
    n, F, C = 2708, 32, 7
    indptr, indices = synth.synth_csr_numpy(n, 4.0, 170, seed=seed)
    rng = np.random.default_rng(seed + 1)
    X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, C, n))
    return n, F, C, indptr, indices, X, y, rng


def _pna(F, H, C, g, dropout=0.0):
    from grapes_amd.modules.gcn import PNA, pna_degree_histogram
    return PNA(F, [H, C], AGG, SCAL, pna_degree_histogram(g), dropout=dropout)


def test_grapes_trainer_with_pna_classifier_matches_oracle():
    """Training steps of the eager trainer: logits and loss of every step, and the parameter gradients of a step without an
    optimiser, against the oracle on the traced subgraphs; the sampler does not see the classifier."""
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    from grapes_amd.step import GrapesTrainer
    n, F, C, indptr, indices, X, y, rng = _cora_like()
    hops, K, B, H = 2, 16, 64, 32
    torch.manual_seed(0)
    gf0, z0 = GCN(F + hops + 1, [H, 1]), GCN(F, [H, 1])
    kept = {}
    for kind in ("pna", "gcn"):
        g = DeviceGraph.from_csr(indptr, indices)
        torch.manual_seed(1)
        c = (_pna(F, H, C, g) if kind == "pna" else GCN(F, [H, C])).cuda()
        gf, z = GCN(F + hops + 1, [H, 1]).cuda(), GCN(F, [H, 1]).cuda()
        gf.load_state_dict(gf0.state_dict()); z.load_state_dict(z0.state_dict())
        tr = GrapesTrainer(g, X.cuda(), y.cuda(), c, gf, z, sampling_hops=hops, num_samples=K, loss_coef=10.0, optimizer_c=None,
                           optimizer_gf=None, philox_seed=7)
        kept[kind] = []
        targets_rng = np.random.default_rng(5)
        for step in range(2):
            targets = torch.from_numpy(targets_rng.permutation(n)[:B].astype(np.int64))
            params = O.model_params(c) if kind == "pna" else None
            for p_ in c.parameters():
                p_.grad = None
            out = tr.step(targets, trace=True)
            kept[kind].append([h["kept"].cpu().numpy().astype(np.int64) for h in out["hops"]])
            if kind != "pna":
                continue
            all_nodes = out["all_nodes"].cpu().long()
            edges = [e.cpu().numpy().astype(np.int64) for e in out["edge_indices"]]
            leaves, flat = O.param_leaves(params)
            ref, hidden = O.pna_forward(X[all_nodes].double(), leaves, edges, full=True)
            lt = out["local_target_ids"].cpu().long()
            ref_loss = torch.nn.functional.cross_entropy(ref[lt], y[targets])
            err = O.rel_err(out["logits"].cpu(), ref.detach())
            print(f"step {step}: {all_nodes.numel()} nodes, logits rel err {err:.2e}, loss_c {float(out['loss_c']):.6f} vs {float(ref_loss.detach()):.6f}")
            assert err <= ACT_TOL
            assert abs(float(out["loss_c"]) - float(ref_loss.detach())) <= ACT_TOL * max(1.0, abs(float(ref_loss.detach())))
            kw = dict(aggregators=AGG, scalers=SCAL, avg_log=params["avg_log"], avg_lin=params["avg_lin"])
            last = O.pna_conv(hidden[0]["out"].detach(), params["convs"][1], edges[0], full=True, **kw)
            _kink_report(hidden, last, all_nodes.numel())
            rg = torch.autograd.grad(ref_loss, flat)
            named = [(k, p_) for k, p_ in c.named_parameters() if k.startswith("conv.")]
            for (name, p_), want in zip(named, rg):
                e = O.rel_err(p_.grad.cpu(), want)
                print(f"{name}: grad rel err {e:.2e}")
                assert e <= GRAD_TOL, name
    for a, b in zip(kept["pna"], kept["gcn"]):                           # the sampler does not see the classifier
        for ka, kb in zip(a, b):
            assert np.array_equal(ka, kb)


def test_graphed_trainer_refuses_a_pna_classifier():
    _need_gpu()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    from grapes_amd.step_graph import GraphedTrainer
    n, F, C, indptr, indices, X, y, _ = _cora_like()
    g = DeviceGraph.from_csr(indptr, indices)
    with pytest.raises(NotImplementedError, match="GCN classifier"):
        GraphedTrainer(g, X.cuda(), y.cuda(), _pna(F, 16, C, g).cuda(), GCN(F + 3, [16, 1]).cuda(), GCN(F, [16, 1]).cuda(), batch_size=32)


def _with_loops(indptr, indices, n, rng, k=50):
    """The CSR with k stored self-loops added (a DeviceGraph keeps them)."""
    rows = np.repeat(np.arange(n), np.diff(indptr))
    v = rng.permutation(n)[:k]
    key = np.unique(np.concatenate([rows * np.int64(n) + np.asarray(indices, dtype=np.int64), v * np.int64(n) + v]))
    r, c = key // n, (key % n).astype(np.int32)
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ip[1:])
    return ip, c


@pytest.mark.parametrize("full_batch", [True, False])
def test_evaluate_with_pna_classifier_matches_oracle(full_batch, monkeypatch):
    _need_gpu()
    from types import SimpleNamespace
    from grapes_amd import eval as E, step_graph
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    n, F, C, indptr, indices, X, y, rng = _cora_like(seed=9)
    indptr, indices = _with_loops(indptr, indices, n, rng)
    hops, K, H = 2, 100000, 32
    g = DeviceGraph.from_csr(indptr, indices)
    torch.manual_seed(3)
    c, gf = _pna(F, H, C, g).cuda(), GCN(F + hops + 1, [H, 1]).cuda()
    mask = torch.zeros(n, dtype=torch.bool); mask[rng.permutation(n)[:640]] = True
    idx = mask.nonzero().squeeze(1)
    args = SimpleNamespace(sampling_hops=hops, num_samples=K, use_indicators=True)
    data = SimpleNamespace(x=X.cuda(), y=y.cuda())

    def no_capture(*a, **k):
        raise AssertionError("evaluate built a GraphedTrainer for a PNA classifier")
    monkeypatch.setattr(step_graph, "GraphedTrainer", no_capture)
    loader = [(idx[o:o + 128],) for o in range(0, idx.numel(), 128)]        # five full batches: a GCN would be captured
    acc, f1, pred = E.evaluate(c, gf, data, args, g, mask=mask.cuda(), loader=loader, full_batch=full_batch, return_predictions=True)
    assert acc == f1 and pred.numel() == idx.numel()
    params = O.model_params(c)
    if full_batch:
        rows = np.repeat(np.arange(n), np.diff(indptr))
        ref = O.pna_forward(X.double(), params, np.stack([rows, np.asarray(indices, dtype=np.int64)]))[idx]
    else:
        # num_samples exceeds every neighbourhood, so the greedy sampler keeps all candidates and the batch graphs are the exact
        # 2-hop neighbourhoods: the oracle rebuilds them from the CSR, stored loops included
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
            want.append(O.pna_forward(X[all_nodes].double(), params, edges)[loc[t]])
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
    n, F, C, indptr, indices, X, y, _ = _cora_like()
    g = DeviceGraph.from_csr(indptr, indices)
    model = _pna(F, 8, C, g).cuda()
    old = full_graph.LARGE_NNZ
    full_graph.LARGE_NNZ = 1                          # (every graph then counts as one of 2^31 or more entries)
    try:
        with pytest.raises(ValueError, match="2\\^31"):
            model(X.cuda(), g)
    finally:
        full_graph.LARGE_NNZ = old


def test_cli_trains_a_pna_classifier():
    _need_gpu()
    r = subprocess.run([sys.executable, "-m", "grapes_amd.main", "--dataset", "cora", "--classifier", "pna", "--max_epochs", "2",
                        "--runs", "1", "--eval_frequency", "1", "--dropout", "0.1", "--hidden_dim", "32"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    losses = [(float(a), float(b)) for a, b in re.findall(r"loss_gfn=([-\w.+]+), loss_c=([-\w.+]+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(v) for p in losses for v in p)
    assert "valid_accuracy=" in r.stdout and "test_accuracy=" in r.stdout and "Acc: " in r.stdout


def test_full_batch_cli_trains_a_pna_classifier():
    _need_gpu()
    r = subprocess.run([sys.executable, "-m", "grapes_amd.full_batch", "--dataset", "cora", "--classifier", "pna", "--max_epochs", "2",
                        "--runs", "1", "--eval_frequency", "2", "--hidden_dim", "32", "--seed", "1", "--lr_gc", "0.01",
                        "--pna_aggregators", "mean,max,std", "--pna_scalers", "identity,attenuation"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    losses = [float(v) for v in re.findall(r"epoch \d+: loss_c=([-\w.+]+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses))
    assert "valid_f1=" in r.stdout and "test_accuracy=" in r.stdout and "Acc: " in r.stdout
