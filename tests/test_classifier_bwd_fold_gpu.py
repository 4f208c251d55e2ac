"""The classifier's backward pass in three launches: the few-row backward aggregation that also forms the layer's input gradient
(grapes_gcn_aggregate_bwd_input) against the two launches it replaces, grapes_gcn_aggregate_bwd -> grapes_linear_bwd_input — dT, dX
and dbias bit for bit; the layers' weight-gradient slabs as one launch (grapes_linear_bwd_weight_slabs_multi) against the launches
one by one; and a captured trainer with the fold on and off."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 64, 127, 129, 300)          # a ragged last row tile, the 128-row slab boundary
GRAPHS = ("loops", "random", "hub")


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda")


def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _graph(kind, n_rows, live, rng):
    """loops: no stored edge (every row is its own term only); random: 1-2 entries per row; hub: that plus one row with 70
    entries.  Edges among the live rows only."""
    from grapes_amd import ops
    m = live
    if kind == "loops" or m < 2:
        src = dst = np.zeros(0, dtype=np.int64)
    else:
        deg = rng.integers(1, 3, m)
        src = np.repeat(np.arange(m), deg)
        dst = rng.integers(0, m, src.size)
        if kind == "hub":
            src = np.concatenate([src, np.full(70, m // 2)])
            dst = np.concatenate([dst, rng.integers(0, m, 70)])
    d_n = None if live == n_rows else torch.tensor([live], dtype=torch.int32, device="cuda")
    return ops.PreparedGraph(_t(src, torch.int32), _t(dst, torch.int32), n_rows, d_n=d_n)


def _operands(n_rows, f, f_in, gated, rng):
    dout = _t(rng.standard_normal((n_rows, f)).astype(np.float32))
    gate = _t(rng.standard_normal((n_rows, f)).astype(np.float32)) if gated else None
    w = _t(rng.standard_normal((f, f_in)).astype(np.float32))
    return dout, gate, w


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("f,f_in", [(47, 256), (256, 256), (40, 64)])
def test_aggregation_with_input_gradient_equals_the_two_launches(f, f_in, gated):
    _cuda()
    from grapes_amd import ops
    rng = np.random.default_rng(100 * f + f_in + int(gated))
    for n_rows in ROWS:
        for kind in GRAPHS:
            prep = _graph(kind, n_rows, n_rows, rng)
            dout, gate, w = _operands(n_rows, f, f_in, gated, rng)
            dt_r, db_r = ops.gcn_aggregate_bwd(dout, prep, relu_out=gate)
            dx_r = ops.linear_bwd_input(dt_r, w, d_n=prep.d_n)
            db = torch.empty(f, dtype=torch.float32, device="cuda")
            got = ops.gcn_aggregate_bwd_input(dout, prep, w, relu_out=gate, dbias=db)
            assert got is not None, (n_rows, kind)
            dt, dx = got
            assert torch.equal(dt, dt_r), (n_rows, kind)
            assert torch.equal(dx, dx_r), (n_rows, kind)
            assert torch.equal(db, db_r), (n_rows, kind)
            assert bool(torch.isfinite(dx).all()) and float(dx.abs().sum()) > 0
    assert int(ops._ticket(torch.device("cuda", 0)).ne(0).sum()) == 0


@pytest.mark.parametrize("f,f_in", [(47, 256), (256, 256), (40, 64)])
@pytest.mark.parametrize("n_rows,live", [(64, 33), (300, 129), (300, 1), (129, 128)])
def test_live_count_below_the_capacity_leaves_the_rows_behind_it(n_rows, live, f, f_in):
    _cuda()
    from grapes_amd import ops
    rng = np.random.default_rng(7 * n_rows + live + f)
    for kind in GRAPHS:
        for gated in (False, True):
            prep = _graph(kind, n_rows, live, rng)
            dout, gate, w = _operands(n_rows, f, f_in, gated, rng)
            dt_r, db_r = ops.gcn_aggregate_bwd(dout, prep, relu_out=gate)
            dx_r = ops.linear_bwd_input(dt_r, w, d_n=prep.d_n)
            dt = torch.full((n_rows, f), 0.25, dtype=torch.float32, device="cuda")
            dx = torch.full((n_rows, f_in), -0.5, dtype=torch.float32, device="cuda")
            db = torch.empty(f, dtype=torch.float32, device="cuda")
            got = ops.gcn_aggregate_bwd_input(dout, prep, w, relu_out=gate, dbias=db, dt=dt, dx=dx)
            assert got is not None
            assert torch.equal(dt[:live], dt_r[:live]) and torch.equal(dx[:live], dx_r[:live]) and torch.equal(db, db_r), (kind, gated)
            assert bool((dt[live:] == 0.25).all()) and bool((dx[live:] == -0.5).all()), (kind, gated)      # the canary


@pytest.mark.parametrize("order", [((47, 256), (256, 256)), ((256, 256), (47, 256))])
def test_carried_by_the_sampler_heads_two_launches(order):
    """The two classifier shapes riding in the sampler heads' backward launches (ops.carry_backward_aggregations): the first call is
    carried by the dense-gradient launch, the second by the narrow aggregation, in both orders — so the one-float and the float4
    form (whose K = 256 image is larger than the partial tiles) each ride in each host.  Hosts and riders keep their bits."""
    _cuda()
    from grapes_amd import ops
    rng = np.random.default_rng(11)
    n_hop, n_rows = 5000, 300                                   # the host's rows (several workgroups), the classifier's
    hop_prep = _graph("random", n_hop, n_hop, rng)
    logits = _t(rng.standard_normal(n_hop).astype(np.float32))
    cand = np.full(n_hop, -1, dtype=np.int64)
    pos = rng.permutation(n_hop)[:n_hop // 2]
    cand[pos] = np.arange(pos.size)
    mask = _t((rng.random(pos.size) < 0.5).astype(np.float32))
    cand_pos = _t(cand, torch.int32)
    scale = _t(np.array([0.75], dtype=np.float32))

    def host():
        s = torch.zeros(1, dtype=torch.float32, device="cuda")
        return ops.SamplerHeadBwdMulti([logits], [mask], [cand_pos], [hop_prep], d_grad_scale=scale, sum_out=s), s

    hb_r, sum_r = host()
    hb_r.launch(0)
    cases = []
    for f, f_in in order:
        prep = _graph("hub", n_rows, n_rows, rng)
        dout, gate, w = _operands(n_rows, f, f_in, True, rng)
        db_r = torch.empty(f, dtype=torch.float32, device="cuda")
        dt_r, dx_r = ops.gcn_aggregate_bwd_input(dout, prep, w, relu_out=gate, dbias=db_r)      # on its own (checked above)
        cases.append((prep, dout, gate, w, dt_r, dx_r, db_r))
    hb, sum_c = host()
    alone0 = ops._BWD_ALONE[0]
    ops.carry_backward_aggregations([lambda: hb.launch(1), lambda: hb.launch(2)])
    got = []
    try:
        for prep, dout, gate, w, _, _, _ in cases:
            db = torch.empty(dout.shape[1], dtype=torch.float32, device="cuda")
            got.append(ops.gcn_aggregate_bwd_input(dout, prep, w, relu_out=gate, dbias=db) + (db,))
    finally:
        ops.flush_backward_hosts()
    torch.cuda.synchronize()
    assert not ops._BWD_HOSTS and ops._BWD_ALONE[0] == alone0     # both hosts were taken, and each carried its record
    for (_, _, _, _, dt_r, dx_r, db_r), (dt, dx, db) in zip(cases, got):
        assert torch.equal(dt, dt_r) and torch.equal(dx, dx_r) and torch.equal(db, db_r)
    assert torch.equal(hb.dlog, hb_r.dlog) and torch.equal(hb.dh, hb_r.dh) and torch.equal(sum_c, sum_r)
    assert float(hb.dh.abs().sum()) > 0
    assert int(ops._ticket(torch.device("cuda", 0)).ne(0).sum()) == 0


def test_shapes_outside_the_launch_are_refused():
    _cuda()
    from grapes_amd import ops
    rng = np.random.default_rng(5)
    prep = _graph("random", 64, 64, rng)
    for f, f_in in ((16, 64), (260, 64), (70, 64)):          # too narrow, too wide, scalar rows beyond one wavefront
        dout, gate, w = _operands(64, f, f_in, False, rng)
        assert ops.gcn_aggregate_bwd_input(dout, prep, w) is None


@pytest.mark.parametrize("n_rows", [33, 129, 300])
def test_weight_gradient_slabs_side_by_side_equal_the_launches_one_by_one(n_rows):
    """dW3 (47 x 256), dW2 (256 x 256) and the gated first layer's dW1 (256 x 100) with its bias gradient: the three slab
    launches as one, then the one slab sum."""
    _cuda()
    from grapes_amd import ops
    rng = np.random.default_rng(n_rows)
    H, C, F = 256, 47, 100
    mk = lambda r, c: _t(rng.standard_normal((r, c)).astype(np.float32))
    dt3, x3 = mk(n_rows, C), mk(n_rows, H)
    dt2, x2 = mk(n_rows, H), mk(n_rows, H)
    d1, act1, ax = mk(n_rows, H), mk(n_rows, H), mk(n_rows, F)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")

    ref = ops.DeferredSlabs()
    w3_r, w2_r, w1_r, b1_r = z(C, H), z(H, H), z(H, F), z(H)
    ops.linear_bwd_weight(dt3, x3, out=w3_r, defer=ref)
    ops.linear_bwd_weight(dt2, x2, out=w2_r, defer=ref)
    ops.linear_bwd_weight_gated(d1, ax, gate=act1, dw=w1_r, dbias=b1_r, defer=ref)
    assert len(ref.sets) == 4                       # (all three took the few-row form)
    ref.flush()

    got = ops.DeferredSlabs()
    w3, w2, w1, b1 = z(C, H), z(H, H), z(H, F), z(H)
    assert got.try_add_multi([(dt3, None, x3, w3, None, None), (dt2, None, x2, w2, None, None), (d1, act1, ax, w1, b1, None)])
    assert len(got.sets) == 4
    got.flush()
    torch.cuda.synchronize()
    assert torch.equal(w3, w3_r) and torch.equal(w2, w2_r) and torch.equal(w1, w1_r) and torch.equal(b1, b1_r)
    assert float(w3.abs().sum()) > 0 and float(b1.abs().sum()) > 0


def _graph_nodes(tr):
    """nodes of the captured step (kernels, and whatever memsets both forms share): what a chain of one step would hold"""
    from grapes_amd import ops
    segs = tr.graph_obj.raw_graphs()
    arr = (ctypes.c_void_p * len(segs))(*segs)
    h, nodes = ctypes.c_void_p(), ctypes.c_int32(0)
    ops._lib.check(ops.lib().grapes_graph_chain_create(arr, len(segs), 1, ctypes.byref(h), ctypes.byref(nodes)), "graph_chain_create")
    ops._lib.check(ops.lib().grapes_graph_chain_destroy(h), "graph_chain_destroy")
    return int(nodes.value)


def test_captured_trainer_with_and_without_the_fold(monkeypatch):
    """A three-layer classifier over 3 hops: captured steps with the classifier's backward pass in three launches and in five
    (GRAPES_CLS_BWD_FOLD=0): losses, kept sets and every parameter of the three nets bit for bit, two kernel nodes fewer."""
    _cuda()
    from grapes_amd import synth
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    from grapes_amd.step_graph import GraphedTrainer
    n, deg, F, C, B, K, hops, H = 3000, 8.0, 32, 19, 32, 32, 3, 64
    tr_steps = 5                      # two eager steps, the capture, two replays (three captured steps)
    indptr, indices = synth.synth_csr_numpy(n, deg, 300, seed=3)
    rng = np.random.default_rng(4)
    X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, C, n)).cuda()
    batches = [torch.from_numpy(rng.permutation(n)[:B].astype(np.int64)).cuda() for _ in range(tr_steps)]

    def run(fold):
        monkeypatch.setenv("GRAPES_DIAG", "1")          # (Python-side switches are read only in a diagnostic session)
        monkeypatch.setenv("GRAPES_CLS_BWD_FOLD", "1" if fold else "0")
        torch.manual_seed(0)
        c, gf, z = GCN(F, [H] * (hops - 1) + [C]).cuda(), GCN(F + hops + 1, [H, 1]).cuda(), GCN(F, [H, 1]).cuda()
        oc = torch.optim.Adam(c.parameters(), lr=1e-3, capturable=True)
        og = torch.optim.Adam(list(gf.parameters()) + list(z.parameters()), lr=1e-4, capturable=True)
        tr = GraphedTrainer(DeviceGraph.from_csr(indptr, indices), X, y, c, gf, z, batch_size=B, sampling_hops=hops,
                            num_samples=K, loss_coef=50.0, optimizer_c=oc, optimizer_gf=og, e_cap=1 << 14, philox_seed=77,
                            capture=True)
        outs = []
        for tg in batches:
            b = tr.step(tg)
            torch.cuda.synchronize()
            tr.check()
            outs.append((float(b["loss_c"]), float(b["loss_gfn"]), [k.clone() for k in b["kept"]],
                         [int(kc) for kc in b["kept_counts"]]))
        assert tr.graph_obj is not None
        params = [p.detach().clone() for net in (c, gf, z) for p in net.parameters()]
        return outs, params, _graph_nodes(tr)

    (a, pa, na), (b, pb, nb) = run(True), run(False)
    for it, (x, w) in enumerate(zip(a, b)):
        assert x[0] == w[0] and x[1] == w[1], it
        assert x[3] == w[3], it
        for ka, kb, kc in zip(x[2], w[2], x[3]):
            assert torch.equal(ka[:kc], kb[:kc]), it
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
    assert na == nb - 2, (na, nb)
