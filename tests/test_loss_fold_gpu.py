"""The classifier's last aggregation that carries the step's losses (grapes_gcn_aggregate_fwd_losses) against the two launches
it replaces, grapes_gcn_aggregate_fwd + grapes_step_losses: logits, loss_c, every row of dlogits and out4 bit for bit; and a
captured trainer with the fold on and off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda")


def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _case(n_rows, C, B, multilabel, seed, live=None):
    """A random graph over n_rows rows (a hub row, empty rows), its transformed features, B target ids of which the first maps to
    row 0 and the second to the last live row (then shuffled); targets beyond the rows there are map to no row (-1)."""
    from grapes_amd import ops
    rng = np.random.default_rng(seed)
    N, hops = 5000, 3
    m = n_rows if live is None else live                     # (edges among the live rows only)
    e = 3 * m if m > 1 else 0
    src, dst = rng.integers(0, m, e), rng.integers(0, m, e)
    if m > 40:
        dst[:40] = m // 2                                    # more than GRAPES_HUB_ROW entries in one row
    d_n = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
    prep = ops.PreparedGraph(_t(src, torch.int32), _t(dst, torch.int32), n_rows, d_n=d_n)
    h = _t(rng.standard_normal((n_rows, C)).astype(np.float32))
    bias = _t(rng.standard_normal(C).astype(np.float32))
    targets = _t(rng.permutation(N)[:B], torch.int32)
    rows = np.full(B, -1, dtype=np.int64)
    k = min(B, m)                                            # (the targets are live rows, as all_nodes holds them)
    perm = rng.permutation(m)
    perm = np.concatenate([[0, m - 1] if m > 1 else [0], perm[(perm != 0) & (perm != m - 1)]])
    rows[:k] = perm[:k]
    rows = rows[rng.permutation(B)] if B > 2 else rows
    node_map = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    node_map[targets.long()] = _t(rows, torch.int32)
    y = _t((rng.random((N, C)) < 0.3).astype(np.float32)) if multilabel else _t(rng.integers(0, C, N), torch.int64)
    stats = _t(rng.standard_normal((hops, 6)).astype(np.float32))
    zcap, nz = 3000, 2111
    zout = _t(rng.standard_normal(zcap).astype(np.float32)); zout[nz:] = float("nan")
    d_nz = torch.tensor([nz], dtype=torch.int32, device="cuda")
    return prep, h, bias, node_map, targets, y, stats, zout, d_nz


@pytest.mark.parametrize("multilabel", [False, True])
@pytest.mark.parametrize("B", [1, 256])
@pytest.mark.parametrize("C", [2, 47])
@pytest.mark.parametrize("n_rows", [1, 65, 1022])
def test_aggregation_with_losses_equals_the_two_launches(n_rows, C, B, multilabel):
    _cuda()
    from grapes_amd import ops
    prep, h, bias, node_map, targets, y, stats, zout, d_nz = _case(n_rows, C, B, multilabel, 1000 * n_rows + 10 * C + B)
    for reinforce in (False, True):
        kw = dict(z_out=zout, d_nz=d_nz, log_z_init=7.0, reinforce=reinforce)
        logits_r = ops.gcn_aggregate_fwd(h, prep, bias, False)
        loss_r, dl_r, out_r = ops.step_losses(logits_r, node_map, targets, y, stats, 1e4, **kw)
        got = ops.gcn_aggregate_fwd_losses(h, prep, bias, node_map, targets, y, stats, 1e4, **kw)
        if C <= 16:                 # the lanes-across-rows aggregation: not this launch's, the trainer keeps the two launches
            assert got is None
            continue
        logits, loss, dl, out4 = got
        assert torch.equal(logits, logits_r) and torch.equal(loss, loss_r) and torch.equal(out4, out_r)
        assert torch.equal(dl, dl_r)                                   # every row: the targets' gradients, zeros elsewhere
        assert float(dl.abs().sum()) > 0 and bool(torch.isfinite(out4).all())
    assert int(ops._ticket(torch.device("cuda", 0)).ne(0).sum()) == 0


@pytest.mark.parametrize("n_rows,C,B,multilabel,live,z", [
    (1022, 121, 301, True, None, True),        # more classes than a wavefront has lanes, a batch beyond one pass of the workgroup
    (1022, 18, 300, False, None, True),        # the narrowest rows this launch takes
    (700, 47, 256, False, 613, True),          # a live count below the capacity: the rows behind it keep their zeros
    (700, 47, 256, False, None, False),        # no log-Z head (random sampling)
    (1022, 44, 256, False, None, True),        # float4 rows: the other aggregation kernel's shape
])
def test_aggregation_with_losses_shapes(n_rows, C, B, multilabel, live, z):
    _cuda()
    from grapes_amd import ops
    prep, h, bias, node_map, targets, y, stats, zout, d_nz = _case(n_rows, C, B, multilabel, 7 * n_rows + C, live=live)
    kw = dict(z_out=zout, d_nz=d_nz, log_z_init=7.0) if z else dict()
    # (rows past the live count are not written by either aggregation: both start from the same matrix)
    logits_r = ops.gcn_aggregate_fwd(h, prep, bias, False, out=torch.full_like(h, 0.25))
    loss_r, dl_r, out_r = ops.step_losses(logits_r, node_map, targets, y, stats, 3.0, **kw)
    got = ops.gcn_aggregate_fwd_losses(h, prep, bias, node_map, targets, y, stats, 3.0, **kw)
    if C % 4 == 0:
        assert got is None
        return
    logits, loss, dl, out4 = got
    m = n_rows if live is None else live
    assert torch.equal(logits[:m], logits_r[:m]) and torch.equal(loss, loss_r) and torch.equal(out4, out_r)
    assert torch.equal(dl, dl_r)
    assert int(ops._ticket(torch.device("cuda", 0)).ne(0).sum()) == 0


def test_captured_trainer_with_and_without_the_fold(monkeypatch):
    """Four captured steps of a GraphedTrainer with the losses inside the last aggregation and as a launch of their own: losses,
    kept sets and every parameter bit for bit."""
    _cuda()
    from grapes_amd import synth
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    from grapes_amd.step_graph import GraphedTrainer
    n, deg, F, C, B, K, hops, H = 3000, 8.0, 32, 19, 64, 32, 2, 64
    tr_steps = 7                      # two eager steps, the capture, four replays
    indptr, indices = synth.synth_csr_numpy(n, deg, 300, seed=3)
    rng = np.random.default_rng(4)
    X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, C, n)).cuda()
    batches = [torch.from_numpy(rng.permutation(n)[:B].astype(np.int64)).cuda() for _ in range(tr_steps)]

    def run(fold):
        monkeypatch.setenv("GRAPES_DIAG", "1")          # (Python-side switches are read only in a diagnostic session)
        monkeypatch.setenv("GRAPES_LOSS_FOLD", "1" if fold else "0")
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
        params = [p.detach().clone() for net in (c, gf, z) for p in net.parameters()]
        return outs, params

    (a, pa), (b, pb) = run(True), run(False)
    for it, (x, w) in enumerate(zip(a, b)):
        assert x[0] == w[0] and x[1] == w[1], it
        assert x[3] == w[3], it
        for ka, kb, kc in zip(x[2], w[2], x[3]):
            assert torch.equal(ka[:kc], kb[:kc]), it
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
