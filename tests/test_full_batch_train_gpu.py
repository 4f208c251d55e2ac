"""Full-batch training (grapes_amd/full_graph.py train_step; full-batch.py:100-105): the row-blocked 64-bit step forced on small
graphs against the fp64 CPU oracle with torch autograd, against the int32 autograd path (same Philox masks), its determinism,
five Adam epochs, its refusals, and one step on papers100M at its real shape."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import grapes_oracle as O


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _graph(asymmetric, seed=3, n=6000):
    """6000 nodes with hub rows longer than the 64-entry item chunk; directed: a third of the entries dropped and self-loops
    stored on every fifth node (PyG replaces them)."""
    from grapes_amd import synth
    indptr, indices = synth.synth_csr_numpy(n, 14.0, 600, seed=seed)
    rng = np.random.default_rng(seed + 1)
    if asymmetric:
        rows = np.repeat(np.arange(n), np.diff(indptr))
        keep = rng.random(len(indices)) > 0.33
        ei = np.stack([np.concatenate([rows[keep], np.arange(0, n, 5)]), np.concatenate([indices[keep], np.arange(0, n, 5)])])
        indptr, indices = O.build_csr(ei, n)
    return indptr, indices, rng


def _setup(asymmetric, F, H, C, multi, seed=3, dropout=0.0):
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    n = 6000
    indptr, indices, rng = _graph(asymmetric, seed)
    X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    y = torch.from_numpy((rng.random((n, C)) < 0.3).astype(np.float32)) if multi else torch.from_numpy(rng.integers(0, C, n))
    train = torch.from_numpy(rng.random(n) < 0.3)
    torch.manual_seed(seed)
    rc = O.GCNRef(F, [H, C])
    with torch.no_grad():
        for p in rc.parameters():
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1)                                       # non-zero biases
    c = GCN(F, [H, C], dropout=dropout).cuda()
    c.load_state_dict(rc.state_dict())
    g = DeviceGraph.from_csr(indptr, indices)
    plan = g.full_graph_plan(hub_chunk=64)                                  # hub rows (and hub sources) cut into work items
    assert int(np.diff(indptr).max()) > 2 * 64 and plan.item_cap >= 3
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    ei = torch.from_numpy(np.stack([rows, indices.astype(np.int64)]))
    return X, y, train, rc, c, g, ei, rng


def _oracle_step(rc, X, y, train, ei):
    """fp64 loss and gradients (order W1, b1, W2, b2) of the reference step with torch autograd on the CPU."""
    r64 = O.GCNRef(X.shape[1], [rc.gcn_layers[0].lin.weight.shape[0], rc.gcn_layers[1].lin.weight.shape[0]]).double()
    r64.load_state_dict({k: v.double() for k, v in rc.state_dict().items()})
    logits, _ = r64(X.double(), ei)
    lt, yt = logits[train], y[train]
    loss = torch.nn.functional.cross_entropy(lt, yt) if y.dim() == 1 else \
        torch.nn.functional.binary_cross_entropy_with_logits(lt, yt.double())
    loss.backward()
    grads = [p.grad for p in _params(r64)]
    # the layer-1 pre-activations (to name the units whose ReLU gate sits within rounding of 0)
    with torch.no_grad():
        pre1 = O.gcn_conv(X.double(), r64.gcn_layers[0].lin.weight, r64.gcn_layers[0].bias, ei)
    return float(loss.detach()), grads, pre1


def _params(m):
    return [m.gcn_layers[0].lin.weight, m.gcn_layers[0].bias, m.gcn_layers[1].lin.weight, m.gcn_layers[1].bias]


def _grads(c):
    return [p.grad.detach().cpu().double().clone() for p in _params(c)]


def _zero(c):
    for p in c.parameters():
        p.grad = None


def _check_grads(got, ref, pre1, what):
    for i, (a, b) in enumerate(zip(got, ref)):
        tol = 1e-4 * float(b.abs().max())
        bad = (a - b).abs() > tol
        if bool(bad.any()):
            # only a layer-1 unit whose pre-activation is within fp32 rounding of 0 on some row may differ: its ReLU gate flips
            assert i in (0, 1), (what, i, float((a - b).abs().max()), tol)
            units = torch.nonzero(bad.reshape(bad.shape[0], -1).any(dim=1)).reshape(-1)
            scale = float(pre1.abs().max())
            for u in units.tolist():
                assert float(pre1[:, u].abs().min()) <= 1e-6 * scale, (what, i, u)


@pytest.mark.parametrize("asymmetric,F,H,C,multi,block", [
    (False, 100, 64, 7, False, 777),         # symmetric, F >= H, CE, ragged blocks
    (True, 48, 128, 11, True, None),         # directed with stored self-loops, F < H, BCE, C % 4 != 0
    (True, 30, 64, 47, False, 777),          # X's columns padded (30 -> 32), C = 47
    (False, 64, 32, 5, True, None),          # F >= H, BCE
    (False, 128, 256, 172, False, None),     # papers100M's widths: C > 64 (several columns per lane in the loss)
])
def test_forced_row_blocked_step_matches_oracle(asymmetric, F, H, C, multi, block):
    _cuda()
    from grapes_amd import full_graph
    X, y, train, rc, c, g, ei, rng = _setup(asymmetric, F, H, C, multi)
    loss, ev = full_graph.train_step(c, X.cuda(), g, y.cuda(), train.cuda(), block_rows=block, large_graph=True)
    ol, og, pre1 = _oracle_step(rc, X, y, train, ei)
    assert ev is None and loss.dim() == 0
    assert abs(float(loss) - ol) <= 1e-5 * abs(ol), (float(loss), ol)
    _check_grads(_grads(c), og, pre1, "forced")
    # gradients ACCUMULATE into p.grad, as loss.backward() would
    g1 = _grads(c)
    full_graph.train_step(c, X.cuda(), g, y.cuda(), train.cuda(), block_rows=block, large_graph=True)
    for a, b in zip(_grads(c), g1):
        assert float((a - 2 * b).abs().max()) <= 1e-6 * float(b.abs().max()) + 1e-30


def _hook(seed):
    state = {"off": 1000}

    def counters(n_elements):
        off = state["off"]
        state["off"] += (int(n_elements) + 3) // 4
        return seed, off
    return counters


@pytest.mark.parametrize("multi", [False, True])
def test_forced_path_equals_int32_autograd_path_with_dropout(multi):
    _cuda()
    from grapes_amd import full_graph
    F, H, C = 64, 128, 9
    X, y, train, rc, c, g, ei, rng = _setup(True, F, H, C, multi, seed=7, dropout=0.3)
    ev_rows = torch.from_numpy(np.sort(rng.permutation(6000)[:900]))
    out = {}
    for large in (False, True):
        _zero(c)
        c.philox_dropout = _hook(1234)
        loss, ev = full_graph.train_step(c, X.cuda(), g, y.cuda(), train.cuda(), eval_rows=ev_rows.cuda(), block_rows=1000,
                                         large_graph=large)
        out[large] = (float(loss), _grads(c), ev.detach().cpu())
    (l0, g0, e0), (l1, g1, e1) = out[False], out[True]
    assert abs(l0 - l1) <= 1e-5 * abs(l0)
    assert torch.equal(e0 == 0, e1 == 0)                                    # the same keep mask on the logits
    assert float((e0 - e1).abs().max()) <= 1e-5 * max(1.0, float(e0.abs().max()))
    assert float((e0 == 0).float().mean()) > 0.2                              # (dropout did drop)
    for i, (a, b) in enumerate(zip(g1, g0)):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), i


def test_two_steps_from_the_same_state_are_bit_identical():
    _cuda()
    from grapes_amd import full_graph
    X, y, train, rc, c, g, ei, rng = _setup(True, 100, 64, 7, False, dropout=0.2)
    res = []
    for _ in range(2):
        _zero(c)
        c.philox_dropout = _hook(99)
        loss, _ = full_graph.train_step(c, X.cuda(), g, y.cuda(), train.cuda(), block_rows=777, large_graph=True)
        res.append((loss.clone(), [p.grad.clone() for p in _params(c)]))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


def test_five_adam_epochs_match_the_oracle():
    _cuda()
    from grapes_amd import full_graph
    X, y, train, rc, c, g, ei, rng = _setup(False, 100, 64, 7, False, seed=11)
    r64 = O.GCNRef(100, [64, 7]).double()
    r64.load_state_dict({k: v.double() for k, v in rc.state_dict().items()})
    opt_r = torch.optim.Adam(r64.parameters(), lr=1e-3)                      # full-batch.py:76
    opt_c = torch.optim.Adam(c.parameters(), lr=1e-3)
    Xc, yc, tc = X.cuda(), y.cuda(), train.cuda()
    for _ in range(5):
        opt_r.zero_grad()
        logits, _ = r64(X.double(), ei)
        torch.nn.functional.cross_entropy(logits[train], y[train]).backward()
        opt_r.step()
        opt_c.zero_grad()
        full_graph.train_step(c, Xc, g, yc, tc, large_graph=True)
        opt_c.step()
    for a, b in zip(_params(c), _params(r64)):
        assert float((a.detach().cpu().double() - b.detach()).abs().max()) <= 1e-4


def test_refusals(monkeypatch):
    _cuda()
    from grapes_amd import full_graph
    from grapes_amd.modules.gcn import GCN
    X, y, train, rc, c, g, ei, rng = _setup(False, 100, 64, 7, False)
    c3 = GCN(100, [64, 64, 7]).cuda()
    with pytest.raises(ValueError, match="two-layer"):
        full_graph.train_step(c3, X.cuda(), g, y.cuda(), train.cuda(), large_graph=True)
    Xc, yc, tc = X.cuda(), y.cuda(), train.cuda()
    monkeypatch.setattr(full_graph, "free_bytes", lambda device: 1 << 20)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError, match="GiB"):
        full_graph.train_step(c, Xc, g, yc, tc, large_graph=True)
    assert torch.cuda.memory_allocated() - before < 1 << 20                   # (the train row ids at most)
    assert all(p.grad is None for p in c.parameters())
    # GCN.forward under autograd on the forced path keeps refusing, and names the trainer
    with pytest.raises(ValueError, match="training.*train_step"):
        c(Xc, g, large_graph=True)


# ---------------------------------------------------------------------------------------------- papers100M at its real shape
OGB_TRAIN, OGB_VALID = 1_207_179, 125_265


def test_papers100m_one_step_real_shape():
    _cuda()
    from grapes_amd import full_graph, ops, synth
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    N, deg, maxdeg, F, C, *_ = synth.CONFIGS["papers100m"]
    rowptr, col = synth.synth_graph_device_chunked(N, deg, maxdeg, seed=0, device="cuda")
    g = DeviceGraph(rowptr, col, N)
    assert g.nnz > 3_000_000_000
    gen = torch.Generator(device="cuda"); gen.manual_seed(2)
    X = synth.randn_rows_(torch.empty(N, F, device="cuda"), generator=gen)
    y = torch.randint(0, C, (N,), device="cuda", generator=gen)
    perm = torch.randperm(N, device="cuda", generator=gen)
    train = torch.zeros(N, dtype=torch.bool, device="cuda"); train[perm[:OGB_TRAIN]] = True
    valid = torch.sort(perm[OGB_TRAIN:OGB_TRAIN + OGB_VALID]).values
    del perm
    torch.manual_seed(0)
    c = GCN(F, [256, C]).cuda()                                               # full-batch.py:73 with the default hidden_dim
    plan = g.full_graph_plan()
    assert plan.symmetric
    R = torch.nonzero(train).reshape(-1).to(torch.int32)
    e_cap = ops.rowlist_entries_cap(plan, R)
    need, parts = full_graph.train_memory_plan(N, F, 256, C, OGB_TRAIN, OGB_VALID, full_graph.DEFAULT_BLOCK_ROWS, plan.item_cap,
                                               ops.rowlist_transpose_bytes(plan, e_cap), e_cap, plan.chunk, False)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss, ev = full_graph.train_step(c, X, g, y, train, eval_rows=valid)        # automatic: nnz >= 2^31 - 1
    torch.cuda.synchronize()
    peak_extra = torch.cuda.max_memory_allocated() - base
    assert peak_extra <= need, (peak_extra, need, parts)
    assert ev.shape == (OGB_VALID, C) and bool(torch.isfinite(loss)) and 0.0 < float(loss) < 20.0
    grads = [p.grad.clone() for p in _params(c)]
    # bit-identical on a second step from the same state
    _zero(c)
    loss2, _ = full_graph.train_step(c, X, g, y, train)
    assert torch.equal(loss, loss2)
    for a, p in zip(grads, _params(c)):
        assert torch.equal(a, p.grad)
    # directional derivative of the whole step: (L(θ+εd) - L(θ-εd)) / 2ε against <∇L, d>.  ε is chosen so that L moves by 1e-4
    # relative.  Two errors remain: the loss is returned in fp32, so one ulp of L (~4.8e-7 at L ~ 5.15) is ~4.6e-4 of the
    # difference; and the O(ε²) curvature term, measured on this shape and direction at 9e-4 (9 % at 1e-3 relative).  5e-3
    # bounds both with room and stays far below what a wrong gradient (a missing term, a wrong scale, a lost gate) misses by.
    dgen = torch.Generator(device="cuda"); dgen.manual_seed(5)
    # d = the gradient plus noise of its own mean size: <∇L, d> ~ |∇L|^2 is well away from 0, and the noise makes d no multiple
    # of what the step returned
    dirs = [a + torch.randn(a.shape, device="cuda", generator=dgen) * a.abs().mean() for a in grads]
    slope = sum(float((a * d).sum()) for a, d in zip(grads, dirs))
    eps = 1e-4 * float(loss) / abs(slope)
    orig = [p.detach().clone() for p in _params(c)]
    lv = []
    for sgn in (1.0, -1.0):
        with torch.no_grad():
            for p, o, d in zip(_params(c), orig, dirs):
                p.copy_(o + sgn * eps * d)
        _zero(c)
        lv.append(float(full_graph.train_step(c, X, g, y, train)[0]))
    with torch.no_grad():
        for p, o in zip(_params(c), orig):
            p.copy_(o)
    fd = (lv[0] - lv[1]) / (2 * eps)
    assert abs(fd - slope) <= 5e-3 * abs(slope), (fd, slope)
    # the transposed gather for 256 sampled sources (half with CSR entries past the 2^31st) against fp64 from its own inputs
    Gm = torch.randn((OGB_TRAIN, (C + 3) // 4 * 4), device="cuda", generator=dgen)
    srcs, src_off, pos = ops.rowlist_transpose(plan, R, e_cap)
    dU = ops.rowlist_gather_t(Gm, srcs, src_off, pos, plan.dinv, plan.chunk)
    late = torch.nonzero(rowptr[srcs.long() + 1] > 2 ** 31).reshape(-1)
    early = torch.nonzero(rowptr[srcs.long() + 1] <= 2 ** 31).reshape(-1)
    pick = torch.cat([early[torch.randperm(early.numel(), device="cuda", generator=dgen)[:128]],
                      late[torch.randperm(late.numel(), device="cuda", generator=dgen)[:128]]])
    Rl = R.long()
    dinv_ref = (rowptr[1:] - rowptr[:-1] + 1).double().rsqrt()                  # (the synthetic CSR stores no self-loops)
    worst = 0.0
    for j in pick.tolist():
        s = int(srcs[j])
        nb = col[int(rowptr[s]):int(rowptr[s + 1])].long()                       # symmetric: the rows whose entries reach s
        cand = torch.cat([nb, torch.tensor([s], device="cuda")])
        at = torch.searchsorted(Rl, cand).clamp_(max=Rl.numel() - 1)
        hit = at[Rl[at] == cand]
        ref = dinv_ref[s] * Gm[hit].double().sum(0)
        scale = float(Gm[hit].abs().sum(0).max()) * float(dinv_ref[s])
        worst = max(worst, float((dU[j].double() - ref).abs().max()) / max(scale, 1e-30))
    assert worst <= 1e-5, worst
    assert int(late.numel()) > 128 and int(early.numel()) > 128
    del g, rowptr, col, X, plan, dU, Gm, srcs, src_off, pos
    torch.cuda.empty_cache()
