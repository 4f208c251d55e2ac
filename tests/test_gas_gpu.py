"""GNNAutoScale on the MI355X (grapes_amd/csrc/gas_kernels.hip, modules/gas.py, gas.py) against the fp64 host oracle of
tests/gas_oracle.py.

The resolve is integers: bit-equal.  Activations and gradients are judged by the project's measure (gat_oracle.rel_err:
max |a - ref| / max(1, max |ref|)) at its tolerances, 1e-5 and 1e-4; the backward of a ReLU is compared on the device's own gates.
Every graph has at most 1 500 nodes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import gas_oracle as GO
from tests.gat_oracle import rel_err

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4
F32, F64 = np.float32, np.float64
N_K, P_K = 1500, 10
LONG = 64                                                                # grapes_vrgcn_long_row(): T - 1, T, T + 1 = 63, 64, 65
DEGREES = [0, 1, LONG - 1, LONG, LONG + 1, 1000]                         # rows 0 .. 5; row 6 stores duplicate entries
HUB, DUP = 5, 6
GUARD = -77777


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(4321)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    assert ops.lib().grapes_vrgcn_long_row() == LONG
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _setup(rowptr, col, part, q):
    """The device graph (entries as stored: duplicates stay), its ClusterData under `part` and a ClusterLoader of q clusters."""
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.cluster import ClusterData, ClusterLoader
    n = len(rowptr) - 1
    g = DeviceGraph(_dev(rowptr.astype(np.int64)), _dev(col.astype(np.int32)), n)
    P = int(part.max()) + 1
    cd = ClusterData(g, P, part=torch.from_numpy(part))
    return SimpleNamespace(g=g, cd=cd, loader=ClusterLoader(cd, q), rowptr=rowptr, col=col, part=part, P=P, n=n)


_KG = {}


def _kernel_graph():
    """1 500 nodes in 10 range clusters of 150: rows 0 .. 5 have DEGREES distinct columns among the nodes 16 .. (the hub's 1 000 fall
    in every cluster: mixed in- and out-of-batch entries), row 6 stores (20, 20, 31, 700), every later row 0 .. 5 random columns (so
    dinv varies).  Loop-free, not symmetric — the kernels read rows only."""
    if "g" not in _KG:
        rng = np.random.default_rng(7)
        rows = [sorted(rng.choice(np.arange(16, N_K), d, replace=False).tolist()) for d in DEGREES] + [[20, 20, 31, 700]]
        for u in range(len(rows), N_K):
            c = rng.choice(N_K, int(rng.integers(0, 6)), replace=False)
            rows.append(sorted(int(v) for v in c if v != u))
        rowptr = np.zeros(N_K + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum([len(r) for r in rows])
        col = np.asarray([v for r in rows for v in r], dtype=np.int32)
        _KG["g"] = (rowptr, col, np.arange(N_K) * P_K // N_K)
    return _KG["g"]


def _resolve(ops, S, clusters, e_cap=None, col=None, status=None):
    """The loader's batch of `clusters` resolved into a buffer with guard values behind e_cap; returns the batch with the oracle's
    (rowptr_h, code, counts) as o_* beside the device's."""
    b = S.loader.batch(clusters)
    node_idx = GO.batch_nodes(S.part, clusters)
    assert np.array_equal(_np(b.node_idx), node_idx)
    b.o_rowptr_h, b.o_code, b.o_counts = GO.resolve(S.rowptr, S.col, node_idx)
    total = len(b.o_code)
    ec = max(total, 1) if e_cap is None else e_cap
    buf = torch.full((ec + 64,), GUARD, dtype=torch.int32, device="cuda")
    out = (torch.empty(b.num_nodes + 1, dtype=torch.int32, device="cuda"), buf, torch.full((2,), -1, dtype=torch.int64, device="cuda"))
    ops.gas_resolve(S.g.rowptr, S.g.col if col is None else col, S.n, b.node_idx, b.num_nodes, S.cd.where, S.loader.stamp,
                    S.loader.serial, ec, status=S.loader.status if status is None else status, out=out)
    b.rowptr_h, b.buf, b.counts, b.e_cap, b.o_node_idx = out[0], buf, out[2], ec, node_idx
    assert bool((buf[ec:] == GUARD).all())                               # nothing behind e_cap
    return b


def _resolved_is_the_oracle(b):
    total = len(b.o_code)
    assert np.array_equal(_np(b.rowptr_h), b.o_rowptr_h)
    assert np.array_equal(_np(b.buf[:total]), b.o_code)
    assert np.array_equal(_np(b.counts), b.o_counts)
    assert bool((b.buf[total:] == GUARD).all())


# ------------------------------------------------------------------------------------------------------------ the resolve
def test_resolve_hand_graph():
    ops = _ops()
    #   0 - 1, 0 - 2, 1 - 2 (cluster 0 = {0, 1, 2}),  2 - 3, 3 - 4 (cluster 1 = {3, 4}),  4 - 5, 5 - 0 (cluster 2 = {5, 6}; 6 is isolated)
    rows = [[1, 2, 5], [0, 2], [0, 1, 3], [2, 4], [3, 5], [0, 4], []]
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    col = np.asarray([v for r in rows for v in r], dtype=np.int32)
    S = _setup(rowptr, col, np.asarray([0, 0, 0, 1, 1, 2, 2]), 2)
    b = _resolve(ops, S, [2, 0])                                         # rows: 5, 6, 0, 1, 2
    assert _np(b.node_idx).tolist() == [5, 6, 0, 1, 2]
    assert _np(b.rowptr_h).tolist() == [0, 2, 2, 5, 7, 10]
    assert _np(b.buf[:10]).tolist() == [2, -5, 3, 4, 0, 2, 4, 2, 3, -4]
    assert _np(b.counts).tolist() == [8, 2]
    _resolved_is_the_oracle(b)
    S.loader.check()


@pytest.mark.parametrize("clusters", [[0, 5], [0], list(range(P_K))], ids=["q2", "q1", "qP"])
def test_resolve_degrees_and_hub(clusters):
    ops = _ops()
    S = _setup(*_kernel_graph(), len(clusters))
    b = _resolve(ops, S, clusters)
    deg = np.diff(b.o_rowptr_h)
    assert deg[:6].tolist() == DEGREES
    hub = b.o_code[b.o_rowptr_h[HUB]:b.o_rowptr_h[HUB + 1]]
    if len(clusters) == P_K:
        assert b.o_counts[1] == 0                                        # no halo
    else:
        assert (hub >= 0).any() and (hub < 0).any()                      # mixed in / out entries
    _resolved_is_the_oracle(b)
    S.loader.check()


def test_resolve_every_entry_is_halo():
    ops = _ops()
    n = 40
    rng = np.random.default_rng(3)
    a, c = rng.integers(0, 20, 90), rng.integers(20, 40, 90)             # entries between {0 .. 19} and {20 .. 39} only
    rowptr, col = GO.csr_from_edges(n, np.concatenate([a, c]), np.concatenate([c, a]))
    S = _setup(rowptr, col, np.arange(n) * 4 // n, 2)
    b = _resolve(ops, S, [1, 0])
    assert b.o_counts[0] == 0 and b.o_counts[1] == len(b.o_code) > 0 and S.loader.batch([1, 0]).edge_index.shape[1] == 0
    _resolved_is_the_oracle(b)
    S.loader.check()


def test_resolve_overflow_reports_the_total():
    ops = _ops()
    from grapes_amd._lib import GrapesHipError
    S = _setup(*_kernel_graph(), 2)
    total = len(GO.resolve(S.rowptr, S.col, GO.batch_nodes(S.part, [0, 5]))[1])
    b = _resolve(ops, S, [0, 5], e_cap=total - 5)
    assert int(b.rowptr_h[-1]) == total and np.array_equal(_np(b.rowptr_h), b.o_rowptr_h)
    assert np.array_equal(_np(b.buf[:total - 5]), b.o_code[:total - 5])
    assert int(S.loader.status.item()) == 1
    with pytest.raises(GrapesHipError, match="edge buffer overflow"):
        S.loader.check()
    _resolved_is_the_oracle(_resolve(ops, S, [0, 5], e_cap=total))       # the retry into a buffer that fits
    S.loader.check()


def test_a_bad_column_raises_through_check():
    ops = _ops()
    from grapes_amd._lib import GrapesHipError
    S = _setup(*_kernel_graph(), 2)
    col = S.g.col.clone()
    at = int(S.rowptr[4]) + 7                                            # an entry of the 65-entry row
    col[at] = N_K + 3
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    b = _resolve(ops, S, [0, 5], col=col, status=status)
    assert int(status.item()) == 4
    p = int(b.o_rowptr_h[4]) + 7
    assert int(b.buf[p]) == ops.GAS_BAD_CODE
    keep = np.ones(len(b.o_code), bool); keep[p] = False
    assert np.array_equal(_np(b.buf[:len(b.o_code)])[keep], b.o_code[keep])
    S.loader.status.copy_(status)
    with pytest.raises(GrapesHipError, match="index out of range"):
        S.loader.check()
    S.loader.check()


def test_two_consecutive_batches_resolve_under_their_own_serial():
    _ops()
    from grapes_amd.modules.gas import GasLoader
    S = _setup(*_kernel_graph(), 3)
    L = GasLoader(S.cd, 3)
    for k, clusters in enumerate([[0, 1, 2], [2, 7, 0], [9, 8, 3]]):
        b = L.batch(clusters)
        assert L.loader.serial == k + 1
        node_idx = GO.batch_nodes(S.part, clusters)
        rowptr_h, code, counts = GO.resolve(S.rowptr, S.col, node_idx)
        assert np.array_equal(_np(b.node_idx), node_idx) and np.array_equal(_np(b.rowptr_h), rowptr_h)
        assert np.array_equal(_np(b.code), code) and (b.num_in, b.num_halo) == tuple(counts.tolist())
        src, dst = GO.induced_edges(rowptr_h, code)
        assert np.array_equal(_np(b.edge_index), np.stack([src, dst]))
        assert b.item_cap == int(np.ceil(np.diff(rowptr_h)[np.diff(rowptr_h) > LONG] / LONG).sum())
    L.check()
    L._h_hint = 100                                                      # a code buffer that is too small is grown, the status stays clean
    b = L.batch([0, 5])
    assert np.array_equal(_np(b.code), GO.resolve(S.rowptr, S.col, GO.batch_nodes(S.part, [0, 5]))[1])
    L.check()


# ------------------------------------------------------------------------------------------------------------ the aggregation
_BATCH = {}


def _agg_batch(clusters=(0, 5)):
    """A GasLoader batch of the kernel graph with what the aggregation reads, shared by the tests below (never modified)."""
    key = tuple(clusters)
    if key not in _BATCH:
        from grapes_amd.modules.gas import GasLoader
        from grapes_amd.modules.vrgcn import VRGraph
        S = _setup(*_kernel_graph(), len(clusters))
        L = GasLoader(S.cd, len(clusters))
        b = L.batch(list(clusters))
        L.check()
        _BATCH[key] = SimpleNamespace(S=S, L=L, b=b, vg=VRGraph(S.g), dv=GO.dinv(S.rowptr), node_idx=_np(b.node_idx).astype(np.int64),
                                      rowptr_h=_np(b.rowptr_h), code=_np(b.code))
    return _BATCH[key]


def _inputs(B, f, seed):
    rng = np.random.default_rng(seed)
    n = len(B.node_idx)
    return (rng.standard_normal((n, f)).astype(F32), rng.standard_normal((N_K, f)).astype(F32), rng.standard_normal((n, f)).astype(F32))


def _fwd(ops, B, h, hbar, **kw):
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.gas_aggregate_fwd(h, hbar, B.vg.dinv, B.b.node_idx, B.b.rowptr_h, B.b.code, status=status, **kw)
    assert int(status.item()) == 0
    return out


@pytest.mark.parametrize("f", [1, 3, 64, 100, 256, 260, 1024])
def test_forward_and_backward_every_width(f):
    """Rows of 0, 1, T - 1, T, T + 1 entries and the 1 000-entry hub, in-batch and history sources mixed."""
    ops = _ops()
    B = _agg_batch()
    h, hbar, da = _inputs(B, f, seed=f)
    a = _fwd(ops, B, _dev(h), _dev(hbar), item_cap=B.b.item_cap)
    ref = GO.aggregate(torch.from_numpy(h), torch.from_numpy(hbar), B.dv, B.node_idx, B.rowptr_h, B.code).numpy()
    ea = rel_err(_np(a), ref)
    dh = ops.gas_aggregate_bwd(_dev(da), B.b.node_idx, B.vg.dinv, B.b.prep)
    src, dst = GO.induced_edges(B.rowptr_h, B.code)
    eg = rel_err(_np(dh), GO.aggregate_bwd(torch.from_numpy(da), B.dv, B.node_idx, src, dst).numpy())
    print(f"[gas] f={f}: A err {ea:.2e}, dH err {eg:.2e}")
    assert B.b.item_cap == 18 and ea <= ACT_TOL and eg <= GRAD_TOL
    B.L.check()


def test_width_258_is_refused():
    ops = _ops()
    B = _agg_batch()
    h, hbar, da = _inputs(B, 258, seed=1)
    with pytest.raises(ValueError, match="width 258 is not built"):
        ops.gas_aggregate_fwd(_dev(h), _dev(hbar), B.vg.dinv, B.b.node_idx, B.b.rowptr_h, B.b.code, item_cap=0)
    with pytest.raises(ValueError, match="width 258 is not built"):
        ops.gas_aggregate_bwd(_dev(da), B.b.node_idx, B.vg.dinv, B.b.prep)


def test_every_row_by_one_group_and_two_calls():
    ops = _ops()
    B = _agg_batch()
    h, hbar, _ = _inputs(B, 100, seed=5)
    ref = GO.aggregate(torch.from_numpy(h), torch.from_numpy(hbar), B.dv, B.node_idx, B.rowptr_h, B.code).numpy()
    dh, dhbar = _dev(h), _dev(hbar)
    one = _fwd(ops, B, dh, dhbar, item_cap=0)
    cut = _fwd(ops, B, dh, dhbar, item_cap=B.b.item_cap)
    counted = _fwd(ops, B, dh, dhbar)                                    # item_cap counted by the wrapper
    assert rel_err(_np(one), ref) <= ACT_TOL and rel_err(_np(cut), ref) <= ACT_TOL
    assert torch.equal(cut, counted) and torch.equal(cut, _fwd(ops, B, dh, dhbar, item_cap=B.b.item_cap))
    assert torch.equal(one, _fwd(ops, B, dh, dhbar, item_cap=0))
    da = _dev(_inputs(B, 100, seed=6)[2])
    assert torch.equal(ops.gas_aggregate_bwd(da, B.b.node_idx, B.vg.dinv, B.b.prep), ops.gas_aggregate_bwd(da, B.b.node_idx, B.vg.dinv, B.b.prep))


def test_nan_where_nothing_may_read():
    """In-batch nodes never read their own history; the rows of a larger H buffer behind the batch's n are never read."""
    ops = _ops()
    B = _agg_batch()
    n, f = len(B.node_idx), 64
    h, hbar, _ = _inputs(B, f, seed=8)
    clean = _fwd(ops, B, _dev(h), _dev(hbar), item_cap=B.b.item_cap)
    hb = _dev(hbar)
    hb[B.b.node_idx.long()] = float("nan")
    hpad = torch.full((n + 9, f), float("nan"), device="cuda")
    hpad[:n] = _dev(h)
    for cap in (0, B.b.item_cap):
        out = _fwd(ops, B, hpad[:n], hb, item_cap=cap)
        assert bool(torch.isfinite(out).all())
        if cap:
            assert torch.equal(out, clean)


def test_every_cluster_gives_p_h_for_any_history():
    ops = _ops()
    B = _agg_batch(tuple(range(P_K)))
    assert B.b.num_halo == 0 and len(B.node_idx) == N_K
    h = np.random.default_rng(9).standard_normal((N_K, 24)).astype(F32)
    hglob = np.zeros((N_K, 24), F32)
    hglob[B.node_idx] = h
    ref = GO.propagate(B.S.rowptr, B.S.col, torch.from_numpy(hglob)).numpy()[B.node_idx]
    hbar = torch.full((N_K, 24), float("nan"), device="cuda")
    assert rel_err(_np(_fwd(ops, B, _dev(h), hbar, item_cap=B.b.item_cap)), ref) <= ACT_TOL


def test_history_equal_to_h_gives_p_hbar():
    ops = _ops()
    B = _agg_batch()
    h, hbar, _ = _inputs(B, 24, seed=10)
    hbar[B.node_idx] = h
    ref = GO.propagate(B.S.rowptr, B.S.col, torch.from_numpy(hbar)).numpy()[B.node_idx]
    assert rel_err(_np(_fwd(ops, B, _dev(h), _dev(hbar), item_cap=B.b.item_cap)), ref) <= ACT_TOL


def test_a_bad_code_is_dropped_and_raises():
    ops = _ops()
    B = _agg_batch()
    h, hbar, _ = _inputs(B, 8, seed=11)
    code = B.b.code.clone()
    at = int(B.rowptr_h[3]) + 2                                          # entries of the 64-entry row
    code[at], code[at + 1], code[at + 2] = len(B.node_idx), -N_K - 1, ops.GAS_BAD_CODE
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.gas_aggregate_fwd(_dev(h), _dev(hbar), B.vg.dinv, B.b.node_idx, B.b.rowptr_h, code, item_cap=0, status=status)
    assert int(status.item()) == 4
    hz, hbz = torch.from_numpy(h), torch.from_numpy(hbar)
    full = GO.aggregate(hz, hbz, B.dv, B.node_idx, B.rowptr_h, B.code).numpy()
    drop = np.zeros_like(full)
    for p in range(at, at + 3):
        c = int(B.code[p])
        v = B.node_idx[c] if c >= 0 else -1 - c
        drop[3] += float(B.dv[B.node_idx[3]] * B.dv[v]) * (h[c] if c >= 0 else hbar[v]).astype(F64)
    assert rel_err(_np(out), full - drop) <= ACT_TOL


# ------------------------------------------------------------------------------------------------------------ the trainer
def _trainer(n, F, widths, C, P, q, partition, seed):
    from grapes_amd.gas import GasTrainer
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    rowptr, col = GO.random_graph(n, 6.0, seed)                          # (duplicate-free, as a DeviceGraph is: the kernel tests store some)
    rng = np.random.default_rng(seed + 1)
    x32 = rng.standard_normal((n, F)).astype(F32)
    y = rng.integers(0, C, n)
    train = rng.random(n) < 0.6
    model = GCN(F, widths + [C]).cuda()
    with torch.no_grad():
        for c in model.gcn_layers:
            c.bias.uniform_(-0.2, 0.2)
    g = DeviceGraph(_dev(rowptr), _dev(col), n)
    tr = GasTrainer(g, _dev(x32), _dev(y), model, torch.optim.SGD(model.parameters(), lr=0.0), num_parts=P, batch_size=q,
                    partition=partition, seed=3, train_mask=_dev(train))
    return SimpleNamespace(tr=tr, model=model, rowptr=rowptr, col=col, x32=x32, y=y, train=train, g=g)


@pytest.mark.parametrize("partition,widths", [("random", [16]), ("range", [16, 12])])
def test_three_steps_against_the_oracle(partition, widths):
    """Three consecutive steps from the same weights (SGD with lr = 0); the second and the third read the histories the steps before
    them wrote."""
    _ops()
    n, F, C, P = 300, 12, 4, 6
    T = _trainer(n, F, widths, C, P, 2, partition, seed=21)
    part = _np(T.tr.cluster_data.part)
    weights = [(c.lin.weight.detach().cpu().double(), c.bias.detach().cpu().double()) for c in T.model.gcn_layers]
    x64, y, train = torch.from_numpy(T.x32).double(), torch.from_numpy(T.y), torch.from_numpy(T.train)
    assert rel_err(_np(T.tr.px), GO.propagate(T.rowptr, T.col, x64).numpy()) <= ACT_TOL
    hist = [torch.zeros(n, w, dtype=torch.float64) for w in widths]
    for stepno, clusters in enumerate([[0, 3], [3, 5], [1, 0]]):
        before = [t.clone() for t in T.tr.store.tables]
        loss, b = T.tr.step(clusters)
        node_idx = GO.batch_nodes(part, clusters)
        assert np.array_equal(_np(b.node_idx), node_idx) and b.num_halo > 0
        if stepno:
            assert all(float(t.abs().max()) > 0 for t in before)         # a non-zero history
        gates = [_np(h > 0) for _, h in b.activations]
        o_loss, dW, db, hist = GO.step(T.rowptr, T.col, x64, y, train, weights, hist, node_idx, gates=gates)
        assert abs(float(loss) - o_loss) <= ACT_TOL * max(1.0, abs(o_loss)), (stepno, float(loss), o_loss)
        for i, conv in enumerate(T.model.gcn_layers):
            ew, eb = rel_err(_np(conv.lin.weight.grad), dW[i].numpy()), rel_err(_np(conv.bias.grad), db[i].numpy())
            print(f"[gas] {partition} L={len(widths) + 1} step {stepno} layer {i}: loss {float(loss):.6f}, dW err {ew:.2e}, db err {eb:.2e}")
            assert ew <= GRAD_TOL and eb <= GRAD_TOL
        rows = _dev(node_idx)
        other = np.ones(n, bool); other[node_idx] = False
        for l, (level, h) in enumerate(b.activations):
            table = T.tr.store[level]
            assert level == l + 1 and torch.equal(table[rows], h) and rel_err(_np(table), hist[l].numpy()) <= ACT_TOL
            assert torch.equal(table[_dev(other)], before[l][_dev(other)])
    T.tr.check()
    T.tr.reset_histories()
    assert all(float(t.abs().max()) == 0 for t in T.tr.store.tables)


def test_every_cluster_gives_the_exact_loss_and_evaluate_is_exact():
    _ops()
    n, P = 300, 6
    T = _trainer(n, 12, [16], 4, P, P, "random", seed=31)
    T.tr.store[1].fill_(float("nan"))                                    # whatever the histories hold
    loss, b = T.tr.step(list(range(P)))
    assert b.num_halo == 0
    weights = [(c.lin.weight.detach().cpu().double(), c.bias.detach().cpu().double()) for c in T.model.gcn_layers]
    z = GO.full_forward(T.rowptr, T.col, torch.from_numpy(T.x32), weights)[-1]
    train = torch.from_numpy(T.train)
    exact = float(torch.nn.functional.cross_entropy(z[train], torch.from_numpy(T.y)[train]))
    assert abs(float(loss) - exact) <= ACT_TOL * max(1.0, abs(exact)), (float(loss), exact)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda"); mask[::2] = True
    val, test = T.tr.evaluate((mask, ~mask))
    pred, m = z.argmax(1).numpy(), _np(mask)
    assert abs(val - float((pred[m] == T.y[m]).mean())) <= 1e-6 and abs(test - float((pred[~m] == T.y[~m]).mean())) <= 1e-6


def test_trainer_refusals(monkeypatch):
    _ops()
    from grapes_amd.gas import GasTrainer
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN, ClusterGCN
    rowptr, col = GO.random_graph(50, 4.0, 3)
    g = DeviceGraph(_dev(rowptr), _dev(col), 50)
    x, y = torch.zeros(50, 4, device="cuda"), torch.zeros(50, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="dropout"):
        GasTrainer(g, x, y, GCN(4, [8, 2], dropout=0.5).cuda(), None, num_parts=4, batch_size=2)
    with pytest.raises(TypeError, match="project's GCN"):
        GasTrainer(g, x, y, ClusterGCN(4, hidden_dims=[8, 2]).cuda(), None, num_parts=4, batch_size=2)
    rp, cl = GO.csr_from_edges(50, np.asarray([0]), np.asarray([1]))     # one one-way entry
    with pytest.raises(ValueError, match="symmetric"):
        GasTrainer(DeviceGraph(_dev(rp), _dev(cl), 50), x, y, GCN(4, [8, 2]).cuda(), None, num_parts=4, batch_size=2)
    with pytest.raises(ValueError, match="batch_size"):
        GasTrainer(g, x, y, GCN(4, [8, 2]).cuda(), None, num_parts=4, batch_size=5)
    monkeypatch.setattr(DeviceGraph, "nnz", property(lambda self: 2 ** 31))
    with pytest.raises(ValueError, match="2\\^31 or more entries"):
        GasTrainer(g, x, y, GCN(4, [8, 2]).cuda(), None, num_parts=4, batch_size=2)


def test_cli_two_epochs(capsys):
    _ops()
    from grapes_amd import gas
    v = gas.main(["--dataset", "cora", "--num_parts", "8", "--batch_size", "2", "--partition", "lp:5:0.1", "--max_epoch", "2",
                  "--hidden_dim", "32", "--seed", "1"])
    out = capsys.readouterr().out
    assert "Partition: label propagation" in out and out.count("Epoch: ") == 2 and "Val: " in out and "Acc: " in out
    assert np.isfinite(v) and 0.0 <= v <= 1.0
