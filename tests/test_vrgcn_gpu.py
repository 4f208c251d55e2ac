"""VR-GCN on the MI355X (grapes_amd/csrc/vrgcn_kernels.hip, modules/vrgcn.py, vrgcn.py) against the fp64 host oracle of
tests/vrgcn_oracle.py.

Activations and gradients are judged by the project's measure (gat_oracle.rel_err: max |a - ref| / max(1, max |ref|)) at its
tolerances, 1e-5 and 1e-4; the backward of a ReLU is compared on the device's own gates, so a pre-activation within fp32 rounding of
0 cannot flip a whole gradient row.  Every graph has at most 1 100 nodes, but the one of the row list past one scan tile (5 000)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import ladies_oracle as LO
from tests import sage_oracle as SO
from tests import vrgcn_oracle as VO
from tests.gat_oracle import rel_err

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4
F32, F64 = np.float32, np.float64
K = 2                                                                    # the fanout of the kernel tests
N_K = 1100
N_BIG = 5000                                                             # the graph of the row list longer than one scan tile (4 096 rows)
DEGREES = [0, K - 1, K, K + 1, 63, 64, 65, 129, 1000]                    # rows 0 .. 8; row 9 stores duplicate entries
HUB, DUP = 8, 9


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(4321)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


_KG = {}


def _kernel_graph(n=N_K):
    """(indptr, indices, kept) over n nodes: rows 0 .. 8 have DEGREES distinct columns among the nodes 16 .., row 9 stores
    (20, 20, 31, 40), every later row 0 .. 5 random columns (so dinv varies); loop-free, not symmetric — the kernels read rows only.
    kept[u] = K of row u's entries (all of them for d <= K), row 9 keeps both copies of its duplicate."""
    if n not in _KG:
        rng = np.random.default_rng(7)
        rows = [sorted(rng.choice(np.arange(16, n), d, replace=False).tolist()) for d in DEGREES] + [[20, 20, 31, 40]]
        for u in range(10, n):
            c = rng.choice(n, int(rng.integers(0, 6)), replace=False)
            rows.append(sorted(int(v) for v in c if v != u))
        ip, ix = SO.csr_from_rows(rows)
        kept = {}
        for u in range(n):
            cols = np.asarray(rows[u], dtype=np.int64)
            kept[u] = cols if len(cols) <= K else cols[np.sort(rng.choice(len(cols), K, replace=False))]
        kept[DUP] = np.array([20, 20], dtype=np.int64)
        _KG[n] = dict(n=n, ip=ip, ix=ix.astype(np.int64), kept=kept, d_rowptr=_dev(ip), d_col=_dev(ix.astype(np.int32)),
                      d_dinv=_dev(VO.dinv(ip).astype(F32)))
    return _KG[n]


def _batch(rows, kept, n=N_K, extra=(3, 500, 1099)):
    """The batch of the listed rows: node_idx = the ascending union of the rows, their kept sources and a few bystanders; the kept
    entries as local lists in the rows' order."""
    node_idx = np.unique(np.concatenate([np.asarray(rows, dtype=np.int64)] + [np.asarray(k, dtype=np.int64) for k in kept] +
                                        [np.asarray(extra, dtype=np.int64)]))
    loc = np.full(n, -1, np.int64)
    loc[node_idx] = np.arange(len(node_idx))
    src = np.concatenate([np.asarray(k, dtype=np.int64) for k in kept]) if len(kept) else np.zeros(0, np.int64)
    dst = np.concatenate([np.full(len(k), u, np.int64) for u, k in zip(rows, kept)]) if len(kept) else np.zeros(0, np.int64)
    return node_idx, loc, loc[src].astype(np.int32), loc[dst].astype(np.int32)


def _run(ops, rows, kept, f, seed, item_cap=None, hbar_from_h=False, col=None, status=None, n=N_K):
    """The forward and the backward of one case on the device and in the oracle."""
    G = _kernel_graph(n)
    rows = np.asarray(rows, dtype=np.int64)
    node_idx, loc, ls, ld = _batch(rows, kept, n)
    n_local, m = len(node_idx), len(rows)
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((n_local, f)).astype(F32)
    Hbar = rng.standard_normal((n, f)).astype(F32)
    if hbar_from_h:
        Hbar[node_idx] = H
    dA = rng.standard_normal((m, f)).astype(F32)
    if len(ls):
        prep = ops.PreparedGraph(_dev(ls), _dev(ld), n_local)
    else:
        from grapes_amd.modules.vrgcn import _KeptEntries
        prep = _KeptEntries(torch.zeros((2, 0), dtype=torch.int32, device="cuda"), n_local, None)
    d_H, d_Hbar = _dev(H), _dev(Hbar)
    keep = d_Hbar.clone()
    d_idx, d_rows, d_rl = _dev(node_idx.astype(np.int32)), _dev(rows.astype(np.int32)), _dev(loc[rows].astype(np.int32))
    pos = np.full(n_local, -1, np.int32)
    pos[loc[rows]] = np.arange(m)
    st = status if status is not None else torch.zeros(1, dtype=torch.int32, device="cuda")
    fwd = lambda: ops.vrgcn_aggregate_fwd(d_H, d_idx, d_Hbar, G["d_dinv"], G["d_rowptr"], G["d_col"] if col is None else col, d_rows,
                                          d_rl, prep, item_cap=item_cap, status=st)
    A, coef = fwd()
    bwd = lambda: ops.vrgcn_aggregate_bwd(_dev(dA), coef, _dev(pos), d_idx, G["d_dinv"], prep, status=st)
    dH = bwd()
    Hg = np.zeros((n, f))
    Hg[node_idx] = H
    out = dict(A=_np(A), dH=_np(dH), fwd=fwd, bwd=bwd, status=st, hbar_same=bool(torch.equal(d_Hbar, keep)), node_idx=node_idx,
               Hg=Hg, Hbar=Hbar.astype(F64), rows=rows)
    if col is None:
        out["A64"] = VO.aggregate(G["ip"], G["ix"], rows, kept, Hg, Hbar)
        out["dH64"] = VO.aggregate_grad(G["ip"], rows, kept, dA, n)[node_idx]
    return out


ALL_ROWS = [HUB, 3, 0, 7, 1, DUP, 5, 2, 6, 4]                            # non-ascending, the 1 000-entry row first


def _check(r, what):
    ea, eg = rel_err(r["A"], r["A64"]), rel_err(r["dH"], r["dH64"])
    print(f"[vrgcn] {what}: A err {ea:.2e}, dH err {eg:.2e}")
    assert int(r["status"].item()) == 0
    assert ea <= ACT_TOL and eg <= GRAD_TOL
    assert r["hbar_same"]                                                # the history is bit-unchanged by both passes


@pytest.mark.parametrize("f", [1, 3, 32, 33, 64, 100, 128, 256, 260])
def test_forward_and_backward_every_width(f):
    ops = _ops()
    G = _kernel_graph()
    deg = np.diff(G["ip"])[ALL_ROWS]
    T = ops.VRGCN_LONG_ROW                                               # both sides of the threshold occur, and the rows next to it
    assert T % 64 == 0 and (deg > T).any() and ((deg > 0) & (deg <= T)).any() and {T - 1, T, T + 1} <= set(deg.tolist())
    assert sorted(deg.tolist()) == sorted(DEGREES + [4])
    _check(_run(ops, ALL_ROWS, [G["kept"][u] for u in ALL_ROWS], f, seed=10 + f), f"f={f}")


def test_width_258_is_refused():
    ops = _ops()
    G = _kernel_graph()
    with pytest.raises(ValueError, match="width 258 is not built"):
        _run(ops, [3], [G["kept"][3]], 258, seed=1)


@pytest.mark.parametrize("name,rows", [("hub last", [3, 0, 7, 1, DUP, 5, 2, 6, 4, HUB]), ("hub alone", [HUB]), ("m = 1", [4]),
                                       ("an empty row alone", [0]), ("no long row", [5, 2, 4]),
                                       ("only long rows", [6, 7])])
@pytest.mark.parametrize("f", [32, 260])
def test_row_lists(name, rows, f):
    ops = _ops()
    G = _kernel_graph()
    longer = np.diff(G["ip"])[rows] > ops.VRGCN_LONG_ROW
    assert not (name == "no long row" and longer.any()) and not (name == "only long rows" and not longer.all())
    _check(_run(ops, rows, [G["kept"][u] for u in rows], f, seed=3), f"{name}, f={f}")


def test_every_row_by_one_group_is_the_same_sum_up_to_rounding():
    """item_cap = 0 walks every row, the 1 000-entry one too, in one group: the other summation order, within the same tolerance."""
    ops = _ops()
    G = _kernel_graph()
    kept = [G["kept"][u] for u in ALL_ROWS]
    _check(_run(ops, ALL_ROWS, kept, 64, seed=5, item_cap=0), "item_cap = 0")
    need = ops.vrgcn_item_cap(G["d_rowptr"], _dev(np.asarray(ALL_ROWS, dtype=np.int32)))
    T = ops.VRGCN_LONG_ROW
    assert need == sum(-(-d // T) for d in np.diff(G["ip"])[ALL_ROWS] if d > T)
    _check(_run(ops, ALL_ROWS, kept, 64, seed=5, item_cap=need + 5), "a capacity above the rows' chunks")


def test_a_row_list_past_one_scan_tile():
    """4 303 distinct listed rows, more than one tile (4 096) of a one-workgroup row-list prefix and five rows to a thread of
    vrgcn_items_k.  The 1 000-entry row is listed first, the rows of 129 and 65 entries behind position 4 096.  item_cap exact, then one too few (the
    overflow bit; the result is then invalid and is not looked at)."""
    ops = _ops()
    G = _kernel_graph(N_BIG)
    rows = [HUB] + list(range(10, 4310)) + [7, 6]
    deg, T = np.diff(G["ip"])[rows], ops.VRGCN_LONG_ROW
    assert len(rows) > 4096 + 2 and deg[0] > T and (deg[-2:] > T).all() and not (deg[1:-2] > T).any()
    need = ops.vrgcn_item_cap(G["d_rowptr"], _dev(np.asarray(rows, dtype=np.int32)))
    assert need == sum(-(-d // T) for d in deg if d > T)
    kept = [G["kept"][u] for u in rows]
    _check(_run(ops, rows, kept, 32, seed=12, item_cap=need, n=N_BIG), "4 303 rows, item_cap exact")
    r = _run(ops, rows, kept, 32, seed=12, item_cap=need - 1, n=N_BIG)
    assert int(r["status"].item()) == 1                                  # GRAPES_STATUS_EDGE_OVERFLOW


def test_two_calls_are_bit_equal():
    ops = _ops()
    G = _kernel_graph()
    for f in (33, 256):
        r = _run(ops, ALL_ROWS, [G["kept"][u] for u in ALL_ROWS], f, seed=6)
        a2, _ = r["fwd"]()
        assert np.array_equal(_np(a2), r["A"]) and np.array_equal(_np(r["bwd"]()), r["dH"])


def test_every_neighbour_kept_gives_p_h_for_any_history():
    ops = _ops()
    G = _kernel_graph()
    kept = [G["ix"][G["ip"][u]:G["ip"][u + 1]] for u in ALL_ROWS]        # fanout -1
    r = _run(ops, ALL_ROWS, kept, 32, seed=8)
    _check(r, "fanout -1")
    P = VO.dense_p(G["ip"], G["ix"], N_K)
    assert rel_err(r["A"], (P @ r["Hg"])[r["rows"]]) <= ACT_TOL


def test_history_equal_to_h_gives_p_hbar_whatever_is_kept():
    ops = _ops()
    G = _kernel_graph()
    r = _run(ops, ALL_ROWS, [G["kept"][u] for u in ALL_ROWS], 32, seed=9, hbar_from_h=True)
    _check(r, "Hbar[node_idx] = H")
    P = VO.dense_p(G["ip"], G["ix"], N_K)
    assert rel_err(r["A"], (P @ r["Hbar"])[r["rows"]]) <= ACT_TOL


def test_a_bad_column_raises_through_check():
    """The kernels write the trainer's status word (the sampler's): check() names the bit and clears it."""
    ops = _ops()
    from grapes_amd._lib import GrapesHipError
    G = _kernel_graph()
    col = G["d_col"].clone()
    col[int(G["ip"][7]) + 5] = N_K + 3                                   # an entry of the 129-entry row
    T = _trainer(50, 4, [8], 3, [2, 2], seed=3)
    status = T.tr.sampler.status
    T.tr.check()                                                         # clean
    r = _run(ops, [7, 2], [G["kept"][7], G["kept"][2]], 32, seed=2, col=col, status=status)
    assert np.isfinite(r["A"]).all()
    with pytest.raises(GrapesHipError, match="index out of range"):
        T.tr.check()
    assert int(status.item()) == 0
    T.tr.check()


# ------------------------------------------------------------------------------------------------------------ the trainer
def _params(model):
    return ([_np(c.lin.weight).astype(F64) for c in model.gcn_layers], [_np(c.bias).astype(F64) for c in model.gcn_layers])


def _trainer(n, F, widths, C, fanouts, seed, loops=0, max_deg=8, lr=0.0):
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    from grapes_amd.vrgcn import VrgcnTrainer
    ip, ix = LO.random_symmetric(n, max_deg, seed, loops=loops)
    rng = np.random.default_rng(seed + 1)
    x32 = rng.standard_normal((n, F)).astype(F32)
    y = rng.integers(0, C, n)
    model = GCN(F, widths + [C]).cuda()
    with torch.no_grad():
        for c in model.gcn_layers:
            c.bias.uniform_(-0.2, 0.2)
    g = DeviceGraph.from_csr(ip, ix)
    tr = VrgcnTrainer(g, _dev(x32), _dev(y), model, torch.optim.SGD(model.parameters(), lr=lr), fanouts=fanouts, seed=3)
    return SimpleNamespace(tr=tr, model=model, ip=ip, ix=ix, x32=x32, y=y, rng=rng, g=g,
                           o=VO.Trainer64(ip, ix, x32, widths))



def _device_gates(b):
    return [_np(h[rows_l.long()] > 0) for _, rows_l, h in b.activations]


@pytest.mark.parametrize("widths,fanouts", [([16], [2, 2]), ([16, 12], [2, 3, 2])])
def test_three_steps_against_the_oracle(widths, fanouts):
    """Three consecutive steps from the same weights (SGD with lr = 0) with injected keys; the second and the third read the
    histories the steps before them wrote."""
    _ops()
    n, F, C, B = 300, 12, 4, 24
    T = _trainer(n, F, widths, C, fanouts, seed=21, loops=5)
    Ws, bs = _params(T.model)
    L = len(fanouts)
    for stepno in range(3):
        targets = T.rng.permutation(n)[:B]
        words = [T.rng.integers(0, 2 ** 32, 40000, dtype=np.uint64).astype(np.uint32) for _ in range(L)]
        before = [t.clone() for t in T.tr.store.tables]
        loss, b = T.tr.step(_dev(targets), keys=[_dev(w.view(np.int32)) for w in words])
        ob = SO.sample(T.o.indptr, T.o.indices, targets, fanouts, keys=words)
        assert np.array_equal(_np(b.node_idx), ob.node_idx)
        if stepno:
            assert all(float(t.abs().max()) > 0 for t in before)         # a non-zero history
        out = T.o.step(Ws, bs, VO.batch_layers(ob), T.y[targets], gates=_device_gates(b))
        assert abs(float(loss) - out.loss) <= ACT_TOL * max(1.0, abs(out.loss)), (stepno, float(loss), out.loss)
        for i, conv in enumerate(T.model.gcn_layers):
            ew, eb = rel_err(_np(conv.lin.weight.grad), out.dW[i]), rel_err(_np(conv.bias.grad), out.db[i])
            print(f"[vrgcn] L={L} step {stepno} layer {i}: loss {float(loss):.6f}, dW err {ew:.2e}, db err {eb:.2e}")
            assert ew <= GRAD_TOL and eb <= GRAD_TOL
        # the histories: exactly the computed rows of each level hold the step's activations, every other row is bit-unchanged
        for l, (rows, h64) in enumerate(out.acts):
            _, rows_l, h = b.activations[l]
            table = T.tr.store[l + 1]
            assert np.array_equal(_np(b.node_idx)[_np(rows_l)], rows)
            assert torch.equal(table[_dev(rows)], h[rows_l.long()]) and rel_err(_np(table[_dev(rows)]), h64) <= ACT_TOL
            other = np.ones(n, bool); other[rows] = False
            assert torch.equal(table[_dev(other)], before[l][_dev(other)])
    T.tr.store.reset()
    assert all(float(t.abs().max()) == 0 for t in T.tr.store.tables)


def test_all_neighbour_fanouts_give_the_exact_loss():
    _ops()
    n, B = 300, 32
    T = _trainer(n, 12, [16], 4, [-1, -1], seed=31)
    T.tr.step(_dev(T.rng.permutation(n)[:B]))                            # (leaves a non-zero history behind)
    targets = T.rng.permutation(n)[:B]
    loss, _ = T.tr.step(_dev(targets))
    with torch.no_grad():
        z = _np(T.model(_dev(T.x32), T.g)[0]).astype(F64)
    exact, _ = VO.loss_and_grad(z[targets], T.y[targets])
    assert abs(float(loss) - exact) <= ACT_TOL * max(1.0, abs(exact)), (float(loss), exact)


def test_stored_self_loops_train_and_evaluate_with_the_oracles_p():
    _ops()
    n, B = 200, 16
    T = _trainer(n, 10, [8], 3, [2, 2], seed=41, loops=25)
    assert T.tr.sampler.graph.nnz == T.g.nnz - 25 and T.tr.full_graph is T.g
    Ws, bs = _params(T.model)
    targets = T.rng.permutation(n)[:B]
    words = [T.rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    loss, b = T.tr.step(_dev(targets), keys=[_dev(w.view(np.int32)) for w in words])
    ob = SO.sample(T.o.indptr, T.o.indices, targets, [2, 2], keys=words)
    out = T.o.step(Ws, bs, VO.batch_layers(ob), T.y[targets], gates=_device_gates(b))
    assert abs(float(loss) - out.loss) <= ACT_TOL * max(1.0, abs(out.loss))
    assert rel_err(_np(T.model.gcn_layers[0].lin.weight.grad), out.dW[0]) <= GRAD_TOL
    P = VO.dense_p(T.o.indptr, T.o.indices, n)                           # of the loop-free copy = gcn_norm's of the graph as stored
    z64 = P @ np.maximum(P @ T.x32.astype(F64) @ Ws[0].T + bs[0], 0) @ Ws[1].T + bs[1]
    with torch.no_grad():
        z = _np(T.model(_dev(T.x32), T.g)[0])
    assert rel_err(z, z64) <= ACT_TOL
    mask = torch.zeros(n, dtype=torch.bool, device="cuda"); mask[::2] = True
    val, test = T.tr.evaluate((mask, ~mask))
    pred = z.argmax(1)
    m = _np(mask)
    assert abs(val - float((pred[m] == T.y[m]).mean())) <= 1e-6 and abs(test - float((pred[~m] == T.y[~m]).mean())) <= 1e-6


def test_trainer_refusals():
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    from grapes_amd.vrgcn import VrgcnTrainer
    ip, ix = LO.random_symmetric(50, 4, 3)
    g = DeviceGraph.from_csr(ip, ix)
    x, y = torch.zeros(50, 4, device="cuda"), torch.zeros(50, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="fanouts"):
        VrgcnTrainer(g, x, y, GCN(4, [8, 2]).cuda(), None, fanouts=[2])
    with pytest.raises(ValueError, match="dropout"):
        VrgcnTrainer(g, x, y, GCN(4, [8, 2], dropout=0.5).cuda(), None, fanouts=[2, 2])
    ipd, ixd = SO.csr_from_rows([[1], []] + [[] for _ in range(48)])       # one one-way entry
    with pytest.raises(ValueError, match="symmetric"):
        VrgcnTrainer(DeviceGraph.from_csr(ipd, ixd), x, y, GCN(4, [8, 2]).cuda(), None, fanouts=[2, 2])


def test_cli_two_epochs(capsys):
    _ops()
    from grapes_amd import vrgcn
    v = vrgcn.main(["--dataset", "cora", "--max_epoch", "2", "--hidden_dim", "32", "--seed", "1"])
    out = capsys.readouterr().out
    assert out.count("Epoch: ") == 2 and "Val: " in out and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0
