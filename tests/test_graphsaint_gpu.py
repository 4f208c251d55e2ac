"""GraphSAINT random-walk training on the MI355X (grapes_amd/saint.py, modules/saint.py, csrc/saint_kernels.hip) against the CPU
restatement in tests/saint_oracle.py, on injected roots and uniforms."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import saint_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _csr_from_edges(src, dst, n):
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    keep = np.ones(len(src), bool)
    keep[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    src, dst = src[keep], dst[keep]
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, src + 1, 1)
    return np.cumsum(indptr), dst.astype(np.int64)


def _graph(n=3000, directed=False, seed=0):
    """Random graph with degree-0 nodes, self-loop-only nodes and a hub row (node 7 -> every node)."""
    rng = np.random.default_rng(seed)
    m = 6 * n
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    iso = np.arange(0, n, 11)                      # isolated
    loops = np.arange(5, n, 13)                    # self-loop only
    bad = np.isin(s, np.concatenate([iso, loops])) | np.isin(d, np.concatenate([iso, loops]))
    s, d = s[~bad], d[~bad]
    if not directed:
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
    hub = np.setdiff1d(np.arange(n), np.concatenate([iso, loops]))
    s = np.concatenate([s, loops, np.full(len(hub), 7)])
    d = np.concatenate([d, loops, hub])
    return _csr_from_edges(s, d, n)


def _dev_graph(indptr, indices):
    from grapes_amd.graph import DeviceGraph
    return DeviceGraph.from_csr(indptr, indices)


def _draws(B, L, n, seed):
    rng = np.random.default_rng(seed)
    roots = rng.integers(0, n, B).astype(np.int32)
    u = rng.random((B, L), dtype=np.float32)
    return roots, u


@pytest.mark.parametrize("L", [0, 1, 2, 4])
def test_walks_bit_exact(L):
    _cuda()
    from grapes_amd import ops
    indptr, indices = _graph()
    g = _dev_graph(indptr, indices)
    B = 300
    roots, u = _draws(B, L, g.num_nodes, L)
    roots[:3] = [0, 5, 7]                  # isolated, self-loop only, hub
    walks, node_idx, cnt = ops.saint_walk_nodes(g.rowptr, g.col, g.num_nodes, B, L, roots=torch.from_numpy(roots).cuda(),
                                                uniforms=torch.from_numpy(u.reshape(-1)).cuda(), node_map=g.node_map)
    ref = O.walk(indptr, indices, roots, u, L)
    assert np.array_equal(walks.cpu().numpy(), ref)
    ns = O.node_set(ref)
    assert int(cnt.item()) == len(ns)
    assert np.array_equal(node_idx[:len(ns)].cpu().numpy(), ns)
    assert np.array_equal(g.node_map[torch.from_numpy(ns).cuda()].cpu().numpy(), np.arange(len(ns)))


def test_long_row_index_stays_below_deg():
    """A row of 2^24 + 3 entries at u = 1 - 2^-24 (fp32(deg) rounds up) and at u = 0.5."""
    _cuda()
    from grapes_amd import ops
    from grapes_amd.graph import DeviceGraph
    deg = 2 ** 24 + 3
    rowptr = torch.tensor([0, deg, deg], dtype=torch.int64, device="cuda")
    col = (torch.arange(deg, device="cuda", dtype=torch.int64) % 2).to(torch.int32) + 0
    col[-8:] = torch.tensor([1, 1, 1, 1, 1, 1, 0, 1], dtype=torch.int32, device="cuda")
    g = DeviceGraph(rowptr, col, 2)
    u = np.array([[1.0 - 2.0 ** -24], [0.5]], dtype=np.float32)
    walks, _, _ = ops.saint_walk_nodes(g.rowptr, g.col, 2, 2, 1, roots=torch.zeros(2, dtype=torch.int32, device="cuda"),
                                       uniforms=torch.from_numpy(u.reshape(-1)).cuda(), node_map=g.node_map)
    col_h = np.arange(deg, dtype=np.int64) % 2
    col_h[-8:] = [1, 1, 1, 1, 1, 1, 0, 1]
    ref = O.walk(np.array([0, deg, deg]), col_h, [0, 0], u, 1)
    assert np.array_equal(walks.cpu().numpy(), ref)
    del g, col


def test_rows_past_2_31_entries():
    """Node 0 holds 2^31 + 64 entries (~8 GiB of col); nodes 1 .. 63 start past entry 2^31."""
    _cuda()
    from grapes_amd import ops
    from grapes_amd.graph import DeviceGraph
    n, big = 64, 2 ** 31 + 64
    degs = np.array([big] + [3] * (n - 1), np.int64)
    rowptr = np.concatenate([[0], np.cumsum(degs)])
    col = torch.empty(int(rowptr[-1]), dtype=torch.int32, device="cuda")
    col[:big].fill_(1)
    col[big - 1] = 2
    tail = np.stack([(np.arange(1, n) + k) % n for k in (1, 2, 3)], 1).astype(np.int32)
    tail.sort(1)
    col[big:] = torch.from_numpy(tail.reshape(-1)).cuda()
    g = DeviceGraph(torch.from_numpy(rowptr).cuda(), col, n)
    B, L = 200, 4
    roots, u = _draws(B, L, n, 9)
    roots[:2] = 0
    u[0, 0] = np.float32(1.0 - 2.0 ** -24)
    walks, _, _ = ops.saint_walk_nodes(g.rowptr, g.col, n, B, L, roots=torch.from_numpy(roots).cuda(),
                                       uniforms=torch.from_numpy(u.reshape(-1)).cuda(), node_map=g.node_map)

    class _Col:                                   # the oracle reads col lazily: host copy only of the tail and node 0's row
        def __getitem__(self, i):
            if i < big:
                return 2 if i == big - 1 else 1
            return int(tail.reshape(-1)[i - big])
    ref = O.walk(rowptr, _Col(), roots, u, L)
    assert np.array_equal(walks.cpu().numpy(), ref)
    del g, col
    torch.cuda.empty_cache()


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("B", [256, 4000])
def test_node_set_and_induced_subgraph(directed, B):
    _cuda()
    from grapes_amd.modules.saint import GraphSAINTRandomWalkSampler
    indptr, indices = _graph(n=20000, directed=directed, seed=B)
    g = _dev_graph(indptr, indices)
    L = 2
    roots, u = _draws(B, L, g.num_nodes, 3)
    ld = GraphSAINTRandomWalkSampler(g, B, L, seed=1)
    b = ld.batch(torch.from_numpy(roots).cuda(), torch.from_numpy(u.reshape(-1)).cuda())
    ns = O.node_set(O.walk(indptr, indices, roots, u, L))
    assert b.num_nodes == len(ns) and np.array_equal(b.node_idx.cpu().numpy(), ns)
    if B == 4000:
        assert b.num_nodes > 2048
    src, dst = O.induced_subgraph(indptr, indices, ns)
    ei = b.edge_index.cpu().numpy()
    assert b.edge_index.dtype == torch.int64 and np.array_equal(ei[0], src) and np.array_equal(ei[1], dst)
    assert np.array_equal(g.node_map[b.node_idx].cpu().numpy(), np.arange(len(ns)))


def _setup(multi=False, embed=False, n=2000, F=24, C=5, H=32, seed=0, train_frac=0.3):
    from grapes_amd.saint import build_model
    indptr, indices = _graph(n=n, seed=seed)
    g = _dev_graph(indptr, indices)
    rng = np.random.default_rng(seed + 7)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).cuda()
    if embed:
        x = torch.nn.Parameter(x)
    y = (torch.from_numpy((rng.random((n, C)) < 0.3).astype(np.float32)) if multi else
         torch.from_numpy(rng.integers(0, C, n))).cuda()
    tm = torch.from_numpy(rng.random(n) < train_frac).cuda()
    torch.manual_seed(seed)
    model = build_model(F, H, C, "cuda")
    return indptr, indices, g, x, y, tm, model


def _check(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = 1e-4 * max(float(np.abs(b).max()), 1e-30)
    assert float(np.abs(a - b).max()) <= tol, (what, float(np.abs(a - b).max()), tol)


@pytest.mark.parametrize("multi,embed", [(False, False), (True, False), (False, True)])
def test_one_step_against_fp64(multi, embed):
    _cuda()
    from grapes_amd.modules.saint import GraphSAINTRandomWalkSampler
    from grapes_amd.saint import masked_loss
    from grapes_amd.target_batch import _GatherX
    indptr, indices, g, x, y, tm, model = _setup(multi, embed)
    B, L = 64, 2
    roots, u = _draws(B, L, g.num_nodes, 5)
    ld = GraphSAINTRandomWalkSampler(g, B, L, seed=0)
    b = ld.batch(torch.from_numpy(roots).cuda(), torch.from_numpy(u.reshape(-1)).cuda())
    ids = b.node_idx.to(torch.int32)
    if embed:
        x.grad = torch.zeros_like(x)
    xr = _GatherX.apply(x, ids, None, None, embed)
    out, _ = model(xr, b.edge_index)
    loss = masked_loss(out, ids, None, tm, y)
    loss.backward()
    ns = b.node_idx.cpu().numpy()
    src, dst = O.induced_subgraph(indptr, indices, ns)
    c1, c2 = model.gcn_layers
    ws = [c1.lin.weight, c1.bias, c2.lin.weight, c2.bias]
    tr = np.nonzero(tm.cpu().numpy()[ns])[0]
    assert len(tr) > 0
    ref_loss, ref_g = O.step_fp64(x.detach().cpu().numpy()[ns], src, dst, len(ns), [w.detach().cpu().numpy() for w in ws], tr,
                                  y.cpu().numpy()[ns])
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    for w, r, name in zip(ws, ref_g[:4], ("W1", "b1", "W2", "b2")):
        _check(w.grad.cpu().numpy(), r, name)
    if embed:
        gx = x.grad.cpu().numpy()
        _check(gx[ns], ref_g[4], "X rows")
        rest = np.ones(g.num_nodes, bool); rest[ns] = False
        assert not gx[rest].any() and np.abs(gx[ns]).sum(1).min() >= 0 and np.abs(gx[ns]).sum() > 0


def test_batch_without_train_rows():
    _cuda()
    from grapes_amd.saint import EagerSaintTrainer
    indptr, indices, g, x, y, tm, model = _setup()
    tm = torch.zeros_like(tm)
    ref = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    tr = EagerSaintTrainer(g, x, y, tm, model, opt, batch_size=32, walk_length=2, seed=4)
    opt.zero_grad()
    loss, _ = tr.step()
    assert torch.isnan(loss)
    for p in model.parameters():
        assert p.grad is not None and not p.grad.any() and not torch.isnan(p.grad).any()
    # torch.optim.Adam with exactly-zero gradients from the same weights
    refp = [torch.nn.Parameter(r) for r in ref]
    ropt = torch.optim.Adam(refp, lr=0.01)
    for r in refp:
        r.grad = torch.zeros_like(r)
    ropt.step()
    for p, r in zip(model.parameters(), refp):
        assert torch.equal(p.detach(), r.detach())
    assert all(s["step"] == 1 for s in opt.state.values())


def test_captured_matches_eager_and_replays_draw_fresh_batches():
    _cuda()
    from grapes_amd.saint import make_trainer
    runs = {}
    for engine in ("eager", "graph", "graph"):
        indptr, indices, g, x, y, tm, model = _setup(n=3000, seed=2)
        tr = make_trainer(engine, g, x, y, tm, model, 0.01, batch_size=128, walk_length=2, seed=77)
        sets = []
        for _ in range(5):
            if engine == "eager":
                _, b = tr.step()
                sets.append((b.node_idx.cpu().numpy(), b.edge_index.cpu().numpy()))
            else:
                tr.step()
                n, e = int(tr.walk_out[2].item()), int(tr.sub_out[2].item())
                sets.append((tr.walk_out[1][:n].long().cpu().numpy(),
                             torch.stack([tr.sub_out[0][:e], tr.sub_out[1][:e]]).long().cpu().numpy()))
        tr.check()
        runs.setdefault(engine, []).append((sets, [p.detach().cpu().numpy() for p in model.parameters()]))
    (es, ew), = runs["eager"]
    (gs, gw), (gs2, gw2) = runs["graph"]
    for a, b in zip(es, gs):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert len({tuple(s[0][:20]) for s in gs}) > 1                   # successive replays draw different batches
    for a, b in zip(gs, gs2):                                          # same seed: the same batches again
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for a, b in zip(gw, gw2):
        assert np.array_equal(a, b)
    for a, b in zip(ew, gw):                                           # torch Adam vs FusedAdam, 5 steps of lr 0.01
        assert float(np.abs(a - b).max()) <= 2e-3


def test_small_e_cap_sets_status_then_recovers():
    _cuda()
    from grapes_amd import _lib
    from grapes_amd.modules.saint import GraphSAINTRandomWalkSampler
    indptr, indices = _graph(n=3000)
    g = _dev_graph(indptr, indices)
    B, L = 64, 2
    ld = GraphSAINTRandomWalkSampler(g, B, L, seed=0, e_cap=8)
    roots, u = _draws(B, L, g.num_nodes, 1)
    ld.sample(torch.from_numpy(roots).cuda(), torch.from_numpy(u.reshape(-1)).cuda())
    with pytest.raises(_lib.GrapesHipError):
        ld.check()
    roots = np.array([0, 5, 11, 22] * 16, np.int32)      # isolated and self-loop-only nodes: one self-loop edge
    b = ld.batch(torch.from_numpy(roots).cuda(), torch.from_numpy(u.reshape(-1)).cuda())
    ns = O.node_set(O.walk(indptr, indices, roots, u, L))
    src, dst = O.induced_subgraph(indptr, indices, ns)
    assert np.array_equal(b.node_idx.cpu().numpy(), ns)
    assert np.array_equal(b.edge_index.cpu().numpy(), np.stack([src, dst]))


def test_cli_cora_three_epochs_two_runs():
    _cuda()
    r = subprocess.run([sys.executable, "-m", "grapes_amd.graphsaint", "--dataset", "cora", "--max_epoch", "3", "--runs", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    ep = [l for l in lines if l.startswith("Epoch: ")]
    assert len(ep) == 6 and ep[0].startswith("Epoch: 01, Loss: ") and ", Val: " in ep[0] and ", Test: " in ep[0], r.stdout
    assert sum(l.startswith("Acc: ") for l in lines) == 1, r.stdout
