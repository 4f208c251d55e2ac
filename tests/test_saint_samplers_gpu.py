"""GraphSAINT node and edge samplers on the MI355X (modules/saint.py, saint.py, csrc/saint_kernels.hip) against the integer
restatement in tests/saint_samplers_oracle.py: the weight table, injected and Philox draws, the distribution, the two trainers
and the driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

from tests import saint_samplers_oracle as S
from tests.test_graphsaint_gpu import _csr_from_edges, _dev_graph, _graph, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graphsaint_cli_rw_seed5.txt")


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _hub_graph(directed, n=30000, seed=0):
    """Sparse random graph with three hub rows of 20000, 12345 and 5000 entries, isolated nodes and stored self-loops."""
    rng = np.random.default_rng(seed)
    m = 4 * n
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    iso = np.arange(0, n, 17)
    bad = np.isin(s, iso) | np.isin(d, iso)
    s, d = s[~bad], d[~bad]
    rest = np.setdiff1d(np.arange(n), iso)
    for hub, k in ((3, 20000), (4, 5000), (9, 12345)):
        s = np.concatenate([s, np.full(k, hub)])
        d = np.concatenate([d, rng.choice(rest, k, replace=False)])
    loops = np.arange(2, n, 19)
    loops = loops[~np.isin(loops, iso)]
    s, d = np.concatenate([s, loops]), np.concatenate([d, loops])
    if not directed:
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
    return _csr_from_edges(s, d, n)


def _graphs():
    return {"cora-like": _graph(n=3000, seed=1), "cora-like directed": _graph(n=3000, directed=True, seed=2),
            "hubs": _hub_graph(False), "hubs directed": _hub_graph(True)}


def _sampler(kind, g, B, **kw):
    from grapes_amd.modules.saint import make_sampler
    return make_sampler(kind, g, B, **kw)


@pytest.mark.parametrize("name", ["cora-like", "cora-like directed", "hubs", "hubs directed"])
def test_weight_table_equals_the_oracle(name):
    _cuda()
    from grapes_amd import ops
    indptr, indices = _graphs()[name]
    g = _dev_graph(indptr, indices)
    if name.startswith("hubs"):
        deg = np.diff(indptr)
        assert deg[3] >= 20000 and deg[9] >= 12345 and 5000 <= deg[4] <= 20000
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cc, blockw, roww = ops.saint_edge_weights(g.rowptr, g.col, g.num_nodes, status=status)
    rc, rb, rr = S.weight_table(indptr, indices)
    assert int(status.item()) == 0
    assert cc.dtype == torch.int32 and blockw.dtype == torch.int64 and roww.dtype == torch.int64
    assert np.array_equal(cc.cpu().numpy(), rc)
    assert np.array_equal(blockw.cpu().numpy(), rb)
    assert np.array_equal(roww.cpu().numpy(), rr)


def _boundary_draws(indptr, indices, kind, B, seed):
    """B values t: 0, total - 1, both sides of every block boundary of the three longest rows, duplicates, random values."""
    rng = np.random.default_rng(seed)
    if kind == "node":
        total = len(indices)
        cum = np.arange(1, total + 1)
    else:
        cum = np.cumsum(S.entry_weights(indptr, indices))
        total = int(cum[-1])
    t = [0, total - 1, 0, total - 1]
    for r in np.argsort(np.diff(indptr))[-3:]:
        a, e = int(indptr[r]), int(indptr[r + 1])
        for j in list(range(a, e, 64)) + [e - 1]:
            t += [int(cum[j]) - 1, int(cum[j - 1]) if j else 0]          # last value of entry j, first value of entry j
    t = np.array(t[:B - 64], dtype=np.int64)
    t = np.clip(t, 0, total - 1)
    dup = rng.choice(t, 32)
    out = np.concatenate([t, dup, rng.integers(0, total, B - len(t) - len(dup))]).astype(np.int64)
    return out, total


@pytest.mark.parametrize("kind", ["node", "edge"])
@pytest.mark.parametrize("name", ["cora-like directed", "hubs", "hubs directed"])
def test_injected_draws_equal_the_oracle(kind, name):
    _cuda()
    indptr, indices = _graphs()[name]
    g = _dev_graph(indptr, indices)
    B = 2048
    t, total = _boundary_draws(indptr, indices, kind, B, 3)
    ld = _sampler(kind, g, B, seed=1)
    b = ld.batch(torch.from_numpy(t).cuda())
    ent, ids = S.node_draw(indptr, t) if kind == "node" else S.edge_draw(indptr, indices, t)
    assert b.entries.dtype == torch.int64 and np.array_equal(b.entries.cpu().numpy(), ent)
    assert b.ids.dtype == torch.int32 and np.array_equal(b.ids.cpu().numpy(), ids)
    ns = S.node_set(ids)
    assert ld.n_cap == (B if kind == "node" else 2 * B) and len(ids) == ld.n_cap
    assert b.num_nodes == len(ns) and np.array_equal(b.node_idx.cpu().numpy(), ns)
    src, dst = S.induced_subgraph(indptr, indices, ns)
    ei = b.edge_index.cpu().numpy()
    assert b.edge_index.dtype == torch.int64 and np.array_equal(ei[0], src) and np.array_equal(ei[1], dst)
    assert np.array_equal(g.node_map[b.node_idx].cpu().numpy(), np.arange(len(ns)))
    assert int(ld.philox_offset.item()) == 0                         # injected draws leave the stream alone


@pytest.mark.parametrize("kind", ["node", "edge"])
def test_out_of_range_draw_sets_the_status_bit(kind):
    _cuda()
    from grapes_amd import _lib
    indptr, indices = _graphs()["cora-like"]
    g = _dev_graph(indptr, indices)
    B = 64
    total = len(indices) if kind == "node" else int(S.entry_weights(indptr, indices).sum())
    ld = _sampler(kind, g, B, seed=1)
    ok = np.full(B, total - 1, np.int64)
    ld.sample(torch.from_numpy(ok).cuda())
    ld.check()
    for bad in (total, -1, 2 ** 62):
        t = ok.copy()
        t[5] = bad
        ld.sample(torch.from_numpy(t).cuda())
        with pytest.raises(_lib.GrapesHipError):
            ld.check()
    ld.sample(torch.from_numpy(ok).cuda())
    ld.check()                                                        # check() cleared the bit


def test_edge_sampler_refuses_total_weight_zero():
    _cuda()
    from grapes_amd.modules.saint import GraphSAINTEdgeSampler
    indptr, indices = _csr_from_edges(np.array([0, 2]), np.array([1, 3]), 4)      # no node has both an in- and an out-entry
    assert S.entry_weights(indptr, indices).sum() == 0
    ld = GraphSAINTEdgeSampler(_dev_graph(indptr, indices), 4, seed=0)
    with pytest.raises(ValueError):
        ld.weights()
    with pytest.raises(ValueError):
        ld.sample()


@pytest.mark.parametrize("kind", ["node", "edge"])
@pytest.mark.parametrize("B", [256, 1001])
def test_philox_draws_equal_the_oracle_and_advance_the_offset(kind, B):
    _cuda()
    indptr, indices = _graphs()["hubs directed"]
    g = _dev_graph(indptr, indices)
    total = len(indices) if kind == "node" else int(S.entry_weights(indptr, indices).sum())
    seed = 2 ** 40 + 12345
    a, b2 = _sampler(kind, g, B, seed=seed), _sampler(kind, g, B, seed=seed)
    off = 0
    for _ in range(3):
        s = a.sample()
        t = S.draw_values(seed, off, B, total)
        ent, ids = S.node_draw(indptr, t) if kind == "node" else S.edge_draw(indptr, indices, t)
        assert np.array_equal(s["entries"].cpu().numpy(), ent) and np.array_equal(s["ids"].cpu().numpy(), ids)
        ns = S.node_set(ids)
        n = int(s["count"].item())
        assert n == len(ns) and np.array_equal(s["node_idx"][:n].cpu().numpy(), ns)
        off += S.offset_advance(B)
        assert off == (2 * B + 3) // 4 * (_ + 1) and int(a.philox_offset.item()) == off
        s2 = b2.sample()                                              # two samplers with one seed agree
        for k in ("ids", "entries", "count"):
            assert torch.equal(s[k], s2[k])
        e = int(s["e_count"].item())
        assert e == int(s2["e_count"].item()) and torch.equal(s["edge_src"][:e], s2["edge_src"][:e])
        assert torch.equal(s["edge_dst"][:e], s2["edge_dst"][:e])
    a.check(); b2.check()


@pytest.mark.parametrize("kind", ["node", "edge"])
def test_captured_replay_equals_the_eager_call(kind):
    _cuda()
    indptr, indices = _graphs()["cora-like"]
    g1, g2 = _dev_graph(indptr, indices), _dev_graph(indptr, indices)
    B = 256
    a, b = _sampler(kind, g1, B, seed=9), _sampler(kind, g2, B, seed=9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a.sample()                                                    # builds the edge table, warms the allocator
    torch.cuda.current_stream().wait_stream(side)
    b.sample()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a.sample()
    for _ in range(3):
        graph.replay()
        ref = b.sample()
        torch.cuda.synchronize()
        n, e = int(ref["count"].item()), int(ref["e_count"].item())
        assert int(out["count"].item()) == n and int(out["e_count"].item()) == e
        for k in ("ids", "entries"):
            assert torch.equal(out[k], ref[k])
        assert torch.equal(out["node_idx"][:n], ref["node_idx"][:n])
        assert torch.equal(out["edge_src"][:e], ref["edge_src"][:e]) and torch.equal(out["edge_dst"][:e], ref["edge_dst"][:e])
        assert torch.equal(a.philox_offset, b.philox_offset)
    a.check(); b.check()


def _small_graph():
    """40 nodes, 201 stored entries (260 drawn pairs, duplicates removed), directed, skewed degrees, among them entries of
    weight 0 (sources without an in-entry pointing at sinks without an out-entry)."""
    rng = np.random.default_rng(5)
    n = 40
    s = rng.integers(0, 30, 260)
    d = (rng.integers(0, 30, 260) ** 2 // 30) % 30                     # skewed towards low ids
    s = np.concatenate([s, [30, 31, 32, 33]])                          # 30 .. 33: sources only; 36 .. 39: sinks only
    d = np.concatenate([d, [36, 37, 38, 39]])
    return _csr_from_edges(s, d, n)


@pytest.mark.parametrize("kind", ["node", "edge"])
def test_distribution_within_five_sigma(kind):
    """Every entry's count over T draws lies within 5 sigma of T p_e, sigma = sqrt(T p_e (1 - p_e)); T is the smallest multiple of
    the batch size with min T p_e >= 100 over the entries that can be drawn.  With about 200 entries a correct sampler misses this
    with probability about 1e-4; the seed is fixed.  The oracle's draws from the same words are held to the same bound."""
    _cuda()
    indptr, indices = _small_graph()
    nnz = len(indices)
    assert 180 <= nnz <= 240
    w = np.ones(nnz, np.int64) if kind == "node" else S.entry_weights(indptr, indices)
    if kind == "edge":
        assert (w == 0).sum() == 4
    total = int(w.sum())
    p = w / total
    B = 4096
    batches = int(np.ceil(100.0 / p[w > 0].min() / B))
    T = batches * B
    assert T * p[w > 0].min() >= 100
    g = _dev_graph(indptr, indices)
    seed = 20261017
    ld = _sampler(kind, g, B, seed=seed)
    got = torch.zeros(nnz, dtype=torch.int64, device="cuda")
    ref = np.zeros(nnz, np.int64)
    off = 0
    for i in range(batches):
        d = ld.draw()
        got += torch.bincount(d["entries"], minlength=nnz)
        t = S.draw_values(seed, off, B, total)
        ent = S.node_draw(indptr, t)[0] if kind == "node" else S.edge_draw(indptr, indices, t)[0]
        ref += np.bincount(ent, minlength=nnz)
        off += S.offset_advance(B)
        if i == 0:
            assert np.array_equal(d["entries"].cpu().numpy(), ent)
    ld.check()
    got = got.cpu().numpy()
    sigma = np.sqrt(T * p * (1 - p))
    for name, cnt in (("oracle", ref), ("device", got)):
        assert cnt.sum() == T
        z = np.abs(cnt - T * p) / np.where(sigma > 0, sigma, 1)
        print(f"{kind} {name}: T = {T}, min T p = {T * p[w > 0].min():.1f}, max |z| = {z[w > 0].max():.3f}")
        assert np.all(cnt[w == 0] == 0), name
        assert np.all(np.abs(cnt - T * p) <= 5 * sigma), (name, float(z.max()))
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("kind", ["node", "edge"])
def test_captured_trainer_matches_eager(kind):
    """As the random-walk test of the two engines: the same batches from one seed, and the weights after 5 steps of lr 0.01 within
    2e-3 (torch Adam against FusedAdam); the step losses within the same 2e-3."""
    _cuda()
    from grapes_amd.saint import make_trainer
    runs = {}
    for engine in ("eager", "graph"):
        indptr, indices, g, x, y, tm, model = _setup(n=3000, seed=2)
        tr = make_trainer(engine, g, x, y, tm, model, 0.01, batch_size=128, walk_length=7, seed=77, sampler=kind)
        assert tr.loader.n_cap == (128 if kind == "node" else 256)
        sets, losses = [], []
        for _ in range(5):
            if engine == "eager":
                loss, b = tr.step()
                losses.append(float(loss))
                sets.append((b.node_idx.cpu().numpy(), b.edge_index.cpu().numpy()))
            else:
                tr.step()
                losses.append(float(tr.lossbuf.item()))
                n, e = int(tr.draw_out[2].item()), int(tr.sub_out[2].item())
                sets.append((tr.draw_out[1][:n].long().cpu().numpy(),
                             torch.stack([tr.sub_out[0][:e], tr.sub_out[1][:e]]).long().cpu().numpy()))
        tr.check()
        runs[engine] = (sets, losses, [p.detach().cpu().numpy() for p in model.parameters()])
    (es, el, ew), (gs, gl, gw) = runs["eager"], runs["graph"]
    for a, b in zip(es, gs):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert len({tuple(s[0][:20]) for s in gs}) > 1
    assert np.all(np.isfinite(el)) and float(np.abs(np.array(el) - np.array(gl)).max()) <= 2e-3, (el, gl)
    for a, b in zip(ew, gw):
        assert float(np.abs(a - b).max()) <= 2e-3


@pytest.mark.parametrize("kind", ["node", "edge"])
def test_one_seeded_epoch_of_both_trainers(kind):
    _cuda()
    from grapes_amd.saint import make_trainer
    out = []
    for engine in ("eager", "graph"):
        indptr, indices, g, x, y, tm, model = _setup(n=3000, seed=3)
        tr = make_trainer(engine, g, x, y, tm, model, 0.01, batch_size=200, num_steps=4, seed=5, sampler=kind)
        out.append((tr.epoch(), [p.detach().cpu().numpy() for p in model.parameters()]))
    (le, we), (lg, wg) = out
    assert np.isfinite(le) and abs(le - lg) <= 2e-3, (le, lg)
    for a, b in zip(we, wg):
        assert float(np.abs(a - b).max()) <= 2e-3


def _cli(*flags):
    r = subprocess.run([sys.executable, "-m", "grapes_amd.graphsaint", "--dataset", "cora", "--max_epoch", "3", "--seed", "5", *flags],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("kind", ["edge", "node"])
def test_cli_three_epochs(kind):
    """Exit status 0, three epochs, finite losses; for the edge sampler the loss goes down over the run (the last epoch's below the
    first's).  An epoch here is ONE step on a freshly drawn batch and the stand-in's labels are random (validation stays at chance),
    so neighbouring epochs are not ordered for any sampler: the random-walk driver of before this change prints 2.0921, 1.6744,
    1.8782 for this seed.  Measured on the MI355X, seed 5: edge 1.9640, 1.9666, 1.5419; node 2.1448, 2.3897, 3.5671 — the node
    sampler's batches (256 degree-proportional draws, a few induced edges, a handful of training rows) are held to finite only."""
    _cuda()
    out = _cli("--sampler", kind)
    losses = [float(m) for m in re.findall(r"^Epoch: \d+, Loss: (\S+),", out, flags=re.M)]
    print(kind, losses)
    assert len(losses) == 3 and np.all(np.isfinite(losses)), out
    if kind == "edge":
        assert losses[2] < losses[0], losses
    assert sum(l.startswith("Acc: ") for l in out.splitlines()) == 1, out


def test_cli_rw_output_is_the_parents():
    """--sampler rw (and no --sampler at all) print what the driver printed before the flag existed (tests/golden: recorded from
    the commit before this one, seed 5)."""
    _cuda()
    want = open(GOLDEN).read()
    assert _cli() == want
    assert _cli("--sampler", "rw") == want
