"""ShaDow-GNN on the MI355X against tests/shadow_oracle.py: every integer output of the ego-net sampler bit for bit (n_id, ptr, batch,
root_n_id, the edge lists, e_id, the counts and the offset's advance) over hand graphs, a graph with a hub row and one whose ego-nets
nearly fill the cap; forced collisions, capacities, bad roots; the segment mean against fp64 at a derived bound; one trainer step
against fp64 rebuilt from the oracle's batch, judged by the project's measure (sage_oracle.rel_err) at the tolerances
tests/test_sage_gpu.py applies, 1e-5 and 1e-4; and the command line."""
import numpy as np
import pytest
import torch

from tests import sage_oracle as SGO
from tests import shadow_oracle as SO

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4                                           # tests/test_sage_gpu.py's
F32, F64 = np.float32, np.float64
MARK = -7
EDGE, NODE, BAD = 1, 2, 4                                                # the status bits


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


def _words(w):
    return _dev(np.ascontiguousarray(w, dtype=np.uint32).view(np.int32))


def _run(ops, ip, ix, roots, depth, k, n_cap, e_cap, pad=5, **kw):
    """The device call into buffers `pad` entries longer than their capacities, filled with MARK -> (outputs as numpy, status)."""
    n = len(ip) - 1
    B = len(roots)
    mk = lambda shape, dt=torch.int32: torch.full(shape if isinstance(shape, tuple) else (shape,), MARK, dtype=dt, device="cuda")
    out = (mk(n_cap + pad), mk(B + 1), mk(n_cap + pad), mk(B), mk((2, e_cap + pad)), mk(e_cap + pad, torch.int64), mk(1), mk(1))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.shadow_sample(_dev(ip), _dev(ix), n, _dev(np.asarray(roots, dtype=np.int32)), depth, k, n_cap=n_cap, e_cap=e_cap, status=status,
                      out=out, **kw)
    return [_np(t) for t in out], int(status.item())


def _same(got, ob, n_cap, e_cap):
    """Every integer output against the oracle's batch ob, and the guard values behind the capacities."""
    n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e = got
    assert int(d_n[0]) == ob.n and int(d_e[0]) == ob.e
    assert np.array_equal(ptr, ob.ptr) and np.array_equal(root_n_id, ob.root_n_id)
    assert np.array_equal(n_id[:ob.n], ob.n_id) and np.array_equal(batch[:ob.n], ob.batch)
    assert np.array_equal(ei[:, :ob.e], ob.edge_index) and np.array_equal(e_id[:ob.e], ob.e_id)
    assert (n_id[ob.n:] == MARK).all() and (batch[ob.n:] == MARK).all() and (ei[:, ob.e:] == MARK).all() and (e_id[ob.e:] == MARK).all()


def _check(ops, ip, ix, roots, depth, k, seed=5, offset=0, words=None, expect_status=0):
    ob = SO.sample(ip, ix, roots, depth, k, seed=seed, philox_offset=offset, words=words)
    n_cap, e_cap = max(ob.n, 1), max(ob.e, 1)
    got, status = _run(ops, ip, ix, roots, depth, k, n_cap, e_cap, philox_seed=seed, philox_offset=offset,
                       words=None if words is None else _words(words))
    assert status == expect_status
    _same(got, ob, n_cap, e_cap)
    return ob


# ---------------------------------------------------------------------------------------------------- hand graphs
def _star(leaves=300):
    """Node 0 is the hub with `leaves` entries (more than the 256 a wavefront walks alone, more than any fanout); every leaf stores
    the hub."""
    return SO.csr([list(range(1, leaves + 1))] + [[0] for _ in range(leaves)])


_HAND = {
    "path": (SO.csr([[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]), [0, 2, 5]),
    "single_node": (SO.csr([[]]), [0]),
    "single_node_with_loop": (SO.csr([[0]]), [0, 0]),
    "isolated_root": (SO.csr([[1], [0], [], [3, 3]]), [2, 3, 0]),                       # node 2 has no entry, node 3 only its loop, twice
    "duplicates_and_loops": (SO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0]]), [0, 1, 2, 3]),
    "star": (_star(), [0, 5, 300, 0]),
}


@pytest.mark.parametrize("name", list(_HAND))
@pytest.mark.parametrize("depth,k", [(1, 1), (2, 2), (3, 5), (1, 64)])
def test_hand_graphs(name, depth, k):
    ops = _ops()
    (ip, ix), roots = _HAND[name]
    _check(ops, ip, ix, roots, depth, k)


def test_forced_collisions_keep_the_first_and_the_last_positions():
    """words all zero: t = 0 at every step, so a long row keeps {0, d - k + 1, ..., d - 1}."""
    ops = _ops()
    ip, ix = _star()
    for k in (1, 2, 5, 64):
        words = np.zeros((1, 1, k), dtype=np.uint32)
        ob = _check(ops, ip, ix, [0], 1, k, words=words)
        assert ob.n_id.tolist() == [0, 1] + list(range(300 - k + 2, 301))           # the hub, leaf position 0, the last k - 1 leaves
    top = np.full((2, 2, 3), 2 ** 32 - 1, dtype=np.uint32)                          # the largest word: t = j, never a collision
    ob = _check(ops, ip, ix, [0, 7], 2, 3, words=top)
    assert ob.n_id[:4].tolist() == [0, 298, 299, 300]


# ---------------------------------------------------------------------------------------------------- the graph with a hub row
_HUB = 7
_G = {}


def _hub_graph():
    """N = 200, about 8 entries per row, row 7 with 1500: longer than the cap, the 1024-thread workgroup (two trips of the long-row
    loops) and every fanout; rows 0 .. 19 store the hub, so that it is a member of ego-nets it is not the root of."""
    if "hub" not in _G:
        ip, ix = SO.random_graph(200, 8, 21, hub=_HUB, hub_degree=1500)
        ix = ix.copy()
        for v in range(20):
            if v != _HUB:
                ix[ip[v]] = _HUB
        _G["hub"] = (ip, ix)
    return _G["hub"]


def _roots(B, seed=2):
    rng = np.random.default_rng(seed)
    head = [_HUB, 3, 3, 11, 199, 0, 4]                                               # the hub itself, a root listed twice
    return (head + rng.integers(0, 200, max(B - len(head), 0)).tolist())[:B] if B > 1 else [3]


@pytest.mark.parametrize("depth,k", [(1, 1), (1, 2), (1, 5), (1, 10), (1, 64), (2, 1), (2, 2), (2, 5), (2, 10), (3, 1), (3, 2), (3, 5)])
def test_hub_graph_every_depth_and_fanout(depth, k):
    ops = _ops()
    ip, ix = _hub_graph()
    ob = _check(ops, ip, ix, _roots(64), depth, k, seed=depth * 100 + k)
    assert np.diff(ob.ptr).max() <= SO.cap(depth, k)
    if k >= 10:                                                                      # the hub is a member beside being a root
        assert (ob.n_id == _HUB).sum() > 2


@pytest.mark.parametrize("B", [1, 7, 300])
def test_hub_graph_batch_sizes(B):
    ops = _ops()
    ip, ix = _hub_graph()
    _check(ops, ip, ix, _roots(B), 2, 5, seed=B, offset=2 ** 40 + 3)


def test_depth_3_with_fanout_10_exceeds_the_cap():
    ops = _ops()
    ip, ix = _hub_graph()
    with pytest.raises(ValueError, match="exceeds the ego-net cap"):
        ops.shadow_sample(_dev(ip), _dev(ix), 200, _dev(np.array([1], dtype=np.int32)), 3, 10, e_cap=10)


def test_an_ego_net_that_nearly_fills_the_cap():
    """N = 5000, about 40 entries per row, k = 31, depth 2: C = 993."""
    ops = _ops()
    if "big" not in _G:
        _G["big"] = SO.random_graph(5000, 40, 33)
    ip, ix = _G["big"]
    ob = _check(ops, ip, ix, [17, 4999, 2500], 2, 31, seed=9)
    assert SO.cap(2, 31) == 993 and np.diff(ob.ptr).max() > 900 and np.diff(ob.ptr).min() > 800


# ---------------------------------------------------------------------------------------------------- the stream
def test_two_calls_follow_the_oracles_offset_and_one_seed_gives_one_batch():
    ops = _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.shadow import ShaDowKHopSampler
    ip, ix = _hub_graph()
    g = DeviceGraph.from_csr(ip, ix)
    roots = _roots(40)
    s = ShaDowKHopSampler(g, 2, 5, seed=77)
    s._e_hint = 8                                                                    # the first buffer is too small: drawn again, doubled
    o1 = SO.sample(ip, ix, roots, 2, 5, seed=77)
    o2 = SO.sample(ip, ix, roots, 2, 5, seed=77, philox_offset=o1.philox_offset)
    assert o1.philox_offset == 40 * 2 and not np.array_equal(o1.n_id, o2.n_id)
    for ob in (o1, o2):
        b = s.sample(_dev(np.asarray(roots)))
        s.check()
        assert s.philox_offset == ob.philox_offset and b.num_nodes == ob.n
        assert np.array_equal(_np(b.node_idx), ob.n_id) and np.array_equal(_np(b.ptr), ob.ptr) and np.array_equal(_np(b.batch), ob.batch)
        assert np.array_equal(_np(b.root_n_id), ob.root_n_id) and np.array_equal(_np(b.edge_index), ob.edge_index)
        assert np.array_equal(_np(b.e_id), ob.e_id) and np.array_equal(_np(b.targets), roots)
        assert np.array_equal(_np(b.local_targets), np.arange(40)) and b.edge_index.dtype == torch.int32
    again = ShaDowKHopSampler(g, 2, 5, seed=77).sample(_dev(np.asarray(roots)))
    assert np.array_equal(_np(again.node_idx), o1.n_id) and np.array_equal(_np(again.edge_index), o1.edge_index)
    # the device offset: read instead of the host value, advanced by B * depth
    d_off = torch.tensor([o1.philox_offset], dtype=torch.int64, device="cuda")
    got, status = _run(ops, ip, ix, roots, 2, 5, o2.n, o2.e, philox_seed=77, philox_offset=12345, d_philox_offset=d_off)
    assert status == 0 and int(d_off.item()) == o2.philox_offset
    _same(got, o2, o2.n, o2.e)
    # a live count below the list: the roots behind it are empty ego-nets, and the offset advances by the live roots
    d_m = torch.tensor([25], dtype=torch.int32, device="cuda")
    d_off = torch.tensor([0], dtype=torch.int64, device="cuda")
    o25 = SO.sample(ip, ix, roots[:25], 2, 5, seed=77)
    got, status = _run(ops, ip, ix, roots, 2, 5, o25.n, o25.e, philox_seed=77, d_m=d_m, d_philox_offset=d_off)
    assert status == 0 and int(d_off.item()) == 50
    assert np.array_equal(got[1], np.concatenate([o25.ptr, np.full(15, o25.n)])) and (got[3][25:] == -1).all()
    assert np.array_equal(got[0][:o25.n], o25.n_id) and np.array_equal(got[4][:, :o25.e], o25.edge_index)


# ---------------------------------------------------------------------------------------------------- capacities and bad ids
def test_capacities_one_below_the_need():
    ops = _ops()
    ip, ix = _hub_graph()
    roots = _roots(20)
    ob = SO.sample(ip, ix, roots, 2, 5, seed=4)
    # edges
    got, status = _run(ops, ip, ix, roots, 2, 5, ob.n, ob.e - 1, philox_seed=4)
    assert status == EDGE and int(got[7][0]) == ob.e - 1 and int(got[6][0]) == ob.n
    assert np.array_equal(got[4][:, :ob.e - 1], ob.edge_index[:, :ob.e - 1]) and (got[4][:, ob.e - 1:] == MARK).all()
    assert np.array_equal(got[5][:ob.e - 1], ob.e_id[:ob.e - 1]) and (got[5][ob.e - 1:] == MARK).all()
    assert np.array_equal(got[0][:ob.n], ob.n_id)
    # nodes
    got, status = _run(ops, ip, ix, roots, 2, 5, ob.n - 1, ob.e, philox_seed=4)
    assert status == NODE and int(got[6][0]) == ob.n - 1 and int(got[7][0]) == ob.e
    assert np.array_equal(got[0][:ob.n - 1], ob.n_id[:ob.n - 1]) and (got[0][ob.n - 1:] == MARK).all() and (got[2][ob.n - 1:] == MARK).all()
    assert np.array_equal(got[1], np.minimum(ob.ptr, ob.n - 1))
    # both, far below
    got, status = _run(ops, ip, ix, roots, 2, 5, 3, 2, philox_seed=4)
    assert status == EDGE | NODE and int(got[6][0]) == 3 and int(got[7][0]) == 2
    assert (got[0][3:] == MARK).all() and (got[4][:, 2:] == MARK).all()


def test_a_root_outside_the_graph_is_an_empty_ego_net():
    ops = _ops()
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.shadow import ShaDowKHopSampler
    ip, ix = _hub_graph()
    ob = _check(ops, ip, ix, [3, 200, -1, 5, 2 ** 31 - 1], 2, 5, expect_status=BAD)
    assert ob.root_n_id.tolist()[1:3] == [-1, -1] and ob.ptr[1] == ob.ptr[2] == ob.ptr[3]
    s = ShaDowKHopSampler(DeviceGraph.from_csr(ip, ix), 2, 5, seed=1)
    s.sample(_dev(np.array([3, 200])))
    with pytest.raises(GrapesHipError, match="ego-net sampler: index out of range"):
        s.check()
    s.check()                                                                        # cleared
    small = ShaDowKHopSampler(DeviceGraph.from_csr(ip, ix), 2, 5, seed=1, e_cap=4)
    small.sample(_dev(np.array([3, 4])))
    with pytest.raises(GrapesHipError, match="ego-net sampler: edge buffer overflow"):
        small.check()


# ---------------------------------------------------------------------------------------------------- the segment mean
_SEGMENTS = (0, 1, 2, 63, 64, 65, 1024, 0)


@pytest.mark.parametrize("f", [1, 3, 64, 100, 256, 257, 1024])
def test_segment_mean_against_fp64(f):
    """Forward: n_b - 1 additions and one division, each rounded once, so element-wise |out - mean| <= gamma_n sum|x| / n with
    gamma_n = n u / (1 - n u) <= (n + 1) u for n <= 1024, u = 2^-24: the bound (n_b + 1) 2^-24 sum|x_i| / n_b.  Backward: g / n_b is
    one correctly rounded division: |dh - g / n| <= 2^-24 |g / n|."""
    ops = _ops()
    ptr = np.concatenate([[0], np.cumsum(_SEGMENTS)]).astype(np.int32)
    n_rows = int(ptr[-1])
    rng = np.random.default_rng(f)
    h = rng.standard_normal((n_rows, f)).astype(F32)
    out = _np(ops.segment_mean_fwd(_dev(h), _dev(ptr)))
    ref = SO.segment_mean64(h, ptr)
    for b, n in enumerate(_SEGMENTS):
        if n == 0:
            assert (out[b] == 0).all()
            continue
        bound = (n + 1) * 2.0 ** -24 * np.abs(h[ptr[b]:ptr[b + 1]].astype(F64)).sum(0) / n
        assert (np.abs(out[b].astype(F64) - ref[b]) <= bound).all(), (b, n)
    g = rng.standard_normal((len(_SEGMENTS), f)).astype(F32)
    dh = _np(ops.segment_mean_bwd(_dev(g), _dev(ptr), n_rows))
    want = SO.segment_mean_bwd64(g, ptr, n_rows)
    assert (np.abs(dh.astype(F64) - want) <= 2.0 ** -24 * np.abs(want)).all()
    # rows of no segment get zeros; a segment outside the rows raises the bad-index bit and counts as empty
    inner = np.array([2, 5, 9], dtype=np.int32)
    dh = _np(ops.segment_mean_bwd(_dev(g[:2]), _dev(inner), 12, out=torch.full((12, f), 3.0, device="cuda")))
    assert (dh[:2] == 0).all() and (dh[9:] == 0).all() and np.array_equal(dh[2:5], np.repeat((g[0] / F32(3))[None], 3, 0))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = _np(ops.segment_mean_fwd(_dev(h[:8]), _dev(np.array([0, 4, 9], dtype=np.int32)), status=status))
    assert int(status.item()) == BAD and (out[1] == 0).all() and (out[0] != 0).any()


# ---------------------------------------------------------------------------------------------------- the model and the trainer
def _gcn_conv64(x, ei, w, b, relu, gate):
    """The project's default GCNConv in fp64: stored loops are dropped, one unit loop per node is added, every other stored entry
    counts (duplicates each): D^-1/2 (A + I) D^-1/2 x Wᵀ + b."""
    n = x.shape[0]
    src, dst = (torch.as_tensor(np.asarray(r, dtype=np.int64)) for r in ei)
    keep = src != dst
    src, dst = torch.cat([src[keep], torch.arange(n)]), torch.cat([dst[keep], torch.arange(n)])
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64))
    coef = deg[src].rsqrt() * deg[dst].rsqrt()
    h = x @ w.T
    out = torch.zeros((n, w.shape[0]), dtype=torch.float64).index_add_(0, dst, coef[:, None] * h[src]) + b
    if gate is not None:
        return out * torch.as_tensor(np.asarray(gate, dtype=F64))
    return out.clamp(min=0) if relu else out


def _forward64(xb, layers, head, ob, conv, pool, gates):
    h, L = xb, len(layers)
    for i, p in enumerate(layers):
        last = i == L - 1
        gate = None if last else gates[i]
        if conv == "sage":
            h = SGO.sage_conv64(h, ob.edge_index, p[0], p[1], p[2], "mean", relu=not last, gate=gate)
        else:
            h = _gcn_conv64(h, ob.edge_index, p[0], p[1], not last, gate)
    out = h[torch.as_tensor(ob.root_n_id.astype(np.int64))]
    if pool:
        M = torch.zeros((len(ob.ptr) - 1, h.shape[0]), dtype=torch.float64)
        for b in range(len(ob.ptr) - 1):
            M[b, ob.ptr[b]:ob.ptr[b + 1]] = 1.0 / (ob.ptr[b + 1] - ob.ptr[b])
        out = torch.cat([out, M @ h], dim=1)
    return out @ head[0].T + head[1]


def _layer_params(model, conv):
    if conv == "sage":
        return [(c.lin_l.weight, c.lin_l.bias, c.lin_r.weight) for c in model.body.convs]
    return [(c.lin.weight, c.bias) for c in model.body.gcn_layers]


@pytest.mark.parametrize("pool", [True, False], ids=["pool", "root"])
@pytest.mark.parametrize("conv", ["sage", "gcn"])
def test_trainer_step_against_fp64(conv, pool):
    """One ShadowTrainer.step (SGD with lr = 0, so the parameters stay): the batch is the oracle's, the logits and every parameter
    gradient are fp64's rebuilt from that batch on the device's ReLU gates (as tests/test_sage_gpu.py judges its step)."""
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.shadow import ShaDow
    from grapes_amd.shadow import ShadowTrainer
    n, F, H, C, B, depth, k = 200, 16, 32, 4, 24, 2, 5
    ip, ix = _hub_graph()
    g = DeviceGraph.from_csr(ip, ix)
    rng = np.random.default_rng(52)
    x32 = rng.standard_normal((n, F)).astype(F32)
    labels = rng.integers(0, C, n)
    model = ShaDow(F, H, C, 3, conv=conv, pool=pool).cuda()
    tr = ShadowTrainer(g, _dev(x32), _dev(labels), model, torch.optim.SGD(model.parameters(), lr=0.0), depth=depth, num_neighbors=k,
                       batch_size=B, seed=8)
    roots = np.concatenate([[_HUB, 3], rng.permutation(n)[:B - 2]])
    loss, b = tr.step(_dev(roots))
    ob = SO.sample(ip, ix, roots, depth, k, seed=8)
    assert np.array_equal(_np(b.node_idx), ob.n_id) and np.array_equal(_np(b.edge_index), ob.edge_index)
    assert np.array_equal(_np(b.ptr), ob.ptr) and np.array_equal(_np(b.root_n_id), ob.root_n_id)
    xb = x32[ob.n_id]
    layers = _layer_params(model, conv)
    with torch.no_grad():                                                # the device's ReLU gates of the hidden layers
        h, gates = _dev(xb), []
        mods = model.body.convs if conv == "sage" else model.body.gcn_layers
        for m in list(mods)[:-1]:
            h = m(h, b.edge_index, relu=True)
            gates.append(_np(h > 0))
        logits = _np(model(_dev(xb), b))
    p64 = [tuple(torch.as_tensor(_np(p).astype(F64)).requires_grad_(True) for p in layer) for layer in layers]
    h64 = tuple(torch.as_tensor(_np(p).astype(F64)).requires_grad_(True) for p in (model.head.weight, model.head.bias))
    z64 = _forward64(torch.as_tensor(xb.astype(F64)), p64, h64, ob, conv, pool, gates)
    l64 = SGO.loss64(z64, np.arange(B), labels[roots])
    l64.backward()
    l64 = l64.detach()
    assert logits.shape == (B, C)
    print(f"[shadow] {conv} pool={pool}: logits err {SGO.rel_err(logits, z64.detach().numpy()):.2e}, loss {float(loss):.6f} / {float(l64):.6f}")
    assert SGO.rel_err(logits, z64.detach().numpy()) <= ACT_TOL
    assert abs(float(loss) - float(l64)) <= ACT_TOL * max(1.0, abs(float(l64)))
    for li, (layer, layer64) in enumerate(zip(layers, p64)):
        for pi, (p, q) in enumerate(zip(layer, layer64)):
            err = SGO.rel_err(_np(p.grad), q.grad.numpy())
            print(f"[shadow] {conv} pool={pool}: layer {li} parameter {pi} grad err {err:.2e}")
            assert err <= GRAD_TOL and np.abs(q.grad.numpy()).max() > 0
    for p, q in zip((model.head.weight, model.head.bias), h64):
        assert SGO.rel_err(_np(p.grad), q.grad.numpy()) <= GRAD_TOL
    val, test = tr.evaluate((_dev(np.arange(n) < 50), _dev(np.arange(n) >= 150)))
    assert 0.0 <= val <= 1.0 and 0.0 <= test <= 1.0 and tr.evaluate((_dev(np.arange(n) < 50),))[0] == val
    assert tr.sampler.philox_offset == B * depth and model.training     # evaluation moved neither the training stream nor the mode


# ---------------------------------------------------------------------------------------------------- the command line
def test_cli_three_epochs_lower_the_loss(capsys):
    _ops()
    import re
    from grapes_amd import shadow
    v = shadow.main(["--dataset", "cora", "--max_epoch", "3", "--hidden_dim", "32", "--seed", "1"])
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"Loss: ([0-9.]+)", out)]
    assert out.count("Epoch: ") == 3 and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[2] < losses[0]
