"""ShaDow-GNN's PPR scope on the MI355X against tests/shadow_ppr_oracle.py: every integer output of ops.shadow_ppr_sample bit for bit
(n_id, ptr, batch, root_n_id, the edge lists, e_id, the counts, score, rounds, stop) with guard values behind the capacities — hand
graphs, the hub graph of the rule's table over its five (alpha, eps) pairs, the edge of the touched-set capacity, batch sizes, repeated
roots, capacities, bad roots; the sampler's batch; one trainer step against the model over the oracle's batch; the command line."""
import numpy as np
import pytest
import torch

from tests import shadow_oracle as SO
from tests import shadow_ppr_oracle as PO

pytestmark = pytest.mark.gpu

MARK = -7
EDGE, NODE, BAD = 1, 2, 4                                                # the status bits
ONE, T = 1 << 30, 4096
PAIRS = [(0.25, 2 ** -10), (0.25, 2 ** -12), (0.25, 2 ** -14), (0.5, 2 ** -16), (0.15, 2 ** -20)]


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _run(ops, ip, ix, roots, k, aq, thr, max_rounds, n_cap, e_cap, pad=5):
    """The device call into buffers `pad` entries longer than their capacities, filled with MARK -> (outputs as numpy, status)."""
    n, B = len(ip) - 1, len(roots)
    mk = lambda shape, dt=torch.int32: torch.full(shape if isinstance(shape, tuple) else (shape,), MARK, dtype=dt, device="cuda")
    out = (mk(n_cap + pad), mk(B + 1), mk(n_cap + pad), mk(B), mk((2, e_cap + pad)), mk(e_cap + pad, torch.int64), mk(1), mk(1),
           mk(n_cap + pad), mk(B), mk(B))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.shadow_ppr_sample(_dev(ip), _dev(ix), n, _dev(np.asarray(roots, dtype=np.int32)), k, aq, thr, max_rounds, n_cap=n_cap, e_cap=e_cap,
                          status=status, out=out)
    return [_np(t) for t in out], int(status.item())


def _same(got, ob):
    """Every integer output against the oracle's batch ob, and the guard values behind the capacities."""
    n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e, score, rounds, stop = got
    assert int(d_n[0]) == ob.n and int(d_e[0]) == ob.e
    assert np.array_equal(rounds, ob.rounds) and np.array_equal(stop, ob.stop)
    assert np.array_equal(ptr, ob.ptr) and np.array_equal(root_n_id, ob.root_n_id)
    assert np.array_equal(n_id[:ob.n], ob.n_id) and np.array_equal(batch[:ob.n], ob.batch) and np.array_equal(score[:ob.n], ob.score)
    assert np.array_equal(ei[:, :ob.e], ob.edge_index) and np.array_equal(e_id[:ob.e], ob.e_id)
    assert (n_id[ob.n:] == MARK).all() and (batch[ob.n:] == MARK).all() and (score[ob.n:] == MARK).all()
    assert (ei[:, ob.e:] == MARK).all() and (e_id[ob.e:] == MARK).all()


def _check(ops, ip, ix, roots, k, alpha=0.25, eps=2 ** -14, max_rounds=32, expect_status=0):
    aq, thr = PO.fixed(alpha, eps)
    ob = PO.sample(ip, ix, roots, k, aq, thr, max_rounds)
    got, status = _run(ops, ip, ix, roots, k, aq, thr, max_rounds, max(ob.n, 1), max(ob.e, 1))
    assert status == expect_status
    _same(got, ob)
    return ob


# ---------------------------------------------------------------------------------------------------- hand graphs
def _star(leaves):
    """Node 0 is the centre with `leaves` entries; every leaf stores the centre."""
    return SO.csr([list(range(1, leaves + 1))] + [[0] for _ in range(leaves)])


_HAND = {
    "path": (SO.csr([[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]), [0, 2, 5]),
    "clique": (SO.csr([[u for u in range(9) if u != v] for v in range(9)]), [0, 4, 8]),
    "star_300": (_star(300), [0, 5, 300]),
    "loops_and_duplicates": (SO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0]]), [0, 1, 2, 3]),
    "isolated_root": (SO.csr([[1], [0], [], [3, 3]]), [2, 3, 0]),                       # deg 0: all mass to p; node 3 only pays itself
    "directed_with_an_empty_row": (SO.csr([[1, 2], [2], [], [0, 2, 2]]), [0, 3, 1, 2]),  # node 2 is reached and has no entry
}


@pytest.mark.parametrize("name", list(_HAND))
@pytest.mark.parametrize("alpha,eps,k", [(0.25, 2 ** -14, 1), (0.25, 2 ** -14, 5), (0.5, 2 ** -20, 200), (0.15, 2 ** -6, 1023)])
def test_hand_graphs(name, alpha, eps, k):
    ops = _ops()
    (ip, ix), roots = _HAND[name]
    ob = _check(ops, ip, ix, roots, k, alpha, eps)
    if name == "star_300" and eps <= 2 ** -14:                            # every leaf ties: the k smallest ids win
        assert ob.n_id[:ob.ptr[1]].tolist() == list(range(0, min(k, 300) + 1))
    if name == "isolated_root":
        assert ob.n_id[:1].tolist() == [2] and ob.score[0] == ONE and ob.rounds[0] == 1 and ob.ptr[1] == 1


# ---------------------------------------------------------------------------------------------------- the hub graph
_HUB = 7
_G = {}


def _hub_graph():
    """N = 3000, about 8 entries per row, row 7 with 2500: the graph of the rule's table."""
    if "hub" not in _G:
        _G["hub"] = SO.random_graph(3000, 8, 1, hub=_HUB, hub_degree=2500)
    return _G["hub"]


def _hub_roots():
    ip, ix = _hub_graph()
    return [0, _HUB, int(ix[ip[_HUB]]), 100, 1234, 2999]


@pytest.mark.parametrize("k", [1, 32, 200, 1023])
@pytest.mark.parametrize("alpha,eps", PAIRS)
def test_hub_graph(alpha, eps, k):
    ops = _ops()
    ip, ix = _hub_graph()
    ob = _check(ops, ip, ix, _hub_roots(), k, alpha, eps)
    assert (ob.n_id == _HUB).sum() >= 1 and int(ip[_HUB + 1] - ip[_HUB]) == 2500   # a member whose row the whole workgroup counts
    if eps == 2 ** -10:
        assert ob.stop.tolist() == [0] * 6 and ob.rounds[1] == 0 and ob.ptr[2] - ob.ptr[1] == 1   # the hub root never pushes
    if (alpha, eps) == (0.25, 2 ** -14):
        assert ob.stop.tolist() == [0, 2, 0, 0, 0, 0]
    if eps <= 2 ** -16:
        assert (ob.stop == 2).sum() >= 4
    if k == 1023 and eps <= 2 ** -12:
        assert np.diff(ob.ptr).max() >= 600


def test_hub_graph_stops_at_max_rounds():
    ops = _ops()
    ip, ix = _hub_graph()
    ob = _check(ops, ip, ix, _hub_roots(), 200, 0.25, 2 ** -14, max_rounds=2)
    assert ob.stop.tolist() == [1, 2, 1, 1, 1, 1] and ob.rounds.tolist() == [2, 1, 2, 2, 2, 2]


# ---------------------------------------------------------------------------------------------------- the edge of the touched-set capacity
def test_the_capacity_edge():
    ops = _ops()
    ip, ix = _star(T - 1)                                                 # |S| + sum deg = 1 + 4095 = T: the round runs
    for k in (5, 1023):
        ob = _check(ops, ip, ix, [0], k)
        assert len(ob.pushes[0].r) == T and (ob.rounds[0], ob.stop[0]) == (1, 2) and ob.n_id.tolist() == list(range(k + 1))
    ip, ix = _star(T)                                                     # 1 + 4096 > T: stop 2 at round 0, the root alone
    ob = _check(ops, ip, ix, [0, 1], 1023)
    assert (ob.rounds[0], ob.stop[0]) == (0, 2) and ob.ptr.tolist()[:2] == [0, 1] and ob.score[0] == ONE >> 2
    ip, ix = _star(5000)                                                  # a leaf root: one round, then the centre's row is too long
    ob = _check(ops, ip, ix, [17], 1023)
    assert (ob.rounds[0], ob.stop[0]) == (1, 2) and ob.n_id.tolist() == [0, 17]


# ---------------------------------------------------------------------------------------------------- batches
def _many_roots(B, seed=2):
    rng = np.random.default_rng(seed)
    head = _hub_roots() + [3, 3]                                          # a root listed twice
    return (head + rng.integers(0, 3000, max(B - len(head), 0)).tolist())[:B] if B > 1 else [3]


@pytest.mark.parametrize("B", [1, 7, 300])
def test_batch_sizes(B):
    ops = _ops()
    ip, ix = _hub_graph()
    _check(ops, ip, ix, _many_roots(B), 32, 0.25, 2 ** -12)


def test_repeated_roots_and_two_calls_give_the_same_bits():
    ops = _ops()
    ip, ix = _hub_graph()
    roots = [1234, 5, 1234, _HUB, _HUB]
    aq, thr = PO.fixed(0.25, 2 ** -14)
    ob = _check(ops, ip, ix, roots, 200)
    seg = lambda a, b: a[ob.ptr[b]:ob.ptr[b + 1]]
    assert np.array_equal(seg(ob.n_id, 0), seg(ob.n_id, 2)) and np.array_equal(seg(ob.score, 0), seg(ob.score, 2))
    first, s1 = _run(ops, ip, ix, roots, 200, aq, thr, 32, ob.n, ob.e)
    again, s2 = _run(ops, ip, ix, roots, 200, aq, thr, 32, ob.n, ob.e)
    assert s1 == s2 == 0 and all(np.array_equal(a, b) for a, b in zip(first, again))
    e0, e2 = (first[4][:, (first[4][1] >= ob.ptr[b]) & (first[4][1] < ob.ptr[b + 1])] - ob.ptr[b] for b in (0, 2))
    assert np.array_equal(e0, e2)                                         # two identical ego-nets


# ---------------------------------------------------------------------------------------------------- capacities and bad ids
def test_capacities_one_below_the_need():
    ops = _ops()
    ip, ix = _hub_graph()
    roots = _many_roots(20)
    aq, thr = PO.fixed(0.25, 2 ** -12)
    ob = PO.sample(ip, ix, roots, 32, aq, thr, 32)
    got, status = _run(ops, ip, ix, roots, 32, aq, thr, 32, ob.n, ob.e - 1)
    assert status == EDGE and int(got[7][0]) == ob.e - 1 and int(got[6][0]) == ob.n
    assert np.array_equal(got[4][:, :ob.e - 1], ob.edge_index[:, :ob.e - 1]) and (got[4][:, ob.e - 1:] == MARK).all()
    assert np.array_equal(got[5][:ob.e - 1], ob.e_id[:ob.e - 1]) and (got[5][ob.e - 1:] == MARK).all()
    assert np.array_equal(got[0][:ob.n], ob.n_id) and np.array_equal(got[8][:ob.n], ob.score)
    got, status = _run(ops, ip, ix, roots, 32, aq, thr, 32, ob.n - 1, ob.e)
    assert status == NODE and int(got[6][0]) == ob.n - 1 and int(got[7][0]) == ob.e
    assert np.array_equal(got[0][:ob.n - 1], ob.n_id[:ob.n - 1]) and (got[0][ob.n - 1:] == MARK).all() and (got[2][ob.n - 1:] == MARK).all()
    assert np.array_equal(got[8][:ob.n - 1], ob.score[:ob.n - 1]) and (got[8][ob.n - 1:] == MARK).all()
    assert np.array_equal(got[1], np.minimum(ob.ptr, ob.n - 1))
    got, status = _run(ops, ip, ix, roots, 32, aq, thr, 32, 3, 2)
    assert status == EDGE | NODE and int(got[6][0]) == 3 and int(got[7][0]) == 2
    assert (got[0][3:] == MARK).all() and (got[8][3:] == MARK).all() and (got[4][:, 2:] == MARK).all()


def test_a_root_outside_the_graph_is_an_empty_ego_net():
    ops = _ops()
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.shadow import ShaDowPPRSampler
    ip, ix = _hub_graph()
    ob = _check(ops, ip, ix, [3, 3000, -1, 5, 2 ** 31 - 1], 32, expect_status=BAD)
    assert ob.root_n_id.tolist()[1:3] == [-1, -1] and ob.ptr[1] == ob.ptr[2] == ob.ptr[3] and ob.rounds[1] == ob.stop[1] == 0
    s = ShaDowPPRSampler(DeviceGraph.from_csr(ip, ix), 32)
    s.sample(_dev(np.array([3, 3000])))
    with pytest.raises(GrapesHipError, match="ego-net sampler: index out of range"):
        s.check()
    s.check()                                                             # cleared
    small = ShaDowPPRSampler(DeviceGraph.from_csr(ip, ix), 32, e_cap=4)
    small.sample(_dev(np.array([3, 4])))
    with pytest.raises(GrapesHipError, match="ego-net sampler: edge buffer overflow"):
        small.check()


# ---------------------------------------------------------------------------------------------------- the sampler, the trainer, the driver
def test_the_samplers_batch():
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.shadow import ShaDowPPRSampler
    ip, ix = _hub_graph()
    roots = _many_roots(40)
    s = ShaDowPPRSampler(DeviceGraph.from_csr(ip, ix), 200, alpha=0.25, eps=2 ** -12, max_rounds=32)
    s._e_hint = 8                                                         # the first buffer is too small: built again, doubled
    ob = PO.sample(ip, ix, roots, 200, *PO.fixed(0.25, 2 ** -12), 32)
    for _ in range(2):                                                    # no stream: the second batch is the first
        b = s.sample(_dev(np.asarray(roots)))
        s.check()
        assert b.num_nodes == ob.n and np.array_equal(_np(b.node_idx), ob.n_id) and np.array_equal(_np(b.ptr), ob.ptr)
        assert np.array_equal(_np(b.batch), ob.batch) and np.array_equal(_np(b.root_n_id), ob.root_n_id)
        assert np.array_equal(_np(b.edge_index), ob.edge_index) and np.array_equal(_np(b.e_id), ob.e_id)
        assert np.array_equal(_np(b.targets), roots) and np.array_equal(_np(b.local_targets), np.arange(40))
        assert np.array_equal(_np(b.rounds), ob.rounds) and np.array_equal(_np(b.stop), ob.stop) and b.edge_index.dtype == torch.int32
        # fixed / 2^30 in fp32: the integer rounded once to fp32's 24 bits (exact below 2^24), the power of two exact
        assert b.score.dtype == torch.float32 and np.array_equal(_np(b.score), ob.score.astype(np.float32) * np.float32(2.0 ** -30))
        small = ob.score < 2 ** 24
        assert small.any() and np.array_equal(_np(b.score).astype(np.float64)[small] * 2.0 ** 30, ob.score[small].astype(np.float64))


@pytest.mark.parametrize("conv", ["sage", "gcn"])
def test_one_trainer_step_runs_the_model_over_the_oracles_batch(conv):
    """The model and the kernels are the same and nothing is drawn: the step's logits are the model's over the oracle's batch, bit for
    bit (SGD with lr = 0 keeps the parameters)."""
    ops = _ops()
    from types import SimpleNamespace
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.shadow import ShaDow
    from grapes_amd.shadow import ShadowTrainer
    torch.manual_seed(4321)
    n, F, H, C, B, k = 3000, 16, 32, 4, 24, 50
    ip, ix = _hub_graph()
    rng = np.random.default_rng(52)
    x = _dev(rng.standard_normal((n, F)).astype(np.float32))
    labels = rng.integers(0, C, n)
    model = ShaDow(F, H, C, 3, conv=conv, pool=True).cuda()
    tr = ShadowTrainer(DeviceGraph.from_csr(ip, ix), x, _dev(labels), model, torch.optim.SGD(model.parameters(), lr=0.0), batch_size=B,
                       scope="ppr", ppr_k=k, ppr_alpha=0.25, ppr_eps=2 ** -12, ppr_rounds=32)
    roots = np.concatenate([[_HUB, 3], rng.permutation(n)[:B - 2]])
    seen = {}
    forward = tr._forward
    tr._forward = lambda xb, b: seen.setdefault("logits", forward(xb, b))
    with pytest.raises(ValueError, match="the PPR scope draws nothing"):
        tr.step(_dev(roots), words=torch.zeros(1, dtype=torch.int32, device="cuda"))
    loss, b = tr.step(_dev(roots))
    ob = PO.sample(ip, ix, roots, k, *PO.fixed(0.25, 2 ** -12), 32)
    oracle_batch = SimpleNamespace(node_idx=_dev(ob.n_id), ptr=_dev(ob.ptr), root_n_id=_dev(ob.root_n_id), edge_index=_dev(ob.edge_index))
    with torch.no_grad():
        want = model(ops.gather_rows(x, oracle_batch.node_idx), oracle_batch)
    got = seen["logits"].detach()
    assert got.shape == (B, C) and torch.equal(got, want) and np.isfinite(float(loss))
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in model.parameters())
    val, test = tr.evaluate((_dev(np.arange(n) < 50), _dev(np.arange(n) >= 2950)))
    assert 0.0 <= val <= 1.0 and 0.0 <= test <= 1.0 and tr.evaluate((_dev(np.arange(n) < 50),))[0] == val and model.training


def test_cli_three_epochs_lower_the_loss(capsys):
    _ops()
    import re
    from grapes_amd import shadow
    v = shadow.main(["--dataset", "cora", "--max_epoch", "3", "--hidden_dim", "32", "--seed", "1", "--scope", "ppr"])
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"Loss: ([0-9.]+)", out)]
    assert out.count("Epoch: ") == 3 and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[2] < losses[0]
