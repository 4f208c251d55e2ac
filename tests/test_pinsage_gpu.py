"""PinSAGE on the MI355X against tests/pinsage_oracle.py.  ops.pinsage_neighbors: nbr, visits and cnt bit for bit with guard values
behind m K — hand graphs, stars (the id tie-break; 70 000 leaves, where (s deg) >> 32 needs the 64-bit product), dead ends and an
isolated root, every (R, L) at which the kernel tiles its roots differently, T above and below the distinct visited nodes, the three
termination words, batch sizes, a device count below m, bad and repeated roots, a device offset over two calls, the error codes.  The
sampler's blocks against the oracle's.  ops.relu_l2norm_fwd / _bwd against fp64 at the bound derived below.  One PinSAGEConv layer and
one PinSAGETrainer step against the fp64 restatement on the oracle's batch, and the command line.

The relu_l2norm bound (u = 2^-24, gamma_n = n u / (1 - n u), standard rounding analysis, any summation order, with or without fma):
the sum of the f squares carries a relative error of at most gamma_f (all terms are non-negative), its square root half of that and one
rounding, the division one more: |out - ref| <= gamma_{f + 3} |ref|.  The backward reads that out (gamma_{f + 3}) in a dot product
of f terms (gamma_f), multiplies by out again, subtracts and divides by the rounded norm; the first-order count stays inside 2 f + 6
roundings on each of the absolute terms: |ds - ref| <= gamma_{2 f + 6} (|g| + |out| sum |g out|) / max(nrm, eps).  Both plus the
smallest subnormal."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pinsage_oracle as PS
from tests import sage_oracle as SG
from tests import shadow_oracle as SO

pytestmark = pytest.mark.gpu

MARK = -7
BAD = 4                                                                  # the status bit
FULL = 2 ** 32 - 1
ACT_TOL, GRAD_TOL = 1e-5, 1e-4                                           # tests/test_sage_gpu.py's


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _mk(*shape):
    return torch.full(shape, MARK, dtype=torch.int32, device="cuda")


# ---------------------------------------------------------------------------------------------------- neighbours
def _run(ops, ip, ix, roots, R, L, tq, T, seed=0, off=0, live=None, d_off=None, pad=5):
    """The device call into flat buffers `pad` entries longer than m K (and m), filled with MARK -> (outputs as numpy, status)."""
    m, K = len(roots), T + 1
    out = (_mk(m * K + pad), _mk(m * K + pad), _mk(m + pad))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_m = None if live is None else _dev(np.array([live], dtype=np.int32))
    ops.pinsage_neighbors(_dev(ip), _dev(ix), len(ip) - 1, _dev(np.asarray(roots, dtype=np.int32)), R, L, tq, T, philox_seed=seed,
                          philox_offset=off, d_philox_offset=d_off, d_m=d_m, status=status, out=out)
    return [_np(t) for t in out], int(status.item())


def _same(got, want, m, K):
    nbr, vis, cnt = got
    assert np.array_equal(nbr[:m * K].reshape(m, K), want.nbr), "nbr"
    assert np.array_equal(vis[:m * K].reshape(m, K), want.visits), "visits"
    assert np.array_equal(cnt[:m], want.cnt), "cnt"
    assert all((a[n:] == MARK).all() for a, n in ((nbr, m * K), (vis, m * K), (cnt, m))), "a guard value was overwritten"


def _check(ops, ip, ix, roots, R, L, tq, T, seed=0, off=0, live=None, expect_status=0, memo=None):
    want = PS.neighbors(ip, ix, roots, R, L, tq, T, seed, off, live=live, memo=memo)
    got, status = _run(ops, ip, ix, roots, R, L, tq, T, seed, off, live=live)
    assert status == expect_status == (BAD if want.bad_index else 0)
    _same(got, want, len(roots), T + 1)
    return want


def _star(leaves):
    """Node 0 is the centre with `leaves` entries; every leaf stores the centre."""
    return SO.csr([list(range(1, leaves + 1))] + [[0] for _ in range(leaves)])


_HAND = {
    "path": (SO.csr([[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]), [0, 2, 5]),
    "clique": (SO.csr([[u for u in range(9) if u != v] for v in range(9)]), [0, 4, 8]),
    "loops_and_duplicates": (SO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0]]), [0, 1, 2, 3]),
    "dead_ends_and_an_isolated_root": (SO.csr([[1, 4], [2], [], [3, 3], [0, 2, 5], [], []]), [6, 0, 3, 4, 2]),
    "star_300": (_star(300), [0, 5, 300]),
}


@pytest.mark.parametrize("name", list(_HAND))
def test_hand_graphs(name):
    ops = _ops()
    (ip, ix), roots = _HAND[name]
    for R, L, p, T in ((1, 1, 0.0, 1), (10, 2, 0.5, 3), (64, 3, 0.25, 5), (200, 5, 0.1, 50), (256, 4, 0.0, 1023)):
        want = _check(ops, ip, ix, roots, R, L, PS.term_q(p), T, seed=11, off=3)
        if name == "dead_ends_and_an_isolated_root":
            assert want.cnt[0] == 1 and (want.nbr[0] == 6).all() and (want.visits[0] == 0).all() and want.cnt[4] == 1
        if name == "star_300" and (R, L) == (256, 4):                    # the centre's leaves tie in runs: ids ascending inside a count
            v, u = want.visits[0, 1:want.cnt[0]], want.nbr[0, 1:want.cnt[0]]
            tie = v[1:] == v[:-1]
            assert tie.sum() > 50 and (np.diff(v) <= 0).all() and (np.diff(u)[tie] > 0).all()


def test_star_of_70000_leaves_needs_the_64_bit_product():
    ops = _ops()
    ip, ix = _star(70000)
    want = _check(ops, ip, ix, [0, 69999, 1], 512, 2, 0, 1023, seed=5)
    leaves = want.nbr[0, 1:want.cnt[0]]
    assert leaves.max() > 65536 and want.cnt[0] > 500                    # (the low 32 bits of s deg alone would say something else)
    assert want.cnt[1] > 400 and want.nbr[1, 1] == 0 and want.visits[1, 1] == 512      # a leaf: the centre 512 times, then leaves once


_G = {}


def _hub_graph():
    """N = 3000, about 8 entries per row, row 7 with 2500."""
    if "hub" not in _G:
        _G["hub"] = SO.random_graph(3000, 8, 1, hub=7, hub_degree=2500)
    return _G["hub"]


def _hub_roots():
    ip, ix = _hub_graph()
    return [0, 7, int(ix[ip[7]]), 100, 1234, 2999, 7]


@pytest.mark.parametrize("R,L", [(1, 1), (10, 2), (63, 1), (64, 1), (65, 1), (200, 5), (256, 4), (1024, 1), (1, 1024)])
def test_parameter_points(R, L):
    """Each (R, L) gives the workgroup another number of roots and the sort another length; T = 1 and 3 lie below the distinct visited
    nodes of the hub where R L allows, 1023 above them everywhere."""
    ops = _ops()
    ip, ix = _hub_graph()
    roots = _hub_roots()
    for tq in (0, 2 ** 31, FULL):
        memo = {}
        for T in (1, 3, 50, 1023):
            want = _check(ops, ip, ix, roots, R, L, tq, T, seed=77, off=9, memo=memo)
            distinct = len(memo[7][0])
            assert np.array_equal(want.nbr[1], want.nbr[6])              # the root listed twice
            if tq == FULL:
                assert (want.cnt == 1).all()
            elif T == 1023:
                assert (want.cnt - 1 == [min(len(memo[v][0]), T) for v in roots]).all() and want.cnt.max() <= min(R * L, 1023) + 1
            if tq == 0 and R * L >= 20 and T <= 3:
                assert distinct > T and want.cnt[1] == T + 1


@pytest.mark.parametrize("m", [1, 7, 300, 5000])
def test_batch_sizes_and_a_device_count_below_m(m):
    ops = _ops()
    ip, ix = _hub_graph()
    roots = np.random.default_rng(m).integers(0, 3000, m).tolist()
    memo = {}
    _check(ops, ip, ix, roots, 10, 2, 2 ** 31, 3, seed=1, memo=memo)
    _check(ops, ip, ix, roots, 10, 2, 2 ** 31, 3, seed=1, live=m - 1 if m > 1 else 0, memo=memo)
    if m == 300:
        _check(ops, ip, ix, roots, 200, 3, 2 ** 30, 50, seed=1)


def test_bad_roots_repeated_roots_and_two_calls_on_a_device_offset():
    ops = _ops()
    ip, ix = _hub_graph()
    roots = [5, 3000, 7, -1, 5, 2 ** 31 - 1, 2999, 5]
    want = _check(ops, ip, ix, roots, 50, 2, 2 ** 30, 10, seed=3, expect_status=BAD)
    clean = PS.neighbors(ip, ix, [5, 7, 5, 2999, 5], 50, 2, 2 ** 30, 10, seed=3)
    assert np.array_equal(want.nbr[[0, 2, 4, 6, 7]], clean.nbr) and np.array_equal(want.visits[[0, 2, 4, 6, 7]], clean.visits)
    assert np.array_equal(want.nbr[0], want.nbr[4]) and np.array_equal(want.nbr[0], want.nbr[7]) and want.cnt[[1, 3, 5]].tolist() == [0, 0, 0]
    for L in (2, 3, 5):
        d_off = _dev(np.array([1000], dtype=np.int64))
        step = (L + 1) // 2
        for call in range(2):
            got, status = _run(ops, ip, ix, roots[:1] + roots[6:], 50, L, 2 ** 30, 10, seed=3, off=123456, d_off=d_off)
            assert status == 0
            _same(got, PS.neighbors(ip, ix, roots[:1] + roots[6:], 50, L, 2 ** 30, 10, seed=3, off=1000 + call * step), 3, 11)
            assert int(d_off.item()) == 1000 + (call + 1) * step


def test_error_codes_past_the_ranges():
    ops = _ops()
    from grapes_amd import _lib
    lib = _lib.load()
    ip, ix = _HAND["path"][0]
    rowptr, col, roots = _dev(ip), _dev(ix), _dev(np.array([0, 1], dtype=np.int32))
    nbr, vis, cnt = _mk(2 * 1025), _mk(2 * 1025), _mk(2)

    def call(R, L, T):
        return lib.grapes_pinsage_neighbors(rowptr.data_ptr(), col.data_ptr(), 6, roots.data_ptr(), 2, None, R, L, 0, T, 0, 0, None,
                                            nbr.data_ptr(), vis.data_ptr(), cnt.data_ptr(), None, None)
    assert call(1025, 1, 3) == -1 and call(205, 5, 3) == -1 and call(1, 1025, 3) == -1 and call(10, 2, 1024) == -1 and call(10, 2, 0) == -1
    torch.cuda.synchronize()
    assert (nbr == MARK).all() and (cnt == MARK).all()
    assert call(1024, 1, 1023) == 0 and call(256, 4, 1) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="R L <= 1024"):
        ops.pinsage_neighbors(rowptr, col, 6, roots, 1025, 1, 0, 3)
    with pytest.raises(ValueError, match="T = 1024 neighbours are not built"):
        ops.pinsage_neighbors(rowptr, col, 6, roots, 10, 2, 0, 1024)


# ---------------------------------------------------------------------------------------------------- the sampler
def test_the_samplers_blocks_are_the_oracles():
    _ops()
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.pinsage import PinSAGESampler
    ip, ix = _hub_graph()
    roots = np.random.default_rng(8).permutation(3000)[:64]
    R, L, T, p, seed = 20, 3, 5, 0.25, 4242
    s = PinSAGESampler(DeviceGraph.from_csr(ip, ix), num_layers=2, num_neighbors=T, num_random_walks=R, walk_length=L,
                       termination_prob=p, seed=seed)
    for call in range(2):                                                # the second batch continues the stream: 2 blocks x ceil(3 / 2)
        b = s.sample(_dev(roots))
        s.check()
        ob = PS.sample(ip, ix, roots, 2, R, L, PS.term_q(p), T, seed=seed, off=4 * call)
        assert len(b.blocks) == 2 and 200 <= ob[0].num_nodes <= 384 and int(s.philox_offset.item()) == 4 * (call + 1)
        for d, (x, o) in enumerate(zip(b.blocks, ob)):
            assert x.num_nodes == o.num_nodes and x.num_slots == o.num_slots and x.num_seeds == len(o.seeds)
            for f in ("seeds", "nbr", "visits", "cnt", "node_idx", "loc", "tptr", "tslot"):
                assert np.array_equal(_np(getattr(x, f)), getattr(o, f)), (d, f)
            assert x.weight.dtype == torch.float32 and np.array_equal(_np(x.weight), o.weight)
            assert np.array_equal(_np(x.self_loc), o.loc[:, 0]) and x.item_cap == (0 if np.diff(o.tptr).max() <= 64 else o.num_slots // 64)
        assert torch.equal(b.blocks[1].seeds, b.blocks[0].node_idx) and torch.equal(b.node_idx, b.blocks[1].node_idx)
        assert b.num_nodes == ob[1].num_nodes and np.array_equal(_np(b.targets), roots) and np.array_equal(_np(b.local_targets), np.arange(64))
    s.sample(_dev(np.array([3, 3000])))
    with pytest.raises(GrapesHipError, match="PinSAGE sampler: index out of range"):
        s.check()
    s.check()                                                             # cleared


# ---------------------------------------------------------------------------------------------------- relu + L2 normalisation
EPS = 1e-3


def _norm_rows(m, f, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((m, f)).astype(np.float32)
    if m >= 5:
        s[0] = -np.abs(s[0]) - 1e-3                                      # all negative: nrm = 0, out = 0
        s[1] = np.abs(s[1]) * np.float32(0.25 * EPS / np.sqrt(f)) + np.float32(0.1 * EPS / np.sqrt(f))     # nrm in (0.1, ~0.9) eps
        s[2] = np.abs(s[2]) * np.float32(4 * EPS) + np.float32(2 * EPS)  # nrm >= 2 eps
    return s, rng.standard_normal((m, f)).astype(np.float32)


@pytest.mark.parametrize("m", [1, 5, 300])
@pytest.mark.parametrize("f", [1, 3, 4, 47, 64, 100, 256, 260, 1024])
def test_relu_l2norm_against_fp64(f, m):
    """The bound of the module docstring.  Every matrix is a column block of a buffer four columns wider and full of NaN, with NaN rows
    behind it: nothing past column f or row m may be read or written."""
    ops = _ops()
    s32, g32 = _norm_rows(m, f, 1000 * f + m)
    nan = float("nan")

    def block(a=None):
        buf = torch.full((m + 2, f + 4), nan, dtype=torch.float32, device="cuda")
        view = buf[:m, :f]
        if a is not None:
            view.copy_(_dev(a))
        return buf, view
    (sb, s), (gb, g), (ob, o), (db, ds) = block(s32), block(g32), block(), block()
    nrm = torch.full((m + 3,), nan, dtype=torch.float32, device="cuda")
    out, n = ops.relu_l2norm_fwd(s, EPS, out=(o, nrm))
    assert out.data_ptr() == o.data_ptr()
    ref, nref = PS.relu_l2norm64(s32, EPS)
    got, gn = _np(o).astype(np.float64), _np(nrm[:m]).astype(np.float64)
    ferr, fbound = np.abs(got - ref), PS.gamma(f + 3) * np.abs(ref) + PS.TINY
    print(f"[pinsage] relu_l2norm f={f} m={m}: fwd max err/bound {float((ferr / fbound).max()):.3f}")
    assert (ferr <= fbound).all() and (np.abs(gn - nref) <= PS.gamma(f + 3) * nref + PS.TINY).all()
    assert torch.isnan(ob[m:]).all() and torch.isnan(ob[:, f:]).all() and torch.isnan(nrm[m:]).all() and np.isfinite(got).all()
    if m >= 5:
        assert gn[0] == 0 and (got[0] == 0).all() and 0 < gn[1] < EPS < gn[2] and (got[1] > 0).all()
    ops.relu_l2norm_bwd(g, o, nrm, s, EPS, ds=ds)
    dref, mag = PS.relu_l2norm_bwd64(g32, s32, EPS)
    dgot = _np(ds).astype(np.float64)
    berr, bbound = np.abs(dgot - dref), PS.gamma(2 * f + 6) * mag + PS.TINY
    print(f"[pinsage] relu_l2norm f={f} m={m}: bwd max err/bound {float((berr / bbound).max()):.3f}")
    assert (berr <= bbound).all() and np.isfinite(dgot).all() and (dgot[s32 <= 0] == 0).all()
    assert torch.isnan(db[m:]).all() and torch.isnan(db[:, f:]).all()
    for buf, a in ((sb, s32), (gb, g32)):                                # the inputs are untouched
        assert np.array_equal(_np(buf[:m, :f]), a) and torch.isnan(buf[m:]).all() and torch.isnan(buf[:, f:]).all()
    c = ops.relu_l2norm_fwd(_dev(s32), EPS)                              # contiguous rows, fresh outputs: the same bits
    assert np.array_equal(_np(c[0]), _np(o)) and np.array_equal(_np(c[1]), _np(nrm[:m]))


# ---------------------------------------------------------------------------------------------------- the layer, the step, the driver
def _small():
    if "small" not in _G:
        _G["small"] = SO.random_graph(60, 5, 31)
    return _G["small"]


def _oracle_blocks(ob):
    return [SimpleNamespace(weight=_dev(b.weight), loc=_dev(b.loc), self_loc=_dev(np.ascontiguousarray(b.loc[:, 0])), cnt=_dev(b.cnt),
                            tptr=_dev(b.tptr), tslot=_dev(b.tslot), num_nodes=b.num_nodes, item_cap=None) for b in ob]


def _p64(t):
    return torch.as_tensor(_np(t).astype(np.float64)).requires_grad_(True)


def test_one_conv_layer_against_the_fp64_restatement():
    _ops()
    from grapes_amd.modules.pinsage import EPS as MEPS, PinSAGEConv
    ip, ix = _small()
    ob = PS.sample(ip, ix, np.random.default_rng(1).permutation(60)[:12], 1, 10, 2, PS.term_q(0.5), 4, seed=6)[0]
    torch.manual_seed(12)
    conv = PinSAGEConv(8, 16, 16).cuda()
    h32 = np.random.default_rng(2).standard_normal((ob.num_nodes, 8)).astype(np.float32)
    g32 = np.random.default_rng(3).standard_normal((12, 16)).astype(np.float32)
    h = _dev(h32).requires_grad_(True)
    out = conv(h, _oracle_blocks([ob])[0])
    out.backward(_dev(g32))
    prm = [_p64(p) for p in (conv.Q.weight, conv.Q.bias, conv.W.weight, conv.W.bias)]
    h64 = torch.as_tensor(h32.astype(np.float64)).requires_grad_(True)
    want = PS.torch_conv(h64, ob, *prm, MEPS)
    want.backward(torch.as_tensor(g32.astype(np.float64)))
    assert out.shape == (12, 16) and ((want > 0).sum(1) >= 2).all()
    errs = {"out": SG.rel_err(_np(out), want.detach().numpy()), "dh": SG.rel_err(_np(h.grad), h64.grad.numpy())}
    for name, p, q in zip(("dQw", "dQb", "dWw", "dWb"), (conv.Q.weight, conv.Q.bias, conv.W.weight, conv.W.bias), prm):
        errs[name] = SG.rel_err(_np(p.grad), q.grad.numpy())
        assert float(q.grad.abs().max()) > 0
    print("[pinsage] conv " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs.pop("out") <= ACT_TOL and max(errs.values()) <= GRAD_TOL


def test_one_trainer_step_against_the_fp64_restatement():
    """Two layers of 16 columns on a 60-node graph.  The step's batch is the oracle's (the seed is given, the stream starts at 0); its
    logits, loss and gradients (SGD with lr = 0 keeps the parameters) are judged against fp64 autograd of the plain-torch
    restatement by tests/test_sage_gpu.py's measure and tolerances."""
    ops = _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.pinsage import EPS as MEPS, PinSAGE
    from grapes_amd.pinsage import PinSAGETrainer
    torch.manual_seed(4321)
    n, F, H, C, B, T, R, L, p, seed = 60, 8, 16, 5, 10, 4, 10, 2, 0.5, 99
    ip, ix = _small()
    rng = np.random.default_rng(52)
    x32 = rng.standard_normal((n, F)).astype(np.float32)
    x, labels = _dev(x32), rng.integers(0, C, n)
    model = PinSAGE(F, [H, H], C).cuda()
    tr = PinSAGETrainer(DeviceGraph.from_csr(ip, ix), x, _dev(labels), model, torch.optim.SGD(model.parameters(), lr=0.0), num_neighbors=T,
                        num_random_walks=R, walk_length=L, termination_prob=p, batch_size=16, seed=seed)
    roots = rng.permutation(n)[:B]
    seen = {}
    forward = tr._forward
    tr._forward = lambda xb, b: seen.setdefault("logits", forward(xb, b))
    loss, b = tr.step(_dev(roots))
    ob = PS.sample(ip, ix, roots, 2, R, L, PS.term_q(p), T, seed=seed, off=0)
    assert all(np.array_equal(_np(x_.nbr), o.nbr) and np.array_equal(_np(x_.node_idx), o.node_idx) for x_, o in zip(b.blocks, ob))
    convs = [tuple(_p64(t) for t in (c.Q.weight, c.Q.bias, c.W.weight, c.W.bias)) for c in model.convs]
    lin = (_p64(model.lin.weight), _p64(model.lin.bias))
    logits = PS.torch_model(torch.as_tensor(x32[ob[1].node_idx].astype(np.float64)), ob, convs, lin, MEPS)
    l64 = SG.loss64(logits, np.arange(B), labels[roots])
    l64.backward()
    got = seen["logits"].detach()
    assert got.shape == (B, C) and SG.rel_err(_np(got), logits.detach().numpy()) <= ACT_TOL
    assert abs(float(loss) - float(l64.detach())) <= ACT_TOL * max(1.0, abs(float(l64.detach())))
    flat = [q for prm in convs for q in prm] + list(lin)
    for (name, prm), q in zip(model.named_parameters(), flat):
        err = SG.rel_err(_np(prm.grad), q.grad.numpy())
        print(f"[pinsage] step d {name} err {err:.2e}")
        assert prm.grad is not None and float(q.grad.abs().max()) > 0 and err <= GRAD_TOL
    before = int(tr.sampler.philox_offset.item())
    masks = (_dev(np.arange(n) < 20), _dev(np.arange(n) >= 40))
    first, again = tr.evaluate(masks), tr.evaluate(masks)
    assert first == again and all(0.0 <= v <= 1.0 for v in first) and model.training
    assert int(tr.sampler.philox_offset.item()) == before == 2 and int(tr.eval_sampler.philox_offset.item()) > 0
    assert ops.PPRGO_MAX_ROOTS == 4096


def test_cli_three_epochs_lower_the_loss(capsys):
    _ops()
    from grapes_amd import pinsage
    v = pinsage.main(["--dataset", "cora", "--max_epoch", "3", "--hidden_dim", "32", "--batch_size", "64", "--lr", "0.01", "--seed", "1"])
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"Loss: ([0-9.]+)", out)]
    assert out.count("Epoch: ") == 3 and np.isfinite(v) and 0.0 <= v <= 1.0
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[2] < losses[0]
