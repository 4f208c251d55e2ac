"""GCNConv(improved, add_self_loops, normalize, bias) on the MI355X (grapes_amd/csrc/wgcn_kernels.hip with a mode): every
floating-point output — out, dx, dW, db, d edge_weight — against the fp64 oracle of tests/gcnconv_modes_oracle.py under the
project's element-wise criterion (oracle/accuracy.py: assert_fp32_accuracy, MAX_FACTOR = 6, RMS_FACTOR = 3, unchanged), and
finite.

Graphs (tests/wgcn_oracle.py): the hand graph (node 2 with two stored loops of different weights, 0 -> 1 stored twice, nodes 0
and 5 without an incoming entry); random_graph(300, 2400, 1) (duplicates, stored loops, one node with many; every row by one lane
group); long_graph() (n = 2304, rows of ~700 entries both ways, rows of exactly 64 and 65: chunks + combine in both directions).
Aggregation widths 1, 7, 64, 260: scalar and float4 columns, 4 slabs.  Weights: uniform, 2^-10 .. 2^10, ones."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc
from tests import gcnconv_modes_oracle as M
from tests import wgcn_oracle as O

pytestmark = pytest.mark.gpu

MODE_NAMES = list(M.MODES)
_GRAPHS, _PROBLEMS = {}, {}


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(4321)                 # the layers' initial weights: the same problem in every run


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph(name):
    """(src, dst, n, edge index on the device) — one tensor per graph, so the layers share its cached structure."""
    if name not in _GRAPHS:
        if name == "hand":
            s, d, _, n = O.hand_graph()
        elif name == "small":
            (s, d), n = O.random_graph(300, 2400, 1), 300
        else:
            s, d, n = O.long_graph()
        _GRAPHS[name] = (s, d, n, torch.from_numpy(np.stack([s, d])).cuda())
    return _GRAPHS[name]


def _problem(name, kind, mode) -> M.ModeProblem:
    key = (name, kind, mode)
    if key not in _PROBLEMS:
        s, d, n, _ = _graph(name)
        w = O.hand_graph()[2] if kind == "hand" else O.weights(kind, len(s), 5)
        _PROBLEMS[key] = M.ModeProblem(s, d, w, n, *M.MODES[mode])
    return _PROBLEMS[key]


def _layer(mode, fi, fo, bias=True, seed=0):
    from grapes_amd.modules.gcn import GCNConv
    imp, asl, nrm = M.MODES[mode]
    layer = GCNConv(fi, fo, improved=imp, add_self_loops=asl, normalize=nrm, bias=bias).cuda()
    if bias:
        with torch.no_grad():
            layer.bias.copy_(_dev((np.random.default_rng(seed).standard_normal(fo) * 0.1).astype(np.float32)))
    return layer


def _judge(got, ref, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite outputs"
    return acc.assert_fp32_accuracy(got, ref[0], ref[1], ref[2], what)


def _layer_case(name, kind, mode, fi, fo, relu, x_grad, weighted=True, bias=True, seed=21):
    """One layer forward + backward judged output by output.  weighted False: no edge_weight is passed and the oracle's weights
    are ones (kind must be "ones").  Returns (layer, out, edge-weight gradient or None, the oracle's result)."""
    _ops()
    s, d, n, ei = _graph(name)
    P = _problem(name, kind, mode)
    rng = np.random.default_rng(seed)
    layer = _layer(mode, fi, fo, bias, seed)
    x = _dev(rng.standard_normal((n, fi)).astype(np.float32)).requires_grad_(x_grad)
    ew = _dev(P.w32).requires_grad_(True) if weighted else None
    dout = rng.standard_normal((n, fo)).astype(np.float32)
    out = layer(x, ei, relu=relu, edge_weight=ew)
    out.backward(_dev(dout))
    r = P.layer(x.detach().cpu().numpy(), layer.lin.weight.detach().cpu().numpy(),
                layer.bias.detach().cpu().numpy() if bias else None, relu, dout,
                gate=(out.detach() > 0).cpu().numpy() if relu else None)
    what = f"{mode} {name} {kind} {fi}->{fo} relu={relu} weighted={weighted} bias={bias}"
    _judge(out, r["out"], what + " out")
    _judge(layer.lin.weight.grad, r["dW"], what + " dW")
    if bias:
        _judge(layer.bias.grad, r["db"], what + " db")
    else:
        assert layer.bias is None
    if weighted:
        _judge(ew.grad, r["dw"], what + " d edge_weight")
    if x_grad:
        _judge(x.grad, r["dx"], what + " dx")
    else:
        assert x.grad is None
    return layer, out, (ew.grad if weighted else None), r


TRANSFORM_FIRST = [("hand", "hand", 8, 7, True), ("small", "uniform", 8, 1, False), ("small", "mixed", 64, 64, True),
                   ("long", "uniform", 260, 260, True), ("long", "mixed", 64, 7, False), ("long", "ones", 64, 64, True)]
AGGREGATE_FIRST = [("small", "mixed", 7, 64, True), ("long", "uniform", 64, 260, True), ("long", "mixed", 7, 8, False),
                   ("hand", "hand", 260, 264, False)]


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("name,kind,fi,fo,relu", TRANSFORM_FIRST)
def test_layer_transform_first(mode, name, kind, fi, fo, relu):
    """f_in >= f_out: H = x Wᵀ, then the aggregation (width f_out) with bias and ReLU; forward and all four gradients."""
    _layer_case(name, kind, mode, fi, fo, relu, True)


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("name,kind,fi,fo,relu", AGGREGATE_FIRST)
def test_layer_aggregate_first(mode, name, kind, fi, fo, relu):
    """f_in < f_out and x without a gradient: (Â x) Wᵀ, the aggregation at width f_in."""
    _layer_case(name, kind, mode, fi, fo, relu, False, seed=22)


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("name,fi,fo,relu,x_grad", [("small", 64, 7, True, True), ("long", 64, 64, False, True),
                                                     ("long", 7, 64, True, False), ("hand", 8, 7, False, True)])
def test_layer_without_edge_weight(mode, name, fi, fo, relu, x_grad):
    """No edge_weight: the same kernels with every weight 1 (the default mode: the unweighted layer), judged against the oracle
    over ones."""
    _layer_case(name, "ones", mode, fi, fo, relu, x_grad, weighted=False, seed=23)


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("name,fi,fo,relu,x_grad", [("long", 64, 7, True, True), ("small", 7, 64, True, False)])
def test_layer_without_bias(mode, weighted, name, fi, fo, relu, x_grad):
    layer, _, _, _ = _layer_case(name, "uniform" if weighted else "ones", mode, fi, fo, relu, x_grad, weighted=weighted, bias=False,
                                 seed=24)
    assert [n for n, _ in layer.named_parameters()] == ["lin.weight"]


def _run(layer, x0, ei, ew0, dout, relu=True):
    layer.zero_grad()
    x = x0.clone().requires_grad_(True)
    ew = ew0.clone().requires_grad_(True) if ew0 is not None else None
    out = layer(x, ei, relu=relu, edge_weight=ew)
    out.backward(dout)
    res = [out.detach().clone(), x.grad.clone(), layer.lin.weight.grad.clone()]
    if layer.bias is not None:
        res.append(layer.bias.grad.clone())
    if ew is not None:
        res.append(ew.grad.clone())
    return res


@pytest.mark.parametrize("weighted", [False, True])
def test_spelled_out_defaults_are_bit_equal_to_the_default_layer(weighted):
    _ops()
    from grapes_amd.modules.gcn import GCNConv
    for name, fi, fo in (("small", 64, 47), ("long", 128, 64)):
        s, d, n, ei = _graph(name)
        torch.manual_seed(5)
        a = GCNConv(fi, fo).cuda()
        torch.manual_seed(5)
        b = GCNConv(fi, fo, improved=False, add_self_loops=True, normalize=True, bias=True).cuda()
        x0, dout = torch.randn(n, fi, device="cuda"), torch.randn(n, fo, device="cuda")
        ew = _dev(O.weights("mixed", len(s), 5)) if weighted else None
        for u, v in zip(_run(a, x0, ei, ew, dout), _run(b, x0, ei, ew, dout)):
            assert torch.equal(u, v)
        with torch.no_grad():                                   # the full-batch inference path of the long graph
            assert torch.equal(a(x0, ei, relu=True, edge_weight=ew), b(x0, ei, relu=True, edge_weight=ew))


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_two_runs_are_bit_equal(mode):
    _ops()
    s, d, n, ei = _graph("long")
    layer = _layer(mode, 128, 64)
    x0, dout = torch.randn(n, 128, device="cuda"), torch.randn(n, 64, device="cuda")
    ew = _dev(O.weights("mixed", len(s), 5))
    for w in (ew, None):
        for u, v in zip(_run(layer, x0, ei, w, dout), _run(layer, x0, ei, w, dout)):
            assert torch.equal(u, v)


def test_without_added_loops_every_stored_loop_has_a_gradient_and_a_sourceless_node_outputs_the_bias():
    _ops()
    for mode in ("no_loops", "plain"):
        layer, out, dew, r = _layer_case("hand", "hand", mode, 8, 7, False, True, seed=25)
        s, d, n, _ = _graph("hand")
        loops2 = np.nonzero((s == 2) & (d == 2))[0]
        assert len(loops2) == 2
        g = dew.cpu().numpy()
        assert np.all(g[loops2] != 0) and g[loops2[0]] == g[loops2[1]]            # both get the loop term, the same one
        want = r["dw"][0].numpy()[loops2]
        assert np.allclose(g[loops2], want, rtol=1e-4, atol=1e-6)                 # (the criterion above judged all of d edge_weight)
        assert torch.equal(out[0].detach(), layer.bias.detach()) and torch.equal(out[5].detach(), layer.bias.detach())
    # the many-loop node of the random graph
    layer, out, dew, r = _layer_case("small", "uniform", "no_loops", 64, 7, True, True, seed=26)
    P = _problem("small", "uniform", "no_loops")
    node = np.bincount(P.src[P.loops]).argmax()
    mine = P.loops[P.src[P.loops] == node]
    assert len(mine) >= 3 and np.all(dew.cpu().numpy()[mine] != 0)


def test_unnormalised_ones_is_the_unweighted_neighbour_sum():
    _ops()
    for name, fi, fo in (("small", 64, 7), ("long", 7, 64)):
        s, d, n, ei = _graph(name)
        P = _problem(name, "ones", "plain")
        layer = _layer("plain", fi, fo)
        x = _dev(np.random.default_rng(27).standard_normal((n, fi)).astype(np.float32))
        with torch.no_grad():
            ones = layer(x, ei, edge_weight=torch.ones(len(s), device="cuda"))
            none = layer(x, ei)
        assert torch.equal(ones, none)
        W, b = layer.lin.weight.detach().cpu().numpy(), layer.bias.detach().cpu().numpy()
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
        # the neighbour sum spelled out: one addition per stored entry, loops included
        H = x.cpu().numpy().astype(np.float64) @ W.astype(np.float64).T
        want = np.zeros_like(H)
        np.add.at(want, d, H[s])
        want += b.astype(np.float64)
        r = P.layer(x.cpu().numpy(), W, b, False, np.zeros((n, fo), np.float32))
        assert np.allclose(r["out64"].numpy(), want, rtol=1e-12, atol=1e-12)
        _judge(ones, r["out"], f"plain ones {name} {fi}->{fo}")


def test_loop_lists_are_in_input_order():
    ops = _ops()
    from grapes_amd.modules.gcn import weighted_structure
    for name in ("hand", "small", "long"):
        s, d, n, ei = _graph(name)
        ws = weighted_structure(ei, n)
        loop_ptr, loop_idx = (t.cpu().numpy() for t in ws.loops())
        loops = np.nonzero(s == d)[0]
        want_ptr = np.concatenate([[0], np.cumsum(np.bincount(s[loops], minlength=n))])
        want_idx = loops[np.lexsort((loops, s[loops]))]                           # by node, a node's loops in input order
        assert np.array_equal(loop_ptr, want_ptr), name
        assert np.array_equal(loop_idx[:len(loops)], want_idx), name
        assert np.bincount(s[loops]).max() >= 2
        s32, d32 = ei[0].to(torch.int32).contiguous(), ei[1].to(torch.int32).contiguous()
        again = ops.WeightedStructure(ws.prep, s32, d32).loops()
        assert torch.equal(again[0], ws.loops()[0]) and torch.equal(again[1][:len(loops)], ws.loops()[1][:len(loops)])
        # the weight pass adds them in that order: lw bit-equal to the host's sequential fp32 sum
        P = _problem(name, "hand" if name == "hand" else "mixed", "no_loops")
        vals = ops.wgcn_weights(ws, _dev(P.w32), ops.WGCN_LOOP_SUM)
        assert np.array_equal(vals.lw[:n].cpu().numpy(), P.lw32), name
        plain = ops.wgcn_weights(ws, None, ops.WGCN_UNNORMALIZED)
        assert plain.dinv is None and np.array_equal(plain.lw[:n].cpu().numpy(), np.bincount(s[loops], minlength=n).astype(np.float32))


@pytest.mark.parametrize("mode", ["improved", "no_loops", "plain"])
def test_other_modes_refuse_prepared_graphs(mode):
    ops = _ops()
    s, d, n, ei = _graph("small")
    layer = _layer(mode, 8, 7)
    x = torch.randn(n, 8, device="cuda")
    prep = ops.PreparedGraph(ei[0].int().contiguous(), ei[1].int().contiguous(), n)
    with pytest.raises(ValueError):
        layer(x, prep)
    with pytest.raises(ValueError):
        layer(x, prep, edge_weight=torch.ones(len(s), device="cuda"))
    with pytest.raises(ValueError):
        layer(x, ei, large_graph=True)
