"""GCNConv with edge weights on the MI355X (grapes_amd/csrc/wgcn_kernels.hip): every floating-point output against the fp64
oracle of tests/wgcn_oracle.py under the project's element-wise criterion (oracle/accuracy.py: MAX_FACTOR = 6, RMS_FACTOR = 3
against a host fp32 baseline that adds the same terms in row order), per output tensor: out, dx, dW, db, d edge_weight.

Graphs: the hand graph of the CPU tests; "small" (n = 300, e = 2400, duplicates and stored loops, every row by one group of lanes);
"long" (n = 2304 > _SMALL_GRAPH, e ~ 12k, a node with ~700 incoming and one with ~700 outgoing entries — chunk + combine in both
directions — and rows of exactly 64 and 65 entries).  Widths 1, 7, 47, 64, 128, 256, 260: scalar columns at 32 and 64 lanes and
with 4 slabs, float4 columns at 32 and 64 lanes and with 4 slabs, the logit width.  Weights: uniform (0, 2), magnitudes spread
over 2^-10 .. 2^10, all ones."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc
from tests import wgcn_oracle as O

pytestmark = pytest.mark.gpu

WIDTHS = (1, 7, 47, 64, 128, 256, 260)
SENTINEL = -12345.5
_CACHE = {}


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(1234)                 # the layers' initial weights: the same problem in every run


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _misaligned(a):
    """a [rows, f] on the device at an address that is 4 mod 16 (the scalar-column kernels)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
    off = next(o for o in range(0, 8) if (buf.data_ptr() + 4 * o) % 16 == 4)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _edges(name):
    if name == "hand":
        s, d, _, n = O.hand_graph()
    elif name == "small":
        s, d = O.random_graph(300, 2400, 1)
        n = 300
    else:
        s, d, n = O.long_graph()
    return s, d, n


class _G:
    """One graph on the device (edge index, PreparedGraph, WeightedStructure) and, per weight kind, its host Problem."""

    def __init__(self, ops, name):
        self.src, self.dst, self.n = _edges(name)
        self.e = len(self.src)
        self.ei = torch.from_numpy(np.stack([self.src, self.dst])).cuda()
        s32, d32 = self.ei[0].to(torch.int32).contiguous(), self.ei[1].to(torch.int32).contiguous()
        self.prep = ops.PreparedGraph(s32, d32, self.n)
        self.ws = ops.WeightedStructure(self.prep, s32, d32)
        self.name, self.problems = name, {}

    def problem(self, kind):
        if kind not in self.problems:
            w = O.hand_graph()[2] if (self.name == "hand" and kind == "hand") else O.weights(kind, self.e, 5)
            self.problems[kind] = O.Problem(self.src, self.dst, w, self.n)
        return self.problems[kind]


def _graph(ops, name) -> _G:
    if name not in _CACHE:
        _CACHE[name] = _G(ops, name)
    return _CACHE[name]


def _judge(got, ref, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite outputs"
    return acc.assert_fp32_accuracy(got, ref[0], ref[1], ref[2], what)


def test_long_graph_takes_the_item_path():
    ops = _ops()
    g = _graph(ops, "long")
    assert g.n > ops._SMALL_GRAPH and int(g.prep.n_items_t) > 0 and int(g.prep.n_items_s) > 0
    P = g.problem("uniform")
    assert P.lens_t[7] >= 690 and P.lens_s[11] >= 690 and P.lens_t[20] == 64 and P.lens_t[21] == 65
    assert _graph(ops, "small").n <= ops._SMALL_GRAPH


def test_structure_is_a_bijection_in_input_order():
    """pos_t / pos_s: the slots of the non-loop entries, each once, duplicates in input order (the host's stable sort gives the
    same numbers); loop_src: the last stored loop; two builds bit-equal."""
    ops = _ops()
    for name in ("hand", "small", "long"):
        g = _graph(ops, name)
        P = g.problem("ones")
        again = ops.WeightedStructure(g.prep, g.ws.edge_src, g.ws.edge_dst)
        for a in ("pos_t", "pos_s", "inv_t", "inv_s", "loop_src"):
            assert torch.equal(getattr(g.ws, a), getattr(again, a)), (name, a)
        m = len(P.keep)
        assert int(g.prep.rowptr_t[g.n]) == m and int(g.prep.rowptr_s[g.n]) == m
        for pos, slot in ((g.ws.pos_t, P.slot_t), (g.ws.pos_s, P.slot_s)):
            pos = pos[:g.e].cpu().numpy()
            assert np.array_equal(np.sort(pos[pos >= 0]), np.arange(m)), name
            assert np.array_equal(pos, slot), name
        assert np.array_equal(g.ws.loop_src[:g.n].cpu().numpy(), P.loop_src), name
        inv = g.ws.inv_t[:m].cpu().numpy()
        assert np.array_equal(g.ws.pos_t.cpu().numpy()[inv], np.arange(m))


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("name", ["small", "long"])
def test_forward_op(name, kind):
    """ops.wgcn_aggregate_fwd at every width, with and without bias and ReLU (one set of reference sums per width)."""
    ops = _ops()
    g = _graph(ops, name)
    P = g.problem(kind)
    vals = ops.wgcn_weights(g.ws, _dev(P.w32))
    d = vals.dinv[:g.n].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(d - P.dinv) <= (P.lens_t + 4) * 2.0 ** -24 * P.dinv)         # an (L + 1)-term fp32 sum, a root, a quotient
    rng = np.random.default_rng(11)
    for f in WIDTHS:
        h = rng.standard_normal((g.n, f)).astype(np.float32)
        bias = (rng.standard_normal(f) * 0.1).astype(np.float32)
        sums = P.aggregate_sums(h)
        hd, bd = _dev(h), _dev(bias)
        for b in (None, bias):
            for relu in (False, True):
                out = ops.wgcn_aggregate_fwd(hd, g.ws, vals, bd if b is not None else None, relu)
                _judge(out, acc.aggregate_finish(sums, b, relu), f"fwd {name} {kind} f={f} bias={b is not None} relu={relu}")


def test_forward_op_hand_graph_and_misaligned_rows():
    ops = _ops()
    g = _graph(ops, "hand")
    P = g.problem("hand")
    vals = ops.wgcn_weights(g.ws, _dev(P.w32))
    assert np.array_equal(vals.lw[:g.n].cpu().numpy(), P.lw32)
    rng = np.random.default_rng(12)
    for f in (1, 7, 64):
        h = rng.standard_normal((g.n, f)).astype(np.float32)
        _judge(ops.wgcn_aggregate_fwd(_dev(h), g.ws, vals), P.aggregate(h), f"fwd hand f={f}")
    g = _graph(ops, "long")
    P = g.problem("uniform")
    vals = ops.wgcn_weights(g.ws, _dev(P.w32))
    h = rng.standard_normal((g.n, 64)).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    out = ops.wgcn_aggregate_fwd(_misaligned(h), g.ws, vals, _dev(bias), True)
    _judge(out, P.aggregate(h, bias, True), "fwd long f=64, rows at 4 mod 16")
    dout = rng.standard_normal((g.n, 64)).astype(np.float32)
    dh, db, dw = ops.wgcn_aggregate_bwd(_misaligned(dout), g.ws, vals, h=_misaligned(h), want_dw=True)
    _judge(dh, P.aggregate(dout, transpose=True), "bwd dh long f=64, rows at 4 mod 16")
    _judge(dw, P.weight_grad(dout, h), "bwd dw long f=64, rows at 4 mod 16")
    _judge(db, acc.colsum_reference(dout), "bwd db long f=64, rows at 4 mod 16")


@pytest.mark.parametrize("f,misaligned", [(256, False), (260, False), (130, False), (256, True)])
def test_backward_op_wide(f, misaligned):
    """ops.wgcn_aggregate_bwd with the ReLU gate and the weight gradient on the long graph at the widths above 128: float4 columns
    at 64 lanes (256) and with 4 slabs (260), scalar columns with 4 slabs (130: no multiple of 4; 256 at an address 4 mod 16) —
    the rows / chunks / combine kernels of both passes, dH, dbias and dw each."""
    ops = _ops()
    g = _graph(ops, "long")
    P = g.problem("mixed")
    vals = ops.wgcn_weights(g.ws, _dev(P.w32))
    rng = np.random.default_rng(40 + f)
    h = rng.standard_normal((g.n, f)).astype(np.float32)
    dout = rng.standard_normal((g.n, f)).astype(np.float32)
    act = np.maximum(rng.standard_normal((g.n, f)), 0).astype(np.float32)            # a ReLU output: about half its entries 0
    put = _misaligned if misaligned else _dev
    dh, db, dw = ops.wgcn_aggregate_bwd(put(dout), g.ws, vals, h=put(h), relu_out=put(act), want_dw=True)
    G = np.where(act > 0, dout, np.float32(0))
    what = f"bwd long f={f}{' at 4 mod 16' if misaligned else ''}"
    _judge(dh, P.aggregate(G, transpose=True), what + " dh")
    _judge(db, acc.colsum_reference(dout, gate=act), what + " db")
    _judge(dw, P.weight_grad(G, h), what + " dw")


def test_rows_past_n_are_untouched():
    ops = _ops()
    g = _graph(ops, "long")
    P = g.problem("uniform")
    vals = ops.wgcn_weights(g.ws, _dev(P.w32))
    cap = g.n + 19
    for f in (7, 128):
        h = torch.full((cap, f), float("nan"), device="cuda")
        h[:g.n] = torch.randn(g.n, f, device="cuda")
        out = torch.full((cap, f), SENTINEL, device="cuda")
        got = ops.wgcn_aggregate_fwd(h, g.ws, vals, None, False, out=out)
        assert got is out and bool((out[g.n:] == SENTINEL).all()) and bool(torch.isfinite(out[:g.n]).all())
        _judge(out[:g.n], P.aggregate(h[:g.n].cpu().numpy()), f"fwd into a padded buffer f={f}")


def _layer_case(ops, name, kind, fi, fo, relu, x_grad, seed):
    from grapes_amd.modules.gcn import GCNConv
    g = _graph(ops, name)
    P = g.problem(kind)
    rng = np.random.default_rng(seed)
    layer = GCNConv(fi, fo).cuda()
    with torch.no_grad():
        layer.bias.copy_(_dev((rng.standard_normal(fo) * 0.1).astype(np.float32)))
    x = _dev(rng.standard_normal((g.n, fi)).astype(np.float32)).requires_grad_(x_grad)
    ew = _dev(P.w32).requires_grad_(True)
    dout = rng.standard_normal((g.n, fo)).astype(np.float32)
    out = layer(x, g.ei, relu=relu, edge_weight=ew)
    out.backward(_dev(dout))
    r = P.layer(x.detach().cpu().numpy(), layer.lin.weight.detach().cpu().numpy(), layer.bias.detach().cpu().numpy(), relu, dout,
                gate=(out.detach() > 0).cpu().numpy() if relu else None)
    what = f"layer {name} {kind} {fi}->{fo} relu={relu}"
    _judge(out, r["out"], what + " out")
    _judge(layer.lin.weight.grad, r["dW"], what + " dW")
    _judge(layer.bias.grad, r["db"], what + " db")
    _judge(ew.grad, r["dw"], what + " d edge_weight")
    if x_grad:
        _judge(x.grad, r["dx"], what + " dx")
    else:
        assert x.grad is None
    return r


@pytest.mark.parametrize("name,kind,fi,fo,relu", [("small", "uniform", 64, 47, True), ("long", "mixed", 128, 128, False),
                                                    ("long", "uniform", 260, 64, True), ("small", "mixed", 32, 1, False),
                                                    ("hand", "hand", 8, 7, True)])
def test_layer_transform_first(name, kind, fi, fo, relu):
    """f_in >= f_out: H = x Wᵀ, then the weighted aggregation with bias and ReLU; forward and all four gradients."""
    _layer_case(_ops(), name, kind, fi, fo, relu, True, 21)


@pytest.mark.parametrize("name,kind,fi,fo,relu", [("small", "mixed", 47, 128, True), ("long", "uniform", 100, 256, True),
                                                    ("long", "mixed", 64, 260, False)])
def test_layer_aggregate_first(name, kind, fi, fo, relu):
    """f_in < f_out and x without a gradient: (Â_w x) Wᵀ; the edge-weight gradient's G is linear_bwd_input(gated dout, W), its H is x."""
    _layer_case(_ops(), name, kind, fi, fo, relu, False, 22)


@pytest.mark.parametrize("fi,fo", [(64, 47), (47, 64)])
def test_weights_only_gradient(fi, fo):
    """x and the layer frozen, edge_weight.requires_grad: both forms give d edge_weight and nothing else."""
    ops = _ops()
    from grapes_amd.modules.gcn import GCNConv
    g = _graph(ops, "long")
    P = g.problem("uniform")
    rng = np.random.default_rng(23)
    layer = GCNConv(fi, fo).cuda().requires_grad_(False)
    x = _dev(rng.standard_normal((g.n, fi)).astype(np.float32))
    ew = _dev(P.w32).requires_grad_(True)
    dout = rng.standard_normal((g.n, fo)).astype(np.float32)
    out = layer(x, g.ei, relu=True, edge_weight=ew)
    out.backward(_dev(dout))
    assert layer.lin.weight.grad is None and layer.bias.grad is None
    r = P.layer(x.cpu().numpy(), layer.lin.weight.cpu().numpy(), layer.bias.cpu().numpy(), True, dout, gate=(out.detach() > 0).cpu().numpy())
    _judge(out, r["out"], f"weights only {fi}->{fo} out")
    _judge(ew.grad, r["dw"], f"weights only {fi}->{fo} d edge_weight")


def test_all_ones_agree_with_the_unweighted_layer_and_none_is_todays_path():
    ops = _ops()
    from grapes_amd.modules.gcn import GCNConv
    rng = np.random.default_rng(24)
    for name in ("small", "long"):                                  # (both lists hold stored loops and duplicates)
        g = _graph(ops, name)
        P = g.problem("ones")
        assert (P.loop_src >= 0).any()
        for fi, fo in ((64, 47), (47, 64)):
            layer = GCNConv(fi, fo).cuda()
            x = _dev(rng.standard_normal((g.n, fi)).astype(np.float32))
            with torch.no_grad():
                plain = layer(x, g.ei, relu=True)
                assert torch.equal(plain, layer(x, g.ei, relu=True, edge_weight=None))
                ones = layer(x, g.ei, relu=True, edge_weight=torch.ones(g.e, device="cuda"))
            with torch.enable_grad():
                assert torch.equal(layer(x, g.ei), layer(x, g.ei, edge_weight=None))
            r = P.layer(x.cpu().numpy(), layer.lin.weight.detach().cpu().numpy(), layer.bias.detach().cpu().numpy(), True,
                        np.zeros((g.n, fo), np.float32))
            _judge(ones, r["out"], f"all ones {name} {fi}->{fo}: weighted")
            _judge(plain, r["out"], f"all ones {name} {fi}->{fo}: unweighted")


def test_zero_weight_loop_on_a_node_without_incoming_entries():
    """deg = 0: dinv = 0, the output row is the bias, every gradient is finite and the loop's is exactly 0."""
    ops = _ops()
    from grapes_amd.modules.gcn import GCNConv
    src, dst = np.array([0, 1, 2, 2, 3]), np.array([1, 0, 2, 3, 0])
    w = np.array([1.0, 0.5, 0.0, 2.0, 0.25], np.float32)
    ei = torch.from_numpy(np.stack([src, dst])).cuda()
    layer = GCNConv(8, 7).cuda()
    with torch.no_grad():
        layer.bias.copy_(torch.arange(1, 8, device="cuda").float())
    rng = np.random.default_rng(25)
    x = _dev(rng.standard_normal((4, 8)).astype(np.float32)).requires_grad_(True)
    ew = _dev(w).requires_grad_(True)
    out = layer(x, ei, edge_weight=ew)
    dout = rng.standard_normal((4, 7)).astype(np.float32)
    out.backward(_dev(dout))
    assert torch.equal(out[2].detach(), layer.bias.detach())
    for t in (x.grad, ew.grad, layer.lin.weight.grad, layer.bias.grad):
        assert bool(torch.isfinite(t).all())
    assert float(ew.grad[2]) == 0.0
    r = O.Problem(src, dst, w, 4).layer(x.detach().cpu().numpy(), layer.lin.weight.detach().cpu().numpy(),
                                        layer.bias.detach().cpu().numpy(), False, dout)
    _judge(out, r["out"], "zero loop out"); _judge(ew.grad, r["dw"], "zero loop d edge_weight"); _judge(x.grad, r["dx"], "zero loop dx")


def test_two_runs_are_bit_equal():
    ops = _ops()
    from grapes_amd.modules.gcn import GCNConv
    g = _graph(ops, "long")
    P = g.problem("mixed")
    layer = GCNConv(128, 64).cuda()
    x0 = torch.randn(g.n, 128, device="cuda")
    dout = torch.randn(g.n, 64, device="cuda")
    runs = []
    for _ in range(2):
        layer.zero_grad()
        x = x0.clone().requires_grad_(True)
        ew = _dev(P.w32).requires_grad_(True)
        out = layer(x, g.ei, relu=True, edge_weight=ew)
        out.backward(dout)
        runs.append([out.detach().clone(), x.grad.clone(), ew.grad.clone(), layer.lin.weight.grad.clone(), layer.bias.grad.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_gcn_routes_a_list_of_weights():
    """GCN with a two-layer list: the hidden layer takes edge_index[-1] with edge_weight[-1], the last layer [0] with [0].  Logits and
    the four parameter gradients under the element-wise criterion: reference, magnitude and fp32 baseline are chained through both
    layers (Problem.chain_forward / chain_backward: each layer's operands are the triples the other layer produced), the hidden
    layer's ReLU gates taken from the device; the chained fp64 reference is itself checked against autograd on forward64."""
    ops = _ops()
    from grapes_amd.modules.gcn import GCN
    n, fi, hid, C = 300, 64, 32, 7
    e0, e1 = O.random_graph(n, 1500, 31), O.random_graph(n, 1800, 32)
    w0, w1 = O.weights("uniform", 1500, 33), O.weights("uniform", 1800, 34)
    ei = [torch.from_numpy(np.stack(e)).cuda() for e in (e0, e1)]
    model = GCN(fi, [hid, C], dropout=0.0).cuda()
    rng = np.random.default_rng(35)
    with torch.no_grad():
        for layer in model.gcn_layers:
            layer.bias.copy_(_dev((rng.standard_normal(layer.out_channels) * 0.1).astype(np.float32)))
    x32 = rng.standard_normal((n, fi)).astype(np.float32)
    x = _dev(x32)
    ew = [_dev(w0), _dev(w1)]
    logits, _ = model(x, ei, edge_weight=ew)
    dout = rng.standard_normal((n, C)).astype(np.float32)
    logits.backward(_dev(dout))
    with torch.no_grad():
        gate = (model.gcn_layers[0](x, ei[1], relu=True, edge_weight=ew[1]) > 0).cpu().numpy()
    npf = lambda p: p.detach().cpu().numpy()
    W1, b1, W2, b2 = (npf(p) for p in (model.gcn_layers[0].lin.weight, model.gcn_layers[0].bias,
                                       model.gcn_layers[1].lin.weight, model.gcn_layers[1].bias))
    P0, P1 = O.Problem(e0[0], e0[1], w0, n), O.Problem(e1[0], e1[1], w1, n)
    x3 = (x32.astype(np.float64), np.abs(x32.astype(np.float64)), x32)
    h3 = P1.chain_forward(x3, W1, b1, gate=gate)                    # hidden layer: edge_index[-1], edge_weight[-1]
    lg3 = P0.chain_forward(h3, W2, b2)                              # last layer: [0], [0]
    d64 = dout.astype(np.float64)
    back2 = P0.chain_backward((d64, np.abs(d64), dout), h3, W2)
    g64 = gate.astype(np.float64)
    G1 = tuple(v * g64.astype(v.dtype) for v in back2["dx"])
    back1 = P1.chain_backward(G1, x3, W1)
    # the chained reference against autograd on the fp64 restatement
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    ps = [t(p).requires_grad_(True) for p in (W1, b1, W2, b2)]
    ref = O.forward64(O.forward64(t(x32), ps[0], ps[1], e1[0], e1[1], t(w1), n, gate=gate), ps[2], ps[3], e0[0], e0[1], t(w0), n)
    ref.backward(t(dout))
    assert np.allclose(ref.detach().numpy(), lg3[0], rtol=1e-11, atol=1e-12)
    got = {"dW1": model.gcn_layers[0].lin.weight.grad, "db1": model.gcn_layers[0].bias.grad,
           "dW2": model.gcn_layers[1].lin.weight.grad, "db2": model.gcn_layers[1].bias.grad}
    want = {"dW1": back1["dW"], "db1": back1["db"], "dW2": back2["dW"], "db2": back2["db"]}
    for (k, v), p in zip(want.items(), ps):
        assert np.allclose(p.grad.numpy(), v[0], rtol=1e-10, atol=1e-12), k
    _judge(logits, lg3, "GCN two layers: logits")
    for k in want:
        _judge(got[k], want[k], f"GCN two layers: {k}")
    # the other routing is a different function
    swapped = O.forward64(O.forward64(t(x32), ps[0], ps[1], e0[0], e0[1], t(w0), n, relu=True), ps[2], ps[3], e1[0], e1[1], t(w1), n)
    assert float((swapped.detach() - ref.detach()).abs().max()) > 1e-2
    # entries may be None: that layer is today's unweighted one
    with torch.no_grad():
        mixed, _ = model(x, ei, edge_weight=[None, ew[1]])
        h = model.gcn_layers[0](x, ei[1], relu=True, edge_weight=ew[1])
        assert torch.equal(mixed, model.gcn_layers[1](h, ei[0]))
    # the refusals that need a device
    with pytest.raises(ValueError):
        model(x, ei, edge_weight=[ew[0].cpu(), ew[1]])
    with pytest.raises(ValueError):
        model(x, ei, edge_weight=[ew[1], ew[0]])                    # wrong lengths
    with pytest.raises(ValueError):
        model.gcn_layers[0](x, ei[1], edge_weight=ew[1].double())
    with pytest.raises(ValueError):
        model.gcn_layers[0](x, ops.PreparedGraph(ei[1][0].int().contiguous(), ei[1][1].int().contiguous(), n), edge_weight=ew[1])
    with pytest.raises(ValueError):
        model(x, ei, edge_weight=[ew[0]])
