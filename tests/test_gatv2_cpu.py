"""CPU checks of the GATv2 classifier (PyG's GATv2Conv, [PyG-recall]): the fp64 oracle of tests/gatv2_oracle.py against the dense
closed form and against torch.autograd, the kink-free input construction of the GPU tests, the module's parameters and refusals,
the no-CPU-path refusal and the drivers' --classifier gatv2 / --gat_heads flags."""
import numpy as np
import pytest
import torch

from tests import gatv2_oracle as O


def _params(fi, heads, c, seed, concat=True, share=False, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    f = heads * c

    def u(*shape):
        return (torch.rand(*shape, generator=g, dtype=O.F64) - 0.5) * 2 * scale
    W_l, b_l, W_r, b_r = u(f, fi), u(f), u(f, fi), u(f)
    att, b = u(1, heads, c), u(f if concat else c) * 0.5
    return (W_l, b_l, None, None, att, b) if share else (W_l, b_l, W_r, b_r, att, b)


_CASES = {
    "isolated_row": (5, [[0, 1, 2], [1, 2, 0]]),
    "stored_self_loop": (4, [[0, 1, 1, 2, 3], [1, 1, 2, 2, 0]]),
    "hub_row": (9, [[1, 2, 3, 4, 5, 6, 7, 8, 0], [0, 0, 0, 0, 0, 0, 0, 0, 1]]),
    "duplicate_edge": (4, [[0, 0, 0, 2, 3], [1, 1, 1, 1, 2]]),
}


@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("concat,share,relu", [(True, False, False), (False, False, True), (True, True, True), (False, True, False)])
def test_oracle_matches_dense_closed_form(name, concat, share, relu):
    n, ei = _CASES[name]
    x = torch.randn(n, 5, generator=torch.Generator().manual_seed(1), dtype=O.F64)
    p = _params(5, 3, 2, seed=2, concat=concat, share=share, scale=2.0)
    a = O.gatv2_conv(x, *p, np.array(ei), 3, concat, relu=relu)
    d = O.gatv2_conv_dense(x, *p, np.array(ei), 3, concat, relu=relu)
    assert a.shape == (n, 6 if concat else 2)
    assert torch.allclose(a, d, rtol=0, atol=1e-12), float((a - d).abs().max())


def test_duplicate_edges_weigh_by_multiplicity_and_an_isolated_row_is_its_own_transform():
    n, ei = _CASES["duplicate_edge"]
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(3), dtype=O.F64)
    p = _params(4, 2, 3, seed=4)
    once = O.gatv2_conv(x, *p, np.array([[0, 2, 3], [1, 1, 2]]), 2)
    thrice = O.gatv2_conv(x, *p, np.array(ei), 2)
    assert float((once[1] - thrice[1]).abs().max()) > 1e-3        # row 1 changes, the others do not
    assert torch.equal(once[[0, 2, 3]], thrice[[0, 2, 3]])
    n, ei = _CASES["isolated_row"]
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(5), dtype=O.F64)
    out = O.gatv2_conv(x, *p, np.array(ei), 2)
    assert torch.allclose(out[3:], x[3:] @ p[0].t() + p[1] + p[5], atol=1e-14)      # (softmax over the self-loop alone: x_l + b)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_analytic_gradients_match_autograd(concat, share, relu):
    n, H, C = 200, 3, 5
    ei = O.random_graph(n, seed=7, mean_deg=5, hub=11, hub_deg=150, n_dup=40, n_loops=20, n_isolated=9, directed_block=12)
    x = torch.randn(n, 12, generator=torch.Generator().manual_seed(8), dtype=O.F64)
    p = _params(12, H, C, seed=9, concat=concat, share=share)
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in (x,) + p]
    out = O.gatv2_conv(*leaves, ei, H, concat, 0.1, relu=relu)
    G = torch.randn(out.shape, generator=torch.Generator().manual_seed(10), dtype=O.F64)
    live = [t for t in leaves if t is not None]
    auto = dict(zip([k for k, t in zip(("dX", "dW_l", "db_l", "dW_r", "db_r", "datt", "db"), leaves) if t is not None],
                    torch.autograd.grad((out * G).sum(), live)))
    ana = O.gatv2_conv_grads(*[None if t is None else t.detach() for t in leaves], ei, G, H, concat, 0.1, relu=relu)
    assert (ana["dW_r"] is None) == share
    for k, ref in auto.items():
        assert ana[k].shape == ref.shape, k
        assert torch.allclose(ana[k], ref, rtol=0, atol=1e-11), (k, float((ana[k] - ref).abs().max()))


def test_layerwise_routing_and_widths():
    """GAT's routing (gcn.py:64-70): layer i of all but the last takes edge_index[-i] and concatenates, the last takes edge_index[0]
    and averages."""
    n, H = 40, 2
    e0, e1 = O.random_graph(n, seed=11, mean_deg=3), O.random_graph(n, seed=12, mean_deg=3)
    x = torch.randn(n, 6, generator=torch.Generator().manual_seed(13), dtype=O.F64)
    p1, p2 = _params(6, H, 4, seed=14), _params(8, H, 3, seed=15, concat=False)
    got = O.gatv2_forward(x, [p1, p2], [e0, e1], H)
    want = O.gatv2_conv(O.gatv2_conv(x, *p1, e1, H, True, relu=True), *p2, e0, H, False)
    assert got.shape == (n, 3) and torch.equal(got, want)


@pytest.mark.parametrize("n,fi,H,C,share", [(400, 24, 4, 16, True), (400, 20, 8, 32, False), (400, 12, 3, 7, False),
                                            (400, 16, 1, 5, False), (400, 32, 2, 128, False)])
def test_quantised_inputs_keep_every_edge_off_the_kink(n, fi, H, C, share):
    """The construction the GPU tests rely on: every z is an odd multiple of 1/128 and fp32 forms it exactly."""
    ei = O.random_graph(n, seed=3, mean_deg=6, hub=17, hub_deg=700, n_dup=30, n_loops=20, n_isolated=8)
    x, (W_l, b_l, W_r, b_r) = O.quantised_layer(n, fi, H, C, seed=5, share=share)
    src, dst = O.edge_set(ei, n)
    x_l32 = x @ W_l.t() + b_l
    x_r32 = x_l32 if share else x @ W_r.t() + b_r
    z32 = x_l32[src] + x_r32[dst]
    x_l64 = x.double() @ W_l.double().t() + b_l.double()
    x_r64 = x_l64 if share else x.double() @ W_r.double().t() + b_r.double()
    z64 = x_l64[src] + x_r64[dst]
    assert float(x.abs().max()) <= 3.0
    assert float(z64.abs().min()) == 1.0 / 128
    assert torch.equal(z32.double(), z64)
    assert torch.equal((z64 * 128).round() % 2, torch.ones_like(z64))


def test_gatv2_state_dict_keys_shapes_and_initialisation():
    from grapes_amd.modules.gcn import GATv2, GATv2Conv
    torch.manual_seed(0)
    conv = GATv2Conv(12, 8, heads=4)
    sd = conv.state_dict()
    assert sorted(sd) == sorted(["att", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "bias"])
    assert sd["att"].shape == (1, 4, 8) and sd["lin_l.weight"].shape == (32, 12) and sd["lin_r.weight"].shape == (32, 12)
    assert sd["lin_l.bias"].shape == (32,) and sd["lin_r.bias"].shape == (32,) and sd["bias"].shape == (32,)
    assert GATv2Conv(12, 8, heads=4, concat=False).state_dict()["bias"].shape == (8,)
    wb, ab = (6.0 / (12 + 32)) ** 0.5, (6.0 / (4 + 8)) ** 0.5                      # glorot: linear weights, att's last two dimensions
    for k in ("lin_l.weight", "lin_r.weight"):
        assert 0.8 * wb < float(sd[k].abs().max()) <= wb
    assert 0.6 * ab < float(sd["att"].abs().max()) <= ab
    assert not torch.equal(sd["lin_l.weight"], sd["lin_r.weight"])
    for k in ("lin_l.bias", "lin_r.bias", "bias"):
        assert float(sd[k].abs().max()) == 0.0
    assert "bias" not in GATv2Conv(4, 4, bias=False).state_dict()
    m = GATv2(12, [16, 7], heads=4)
    assert len(m.gat_layers) == 2 and all(isinstance(l, GATv2Conv) for l in m.gat_layers)
    first, last = m.gat_layers
    assert (first.heads, first.concat, first.out_channels) == (4, True, 16)
    assert (last.in_channels, last.heads, last.concat, last.out_channels) == (64, 4, False, 7)
    assert m.state_dict()["gat_layers.1.lin_l.weight"].shape == (28, 64) and m.state_dict()["gat_layers.1.bias"].shape == (7,)
    assert len(GATv2(5, [3]).gat_layers) == 1 and not hasattr(m, "dropout")


def test_share_weights_drops_the_lin_r_keys():
    from grapes_amd.modules.gcn import GATv2Conv
    conv = GATv2Conv(6, 4, heads=2, share_weights=True)
    assert conv.lin_r is conv.lin_l
    assert sorted(conv.state_dict()) == sorted(["att", "lin_l.weight", "lin_l.bias", "bias"])
    assert len(list(conv.parameters())) == 4
    other = GATv2Conv(6, 4, heads=2, share_weights=True)
    other.load_state_dict(conv.state_dict())                                      # (strict: no lin_r.* key is missed)
    assert torch.equal(other.lin_r.weight, conv.lin_l.weight)


def test_helpers_know_the_gatv2_classifier():
    from grapes_amd.modules.gcn import GATv2, classifier_layers, classifier_needs_loops
    m = GATv2(6, [4, 3], heads=2)
    assert classifier_layers(m) is m.gat_layers and classifier_needs_loops(m) is False


@pytest.mark.parametrize("kw,word", [(dict(dropout=0.1), "dropout"), (dict(edge_dim=4), "edge_dim"),
                                     (dict(add_self_loops=False), "add_self_loops"), (dict(fill_value=0.0), "fill_value"),
                                     (dict(fill_value="add"), "fill_value")])
def test_out_of_scope_gatv2conv_arguments_are_refused(kw, word):
    from grapes_amd.modules.gcn import GATv2Conv
    with pytest.raises(NotImplementedError, match=word):
        GATv2Conv(4, 4, **kw)


def test_shape_rules_raise_value_errors():
    from grapes_amd import ops
    from grapes_amd.modules.gcn import GATv2Conv
    for heads, c in ((1, 5), (3, 7), (16, 4), (8, 128), (1, 1024), (2, 128), (16, 16), (1, 256), (4, 64)):
        ops._gatv2_shape(heads, c)
    for heads, c, word in ((0, 8, "heads"), (17, 4, "heads"), (2, 516, "1024"), (3, 87, "256"), (1, 257, "256"), (8, 0, "256")):
        with pytest.raises(ValueError, match=word):
            ops._gatv2_shape(heads, c)
        with pytest.raises(ValueError, match=word):
            GATv2Conv(4, c, heads=heads)
    for slope in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="negative_slope"):
            GATv2Conv(4, 4, negative_slope=slope)
    assert GATv2Conv(4, 4, negative_slope=0.0).negative_slope == 0.0


def test_gatv2_has_no_cpu_path():
    from grapes_amd import ops
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules.gcn import GATv2
    m = GATv2(4, [8, 3], heads=2)
    with pytest.raises(GrapesHipError):
        m(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))
    with pytest.raises(GrapesHipError):
        m.gat_layers[0](torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))
    h = torch.randn(4, 8)
    with pytest.raises(GrapesHipError):
        ops.gatv2_aggregate_fwd(h, h, torch.randn(8), None, 2)
    with pytest.raises(GrapesHipError):
        ops.gatv2_aggregate_bwd(h, h, None, h, h, torch.randn(8), torch.randn(4, 2, 2), None, 2)


@pytest.mark.parametrize("mod", ["main", "full_batch"])
def test_classifier_gatv2_flags(mod):
    import importlib
    cli = importlib.import_module(f"grapes_amd.{mod}")
    args = cli.parse_args(["--classifier", "gatv2", "--gat_heads", "4"])
    assert args.classifier == "gatv2" and args.gat_heads == 4
    with pytest.raises(ValueError, match="dropout"):
        cli.parse_args(["--classifier", "gatv2", "--dropout", "0.5"])
    with pytest.raises(ValueError, match="heads"):
        cli.parse_args(["--classifier", "gatv2", "--gat_heads", "17"])


def test_gat_heads_is_absent_from_a_plain_full_batch_namespace():
    from grapes_amd import full_batch, main
    assert not hasattr(full_batch.parse_args([]), "gat_heads")
    assert not hasattr(full_batch.parse_args(["--classifier", "gatv2"]), "gat_heads")      # (build_gatv2's default: 1)
    assert main.parse_args([]).gat_heads == 1


def test_classifier_gatv2_refuses_the_captured_engine():
    from grapes_amd import main as cli
    with pytest.raises(ValueError, match="--classifier gatv2 runs on the eager engine: the captured step \\(--engine graph\\) is GCN only"):
        cli.parse_args(["--classifier", "gatv2", "--engine", "graph"])
    assert cli.parse_args(["--classifier", "gatv2", "--engine", "eager"]).engine == "eager"
    assert cli.parse_args(["--classifier", "gatv2"]).engine == "auto"     # resolved to eager in train()


def test_header_and_ctypes_table_declare_the_four_entry_points():
    import os
    from grapes_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grapes_hip.h")).read()
    for name in ("grapes_gatv2_aggregate_fwd", "grapes_gatv2_aggregate_workspace_bytes", "grapes_gatv2_aggregate_bwd",
                 "grapes_gatv2_aggregate_bwd_workspace_bytes"):
        assert name in _lib.SIGNATURES and f" {name}(" in header
