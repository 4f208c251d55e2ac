"""CPU checks of the GAT classifier (reference modules/gcn.py:45-72): the fp64 oracle of tests/gat_oracle.py against the dense
closed form and against torch.autograd, the module's parameters, the no-CPU-path refusal and the drivers' --classifier flag."""
import numpy as np
import pytest
import torch

from tests import gat_oracle as O


def _params(fi, c, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(c, fi, generator=g, dtype=O.F64) - 0.5) * 2 * scale
    a_s = (torch.rand(c, generator=g, dtype=O.F64) - 0.5) * 2 * scale
    a_d = (torch.rand(c, generator=g, dtype=O.F64) - 0.5) * 2 * scale
    b = (torch.rand(c, generator=g, dtype=O.F64) - 0.5)
    return W, a_s, a_d, b


# SURVEY's five hand-sized cases + a duplicated edge
_CASES = {
    "isolated_row": (5, [[0, 1, 2], [1, 2, 0]]),                                  # nodes 3, 4 have no edge at all
    "pure_source": (4, [[0, 0, 0, 1], [1, 2, 3, 2]]),                             # node 0 only sends
    "stored_self_loop": (4, [[0, 1, 1, 2, 3], [1, 1, 2, 2, 0]]),                  # (1,1), (2,2) stored: dropped, unit loop added
    "directed_block": (6, [[0, 1, 2, 0, 1, 2], [3, 4, 5, 4, 5, 3]]),              # one-way edges 0..2 -> 3..5
    "hub_row": (9, [[1, 2, 3, 4, 5, 6, 7, 8, 0], [0, 0, 0, 0, 0, 0, 0, 0, 1]]),   # node 0 receives from everyone
    "duplicate_edge": (4, [[0, 0, 0, 2, 3], [1, 1, 1, 1, 2]]),                    # 0 -> 1 three times: counted three times
}


@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("relu", [False, True])
def test_oracle_matches_dense_closed_form(name, relu):
    n, ei = _CASES[name]
    x = torch.randn(n, 5, generator=torch.Generator().manual_seed(1), dtype=O.F64)
    p = _params(5, 3, seed=2, scale=2.0)
    a = O.gat_conv(x, *p, np.array(ei), relu=relu)
    d = O.gat_conv_dense(x, *p, np.array(ei), relu=relu)
    assert torch.allclose(a, d, rtol=0, atol=1e-12), float((a - d).abs().max())


def test_duplicate_edges_weigh_by_multiplicity():
    n, ei = _CASES["duplicate_edge"]
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(3), dtype=O.F64)
    p = _params(4, 2, seed=4)
    once = O.gat_conv(x, *p, np.array([[0, 2, 3], [1, 1, 2]]))
    thrice = O.gat_conv(x, *p, np.array(ei))
    assert float((once[1] - thrice[1]).abs().max()) > 1e-3        # row 1 changes, the others do not
    assert torch.equal(once[[0, 2, 3]], thrice[[0, 2, 3]])


def test_isolated_row_is_its_own_transform():
    n, ei = _CASES["isolated_row"]
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(5), dtype=O.F64)
    W, a_s, a_d, b = _params(4, 3, seed=6)
    out = O.gat_conv(x, W, a_s, a_d, b, np.array(ei))
    assert torch.allclose(out[3:], x[3:] @ W.t() + b, atol=1e-14)


@pytest.mark.parametrize("relu", [False, True])
def test_analytic_gradients_match_autograd(relu):
    n = 300
    ei = O.random_graph(n, seed=7, mean_deg=5, hub=11, hub_deg=150, n_dup=40, n_loops=20, n_isolated=9, directed_block=12)
    x = torch.randn(n, 12, generator=torch.Generator().manual_seed(8), dtype=O.F64)
    leaves = [t.clone().requires_grad_(True) for t in (x,) + _params(12, 7, seed=9)]
    out = O.gat_conv(*leaves, ei, relu=relu)
    G = torch.randn(out.shape, generator=torch.Generator().manual_seed(10), dtype=O.F64)
    auto = torch.autograd.grad((out * G).sum(), leaves)
    ana = O.gat_conv_grads(*[t.detach() for t in leaves], ei, G, relu=relu)
    for got, ref, name in zip((ana["dX"], ana["dW"], ana["da_src"], ana["da_dst"], ana["db"]), auto,
                              ("dX", "dW", "da_src", "da_dst", "db")):
        assert torch.allclose(got, ref, rtol=0, atol=1e-11), (name, float((got - ref).abs().max()))


def test_layerwise_routing_matches_the_reference_order():
    """gcn.py:64-70: layer i of all but the last takes edge_index[-i], the last takes edge_index[0]."""
    n = 40
    e0, e1 = O.random_graph(n, seed=11, mean_deg=3), O.random_graph(n, seed=12, mean_deg=3)
    x = torch.randn(n, 6, generator=torch.Generator().manual_seed(13), dtype=O.F64)
    p1, p2 = _params(6, 8, seed=14), _params(8, 3, seed=15)
    got = O.gat_forward(x, [p1, p2], [e0, e1])
    want = O.gat_conv(O.gat_conv(x, *p1, e1, relu=True), *p2, e0)
    assert torch.equal(got, want)


def test_gat_state_dict_keys_and_shapes():
    from grapes_amd.modules.gcn import GAT, GATConv
    m = GAT(12, [16, 7])
    assert len(m.gat_layers) == 2 and all(isinstance(l, GATConv) for l in m.gat_layers)
    sd = m.state_dict()
    assert sorted(sd) == sorted(f"gat_layers.{i}.{k}" for i in range(2) for k in ("lin.weight", "att_src", "att_dst", "bias"))
    assert sd["gat_layers.0.lin.weight"].shape == (16, 12) and sd["gat_layers.1.lin.weight"].shape == (7, 16)
    assert sd["gat_layers.0.att_src"].shape == (1, 1, 16) and sd["gat_layers.1.att_dst"].shape == (1, 1, 7)
    assert sd["gat_layers.1.bias"].shape == (7,) and float(sd["gat_layers.1.bias"].abs().max()) == 0.0
    bound = (6.0 / (1 + 16)) ** 0.5                                    # glorot on [1, 1, C]
    assert float(sd["gat_layers.0.att_src"].abs().max()) <= bound
    one = GAT(5, [3])                                                  # a single layer, as the reference's constructor allows
    assert len(one.gat_layers) == 1 and not hasattr(m, "dropout")


def test_gat_has_no_cpu_path():
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules.gcn import GAT
    m = GAT(4, [8, 3])
    with pytest.raises(GrapesHipError):
        m(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))
    with pytest.raises(GrapesHipError):
        m.gat_layers[0](torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))


def test_out_of_scope_gatconv_arguments_are_refused():
    from grapes_amd.modules.gcn import GATConv
    for kw in (dict(heads=2), dict(dropout=0.1), dict(edge_dim=4)):
        with pytest.raises(NotImplementedError):
            GATConv(4, 4, **kw)


def test_ops_wrappers_refuse_cpu_tensors():
    from grapes_amd import ops
    from grapes_amd._lib import GrapesHipError
    h = torch.randn(4, 8)
    with pytest.raises(GrapesHipError):
        ops.gat_scores(h, torch.randn(8), torch.randn(8))
    with pytest.raises(GrapesHipError):
        ops.gat_aggregate_fwd(h, torch.randn(4), torch.randn(4), None)
    with pytest.raises(GrapesHipError):
        ops.gat_aggregate_bwd(h, h, h, torch.randn(4), torch.randn(4), torch.randn(4, 2), torch.randn(8), torch.randn(8), None)


@pytest.mark.parametrize("mod", ["main", "full_batch"])
def test_classifier_flag(mod):
    import importlib
    cli = importlib.import_module(f"grapes_amd.{mod}")
    assert getattr(cli.parse_args([]), "classifier", "gcn") == "gcn"
    assert cli.parse_args(["--classifier", "gat"]).classifier == "gat"
    with pytest.raises(ValueError, match="dropout"):
        cli.parse_args(["--classifier", "gat", "--dropout", "0.5"])
    with pytest.raises((ValueError, SystemExit)):
        cli.parse_args(["--classifier", "sage"])
    with pytest.raises(NotImplementedError):                           # the reference's flag keeps its refusal
        cli.parse_args(["--model_type", "gat"])


def test_classifier_gat_refuses_the_captured_engine():
    from grapes_amd import main as cli
    with pytest.raises(ValueError, match="engine"):
        cli.parse_args(["--classifier", "gat", "--engine", "graph"])
    assert cli.parse_args(["--classifier", "gat", "--engine", "eager"]).engine == "eager"
    assert cli.parse_args(["--classifier", "gat"]).engine == "auto"     # resolved to eager in train()
