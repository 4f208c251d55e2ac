"""CPU checks of the GCN2 classifier (reference modules/gcn.py:76-117): the fp64 oracle of tests/gcn2_oracle.py against the dense
closed form and against torch.autograd, the two places where GCN2Conv(normalize=False) differs from the gcn_norm path (stored
self-loops count, duplicates weigh by multiplicity), the reachability of the GPU tests' tolerances in fp32, the module surface
and the drivers' --classifier gcn2 flags."""
import numpy as np
import pytest
import torch

from tests import gcn2_oracle as O

ACT_TOL, GRAD_TOL = 1e-5, 1e-4          # the GPU tests' tolerances (the project's)


def _weights(c, seed, shared):
    g = torch.Generator().manual_seed(seed)
    W1 = (torch.rand(c, c, generator=g, dtype=O.F64) - 0.5) * 2
    W2 = None if shared else (torch.rand(c, c, generator=g, dtype=O.F64) - 0.5) * 2
    return W1, W2


# the hand-sized cases of tests/test_gat_cpu.py
_CASES = {
    "isolated_row": (5, [[0, 1, 2], [1, 2, 0]]),                                  # nodes 3, 4 have no edge at all
    "pure_source": (4, [[0, 0, 0, 1], [1, 2, 3, 2]]),                             # node 0 only sends
    "stored_self_loop": (4, [[0, 1, 1, 2, 3], [1, 1, 2, 2, 0]]),                  # (1,1), (2,2) stored: they count
    "directed_block": (6, [[0, 1, 2, 0, 1, 2], [3, 4, 5, 4, 5, 3]]),              # one-way edges 0..2 -> 3..5
    "hub_row": (9, [[1, 2, 3, 4, 5, 6, 7, 8, 0], [0, 0, 0, 0, 0, 0, 0, 0, 1]]),   # node 0 receives from everyone
    "duplicate_edge": (4, [[0, 0, 0, 2, 3], [1, 1, 1, 1, 2]]),                    # 0 -> 1 three times: counted three times
}


@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("relu", [False, True])
def test_oracle_matches_dense_closed_form(name, shared, relu):
    n, ei = _CASES[name]
    g = torch.Generator().manual_seed(1)
    x, x0 = torch.randn(n, 5, generator=g, dtype=O.F64), torch.randn(n, 5, generator=g, dtype=O.F64)
    W1, W2 = _weights(5, 2, shared)
    a = O.gcn2_conv(x, x0, W1, W2, np.array(ei), 0.1, O.beta_of(0.5, 2), relu=relu)
    d = O.gcn2_conv_dense(x, x0, W1, W2, np.array(ei), 0.1, O.beta_of(0.5, 2), relu=relu)
    assert torch.allclose(a, d, rtol=0, atol=1e-12), float((a - d).abs().max())


def _conv(n, ei, c=4, seed=3, alpha=0.1, beta=0.4, shared=True):
    g = torch.Generator().manual_seed(seed)
    x, x0 = torch.randn(n, c, generator=g, dtype=O.F64), torch.randn(n, c, generator=g, dtype=O.F64)
    W1, W2 = _weights(c, seed + 1, shared)
    return x, x0, W1, W2, O.gcn2_conv(x, x0, W1, W2, np.array(ei), alpha, beta)


def test_a_stored_self_loop_changes_its_row():
    n, ei = _CASES["stored_self_loop"]
    without = [[s for s, d in zip(*ei) if s != d], [d for s, d in zip(*ei) if s != d]]
    x, x0, W1, _, with_loops = _conv(n, ei)
    no_loops = O.gcn2_conv(x, x0, W1, None, np.array(without), 0.1, 0.4)
    assert float((with_loops[1] - no_loops[1]).abs().max()) > 1e-3 and float((with_loops[2] - no_loops[2]).abs().max()) > 1e-3
    assert torch.equal(with_loops[[0, 3]], no_loops[[0, 3]])            # rows without a stored loop do not change
    S1 = 0.9 * (x[0] + x[1]) + 0.1 * x0[1]                               # row 1: the edge 0 -> 1 and its own stored loop
    assert torch.allclose(with_loops[1], 0.6 * S1 + 0.4 * (S1 @ W1), atol=1e-14)


def test_duplicate_edges_weigh_by_multiplicity():
    n, ei = _CASES["duplicate_edge"]
    x, x0, W1, _, thrice = _conv(n, ei)
    once = O.gcn2_conv(x, x0, W1, None, np.array([[0, 2, 3], [1, 1, 2]]), 0.1, 0.4)
    assert float((once[1] - thrice[1]).abs().max()) > 1e-3
    assert torch.equal(once[[0, 2, 3]], thrice[[0, 2, 3]])
    S1 = 0.9 * (3 * x[0] + x[2]) + 0.1 * x0[1]
    assert torch.allclose(thrice[1], 0.6 * S1 + 0.4 * (S1 @ W1), atol=1e-14)


def test_isolated_row_keeps_only_the_initial_residual():
    n, ei = _CASES["isolated_row"]
    x, x0, W1, _, out = _conv(n, ei, alpha=0.25, beta=0.3)
    assert torch.allclose(out[3:], 0.7 * 0.25 * x0[3:] + 0.3 * 0.25 * (x0[3:] @ W1), atol=1e-14)


def test_alpha_zero_ignores_x0_and_no_theta_gives_beta_one():
    n, ei = _CASES["hub_row"]
    x, x0, W1, _, out = _conv(n, ei, alpha=0.0)
    assert torch.equal(out, O.gcn2_conv(x, 7.0 * x0 + 1.0, W1, None, np.array(ei), 0.0, 0.4))
    assert O.beta_of(None, None) == 1.0 and O.beta_of(0.5, None) == 1.0 and O.beta_of(None, 3) == 1.0
    assert abs(O.beta_of(0.5, 2) - np.log(1.25)) < 1e-15
    S = 0.9 * O.propagate(x, np.array(ei)) + 0.1 * x0
    assert torch.allclose(O.gcn2_conv(x, x0, W1, None, np.array(ei), 0.1, 1.0), S @ W1, atol=1e-14)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("relu", [False, True])
def test_analytic_gradients_match_autograd(shared, relu):
    n, c = 300, 12
    ei = O.random_graph(n, seed=7, mean_deg=5, hub=11, hub_deg=150, n_dup=40, n_loops=20, n_isolated=9, directed_block=12)
    g = torch.Generator().manual_seed(8)
    x, x0 = torch.randn(n, c, generator=g, dtype=O.F64), torch.randn(n, c, generator=g, dtype=O.F64)
    W1, W2 = _weights(c, 9, shared)
    leaves = [t.clone().requires_grad_(True) for t in (x, x0, W1) + (() if shared else (W2,))]
    out = O.gcn2_conv(leaves[0], leaves[1], leaves[2], None if shared else leaves[3], ei, 0.1, O.beta_of(0.5, 2), relu=relu)
    G = torch.randn(out.shape, generator=g, dtype=O.F64)
    auto = torch.autograd.grad((out * G).sum(), leaves)
    ana = O.gcn2_conv_grads(x, x0, W1, W2, ei, 0.1, O.beta_of(0.5, 2), G, relu=relu)
    for name, ref in zip(("dx", "dx0", "dW1", "dW2"), auto):
        assert torch.allclose(ana[name], ref, rtol=0, atol=1e-11), (name, float((ana[name] - ref).abs().max()))


def test_layerwise_routing_matches_the_reference_order():
    """gcn.py:106-113: conv i of all but the last takes edge_index[-i], the last takes edge_index[0]; every conv sees x_0."""
    n, H = 40, 6
    e0, e1 = O.random_graph(n, seed=11, mean_deg=3, n_loops=4), O.random_graph(n, seed=12, mean_deg=3, n_loops=4)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(n, 5, generator=g, dtype=O.F64)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=O.F64) * 0.5
    params = dict(lin0=(rnd(H, 5), rnd(H)), lin1=(rnd(3, H), rnd(3)), convs=[(rnd(H, H), None), (rnd(H, H), None)],
                  betas=[O.beta_of(0.5, 1), O.beta_of(0.5, 2)], alpha=0.1)
    got = O.gcn2_forward(x, params, [e0, e1])
    x0 = torch.relu(x @ params["lin0"][0].t() + params["lin0"][1])
    h = O.gcn2_conv(x0, x0, params["convs"][0][0], None, e1, 0.1, params["betas"][0], relu=True)
    want = O.gcn2_conv(h, x0, params["convs"][1][0], None, e0, 0.1, params["betas"][1]) @ params["lin1"][0].t() + params["lin1"][1]
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", range(len(O.CONV_CASES)))
def test_gpu_conv_inputs_are_reachable_in_fp32(case):
    """The inputs of tests/test_gcn2_gpu.py's single-conv test: an fp32 torch-CPU evaluation of the same formulas (not the code
    under test) is inside the GPU tolerances against the fp64 oracle, at most 1 % of the pre-activations lie within 1e-5 of zero,
    and the generated graph has the hard cases."""
    c, shared, relu, alpha = O.CONV_CASES[case]
    ei, x, x0, W1, W2, G, beta = O.conv_case(c, shared, seed=case + 1)
    hub, dup, loops, isolated = O.graph_properties(ei)
    assert hub > 2000 and dup >= 60 and loops >= 40 and isolated >= 25
    d = lambda t: None if t is None else t.double()
    ref = O.gcn2_conv(d(x), d(x0), d(W1), d(W2), ei, alpha, beta, relu=relu, full=True)
    if relu:
        G, near = O.kink_free_gradient(G, ref["pre"])
        assert near <= 0.01 * ref["pre"].numel()
    gr = O.gcn2_conv_grads(d(x), d(x0), d(W1), d(W2), ei, alpha, beta, d(G), relu=relu)
    leaves = [t.clone().requires_grad_(True) for t in (x, x0, W1) + (() if shared else (W2,))]
    out = O.gcn2_conv(leaves[0], leaves[1], leaves[2], None if shared else leaves[3], ei, alpha, beta, relu=relu)
    assert out.dtype == torch.float32
    grads = torch.autograd.grad(out, leaves, G)
    assert O.rel_err(out.detach(), ref["out"]) <= ACT_TOL
    for name, got in zip(("dx", "dx0", "dW1", "dW2"), grads):
        assert O.rel_err(got, gr[name]) <= GRAD_TOL, name


def test_gpu_model_inputs_meet_the_kink_cap():
    """tests/test_gcn2_gpu.py's two-layer model test builds its model and inputs with these seeds: the oracle's hidden
    pre-activations (lins[0] and the first conv) have at most 1 % of their entries within 1e-5 of zero."""
    from grapes_amd.modules.gcn import GCN2
    torch.manual_seed(54)
    model = GCN2(48, [64, 7], alpha=0.1, theta=0.5)
    x = torch.randn(O.N, 48, generator=torch.Generator().manual_seed(53))
    _, pres = O.gcn2_forward(x.double(), O.model_params(model), [O.gpu_graph(51), O.gpu_graph(52)], full=True)
    for p in pres:
        assert int((p.abs() < O.KINK).sum()) <= 0.01 * p.numel()


def test_gcn2_state_dict_keys_shapes_and_betas():
    from grapes_amd.modules.gcn import GCN2, GCN2Conv, classifier_layers
    m = GCN2(12, [16, 7, 7], alpha=0.1, theta=0.5)
    assert len(m.conv) == 3 and all(isinstance(l, GCN2Conv) for l in m.conv) and classifier_layers(m) is m.conv
    sd = m.state_dict()
    assert sorted(sd) == sorted(["lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias"] + [f"conv.{i}.weight1" for i in range(3)])
    assert sd["lins.0.weight"].shape == (16, 12) and sd["lins.0.bias"].shape == (16,)
    assert sd["lins.1.weight"].shape == (7, 16) and sd["lins.1.bias"].shape == (7,)       # hidden_dims[0] -> hidden_dims[1]
    assert all(sd[f"conv.{i}.weight1"].shape == (16, 16) for i in range(3))                 # every conv at hidden_dims[0]
    for i, l in enumerate(m.conv):
        assert abs(l.beta - np.log(0.5 / (i + 1) + 1)) < 1e-12 and l.alpha == 0.1
    assert float(sd["conv.0.weight1"].abs().max()) <= (6.0 / 32) ** 0.5                     # glorot on [16, 16]
    u = GCN2(12, [16, 7], alpha=0.2, theta=1.0, shared_weights=False, dropout=0.5)
    assert sorted(k for k in u.state_dict() if k.startswith("conv")) == ["conv.0.weight1", "conv.0.weight2", "conv.1.weight1", "conv.1.weight2"]
    assert u.dropout == 0.5 and u.state_dict()["conv.1.weight2"].shape == (16, 16)
    assert GCN2Conv(8, 0.1).beta == 1.0 and GCN2Conv(8, 0.1).weight2 is None
    ref = O.model_params(m)
    assert len(ref["convs"]) == 3 and ref["convs"][0][1] is None


def test_refusals():
    from grapes_amd import ops
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules.gcn import GCN2, GCN2Conv
    for kw in (dict(normalize=True), dict(cached=True), dict(add_self_loops=False)):
        with pytest.raises(NotImplementedError):
            GCN2Conv(4, 0.1, 0.5, 1, **kw)
    m = GCN2(4, [8, 3], alpha=0.1, theta=0.5)
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(GrapesHipError):
        m(torch.randn(5, 4), ei)
    with pytest.raises(GrapesHipError):
        m.conv[0](torch.randn(5, 8), torch.randn(5, 8), ei)
    with pytest.raises(GrapesHipError):
        m.lins[0](torch.randn(5, 4))
    h = torch.randn(4, 8)
    with pytest.raises(GrapesHipError):
        ops.gcn2_propagate_fwd(h, h, None, 0.1)
    with pytest.raises(GrapesHipError):
        ops.gcn2_propagate_bwd(h, None, 0.1)
    with pytest.raises(GrapesHipError):
        ops.gcn2_mix_fwd(h, h, 0.5, 0.5)
    with pytest.raises(GrapesHipError):
        ops.gcn2_loop_counts(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 4)


def test_unequal_rows_are_refused(monkeypatch):
    """x and x_0 must have the same rows; the check comes before any launch (the device test is faked, no kernel runs)."""
    from grapes_amd.modules.gcn import GCN2Conv
    conv = GCN2Conv(8, 0.1, 0.5, 1)

    class _OnDevice(torch.Tensor):
        is_cuda = True
    x, x0 = torch.randn(5, 8).as_subclass(_OnDevice), torch.randn(6, 8).as_subclass(_OnDevice)
    with pytest.raises(ValueError, match="same rows"):
        conv(x, x0, torch.tensor([[0, 1], [1, 2]]))


@pytest.mark.parametrize("mod", ["main", "full_batch"])
def test_classifier_gcn2_flags(mod):
    import importlib
    cli = importlib.import_module(f"grapes_amd.{mod}")
    a = cli.parse_args(["--classifier", "gcn2", "--gcn2_alpha", "0.2", "--gcn2_theta", "1.0", "--gcn2_shared_weights", "false",
                        "--dropout", "0.5"])
    assert a.classifier == "gcn2" and a.gcn2_alpha == 0.2 and a.gcn2_theta == 1.0 and a.gcn2_shared_weights is False
    assert a.dropout == 0.5                                            # the model has a dropout (gcn.py:80)
    assert cli.parse_args(["--classifier", "gcn2"]).classifier == "gcn2"
    with pytest.raises((ValueError, SystemExit)):
        cli.parse_args(["--classifier", "sage"])


def test_gcn2_defaults_and_model_shape():
    from grapes_amd import full_batch, main as cli
    a = cli.parse_args(["--classifier", "gcn2"])
    assert (a.gcn2_alpha, a.gcn2_theta, a.gcn2_shared_weights) == (0.1, 0.5, True)
    with pytest.raises(ValueError, match="engine"):
        cli.parse_args(["--classifier", "gcn2", "--engine", "graph"])
    assert cli.parse_args(["--classifier", "gcn2", "--engine", "eager"]).engine == "eager"
    assert cli.parse_args(["--classifier", "gcn2"]).engine == "auto"        # resolved to eager in train()
    # full_batch: the new flags are absent unless given, and the plain flag set is what it was
    assert set(vars(full_batch.parse_args([]))) == set(vars(full_batch.parse_args(["--hidden_dim", "8"])))
    assert not any(k.startswith("gcn2_") or k == "classifier" for k in vars(full_batch.parse_args([])))
    fb = full_batch.parse_args(["--classifier", "gcn2", "--gcn2_alpha", "0.3"])
    assert fb.gcn2_alpha == 0.3 and not hasattr(fb, "gcn2_theta")
    a.hidden_dim, a.dropout = 16, 0.25
    m = cli.build_gcn2(a, 10, 5, 3)                                          # one conv per hop, lins[1]: hidden_dim -> C
    assert len(m.conv) == 3 and m.lins[1].weight.shape == (5, 16) and m.conv[2].weight1.shape == (16, 16) and m.dropout == 0.25
    fb.hidden_dim, fb.dropout = 16, 0.0
    m2 = cli.build_gcn2(fb, 10, 5, 2)
    assert len(m2.conv) == 2 and m2.conv[0].alpha == 0.3 and abs(m2.conv[1].beta - np.log(1.25)) < 1e-12
