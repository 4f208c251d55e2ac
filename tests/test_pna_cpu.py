"""CPU checks of the PNA classifier (reference modules/gcn.py:120-149): the fp64 oracle of tests/pna_oracle.py against a dense
closed form and against torch.autograd, the a_i + b_j decomposition the kernels rest on, the empty-row values, duplicates by
multiplicity, the degree averages, the reachability of the GPU tests' tolerances in fp32 (and what an uncentred variance does to
them), the kink caps on the GPU tests' inputs, the module surface and the drivers' --classifier pna flags."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import pna_oracle as O

ACT_TOL, GRAD_TOL = 1e-5, 1e-4          # the GPU tests' tolerances (the project's)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGG, SCAL = O.AGGREGATORS, O.SCALERS
ALL_AGG = ["mean", "min", "max", "std", "var", "sum"]
ALL_SCAL = ["identity", "amplification", "attenuation", "linear", "inverse_linear"]

# the hand-sized cases of tests/test_gat_cpu.py
_CASES = {
    "isolated_row": (5, [[0, 1, 2], [1, 2, 0]]),                                  # nodes 3, 4 have no edge at all
    "pure_source": (4, [[0, 0, 0, 1], [1, 2, 3, 2]]),                             # node 0 only sends
    "stored_self_loop": (4, [[0, 1, 1, 2, 3], [1, 1, 2, 2, 0]]),                  # (1,1), (2,2) stored: they count
    "directed_block": (6, [[0, 1, 2, 0, 1, 2], [3, 4, 5, 4, 5, 3]]),              # one-way edges 0..2 -> 3..5
    "hub_row": (9, [[1, 2, 3, 4, 5, 6, 7, 8, 0], [0, 0, 0, 0, 0, 0, 0, 0, 1]]),   # node 0 receives from everyone
    "duplicate_edge": (4, [[0, 0, 0, 2, 3], [1, 1, 1, 1, 2]]),                    # 0 -> 1 three times: counted three times
}


def _params(F, C, n_blocks, seed, dtype=O.F64):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(*s, generator=g, dtype=dtype) - 0.5) * 2
    return mk(F, 2 * F), mk(F), mk(C, n_blocks * F), mk(C), mk(C, C), mk(C)


def _hand(name, aggregators=ALL_AGG, scalers=ALL_SCAL, F=3, C=4):
    n, ei = _CASES[name]
    ei = np.array(ei)
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(1), dtype=O.F64)
    P = _params(F, C, 1 + len(aggregators) * len(scalers), 2)
    avg_log, avg_lin = O.degree_averages(O.degree_histogram(ei, n))
    return n, ei, x, P, avg_log, avg_lin


@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("relu", [False, True])
def test_oracle_matches_dense_closed_form(name, relu):
    n, ei, x, P, avg_log, avg_lin = _hand(name)
    a = O.pna_conv(x, P, ei, ALL_AGG, ALL_SCAL, avg_log, avg_lin, relu=relu)
    d = O.pna_conv_dense(x, P, ei, ALL_AGG, ALL_SCAL, avg_log, avg_lin, relu=relu)
    assert torch.allclose(a, d, rtol=0, atol=1e-12), float((a - d).abs().max())


@pytest.mark.parametrize("name", sorted(_CASES))
def test_decomposition_matches_the_literal_form(name):
    """pre_nn([x_i | x_j]) = a_i + b_j: the kernels' form (centred variance) against the literal per-edge form, at 1e-12."""
    n, ei, x, P, avg_log, avg_lin = _hand(name)
    r = O.pna_conv(x, P, ei, ALL_AGG, ALL_SCAL, avg_log, avg_lin, full=True)
    z, _ = O.pna_conv_decomposed(x, P, ei, ALL_AGG, ALL_SCAL, avg_log, avg_lin)
    assert float((z - r["z"]).abs().max()) <= 1e-12


def test_decomposition_matches_the_literal_form_on_a_gpu_test_input():
    ei, x, P, G, avg_log, avg_lin = O.conv_case(7, 16, seed=1)
    Pd = tuple(t.double() for t in P)
    r = O.pna_conv(x.double(), Pd, ei, AGG, SCAL, avg_log, avg_lin, full=True)
    z, _ = O.pna_conv_decomposed(x.double(), Pd, ei, AGG, SCAL, avg_log, avg_lin)
    assert float((z - r["z"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("relu", [False, True])
def test_analytic_gradients_match_autograd(name, relu):
    n, ei, x, P, avg_log, avg_lin = _hand(name)
    leaves = [t.clone().requires_grad_(True) for t in (x,) + P]
    out = O.pna_conv(leaves[0], tuple(leaves[1:]), ei, ALL_AGG, ALL_SCAL, avg_log, avg_lin, relu=relu)
    G = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=O.F64)
    want = torch.autograd.grad(out, leaves, G)
    got = O.pna_conv_grads(x, P, ei, ALL_AGG, ALL_SCAL, avg_log, avg_lin, G, relu=relu)
    for k, w in zip(O.GRAD_NAMES, want):
        assert float((got[k] - w).abs().max()) <= 1e-11, k


def test_analytic_gradients_match_autograd_on_a_gpu_test_input():
    ei, x, P, G, avg_log, avg_lin = O.conv_case(7, 16, seed=1)
    leaves = [t.double().requires_grad_(True) for t in (x,) + P]
    r = O.pna_conv(leaves[0], tuple(leaves[1:]), ei, AGG, SCAL, avg_log, avg_lin, relu=True, full=True)
    G, _, _, _ = O.kink_free_gradient(G.double(), r, O.N, True)
    want = torch.autograd.grad(r["out"], leaves, G)
    got = O.pna_conv_grads(x.double(), tuple(t.double() for t in P), ei, AGG, SCAL, avg_log, avg_lin, G, relu=True)
    for k, w in zip(O.GRAD_NAMES, want):
        assert O.rel_err(got[k], w) <= 1e-11, k


def test_empty_row_values():
    """A row without an incoming message: mean, min, max 0 and std sqrt(1e-5), times its scalers (d = 0: amplification 0)."""
    n, ei, x, P, avg_log, avg_lin = _hand("isolated_row", AGG, SCAL)
    r = O.pna_conv(x, P, ei, AGG, SCAL, avg_log, avg_lin, full=True)
    F = x.shape[1]
    for row in (3, 4):
        blocks = r["z"][row, F:].reshape(len(SCAL), len(AGG), F)
        assert bool((blocks[:, :3] == 0).all())
        assert torch.allclose(blocks[0, 3], torch.full((F,), math.sqrt(1e-5), dtype=O.F64), atol=1e-15)      # identity
        assert bool((blocks[1, 3] == 0).all())                                                                # log(0 + 1) = 0
        assert torch.allclose(blocks[2, 3], torch.full((F,), math.sqrt(1e-5) * avg_log / math.log(2), dtype=O.F64), atol=1e-15)
        assert bool((r["z"][row, :F] == x[row]).all())


def test_duplicates_count_by_multiplicity_and_loops_count():
    n, ei, x, P, avg_log, avg_lin = _hand("duplicate_edge", ["mean", "sum", "var"], ["identity"])
    r = O.pna_conv(x, P, ei, ["mean", "sum", "var"], ["identity"], avg_log, avg_lin, full=True)
    F = x.shape[1]
    a, b = x @ P[0][:, :F].t() + P[1], x @ P[0][:, F:].t()
    m = torch.stack([a[1] + b[0]] * 3 + [a[1] + b[2]])                    # row 1: 0 -> 1 three times and 2 -> 1
    assert float(r["d"][1]) == 4
    assert torch.allclose(r["agg"]["mean"][1], m.mean(0), atol=1e-14) and torch.allclose(r["agg"]["sum"][1], m.sum(0), atol=1e-14)
    assert torch.allclose(r["agg"]["var"][1], m.var(0, unbiased=False), atol=1e-14)
    once = np.array([[0, 2, 3], [1, 1, 2]])
    r1 = O.pna_conv(x, P, once, ["mean", "sum", "var"], ["identity"], avg_log, avg_lin, full=True)
    assert float((r1["agg"]["mean"][1] - r["agg"]["mean"][1]).abs().max()) > 1e-3
    n, ei, x, P, avg_log, avg_lin = _hand("stored_self_loop", ["sum"], ["identity"])
    r = O.pna_conv(x, P, ei, ["sum"], ["identity"], avg_log, avg_lin, full=True)
    a, b = x @ P[0][:, :F].t() + P[1], x @ P[0][:, F:].t()
    assert float(r["d"][1]) == 2 and torch.allclose(r["agg"]["sum"][1], 2 * a[1] + b[0] + b[1], atol=1e-14)   # 0 -> 1 and (1, 1)


def test_degree_averages_from_a_histogram():
    from grapes_amd.modules.gcn import pna_degree_averages, pna_degree_histogram
    deg = torch.tensor([2, 0, 3, 1])                                      # two nodes of in-degree 0, three of 2, one of 3
    avg_log, avg_lin = pna_degree_averages(deg)
    assert abs(avg_log - (3 * math.log(3) + math.log(4)) / 6) < 1e-15 and abs(avg_lin - 9 / 6) < 1e-15
    assert O.degree_averages(deg) == pytest.approx((avg_log, avg_lin), abs=1e-15)
    ei = torch.tensor([[0, 1, 2, 2, 3], [1, 1, 1, 0, 0]])
    assert pna_degree_histogram(ei, 5).tolist() == [3, 0, 1, 1]           # nodes 2, 3, 4: 0; node 0: 2; node 1: 3
    assert O.degree_histogram(ei.numpy(), 5).tolist() == [3, 0, 1, 1]
    with pytest.raises(ValueError):
        pna_degree_averages(torch.zeros(3))


# (F, C, offset added to the N(0, 1) features, the uncentred form's error on the in-degree-1 rows must exceed this)
_FP32_CASES = [(7, 16, 0.0, ACT_TOL), (100, 47, 0.0, 0.5 * ACT_TOL), (100, 47, 1.0, ACT_TOL)]


@pytest.mark.parametrize("F,C,shift,hazard", _FP32_CASES)
def test_fp32_evaluation_reaches_the_gpu_tolerances_and_the_uncentred_variance_does_not(F, C, shift, hazard):
    """The kernels' formulas evaluated in fp32 on a GPU test's inputs: with the CENTRED variance post_nn's operand is inside the
    activation tolerance — on the whole, and on the std entries of the in-degree-1 rows, where the true variance is 0 and std =
    sqrt(1e-5) magnifies an absolute error of the variance 160 times (measured 3e-11 there: the centred variance of one message
    is exactly 0).  The same evaluation from raw moments, E[b²] − E[b]², loses those rows once the subtraction is contracted into a
    fused multiply-add (the compiler's default on the GPU: the product is then exact and the rounding of E[b²] survives).  Measured
    on the in-degree-1 rows: 1.4e-5 at F = 7 and 8.6e-6 at F = 100 on the N(0, 1) test inputs — at the tolerance, five orders
    above the centred form — and 3.5e-5 at F = 100 once the features carry an offset of 1 (the error grows with b², as behind a
    ReLU).  Without the contraction a single message cancels exactly on a CPU (3e-11 again) and the damage moves to rows of
    near-equal neighbours (the whole operand: 1.7e-6 against 3.1e-7).  Measured here, not assumed."""
    ei, x, P, G, avg_log, avg_lin = O.conv_case(F, C, seed=1)
    x = x + shift
    Pd = tuple(t.double() for t in P)
    ref = O.pna_conv(x.double(), Pd, ei, AGG, SCAL, avg_log, avg_lin, full=True)
    d = ref["d"]
    one = d == 1
    assert int(one.sum()) >= 10
    std_cols = slice(F + 3 * F, F + 4 * F)                               # identity block, the std aggregate
    res = {}
    for name, kw in (("centred", dict(centred=True)), ("raw", dict(centred=False)), ("raw+fma", dict(centred=False, fma=True))):
        z, _ = O.pna_conv_decomposed(x, P, ei, AGG, SCAL, avg_log, avg_lin, **kw)
        res[name] = (O.rel_err(z, ref["z"]), O.rel_err(z[one][:, std_cols], ref["z"][one][:, std_cols]))
        print(f"F {F} offset {shift} {name}: z rel err {res[name][0]:.2e}, std on the {int(one.sum())} in-degree-1 rows {res[name][1]:.2e}")
    assert res["centred"][0] <= ACT_TOL and res["centred"][1] <= 1e-7     # one message: the centred variance is exactly 0
    assert res["raw+fma"][1] > hazard and res["raw+fma"][1] > 1e4 * res["centred"][1]        # the hazard
    out32 = (O.pna_conv_decomposed(x, P, ei, AGG, SCAL, avg_log, avg_lin)[0] @ P[2].t() + P[3]) @ P[4].t() + P[5]
    assert O.rel_err(out32, ref["out"]) <= ACT_TOL


@pytest.mark.parametrize("case", range(len(O.CONV_CASES)))
def test_kink_caps_hold_on_the_gpu_test_inputs(case):
    """The oracle alone meets the 1 % caps on the single-conv inputs of tests/test_pna_gpu.py, and the graph has the hard cases."""
    F, C, relu = O.CONV_CASES[case]
    if F > 700:
        F, C = 64, C                                                     # (the widest case's oracle is left to the GPU test itself)
    ei, x, P, G, avg_log, avg_lin = O.conv_case(F, C, seed=case + 1)
    hub, dup, loops, isolated = O.graph_properties(ei)
    assert hub > 2000 and dup >= 60 and loops >= 40 and isolated >= 25
    r = O.pna_conv(x.double(), tuple(t.double() for t in P), ei, AGG, SCAL, avg_log, avg_lin, relu=relu, full=True)
    G2, near, bad, rows = O.kink_free_gradient(G.double(), r, O.N, relu)
    print(f"F {F}: ReLU kinks {near} of {r['pre'].numel()}, aggregate kinks {bad} of {O.N * F} in {rows} rows")
    assert near <= 0.01 * r["pre"].numel() and bad <= 0.01 * O.N * F
    assert bad <= 0.002 * O.N * F                                        # far inside the cap
    assert rows < 0.5 * O.N and bool((G2[r["d"] == 1] != 0).any())      # the in-degree-1 rows keep their gradient


def test_module_parameter_names_and_shapes():
    from grapes_amd.modules.gcn import PNA, PNAConv, classifier_layers, classifier_needs_loops
    deg = torch.tensor([1, 5, 9, 3])
    m = PNA(10, [16, 7], AGG, SCAL, deg, dropout=0.2)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {}
    for i, (fi, fo) in enumerate([(10, 16), (16, 7)]):
        want.update({f"conv.{i}.pre_nn.weight": (fi, 2 * fi), f"conv.{i}.pre_nn.bias": (fi,), f"conv.{i}.post_nn.weight": (fo, 13 * fi),
                     f"conv.{i}.post_nn.bias": (fo,), f"conv.{i}.lin.weight": (fo, fo), f"conv.{i}.lin.bias": (fo,)})
    want.update({"lins.weight": (7, 10), "lins.bias": (7,)})             # gcn.py:134
    assert shapes == want
    assert isinstance(m.conv[0], PNAConv) and classifier_layers(m) is m.conv and classifier_needs_loops(m)
    assert m.dropout == 0.2 and m.drop_input is True
    c = PNAConv(6, 4, ["mean", "sum"], ["identity", "linear"], deg)
    assert tuple(c.post_nn.weight.shape) == (4, 5 * 6)
    assert abs(c.avg_deg["log"] - O.degree_averages(deg)[0]) < 1e-15 and abs(c.avg_deg["lin"] - O.degree_averages(deg)[1]) < 1e-15
    bound = 1 / math.sqrt(12)                                            # Linear's reset: U(±1/sqrt(in))
    assert float(c.pre_nn.weight.detach().abs().max()) <= bound and float(c.pre_nn.bias.detach().abs().max()) <= bound


def test_refusals():
    from grapes_amd.modules.gcn import PNA, PNAConv
    deg = torch.tensor([1, 5, 9, 3])
    for kw in (dict(towers=2), dict(pre_layers=2), dict(post_layers=2), dict(divide_input=True), dict(edge_dim=4), dict(train_norm=True)):
        with pytest.raises(NotImplementedError):
            PNAConv(8, 8, AGG, SCAL, deg, **kw)
    with pytest.raises(NotImplementedError, match="median"):
        PNAConv(8, 8, ["mean", "median"], SCAL, deg)
    with pytest.raises(NotImplementedError, match="exponential"):
        PNAConv(8, 8, AGG, ["exponential"], deg)
    with pytest.raises(NotImplementedError, match="batch_norm"):
        PNA(8, [8, 3], AGG, SCAL, deg, batch_norm=True)
    with pytest.raises(NotImplementedError, match="residual"):
        PNA(8, [8, 3], AGG, SCAL, deg, residual=True)


def test_there_is_no_cpu_path():
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules.gcn import PNA, PNAConv
    deg = torch.tensor([1, 5, 9, 3])
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(GrapesHipError, match="no CPU path"):
        PNAConv(4, 3, AGG, SCAL, deg)(torch.randn(2, 4), ei)
    with pytest.raises(GrapesHipError, match="no CPU path"):
        PNA(4, [4, 3], AGG, SCAL, deg)(torch.randn(2, 4), ei)


def test_cli_flags_of_both_drivers():
    from grapes_amd import full_batch, main
    a = main.parse_args(["--classifier", "pna"])
    assert a.pna_aggregators == "mean,min,max,std" and a.pna_scalers == "identity,amplification,attenuation" and a.engine == "auto"
    a = main.parse_args(["--classifier", "pna", "--pna_aggregators", "mean,sum", "--pna_scalers", "identity", "--dropout", "0.3"])
    assert main._name_list(a.pna_aggregators) == ["mean", "sum"] and a.dropout == 0.3
    with pytest.raises(ValueError, match="captured step"):
        main.parse_args(["--classifier", "pna", "--engine", "graph"])
    with pytest.raises(NotImplementedError, match="median"):
        main.parse_args(["--classifier", "pna", "--pna_aggregators", "median"])
    with pytest.raises(ValueError):
        main.parse_args(["--classifier", "sage"])
    with pytest.raises(NotImplementedError):
        main.parse_args(["--model_type", "gat"])
    f = full_batch.parse_args(["--classifier", "pna", "--pna_scalers", "identity,linear", "--dropout", "0.1"])
    assert f.classifier == "pna" and f.pna_scalers == "identity,linear" and not hasattr(f, "pna_aggregators")
    assert not hasattr(full_batch.parse_args([]), "pna_scalers")           # a plain run's arguments stay the reference's
    with pytest.raises(NotImplementedError, match="exponential"):
        full_batch.parse_args(["--classifier", "pna", "--pna_scalers", "exponential"])
    from types import SimpleNamespace
    args = SimpleNamespace(hidden_dim=16, dropout=0.25, pna_aggregators="mean,max", pna_scalers="identity,attenuation")
    g = SimpleNamespace(rowptr=torch.tensor([0, 1, 2, 3]), col=torch.tensor([1, 2, 1]), num_nodes=3)
    m = main.build_pna(args, 6, 4, 3, g)
    assert [c.in_channels for c in m.conv] == [6, 16, 16] and m.conv[-1].out_channels == 4 and m.dropout == 0.25
    assert m.conv[0].aggregators == ["mean", "max"] and tuple(m.conv[0].post_nn.weight.shape) == (16, 5 * 6)


def test_header_and_signatures_have_the_entry_points():
    from grapes_amd import _lib
    names = ["grapes_pna_aggregate_fwd", "grapes_pna_aggregate_fwd_workspace_bytes", "grapes_pna_aggregate_bwd",
             "grapes_pna_aggregate_bwd_workspace_bytes", "grapes_pna_add_input_grad"]
    with open(os.path.join(ROOT, "include", "grapes_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)             # (prototypes only: the comments name the functions too)
    for name in names:
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\s*\(", header), name
    with open(os.path.join(ROOT, "include", "grapes_hip.h")) as f:
        assert "modules/gcn.py:120-149" in f.read()
    nargs = lambda name: len(re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).split(","))
    for name in names:
        assert nargs(name) == len(_lib.SIGNATURES[name][1]), name
    with open(os.path.join(ROOT, "grapes_amd", "csrc", "Makefile")) as f:
        assert "build/pna_kernels.o" in f.read()


def test_torch_geometric_cross_check():
    """Where torch_geometric is installed: the oracle against PyG's own PNAConv."""
    pyg = pytest.importorskip("torch_geometric")
    from torch_geometric.nn import PNAConv
    n, ei, x, P, avg_log, avg_lin = _hand("hub_row", AGG, SCAL, F=4, C=5)
    deg = O.degree_histogram(ei, n)
    conv = PNAConv(4, 5, AGG, SCAL, deg, towers=1, pre_layers=1, post_layers=1, divide_input=False).double()
    sd = conv.state_dict()
    keys = [k for k in sd if k.endswith("weight") or k.endswith("bias")]
    P = tuple(sd[k] for k in sorted(keys, key=lambda k: (("pre" not in k) + ("lin." in k), "bias" in k)))
    ours = O.pna_conv(x, P, ei, AGG, SCAL, avg_log, avg_lin)
    assert torch.allclose(conv(x, torch.as_tensor(ei)), ours, atol=1e-10), pyg.__version__
