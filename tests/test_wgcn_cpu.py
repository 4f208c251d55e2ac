"""CPU checks of GCNConv with edge weights: the module signatures, the host oracle of tests/wgcn_oracle.py against the dense formula
and its closed-form edge-weight gradient against autograd on a hand graph, the C-ABI tables for the new entry points, and the
refusals of the module API that need no GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import wgcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grapes_wgcn_structure", "grapes_wgcn_weights", "grapes_wgcn_aggregate_fwd", "grapes_wgcn_aggregate_bwd")
NEW_SIZES = ("grapes_wgcn_structure_workspace_bytes", "grapes_wgcn_aggregate_workspace_bytes",
             "grapes_wgcn_aggregate_bwd_workspace_bytes")


def test_forward_signatures_carry_edge_weight():
    from grapes_amd.modules.gcn import GCN, GCNConv
    p = inspect.signature(GCNConv.forward).parameters
    assert list(p) == ["self", "x", "edge_index", "relu", "large_graph", "edge_weight"]
    assert p["edge_weight"].default is None and p["relu"].default is False and p["large_graph"].default is None
    p = inspect.signature(GCN.forward).parameters
    assert list(p) == ["self", "x", "edge_index", "large_graph", "edge_weight"]
    assert p["edge_weight"].default is None and p["large_graph"].default is None


def _hand_layer(seed=0, fi=5, fo=3):
    rng = np.random.default_rng(seed)
    src, dst, w, n = O.hand_graph()
    x = rng.standard_normal((n, fi)).astype(np.float32)
    W = rng.standard_normal((fo, fi)).astype(np.float32)
    b = rng.standard_normal(fo).astype(np.float32)
    dout = rng.standard_normal((n, fo)).astype(np.float32)
    return src, dst, w, n, x, W, b, dout


def test_hand_graph_holds_every_case():
    src, dst, w, n = O.hand_graph()
    P = O.Problem(src, dst, w, n)
    assert P.lens_t[5] == 0 and P.lens_s[5] == 0 and P.loop_src[5] == -1                 # isolated
    assert P.lens_t[0] == 0 and P.lens_s[0] > 0                                         # a pure source
    assert P.lw.tolist() == [1.0, 2.5, 1.5, 1.0, 1.0, 1.0]                              # a stored loop; two loops, the last wins
    assert P.loop_src.tolist() == [-1, 1, 5, -1, -1, -1]
    pairs = list(zip(src.tolist(), dst.tolist()))
    assert (3, 4) in pairs and (4, 3) in pairs and pairs.count((0, 1)) == 2 and w[pairs.index((0, 3))] == 0.0
    # deg = lw + incoming weights; the isolated node's is its unit loop
    assert np.allclose(P.deg, [1.0, 2.5 + 0.5 + 1.25, 1.5 + 1.0 + 3.0, 1.0 + 0.25 + 0.0, 1.0 + 2.0, 1.0])
    # duplicates sit in input order in both row orders
    assert P.order_t.tolist().index(0) + 1 == P.order_t.tolist().index(2)
    assert P.order_s.tolist().index(0) + 1 == P.order_s.tolist().index(2)


def test_oracle_agrees_with_the_dense_formula():
    src, dst, w, n, x, W, b, _ = _hand_layer()
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    got = O.forward64(t(x), t(W), t(b), src, dst, t(w), n).numpy()
    want = O.dense_forward(x, W, b, src, dst, w, n)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13)
    P = O.Problem(src, dst, w, n)
    ref, mag, base = P.layer(x, W, b, False, np.zeros((n, W.shape[0]), np.float32))["out"]
    assert np.allclose(ref.numpy(), want, rtol=1e-13, atol=1e-13)
    assert np.all(np.abs(base.numpy() - want) <= 2.0 ** -20 * mag.numpy())
    # an out-of-range entry is dropped
    src2, dst2, w2 = np.append(src, [9, 2]), np.append(dst, [1, -1]), np.append(w, [7.0, 7.0]).astype(np.float32)
    assert np.allclose(O.forward64(t(x), t(W), t(b), src2, dst2, t(w2), n).numpy(), want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("relu", [False, True])
def test_closed_form_weight_gradient_agrees_with_autograd(relu):
    src, dst, w, n, x, W, b, dout = _hand_layer(seed=1)
    r = O.Problem(src, dst, w, n).layer(x, W, b, relu, dout)
    auto, closed = r["dw"][0].numpy(), r["dw_closed"].numpy()
    assert np.allclose(auto, closed, rtol=1e-12, atol=1e-13)
    assert closed[3] == 0.0 and auto[3] == 0.0                      # the overridden loop of node 2
    assert closed[5] != 0.0 and closed[1] != 0.0                    # the loops that set lw
    assert closed[7] != 0.0                                         # a zero weight still has a gradient
    assert np.all(np.abs(r["dw"][2].numpy() - closed) <= 2.0 ** -18 * r["dw"][1].numpy())
    # dh of the aggregation against autograd's dx: dx = dh W
    assert np.allclose(r["dh"][0].numpy() @ W.astype(np.float64), r["dx"][0].numpy(), rtol=1e-12, atol=1e-13)


def test_zero_degree_node_has_finite_zero_gradients():
    """A node whose only entry is a stored loop of weight 0: deg = 0, dinv = 0, and the loop's gradient is exactly 0."""
    src, dst = np.array([0, 1, 2]), np.array([1, 0, 2])
    w = np.array([1.0, 0.5, 0.0], np.float32)
    rng = np.random.default_rng(2)
    x, W, b = rng.standard_normal((3, 4)).astype(np.float32), rng.standard_normal((2, 4)).astype(np.float32), np.ones(2, np.float32)
    P = O.Problem(src, dst, w, 3)
    assert P.dinv[2] == 0.0 and P.dinv32[2] == 0.0
    r = P.layer(x, W, b, False, np.ones((3, 2), np.float32))
    assert np.array_equal(r["out"][0].numpy()[2], [1.0, 1.0])
    assert r["dw"][0][2] == 0.0 and r["dw_closed"][2] == 0.0 and bool(torch.isfinite(r["dw"][0]).all())


def test_new_symbols_are_exported_and_bound():
    from grapes_amd import _lib
    src = open(os.path.join(ROOT, "include", "grapes_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW + NEW_SIZES:
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    lib = _lib.load()                       # the built library: binds every name of SIGNATURES, raises on a missing symbol
    for name in NEW + NEW_SIZES:
        assert getattr(lib, name) is not None
    assert lib.grapes_wgcn_aggregate_workspace_bytes(3, 8) >= 3 * 8 * 4
    assert lib.grapes_wgcn_aggregate_bwd_workspace_bytes(10, 20, 0, 8) >= (10 * 8 + 20 + 3 * 10) * 4
    from grapes_amd import ops
    for name in ("WeightedStructure", "wgcn_weights", "wgcn_aggregate_fwd", "wgcn_aggregate_bwd"):
        assert hasattr(ops, name)
    mk = open(os.path.join(ROOT, "grapes_amd", "csrc", "Makefile")).read()
    assert "build/wgcn_kernels.o" in mk


def test_value_errors_that_need_no_gpu():
    from grapes_amd import ops
    from grapes_amd.modules.gcn import GCN, GCNConv
    layer = GCNConv(4, 3)
    x = torch.zeros(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    ok = torch.ones(3)
    for bad in (torch.ones(4), torch.ones(3, dtype=torch.float64), torch.ones(3, 1), torch.ones(3, device="meta"), [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError):
            layer(x, ei, edge_weight=bad)
    with pytest.raises(ValueError):
        layer(x, ei, large_graph=True, edge_weight=ok)
    prep = object.__new__(ops.PreparedGraph)                        # (a shell: the refusal comes before anything is read)
    with pytest.raises(ValueError):
        layer(x, prep, edge_weight=ok)
    # a well-formed call gets past the checks and stops at the missing device
    with pytest.raises(ops._lib.GrapesHipError):
        layer(x, ei, edge_weight=ok)
    model = GCN(4, [8, 3])
    with pytest.raises(ValueError):
        model(x, [ei, ei], edge_weight=[ok])                        # list-length mismatch
    with pytest.raises(ValueError):
        model(x, [ei, ei], edge_weight=ok)                          # a list of edges takes a list
    with pytest.raises(ValueError):
        model(x, ei, edge_weight=[ok, ok])
    with pytest.raises(ValueError):
        model(x, [ei, ei], edge_weight=[ok, torch.ones(2)])
    with pytest.raises(ValueError):
        model(x, prep, edge_weight=ok)
    with pytest.raises(ops._lib.GrapesHipError):
        model(x, [ei, ei], edge_weight=[None, ok])                  # entries may be None
