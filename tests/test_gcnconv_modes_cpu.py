"""GCNConv's constructor arguments (improved, cached, add_self_loops, normalize, bias) without a GPU: what the constructor accepts,
resolves and refuses, the parameters it registers, that no mode has a CPU path, and the oracle of tests/gcnconv_modes_oracle.py
against a dense fp64 closed form and against its own closed forms on the hand graph (node 2 with two stored loops of different
weights, the entry 0 -> 1 stored twice, nodes 0 and 5 without an incoming entry)."""
import numpy as np
import pytest
import torch

from tests import gcnconv_modes_oracle as M
from tests import wgcn_oracle as O


def _conv():
    from grapes_amd.modules.gcn import GCNConv
    return GCNConv


def test_constructor_defaults_and_add_self_loops_resolution():
    GCNConv = _conv()
    d = GCNConv(5, 3)
    assert (d.improved, d.cached, d.add_self_loops, d.normalize) == (False, False, True, True) and d.bias is not None
    assert GCNConv(5, 3, normalize=False).add_self_loops is False           # None means "as normalize"
    assert GCNConv(5, 3, normalize=True, add_self_loops=None).add_self_loops is True
    assert GCNConv(5, 3, add_self_loops=False).normalize is True
    assert GCNConv(5, 3, improved=True).improved is True
    p = GCNConv(5, 3, False, False, None, True, True)                       # PyG's positional order
    assert (p.improved, p.add_self_loops, p.normalize) == (False, True, True)


def test_refusals():
    GCNConv = _conv()
    with pytest.raises(ValueError):
        GCNConv(5, 3, add_self_loops=True, normalize=False)
    with pytest.raises(NotImplementedError):
        GCNConv(5, 3, cached=True)


def test_bias_false_registers_none():
    GCNConv = _conv()
    layer = GCNConv(5, 3, bias=False)
    assert layer.bias is None and "bias" in layer._parameters
    assert sorted(layer.state_dict().keys()) == ["lin.weight"]
    assert [n for n, _ in layer.named_parameters()] == ["lin.weight"]
    layer.reset_parameters()
    assert sorted(GCNConv(5, 3).state_dict().keys()) == ["bias", "lin.weight"]


def test_spelled_out_defaults_build_the_same_layer():
    GCNConv = _conv()
    torch.manual_seed(7)
    a = GCNConv(6, 4)
    torch.manual_seed(7)
    b = GCNConv(6, 4, improved=False, add_self_loops=True, normalize=True, bias=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a._default_mode() and b._default_mode()
    for kw in (dict(improved=True), dict(add_self_loops=False), dict(normalize=False)):
        assert not GCNConv(6, 4, **kw)._default_mode()


@pytest.mark.parametrize("kw", [dict(improved=True), dict(add_self_loops=False), dict(normalize=False), dict(bias=False)])
def test_no_cpu_path(kw):
    from grapes_amd import _lib
    layer = _conv()(4, 3, **kw)
    x, ei = torch.zeros(5, 4), torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(_lib.GrapesHipError):
        layer(x, ei)
    with pytest.raises(_lib.GrapesHipError):
        layer(x, ei, edge_weight=torch.ones(3))


@pytest.mark.parametrize("kw", [dict(improved=True), dict(add_self_loops=False), dict(normalize=False)])
def test_other_modes_take_an_edge_index_tensor_only(kw):
    layer = _conv()(4, 3, **kw)
    x = torch.zeros(5, 4)
    with pytest.raises(ValueError):
        layer(x, object())
    with pytest.raises(ValueError):
        layer(x, torch.zeros(2, 3, dtype=torch.long), large_graph=True)
    with pytest.raises(ValueError):
        layer(x, torch.zeros(3, 3, dtype=torch.long))


# ------------------------------------------------------------------------------------------------------------ the oracle
def _hand():
    src, dst, w, n = O.hand_graph()
    assert np.sum((src == 2) & (dst == 2)) == 2 and len(set(w[(src == 2) & (dst == 2)])) == 2       # two loops, two weights
    assert np.sum((src == 0) & (dst == 1)) == 2                                                    # a duplicate edge
    assert not np.any(dst == 0) and not np.any(dst == 5)                                           # no incoming entry
    return src, dst, w, n


def _operands(n, fi, fo, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, fi)), rng.standard_normal((fo, fi)) * 0.3, rng.standard_normal(fo) * 0.1


@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("weighted", [True, False])
def test_oracle_matches_the_dense_closed_form(mode, weighted):
    src, dst, w, n = _hand()
    if not weighted:
        w = np.ones_like(w)
    imp, asl, nrm = M.MODES[mode]
    x, W, b = _operands(n, 5, 4, 3)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    got = M.forward64(t(x), t(W), t(b), src, dst, t(w), n, improved=imp, add_self_loops=asl, normalize=nrm).numpy()
    want = M.dense_forward(x, W, b, src, dst, w, n, improved=imp, add_self_loops=asl, normalize=nrm)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-13)
    if mode != "plain":
        nob = M.forward64(t(x), t(W), None, src, dst, t(w), n, improved=imp, add_self_loops=asl, normalize=nrm).numpy()
        assert np.allclose(nob, want - b, rtol=1e-12, atol=1e-13)
    if mode in ("no_loops", "plain"):
        assert np.array_equal(got[0], b) and np.array_equal(got[5], b)        # no incoming entry: the bias
    if mode == "default":
        assert np.allclose(got, O.forward64(t(x), t(W), t(b), src, dst, t(w), n).numpy(), rtol=1e-13, atol=1e-14)


def test_rules_differ_where_they_should():
    src, dst, w, n = _hand()
    x, W, b = _operands(n, 5, 4, 4)
    outs = {m: M.dense_forward(x, W, b, src, dst, w, n, *M.MODES[m]) for m in M.MODES}
    names = list(outs)
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            assert np.abs(outs[names[i]] - outs[names[j]]).max() > 1e-3, (names[i], names[j])
    # improved has no effect without added loops
    assert np.array_equal(M.dense_forward(x, W, b, src, dst, w, n, True, False, True), outs["no_loops"])


@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("graph", ["hand", "small"])
def test_problem_closed_forms_match_autograd(mode, graph):
    """ModeProblem's lw-form sums and its closed-form weight gradient against autograd on forward64, with a ReLU and a bias."""
    if graph == "hand":
        src, dst, w, n = _hand()
    else:
        (src, dst), n = O.random_graph(60, 400, 2), 60
        w = O.weights("uniform", 400, 3)
    imp, asl, nrm = M.MODES[mode]
    P = M.ModeProblem(src, dst, w, n, imp, asl, nrm)
    x, W, b = _operands(n, 6, 5, 5)
    dout = np.random.default_rng(6).standard_normal((n, 5))
    r = P.layer(x, W, b, True, dout)
    assert np.allclose(r["out"][0].numpy(), r["out64"].numpy(), rtol=1e-5, atol=1e-6)       # (H is the fp32-rounded operands')
    assert np.allclose(r["dw_closed"].numpy(), r["dw"][0].numpy(), rtol=1e-9, atol=1e-11)
    loops = P.loops
    assert len(loops) >= 3
    if mode in ("no_loops", "plain"):
        assert np.all(r["dw"][1].numpy()[loops] > 0)                      # every stored loop carries a gradient
    nob = P.layer(x, W, None, False, dout)
    assert "db" not in nob and np.allclose(nob["dw_closed"].numpy(), nob["dw"][0].numpy(), rtol=1e-9, atol=1e-11)


def test_loop_sum_is_in_input_order():
    src, dst, w, n = _hand()
    P = M.ModeProblem(src, dst, w, n, add_self_loops=False)
    assert P.lw32[2] == np.float32(np.float32(0.75) + np.float32(1.5)) and P.lw32[1] == np.float32(2.5) and P.lw32[0] == 0
    assert list(P.loops) == [1, 3, 5]
    Q = M.ModeProblem(src, dst, w, n, improved=True)
    assert Q.lw[2] == 1.5 and Q.lw[0] == 2.0 and Q.lw[1] == 2.5
