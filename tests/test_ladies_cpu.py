"""LADIES / FastGCN without a GPU: the C surface, the host oracle (tests/ladies_oracle.py) against a dense brute force of the
definitions, the shifted-logit argument the sampler rests on, the draw's distribution, and the driver's arguments."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import portable_math as pm
from tests import ladies_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("grapes_ladies_importance", "grapes_ladies_layer", "grapes_ladies_layer_workspace_bytes")
F32 = np.float32


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    from grapes_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.DIAG_LIB_PATH):
        ge.build()
    return _lib


def test_header_table_and_both_libraries_carry_the_entry_points(built_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grapes_hip.h")).read(), flags=re.S)
    prod, diag = ctypes.CDLL(built_lib.LIB_PATH), ctypes.CDLL(built_lib.DIAG_LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in grapes_hip.h"
        assert name in built_lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(prod, name) and hasattr(diag, name), f"{name} is not exported"
    assert built_lib.load().grapes_abi_version() == 304


def test_layer_workspace_is_a_host_call_that_grows(built_lib):
    lib = built_lib.load()
    sizes = [lib.grapes_ladies_layer_workspace_bytes(m) for m in (1, 64, 4096)]
    assert sizes[0] > 0 and sizes[0] < sizes[1] < sizes[2] and sizes[2] >= 3 * 4 * 4096


# ---------------------------------------------------------------------------------------------------- oracle vs brute force
def _brute_layer(P, prev, after, pi):
    """{(i, j): w} by the definition, with P dense: the v_ij / D_i = P_ij cancel D_i in the row normalisation."""
    out = {}
    for i in prev:
        q = {j: P[i, j] / pi[j] for j in after if P[i, j] > 0}
        s = sum(q.values())
        out.update({(i, j): v / s for j, v in q.items()})
    return out


def test_hand_graph_has_a_stored_loop_and_an_isolated_node():
    indptr, indices, n = LO.hand_graph()
    assert n == 12 and indptr[12] - indptr[11] == 0 and 2 in indices[indptr[2]:indptr[3]]
    P = LO.dense_p(indptr, indices, n)
    assert np.allclose(P.sum(1), 1.0) and P[11, 11] == 1.0 and np.isclose(P[2, 2], 2.0 / 4.0)


@pytest.mark.parametrize("kind", ["ladies", "fastgcn"])
def test_oracle_agrees_with_the_dense_definitions(kind):
    indptr, indices, n = LO.hand_graph()
    P = LO.dense_p(indptr, indices, n)
    targets = np.array([5, 2, 11])                                       # unsorted; the loop node and the isolated node
    rng = np.random.default_rng(3)
    u = [rng.random(n).astype(F32) for _ in range(3)]
    b = LO.sample(indptr, indices, n, targets, 4, 3, kind=kind, uniforms=u)
    prev = targets
    for L in b.layers:
        assert np.array_equal(L.prev, prev)
        rows = np.arange(n) if kind == "fastgcn" else prev
        pi = (P[rows] ** 2).sum(0)
        cand = np.nonzero(P[prev].sum(0) > 0)[0] if kind == "ladies" else np.arange(n)
        assert np.array_equal(L.candidates, cand)
        assert np.allclose(L.pi, pi[cand], rtol=1e-13, atol=0) and (L.pi > 0).all()
        assert np.array_equal(L.terms, (P[rows][:, cand] > 0).sum(0))
        assert len(L.sampled) == min(len(cand), 4) and np.isin(L.sampled, cand).all()
        if kind == "ladies":
            assert np.isin(targets, L.after).all() and np.array_equal(L.after, np.union1d(L.sampled, targets))
        else:
            assert np.array_equal(L.after, np.sort(L.sampled))
        want = _brute_layer(P, prev, L.after, pi)
        got = {(int(i), int(j)): w for j, i, w in zip(L.src, L.dst, L.w)}
        assert got.keys() == want.keys()
        assert all(np.isclose(got[k], want[k], rtol=1e-12) for k in want)
        order = [(int(np.nonzero(prev == i)[0][0]), int(j)) for j, i in zip(L.src, L.dst)]
        assert order == sorted(order)                                    # rows in prev's order, ascending j within a row
        sums = np.zeros(n)
        np.add.at(sums, L.dst, L.w)
        assert all(np.isclose(sums[i], 1.0, rtol=1e-12) or sums[i] == 0.0 for i in prev)
        if kind == "ladies":
            assert (sums[prev] > 0).all()                                # a LADIES row always keeps its own diagonal
        prev = L.after
    assert np.array_equal(b.node_idx, np.unique(np.concatenate([targets] + [L.after for L in b.layers])))
    for ei, L in zip(b.edge_index, b.layers):
        assert np.array_equal(b.node_idx[ei[0]], L.src) and np.array_equal(b.node_idx[ei[1]], L.dst)


def test_fastgcn_importance_is_global_and_targets_are_not_forced():
    indptr, indices, n = LO.hand_graph()
    P = LO.dense_p(indptr, indices, n)
    u = [np.random.default_rng(5).random(n).astype(F32)] * 2
    a = LO.sample(indptr, indices, n, np.array([0]), 3, 2, kind="fastgcn", uniforms=u)
    b = LO.sample(indptr, indices, n, np.array([9, 10]), 3, 2, kind="fastgcn", uniforms=u)
    for L in a.layers + b.layers:
        assert np.allclose(L.pi, (P ** 2).sum(0), rtol=1e-13)
    assert np.array_equal(a.layers[0].after, b.layers[0].after)          # the draw does not depend on the targets
    assert not np.isin([9, 10], b.layers[0].after).all()
    empty = [i for i in b.layers[0].prev if not (b.layers[0].dst == i).any()]
    assert empty, "the case is meant to have a row without a kept column"


# ---------------------------------------------------------------------------------------------------- the shifted logits
def _logit32(pi, m):
    """l = logf(pi) - C, C = 20 + logf(float(m)), in fp32 with the portable logf — the kernel's arithmetic."""
    C = (F32(20.0) + pm.p_logf(np.array([m], F32))).astype(F32)
    return (pm.p_logf(np.asarray(pi, dtype=F32)) - C).astype(F32)


def test_log_sigmoid_is_the_identity_on_the_shifted_logits():
    """pi_j <= |prev| = m, so l <= -20, where sigmoid(l) = exp(l) and log(exp(l)) = l in fp32, bit for bit: the draw's keys are
    log pi + Gumbel - C.  Every pair of the listed pi and m inside that domain (pi <= m)."""
    pis, ms, seen = (1e-13, 1e-4, 0.02, 1.0 / 9.0, 1.0, 1e7), (1.0, 16.0, 1e7), 0
    for m in ms:
        pi = np.array([p for p in pis if p <= m], F32)
        l = _logit32(pi, m)
        assert (l <= -20.0).all() and l.min() >= -67.0
        back = pm.p_logf(pm.p_sigmoid(l))
        assert np.array_equal(back.view(np.uint32), l.view(np.uint32)), (m, l, back)
        seen += len(pi)
    assert seen == 5 + 5 + 6 and _logit32([1e-13], 1e7)[0] < -65.0


def test_draw_frequencies_follow_pi():
    """k = 1 of 8 candidates, 20 000 draws on the Philox stream (1234, 0): every winning frequency within 4 binomial sigma of
    pi / sum pi (deterministic: the stream is fixed)."""
    pi = np.array([1 / 9, 1 / 16 + 1 / 25, 1.0, 1 / 4, 3 / 49, 1e-4, 0.3, 0.02])
    T, n = 20000, len(pi)
    l = _logit32(pi, 16.0)
    u = pm.philox_uniform(1234, 0, T * n).reshape(T, n)
    keys = pm.gumbel_keys(np.tile(l, T), u.reshape(-1)).reshape(T, n)
    wins = np.bincount(np.argmax(keys, axis=1), minlength=n)
    one = LO.draw(l, np.arange(n), 1, u[0])                              # the oracle's draw is that argmax
    assert len(one) == 1 and one[0] == np.argmax(keys[0])
    p = pi / pi.sum()
    z = (wins - T * p) / np.sqrt(T * p * (1 - p))
    print("z =", np.round(z, 2))
    assert np.abs(z).max() <= 4.0, z


# ---------------------------------------------------------------------------------------------------- the driver
def test_cli_arguments():
    from grapes_amd import ladies
    a = ladies.parse_args(["--dataset", "cora"])
    assert (a.sampler, a.samp_num, a.batch_size, a.hidden_dim, a.num_layers, a.lr) == ("ladies", 64, 512, 256, 2, 1e-3)
    assert a.dropout == 0.0 and a.runs == 1 and a.seed is None and a.e_cap is None and a.eval_frequency == 1 and a.max_epoch == 100
    b = ladies.parse_args(["--dataset", "cora", "--sampler", "fastgcn", "--samp_num", "8", "--num_layers", "3", "--e_cap", "100",
                           "--max_epoch", "2", "--seed", "7", "--dropout", "0.5", "--runs", "2", "--eval_frequency", "5"])
    assert (b.sampler, b.samp_num, b.num_layers, b.e_cap, b.max_epoch, b.seed, b.dropout, b.runs, b.eval_frequency) == \
        ("fastgcn", 8, 3, 100, 2, 7, 0.5, 2, 5)
    with pytest.raises(SystemExit):
        ladies.parse_args(["--dataset", "cora", "--sampler", "asgcn"])
    with pytest.raises(SystemExit):
        ladies.parse_args([])
    with pytest.raises(ValueError):
        ladies.parse_args(["--dataset", "cora", "--batch_size", "5000"])


def test_unknown_kind_is_refused_before_any_device_work():
    from grapes_amd.modules.ladies import LayerWiseSampler
    with pytest.raises(ValueError, match="ladies, fastgcn"):
        LayerWiseSampler(object(), 4, 2, kind="asgcn")
