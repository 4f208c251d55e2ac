"""CPU checks of GraphSAINT's normalisation: the numpy oracle of tests/saint_norm_oracle.py by hand and against torch, the driver's
two flags, and the refusals of the samplers and the ops wrappers."""
import numpy as np
import pytest
import torch

from tests import saint_norm_oracle as NO
from tests.test_graphsaint_cpu import COL, ROWPTR

F32 = np.float32


def test_oracle_counts_and_norms_by_hand():
    """Entries of the 6-node graph: j0 (0,1)  j1 (1,0)  j2 (1,2)  j3 (2,1)  j4 (2,3)  j5 (3,3)  j6 (4,3).  Sets {0,1}, {0,1,2}, {4}
    (the second given with a duplicate): nodes 3 and 5 are never sampled, j5 is 0 / 0, j4 and j6 are x / 0."""
    nc, ec, total = NO.coverage_counts(ROWPTR, COL, [[0, 1], [2, 0, 1, 1], [4]])
    assert nc.tolist() == [2, 2, 1, 0, 1, 0]
    assert ec.tolist() == [2, 2, 1, 1, 0, 0, 0]
    assert total == 6
    en, nn = NO.norms(ROWPTR, nc, ec, 3)
    assert en.dtype == np.float32 and nn.dtype == np.float32
    assert en.tolist() == [1.0, 1.0, 2.0, 1.0, F32(1e4), F32(0.1), F32(1e4)]
    never = (F32(3) / F32(0.1)) / F32(6)
    assert nn.tolist() == [0.25, 0.25, 0.5, never, 0.5, never] and abs(float(never) - 5.0) < 1e-6


def test_oracle_norm_rules_on_a_count_table():
    """One row of four entries: counts that give an ordinary quotient, a quotient above 1e4, x / 0 and — in a row whose node count
    is 0 — 0 / 0 and 0 / x."""
    rowptr = np.array([0, 4, 6])
    en, nn = NO.norms(rowptr, np.array([30000, 0]), np.array([7, 2, 0, 30000, 0, 5]), 12)
    assert en.tolist() == [F32(30000) / F32(7), F32(1e4), F32(1e4), 1.0, F32(0.1), 0.0]
    assert nn.tolist() == [(F32(12) / F32(30000)) / F32(2), (F32(12) / F32(0.1)) / F32(2)]


@pytest.mark.parametrize("C", [7, 70])
def test_oracle_weighted_ce_equals_torch(C):
    rng = np.random.default_rng(C)
    n = 40
    z, y = 2 * rng.standard_normal((n, C)), rng.integers(0, C, n)
    w, train = rng.random(n) * 3, rng.random(n) < 0.4
    loss, g, _, _ = NO.weighted_loss(z, y, w, train)
    ref_loss, ref_g = NO.torch_weighted_ce(z, y, w, train)
    assert abs(loss - ref_loss) <= 1e-12 * abs(ref_loss)
    assert np.abs(g - ref_g).max() <= 1e-13
    assert not g[~train].any()
    # w = 1 / T everywhere: the mean loss
    T = int(train.sum())
    mean, gm, _, _ = NO.weighted_loss(z, y, np.full(n, 1.0 / T), train)
    zt = torch.tensor(z, requires_grad=True)
    ref = torch.nn.functional.cross_entropy(zt[torch.as_tensor(train)], torch.as_tensor(y)[torch.as_tensor(train)])
    ref.backward()
    assert abs(mean - float(ref.detach())) <= 1e-12 * float(ref.detach()) and np.abs(gm - zt.grad.numpy()).max() <= 1e-14


def test_oracle_weighted_bce_equals_torch():
    rng = np.random.default_rng(3)
    n, C = 30, 9
    z, y = 2 * rng.standard_normal((n, C)), (rng.random((n, C)) < 0.3).astype(np.float64)
    w, train = rng.random(n) * 3, rng.random(n) < 0.5
    loss, g, _, _ = NO.weighted_loss(z, y, w, train)
    zt = torch.tensor(z, requires_grad=True)
    el = torch.nn.functional.binary_cross_entropy_with_logits(zt, torch.as_tensor(y), reduction="none").mean(1)
    ref = (el * torch.as_tensor(w))[torch.as_tensor(train)].sum()
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-12 * float(ref.detach()) and np.abs(g - zt.grad.numpy()).max() <= 1e-13
    T = int(train.sum())
    mean = NO.weighted_loss(z, y, np.full(n, 1.0 / T), train)[0]
    tm = torch.as_tensor(train)
    assert abs(mean - float(torch.nn.functional.binary_cross_entropy_with_logits(zt[tm], torch.as_tensor(y)[tm]).detach())) <= 1e-12
    assert NO.weighted_loss(z, y, w, np.zeros(n, bool))[0] == 0                 # no training row: 0


def test_oracle_normalised_step_equals_autograd():
    rng = np.random.default_rng(11)
    n, F, H, C = 12, 5, 6, 4
    src, dst = rng.integers(0, n, 40), rng.integers(0, n, 40)
    P = NO.wgcn_dense(src, dst, rng.random(40) * 2, n)
    ws = [rng.standard_normal(s) for s in ((H, F), (H,), (C, H), (C,))]
    x, y, w, train = rng.standard_normal((n, F)), rng.integers(0, C, n), rng.random(n), rng.random(n) < 0.6
    loss, grads, _ = NO.normalised_step(x, P, ws, y, w, train)
    tw = [torch.tensor(t, requires_grad=True) for t in ws]
    Pt = torch.as_tensor(P)
    zt = Pt @ (torch.relu(Pt @ (torch.as_tensor(x) @ tw[0].T) + tw[1]) @ tw[2].T) + tw[3]
    ref = (torch.nn.functional.cross_entropy(zt, torch.as_tensor(y), reduction="none") * torch.as_tensor(w))[torch.as_tensor(train)].sum()
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    for a, b in zip(grads, tw):
        assert np.abs(a - b.grad.numpy()).max() <= 1e-12


def test_cli_flags():
    from grapes_amd.graphsaint import parse_args
    a = parse_args(["--dataset", "cora"])
    assert a.sample_coverage == 0 and a.use_normalization is False
    with pytest.raises(ValueError):
        parse_args(["--dataset", "cora", "--sample_coverage", "5"])
    a = parse_args(["--dataset", "cora", "--use_normalization"])
    assert a.use_normalization is True and a.sample_coverage == 0
    a = parse_args(["--dataset", "cora", "--use_normalization", "--sample_coverage", "5", "--sampler", "edge", "--engine", "eager"])
    assert a.use_normalization is True and a.sample_coverage == 5


def test_estimate_norm_refuses_zero_and_the_constructors_still_refuse_coverage():
    from grapes_amd.modules import saint
    for cls in (saint.GraphSAINTRandomWalkSampler, saint.GraphSAINTNodeSampler, saint.GraphSAINTEdgeSampler):
        for bad in (0, -3):
            with pytest.raises(ValueError):
                object.__new__(cls).estimate_norm(bad)
    with pytest.raises(NotImplementedError, match="estimate_norm"):
        saint.GraphSAINTRandomWalkSampler(object(), batch_size=4, walk_length=2, sample_coverage=100)
    with pytest.raises(NotImplementedError, match="estimate_norm"):
        saint.GraphSAINTNodeSampler(object(), batch_size=4, sample_coverage=1)
    with pytest.raises(NotImplementedError, match="estimate_norm"):
        saint.make_sampler("edge", object(), 4, sample_coverage=1)


def test_ops_wrappers_refuse_cpu_tensors():
    from grapes_amd import _lib, ops
    rowptr, col = torch.as_tensor(ROWPTR), torch.as_tensor(COL, dtype=torch.int32)
    idx, cnt, nmap = torch.zeros(4, dtype=torch.int32), torch.ones(1, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(_lib.GrapesHipError):
        ops.saint_coverage_count(rowptr, col, 6, idx, cnt, nmap)
    with pytest.raises(_lib.GrapesHipError):
        ops.saint_norms(rowptr, 6, torch.zeros(6, dtype=torch.int32), torch.zeros(7, dtype=torch.int32), 3)
    with pytest.raises(_lib.GrapesHipError):
        ops.saint_subgraph(rowptr, col, idx, cnt, nmap, 8, ids=True)
    with pytest.raises(_lib.GrapesHipError):
        ops.saint_masked_loss(torch.zeros(4, 3), 3, idx, cnt, torch.zeros(6, dtype=torch.bool), torch.zeros(6, dtype=torch.int64),
                              node_norm=torch.ones(6))
