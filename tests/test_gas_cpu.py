"""GNNAutoScale without a GPU: the oracle (tests/gas_oracle.py) against a dense restatement and against the exact full-graph model,
the push, the codes, the C surface and the command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import gas_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _partition(n, P, kind, seed=0):
    pos = np.arange(n) * P // n
    if kind == "range":
        return pos
    part = np.empty(n, dtype=np.int64)
    part[np.random.default_rng(seed).permutation(n)] = pos
    return part


def _weights(dims, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(dims[i + 1], dims[i], generator=gen, dtype=F64) * 0.5, torch.randn(dims[i + 1], generator=gen, dtype=F64) * 0.1)
            for i in range(len(dims) - 1)]


def _dense_p(rowptr, col):
    """D^-1/2 (A + I) D^-1/2 with A[u, v] = the number of stored entries (u, v)."""
    n = len(rowptr) - 1
    A = np.zeros((n, n))
    for u in range(n):
        for v in col[rowptr[u]:rowptr[u + 1]]:
            A[u, v] += 1
    dv = GO.dinv(rowptr).numpy()
    return torch.from_numpy(dv[:, None] * (A + np.eye(n)) * dv[None, :])


def test_aggregate_and_backward_against_the_dense_restatement():
    n, f = 30, 5
    rowptr, col = GO.random_graph(n, 4.0, seed=1, dup=(3, 7))            # (3, 7) stored twice, (7, 3) once
    assert list(col[rowptr[3]:rowptr[4]]).count(7) == 2 and list(col[rowptr[7]:rowptr[8]]).count(3) == 1
    part = _partition(n, 5, "random", seed=2)
    clusters = [int(part[3]), int(part[7])] if part[3] != part[7] else [int(part[3]), (int(part[3]) + 1) % 5]
    node_idx = GO.batch_nodes(part, clusters)
    assert 3 in node_idx and 7 in node_idx and len(node_idx) < n
    rowptr_h, code, counts = GO.resolve(rowptr, col, node_idx)
    assert counts[0] > 0 and counts[1] > 0
    gen = torch.Generator().manual_seed(3)
    h = torch.randn(len(node_idx), f, generator=gen, dtype=F64, requires_grad=True)
    hbar = torch.randn(n, f, generator=gen, dtype=F64)
    dv = GO.dinv(rowptr)
    P = _dense_p(rowptr, col)
    m_in = torch.zeros(n, dtype=F64)
    m_in[node_idx] = 1.0
    S = torch.zeros(n, len(node_idx), dtype=F64)
    S[node_idx, np.arange(len(node_idx))] = 1.0
    dense = (P * m_in[None, :])[node_idx] @ (S @ h) + (P * (1.0 - m_in)[None, :])[node_idx] @ hbar
    a = GO.aggregate(h.detach(), hbar, dv, node_idx, rowptr_h, code)
    assert torch.allclose(a, dense.detach(), rtol=1e-12, atol=1e-13)
    da = torch.randn(len(node_idx), f, generator=gen, dtype=F64)
    (dh_dense,) = torch.autograd.grad(dense, h, da)
    src, dst = GO.induced_edges(rowptr_h, code)
    dh = GO.aggregate_bwd(da, dv, node_idx, src, dst)
    assert torch.allclose(dh, dh_dense, rtol=1e-12, atol=1e-13)
    # a backward by symmetry — the forward's own in-batch entries transposed in place — is another sum on this multiset
    wrong = GO.aggregate_bwd(da, dv, node_idx, dst, src)
    assert not torch.allclose(wrong, dh_dense, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("kind", ["random", "range"])
def test_exact_once_the_histories_are_fresh(kind):
    n, P = 60, 6
    rowptr, col = GO.random_graph(n, 5.0, seed=4)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, 7, generator=gen, dtype=F64)
    weights = _weights([7, 6, 5, 3], seed=6)
    full = GO.full_forward(rowptr, col, x, weights)
    part = _partition(n, P, kind, seed=7)
    px = GO.propagate(rowptr, col, x)
    for clusters in ([1], [4, 0], [2, 5, 3]):
        node_idx = GO.batch_nodes(part, clusters)
        rowptr_h, code, _ = GO.resolve(rowptr, col, node_idx)
        logits, acts = GO.forward(rowptr, col, px, weights, full[:-1], node_idx, rowptr_h, code)
        assert torch.allclose(logits, full[-1][node_idx], rtol=1e-11, atol=1e-12)
        for a, hfull in zip(acts, full[:-1]):
            assert torch.allclose(a, hfull[node_idx], rtol=1e-11, atol=1e-12)


def test_every_cluster_is_the_full_batch_whatever_the_histories_hold():
    n, P = 40, 4
    rowptr, col = GO.random_graph(n, 4.0, seed=8)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(n, 6, generator=gen, dtype=F64)
    y = torch.randint(0, 3, (n,), generator=gen)
    train = torch.rand(n, generator=gen) < 0.6
    weights = _weights([6, 5, 3], seed=10)
    hist = [torch.randn(n, 5, generator=gen, dtype=F64) * 100]
    part = _partition(n, P, "random", seed=11)
    node_idx = GO.batch_nodes(part, [2, 0, 3, 1])
    _, code, counts = GO.resolve(rowptr, col, node_idx)
    assert counts[1] == 0 and (code >= 0).all()
    loss, dW, db, _ = GO.step(rowptr, col, x, y, train, weights, hist, node_idx)
    ws = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in weights]
    ref = torch.nn.functional.cross_entropy(GO.full_forward(rowptr, col, x, ws)[-1][train], y[train])
    ref.backward()
    ref = float(ref.detach())
    assert abs(loss - ref) <= 1e-12 * max(1.0, abs(ref))
    for (w, b), gw, gb in zip(ws, dW, db):
        assert torch.allclose(gw, w.grad, rtol=1e-10, atol=1e-12) and torch.allclose(gb, b.grad, rtol=1e-10, atol=1e-12)


def test_push_writes_the_batch_rows_and_nothing_else():
    n, P = 50, 5
    rowptr, col = GO.random_graph(n, 4.0, seed=12)
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(n, 6, generator=gen, dtype=F64)
    y = torch.randint(0, 3, (n,), generator=gen)
    train = torch.ones(n, dtype=torch.bool)
    weights = _weights([6, 5, 4, 3], seed=14)
    hist = [torch.randn(n, 5, generator=gen, dtype=F64), torch.randn(n, 4, generator=gen, dtype=F64)]
    before = [h.clone() for h in hist]
    node_idx = GO.batch_nodes(_partition(n, P, "range"), [3, 1])
    _, _, _, new = GO.step(rowptr, col, x, y, train, weights, hist, node_idx)
    rowptr_h, code, _ = GO.resolve(rowptr, col, node_idx)
    _, acts = GO.forward(rowptr, col, GO.propagate(rowptr, col, x), weights, hist, node_idx, rowptr_h, code)
    rest = np.setdiff1d(np.arange(n), node_idx)
    for h0, h1, hb, a in zip(before, new, hist, acts):
        assert torch.equal(hb, h0)                                       # the step's inputs are not modified
        assert torch.equal(h1[node_idx], a) and bool((a >= 0).all())     # post-ReLU, all n rows
        assert torch.equal(h1[rest], h0[rest])


def test_codes_against_set_membership():
    n, P = 80, 8
    rowptr, col = GO.random_graph(n, 6.0, seed=15, dup=(5, 9))
    part = _partition(n, P, "random", seed=16)
    for clusters in ([0], [7, 2, 3], list(range(P))):
        node_idx = GO.batch_nodes(part, clusters)
        members = set(int(v) for v in node_idx)
        rowptr_h, code, counts = GO.resolve(rowptr, col, node_idx)
        assert np.array_equal(np.diff(rowptr_h), np.diff(rowptr)[node_idx]) and rowptr_h[0] == 0 and rowptr_h[-1] == len(code)
        want_in = 0
        for i, u in enumerate(node_idx):
            for t, v in enumerate(col[rowptr[u]:rowptr[u + 1]]):
                c = int(code[rowptr_h[i] + t])
                if int(v) in members:
                    assert c >= 0 and node_idx[c] == v
                    want_in += 1
                else:
                    assert c == -1 - int(v)
        assert counts[0] == want_in and counts[0] + counts[1] == len(code)
        src, dst = GO.induced_edges(rowptr_h, code)
        assert len(src) == want_in and (np.diff(dst) >= 0).all()


# ------------------------------------------------------------------------------------------------------------ the C surface
_NEW = {"grapes_gas_resolve_workspace_bytes": 1, "grapes_gas_resolve": 17, "grapes_gas_aggregate_workspace_bytes": 3,
        "grapes_gas_aggregate_fwd": 18, "grapes_gas_aggregate_bwd": 13}


def test_header_ctypes_makefile_and_both_libraries_agree():
    import __graft_entry__ as ge
    from grapes_amd import _lib, ops
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.DIAG_LIB_PATH)):
        ge.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grapes_hip.h")).read(), flags=re.S)
    libs = [ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib.DIAG_LIB_PATH)]
    for name, nargs in _NEW.items():
        m = re.search(r"\b(?:int|int32_t|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).strip().split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert all(hasattr(lib, name) for lib in libs), name
    assert "#define GRAPES_ABI_VERSION 304" in src
    bound = _lib.load()
    assert bound.grapes_abi_version() == 304
    assert bound.grapes_gas_resolve_workspace_bytes(10) >= 11 * 4                       # host helpers: callable without a GPU
    assert bound.grapes_gas_aggregate_workspace_bytes(10, 3, 8) >= 11 * 4 + 3 * 8 * 4
    assert ops.GAS_CHUNK == 64 and ops.GAS_BAD_CODE == GO.BAD_CODE
    mk = open(os.path.join(ROOT, "grapes_amd", "csrc", "Makefile")).read()
    assert "gas_kernels.o" in mk and "hist_rows.h" in mk
    assert os.path.exists(os.path.join(ROOT, "grapes_amd", "csrc", "gas_kernels.hip"))


_DEFAULTS = dict(dataset="cora", num_parts=32, batch_size=4, partition="random", partition_file=None, hidden_dim=256, num_layers=2,
                 lr=1e-3, max_epoch=100, eval_frequency=1, dropout=0.0, runs=1, seed=None)


def test_parse_args():
    from grapes_amd import gas
    assert vars(gas.parse_args(["--dataset", "cora"])) == _DEFAULTS
    a = gas.parse_args(["--dataset", "cora", "--num_parts", "32", "--batch_size", "4", "--partition", "lp:30:0.1", "--max_epoch", "50"])
    assert (a.partition, a.max_epoch) == ("lp:30:0.1", 50)
    b = gas.parse_args(["--dataset", "reddit", "--num_parts", "8", "--batch_size", "8", "--partition", "file", "--partition_file", "p.npy",
                        "--hidden_dim", "32", "--num_layers", "3", "--lr", "0.01", "--eval_frequency", "2", "--runs", "3", "--seed", "5"])
    assert vars(b) == dict(dataset="reddit", num_parts=8, batch_size=8, partition="file", partition_file="p.npy", hidden_dim=32,
                           num_layers=3, lr=0.01, max_epoch=100, eval_frequency=2, dropout=0.0, runs=3, seed=5)
    with pytest.raises(SystemExit, match="--dataset is required"):
        gas.parse_args([])
    with pytest.raises(ValueError, match="--dropout other than 0"):
        gas.parse_args(["--dataset", "cora", "--dropout", "0.5"])
    with pytest.raises(ValueError, match="at most --num_parts"):
        gas.parse_args(["--dataset", "cora", "--num_parts", "2", "--batch_size", "3"])
    with pytest.raises(ValueError, match="--partition_file"):
        gas.parse_args(["--dataset", "cora", "--partition", "file"])
    with pytest.raises(ValueError, match="at least 1"):
        gas.parse_args(["--dataset", "cora", "--hidden_dim", "0"])
    for bad in ("metis", "lp:x", "lp:1:2:3", "lp:-1"):
        with pytest.raises(SystemExit):
            gas.parse_args(["--dataset", "cora", "--partition", bad])
    for other in (["--diag_lambda", "0.1"], ["--fanouts", "2,2"], ["--classifier", "gcn"], ["--model_type", "gcn"]):
        with pytest.raises(SystemExit):                                  # no flag of another driver
            gas.parse_args(["--dataset", "cora"] + other)


def test_refusals_and_no_cpu_path():
    from types import SimpleNamespace
    from grapes_amd import _lib, ops
    from grapes_amd.gas import GasTrainer
    from grapes_amd.modules.gas import GasLayerFn, gas_forward
    from grapes_amd.modules.gcn import GCN, ClusterGCN
    x, y = torch.zeros(5, 4), torch.zeros(5, dtype=torch.long)
    with pytest.raises(TypeError, match="project's GCN"):
        GasTrainer(None, x, y, ClusterGCN(4, hidden_dims=[8, 2]), None)
    with pytest.raises(ValueError, match="dropout"):
        GasTrainer(None, x, y, GCN(4, [8, 2], dropout=0.5), None)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        GasTrainer(None, x, y, GCN(4, [8, 2]), None)
    with pytest.raises(TypeError, match="project's GCN"):
        gas_forward(ClusterGCN(4, hidden_dims=[8, 2]), None, None, None, None)
    with pytest.raises(ValueError, match="dropout"):
        gas_forward(GCN(4, [8, 2], dropout=0.1), None, None, None, None)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    h, hbar = torch.zeros(3, 4), torch.zeros(5, 4)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        ops.gas_resolve(torch.zeros(6, dtype=torch.int64), i32(0), 5, i32(0, 1, 2), 3, torch.zeros((5, 2), dtype=torch.int32),
                        torch.zeros((2, 2), dtype=torch.int32), 1, 16)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        ops.gas_aggregate_fwd(h, hbar, torch.ones(5), i32(0, 1, 2), i32(0, 0, 0, 0), i32(0), item_cap=0)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        ops.gas_aggregate_bwd(h, i32(0, 1, 2), torch.ones(5), None)
    lay = SimpleNamespace(node_idx=i32(0, 1, 2), dinv=torch.ones(5), rowptr_h=i32(0, 0, 0, 0), code=i32(0), prep=None, item_cap=0,
                          status=None)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        GasLayerFn.apply(h, hbar, lay)
