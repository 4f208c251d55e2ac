"""LINKX without a GPU: tests/linkx_oracle.py against dense restatements in fp64, the model's forward against the five lines written
out, the C surface, the refusals and the command line's parsing."""
import numpy as np
import pytest
import torch

from tests import linkx_oracle as LO

F64 = np.float64


def _graph():
    """12 nodes: duplicates (row 0 stores 5 twice, row 4 stores 1 three times), loops (rows 2 and 7), an empty row (3), a directed
    entry pattern; the batch repeats row 0 and row 4."""
    rows_of = [[5, 1, 5, 9], [0], [2, 2, 11], [], [1, 1, 6, 1], [4], [0, 5], [7, 3], [10, 9, 8], [9], [0, 11], [1]]
    ip, ix = LO.csr(rows_of, 12)
    return ip, ix, [0, 4, 3, 0, 8, 2, 4, 11, 7]


def test_batch_tables_match_a_dense_restatement():
    ip, ix, rows = _graph()
    bt = LO.batch(ip, ix, rows)
    A = LO.count_matrix(ip, ix, rows)
    assert np.array_equal(bt.bptr, np.concatenate([[0], np.cumsum(A.sum(1))]).astype(np.int32)) and bt.e == int(A.sum())
    cols = np.nonzero(A.sum(0))[0]
    assert np.array_equal(bt.uniq, cols) and bt.n_u == len(cols)
    trow = []
    for j in cols:                                                       # nonzero by column: batch rows ascending, c copies adjacent
        for b in np.nonzero(A[:, j])[0]:
            trow += [b] * int(A[b, j])
    assert np.array_equal(bt.trow, trow)
    assert np.array_equal(np.diff(bt.tptr), A.sum(0)[cols].astype(np.int64)) and bt.tptr[0] == 0
    assert bt.seg_max == int(A.sum(0).max()) and bt.row_max == int(A.sum(1).max())
    assert A[0, 5] == 2 and A[1, 1] == 3 and A[2].sum() == 0 and A[5, 2] == 2


def test_forward_and_sparse_gradient_match_the_dense_ones():
    ip, ix, rows = _graph()
    rng = np.random.default_rng(0)
    W, b = rng.standard_normal((12, 5)), rng.standard_normal(5)
    A = LO.count_matrix(ip, ix, rows)
    out, mag = LO.fwd(ip, ix, rows, W, b)
    assert np.allclose(out, A @ W + b, rtol=0, atol=1e-13) and np.allclose(mag, A @ np.abs(W) + np.abs(b), rtol=0, atol=1e-13)
    assert np.array_equal(out[2], b)                                     # the empty row
    Wt, bt_ = torch.tensor(W, requires_grad=True), torch.tensor(b, requires_grad=True)
    co = torch.tensor(rng.standard_normal((len(rows), 5)))
    (LO.bag(Wt, bt_, ip, ix, rows) * co).sum().backward()
    Wd, bd = torch.tensor(W, requires_grad=True), torch.tensor(b, requires_grad=True)
    ((torch.tensor(A) @ Wd + bd) * co).sum().backward()
    assert Wt.grad.is_sparse
    sp = Wt.grad.coalesce()
    nz = np.nonzero(A.sum(0))[0]
    assert np.array_equal(sp.indices().numpy()[0], nz)
    assert np.allclose(sp.values().numpy(), Wd.grad.numpy()[nz], rtol=0, atol=1e-13)
    assert np.abs(np.delete(Wd.grad.numpy(), nz, axis=0)).max() == 0 and np.allclose(bt_.grad.numpy(), bd.grad.numpy())


def test_update_is_sparse_adam_over_partly_overlapping_steps():
    rng = np.random.default_rng(1)
    N, H = 40, 6
    p0 = rng.standard_normal((N, H))
    p, m, v = p0.copy(), np.zeros((N, H)), np.zeros((N, H))
    tp = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.SparseAdam([tp], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
    touched = [np.arange(0, 12), np.arange(8, 20), np.array([0, 19, 25]), np.arange(8, 12), np.array([30])]
    never = np.setdiff1d(np.arange(N), np.concatenate(touched))
    for t, uniq in enumerate(touched, 1):
        g = rng.standard_normal((len(uniq), H))
        LO.adam_rows(p, m, v, uniq, g, 0.01, 0.9, 0.999, 1e-8, t)
        tp.grad = torch.sparse_coo_tensor(torch.tensor(uniq)[None], torch.tensor(g), (N, H))
        opt.step()
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-15, t
    st = opt.state[tp]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-15 and np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-15
    assert int(st["step"]) == 5                                          # t counts calls: row 30 was first touched at t = 5
    assert np.array_equal(p[never], p0[never]) and (m[never] == 0).all() and (v[never] == 0).all()
    ss5 = 0.01 * np.sqrt(1 - 0.999 ** 5) / (1 - 0.9 ** 5)               # ... and its first step used t = 5's step size
    assert np.allclose(p[30] - p0[30], -ss5 * m[30] / (np.sqrt(v[30]) + 1e-8), rtol=1e-12, atol=0)


def _model(**kw):
    from grapes_amd.modules.linkx import LINKX
    torch.manual_seed(3)
    return LINKX(12, 7, 8, 3, **kw)


def test_linkx_keys_init_and_forward_are_the_five_lines():
    from grapes_amd.modules import linkx as ML
    model = _model(num_node_layers=2, num_final_layers=3).double()
    assert sorted(model.state_dict()) == sorted(
        ["edge_lin.weight", "edge_lin.bias", "cat_lin1.weight", "cat_lin1.bias", "cat_lin2.weight", "cat_lin2.bias"] +
        [f"node_mlp.lins.{k}.{w}" for k in range(2) for w in ("weight", "bias")] +
        [f"final_mlp.lins.{k}.{w}" for k in range(3) for w in ("weight", "bias")])
    assert model.edge_lin.weight.shape == (12, 8) and model.edge_lin.weight.abs().max() <= 1 / np.sqrt(12)
    assert model.edge_lin.bias.abs().max() <= 1 / np.sqrt(12)
    assert all(q is not model.edge_lin.weight for q in model.dense_parameters())
    assert len(model.dense_parameters()) == len(list(model.parameters())) - 1
    ip, ix, rows = _graph()
    A = torch.tensor(LO.count_matrix(ip, ix, rows))
    xb = torch.tensor(np.random.default_rng(2).standard_normal((len(rows), 7)))
    sd = model.state_dict()
    want = LO.linkx_forward(sd, A, xb)
    got = model.head(A @ sd["edge_lin.weight"] + sd["edge_lin.bias"], xb)   # the layer's output stated densely, then the model's own head
    assert got.shape == (len(rows), 3) and torch.allclose(got, want, rtol=0, atol=1e-12)
    # ... and the same five lines once more, with nothing shared
    out = A @ sd["edge_lin.weight"] + sd["edge_lin.bias"]
    out = out + out @ sd["cat_lin1.weight"].T + sd["cat_lin1.bias"]
    x = torch.relu(xb @ sd["node_mlp.lins.0.weight"].T + sd["node_mlp.lins.0.bias"]) @ sd["node_mlp.lins.1.weight"].T + sd["node_mlp.lins.1.bias"]
    out = torch.relu(out + x + x @ sd["cat_lin2.weight"].T + sd["cat_lin2.bias"])
    h = torch.relu(out @ sd["final_mlp.lins.0.weight"].T + sd["final_mlp.lins.0.bias"])
    h = torch.relu(h @ sd["final_mlp.lins.1.weight"].T + sd["final_mlp.lins.1.bias"])
    assert torch.allclose(got, h @ sd["final_mlp.lins.2.weight"].T + sd["final_mlp.lins.2.bias"], rtol=0, atol=1e-12)
    assert ML.GRADS == ("fused", "sparse")


def test_refusals():
    from grapes_amd import ops
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.linkx import LinkxTrainer
    from grapes_amd.modules.linkx import LINKX, AdjacencyBag, BagAdam
    with pytest.raises(NotImplementedError, match="num_edge_layers"):
        LINKX(12, 7, 8, 3, num_edge_layers=2)
    with pytest.raises(NotImplementedError, match="normalisation"):
        LINKX(12, 7, 8, 3, norm="batch_norm")
    with pytest.raises(ValueError, match="grad="):
        AdjacencyBag(12, 8, grad="dense")
    with pytest.raises(ValueError, match="width"):
        AdjacencyBag(12, 1023)
    with pytest.raises(ValueError, match="fused"):
        BagAdam(AdjacencyBag(12, 8, grad="sparse"))
    opt = BagAdam(AdjacencyBag(12, 8))
    with pytest.raises(RuntimeError, match="pending"):
        opt.step()
    z = torch.zeros
    i32 = lambda *s: z(*s, dtype=torch.int32)
    with pytest.raises(GrapesHipError):                                  # no CPU path
        ops.bag_fwd(z(13, dtype=torch.int64), i32(4), 12, i32(3), z(12, 8))
    with pytest.raises(GrapesHipError):
        ops.bag_batch(z(13, dtype=torch.int64), i32(4), 12, i32(3), (z(1, dtype=torch.int64), i32(12)), 8, 8)
    with pytest.raises(GrapesHipError):
        ops.bag_bwd(z(3, 8), i32(2), i32(1), 1, 1)
    with pytest.raises(GrapesHipError):
        ops.bag_bwd_adam(z(3, 8), i32(2), i32(1), i32(1), 1, 1, z(12, 8), z(12, 8), z(12, 8), 1e-3, 0.9, 0.999, 1e-8, 1)
    model = _model()
    with pytest.raises(TypeError, match="LINKX"):
        LinkxTrainer(None, z(12, 7), z(12), torch.nn.Linear(2, 2), torch.optim.SGD(model.dense_parameters(), lr=0.1))
    with pytest.raises(ValueError, match="gradient"):
        LinkxTrainer(None, z(12, 7, requires_grad=True), z(12), model, torch.optim.SGD(model.dense_parameters(), lr=0.1))
    with pytest.raises(ValueError, match="edge_lin.weight"):
        LinkxTrainer(None, z(12, 7), z(12), model, torch.optim.SGD(model.parameters(), lr=0.1))
    assert ops.bag_fwd_item_cap(1000, 64) == 0 and ops.bag_fwd_item_cap(1000, 65) == 15 and ops.bag_fwd_item_cap(1000) == 15
    assert ops.bag_bwd_item_cap(1000, 64) == 0 and ops.bag_bwd_item_cap(1000, 65) == 31
    assert abs(ops.bag_adam_step_size(0.01, 0.9, 0.999, 3) - 0.01 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)) < 1e-18


def test_c_surface():
    from grapes_amd import _lib
    lib = _lib.load()
    for name in ("grapes_bag_batch", "grapes_bag_fwd", "grapes_bag_bwd", "grapes_bag_bwd_adam", "grapes_bag_batch_workspace_bytes",
                 "grapes_bag_fwd_workspace_bytes", "grapes_bag_bwd_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.grapes_abi_version() == 304
    assert lib.grapes_bag_batch_workspace_bytes(0, 8, 8) == 0 and lib.grapes_bag_batch_workspace_bytes(4, 8, 100) >= (4 + 5 + 24 + 4) * 4
    assert lib.grapes_bag_fwd_workspace_bytes(4097, 0, 8) == 0 and lib.grapes_bag_fwd_workspace_bytes(4, 10, 8) >= 10 * 8 * 4
    assert lib.grapes_bag_bwd_workspace_bytes(5, (1 << 22) + 1, 8) == 0 and lib.grapes_bag_bwd_workspace_bytes(5, 3, 8) >= 3 * 8 * 4
    # host-side refusals: no launch happens for these arguments
    assert lib.grapes_bag_batch(None, None, 10, None, 1, None, None, 4, 4, None, None, None, None, None, None, None, None) == -1
    assert lib.grapes_bag_fwd(None, None, 10, None, 1, None, 8, None, 8, None, 8, 0, None, None, None) == -1
    assert lib.grapes_bag_bwd(None, 8, 1, None, None, 1, 1, 8, None, 8, 0, None, None, None) == -1
    assert lib.grapes_bag_bwd_adam(None, 8, 1, None, None, None, 1, 1, 10, 8, None, 8, None, None, 8, 0.1, 0.001, 1e-8, 1e-3, 0, None,
                                   None, None) == -1


def test_command_line_parsing():
    from grapes_amd import linkx
    a = linkx.parse_args(["--dataset", "cora"])
    assert (a.hidden_dim, a.num_node_layers, a.num_final_layers, a.dropout, a.lr, a.bag_lr, a.bag_grad, a.batch_size) == \
        (256, 1, 2, 0.0, 1e-3, 1e-3, "fused", 512)
    a = linkx.parse_args(["--dataset", "cora", "--bag_grad", "sparse", "--bag_lr", "0.01", "--hidden_dim", "64", "--num_final_layers", "3"])
    assert (a.bag_grad, a.bag_lr, a.hidden_dim, a.num_final_layers) == ("sparse", 0.01, 64, 3)
    with pytest.raises(SystemExit):
        linkx.parse_args(["--dataset", "cora", "--bag_grad", "dense"])
    with pytest.raises(SystemExit):
        linkx.parse_args([])
    with pytest.raises(ValueError):
        linkx.parse_args(["--dataset", "cora", "--num_node_layers", "0"])
    with pytest.raises(ValueError):
        linkx.parse_args(["--dataset", "cora", "--hidden_dim", "1023"])
    with pytest.raises(ValueError):
        linkx.parse_args(["--dataset", "cora", "--num_layers", "2"])
    with pytest.raises(ValueError):
        linkx.parse_args(["--dataset", "cora", "--batch_size", "5000"])
