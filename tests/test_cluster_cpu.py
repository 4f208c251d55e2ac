"""Cluster-GCN without a GPU: tests/cluster_oracle.py against brute force — the batch against a dense-mask induced subgraph, the conv
against a dense closed form under torch fp64 autograd — the partition tables of modules/cluster.py, the command line, and the
refusal of host tensors."""
import os

import numpy as np
import pytest
import torch

from tests import cluster_oracle as CO

F64 = np.float64
ENTRY_POINTS = ("grapes_cluster_batch", "grapes_cluster_batch_workspace_bytes", "grapes_rootsum_aggregate_fwd",
                "grapes_rootsum_aggregate_bwd", "grapes_rootsum_aggregate_workspace_bytes")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    from grapes_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.DIAG_LIB_PATH):
        ge.build()
    return _lib


def test_both_libraries_carry_the_entry_points_and_the_abi_stays(built_lib):
    import ctypes
    prod, diag = ctypes.CDLL(built_lib.LIB_PATH), ctypes.CDLL(built_lib.DIAG_LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in built_lib.SIGNATURES and hasattr(prod, name) and hasattr(diag, name)
    lib = built_lib.load()
    assert lib.grapes_abi_version() == 304
    assert lib.grapes_cluster_batch_workspace_bytes(2000, 500) > lib.grapes_cluster_batch_workspace_bytes(1000, 500) >= 1001 * 4 + 500 * 16


def _graphs():
    star = CO.csr([list(range(1, 301))] + [[0] for _ in range(300)])
    return {
        "path": (CO.csr([[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]), [0, 1, 0, 2, 1, 2], 3),
        "dups_loops": (CO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0]]), [1, 0, 1, 3], 4),     # cluster 2 is empty
        "star": (star, (np.arange(301) * 7 // 301).tolist(), 7),
        "random": (CO.random_graph(200, 6, 3, hub=11, hub_degree=500), np.random.default_rng(4).integers(0, 9, 200).tolist(), 9),
    }


@pytest.mark.parametrize("name", list(_graphs()))
def test_oracle_batch_against_the_dense_mask(name):
    (ip, ix), part, P = _graphs()[name]
    rng = np.random.default_rng(5)
    lists = [[0], list(range(P)), list(range(P))[::-1], rng.permutation(P)[:max(P // 2, 1)].tolist()]
    for clusters in lists:
        b = CO.batch(ip, ix, part, P, clusters)
        node_idx, ei, eid = CO.dense_batch(ip, ix, part, clusters)
        assert b.status == 0 and b.n == len(node_idx) and b.e == len(eid)
        assert np.array_equal(b.node_idx, node_idx) and np.array_equal(b.edge_index, ei) and np.array_equal(b.e_id, eid)
        assert np.array_equal(b.rowptr, np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=b.n))]))
        assert np.array_equal(ix[b.e_id], b.node_idx[b.edge_index[0]])               # row 0 holds the neighbours
        assert np.array_equal(np.diff(b.cptr), [list(part).count(c) for c in clusters])


@pytest.mark.parametrize("name", list(_graphs()))
def test_all_clusters_in_one_batch_give_every_entry_once(name):
    (ip, ix), part, P = _graphs()[name]
    for clusters in (list(range(P)), list(range(P))[::-1]):
        b = CO.batch(ip, ix, part, P, clusters)
        assert b.n == len(ip) - 1 and b.e == len(ix) and b.walked == len(ix)
        assert np.array_equal(np.sort(b.e_id), np.arange(len(ix)))
        assert np.array_equal(np.sort(b.node_idx), np.arange(len(ip) - 1))


def test_oracle_overflow_and_bad_id_outcomes():
    (ip, ix), part, P = _graphs()["random"]
    full = CO.batch(ip, ix, part, P, [1, 4, 6])
    cut = CO.batch(ip, ix, part, P, [1, 4, 6], e_cap=full.e - 1)
    assert cut.status == CO.EDGE and cut.e == full.e - 1 and cut.n == full.n
    assert np.array_equal(cut.edge_index, full.edge_index[:, :-1]) and cut.rowptr[-1] == cut.e
    over = CO.batch(ip, ix, part, P, [1, 4, 6], n_cap=full.n - 1)
    assert over.status == CO.NODE and over.n == 0 and over.e == 0 and not over.cptr.any() and not over.rowptr_full.any()
    for bad in ([1, -1], [1, P], [1, 4, 1]):
        b = CO.batch(ip, ix, part, P, bad)
        assert b.status == CO.BAD and b.n == 0 and b.e == 0 and not b.cptr.any()
    few = CO.batch(ip, ix, part, P, [1, 4, 6], item_cap=3)
    assert few.status == CO.EDGE and few.e < full.e and np.array_equal(few.edge_index, full.edge_index[:, :few.e])


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_conv_oracle_against_the_dense_closed_form(lam):
    rng = np.random.default_rng(8)
    n, fi, fo = 23, 5, 4
    ei = np.array([rng.integers(0, n, 90), rng.integers(0, n, 90)])
    ei[:, :4] = [[3, 3, 7, 7], [3, 3, 9, 9]]                                         # a loop stored twice, a duplicate entry
    ei[1][ei[1] == 0] = 1                                                            # node 0: no incoming entry
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=F64))
    x, wo, b, wr, g = (rng.standard_normal(s) for s in ((n, fi), (fo, fi), (fo,), (fo, fi), (n, fo)))
    leaves = [t(a).requires_grad_(True) for a in (x, wo, b, wr)]
    dense = CO.dense_conv64(leaves[0], ei, leaves[1], leaves[2], leaves[3], lam)
    (dense * t(g)).sum().backward()
    out = CO.conv64(t(x), ei, t(wo), t(b), t(wr), lam).numpy()
    assert np.abs(out - dense.detach().numpy()).max() <= 1e-12
    for got, leaf in zip(CO.conv_backward64(x, ei, wo, wr, lam, g), (leaves[0], leaves[1], leaves[2], leaves[3])):
        assert np.abs(got - leaf.grad.numpy()).max() <= 1e-11
    relu = CO.conv64(t(x), ei, t(wo), t(b), t(wr), lam, relu=True).numpy()
    assert np.array_equal(relu, np.maximum(out, 0)) and (relu == 0).any()
    assert np.array_equal(CO.degrees(ei, n)[[0, 3]], [1.0, 1.0 + ((ei[1] == 3) & (ei[0] != 3)).sum()])


# ---------------------------------------------------------------------------------------------------- the partition tables
def _valid_tables(part, P):
    from grapes_amd.modules.cluster import partition_tables
    perm, partptr, where = (a.numpy() for a in partition_tables(torch.as_tensor(part), P))
    operm, optr, owhere = CO.partition_tables(part, P)
    assert perm.dtype == np.int32 and partptr.dtype == np.int32 and where.dtype == np.int32 and where.shape == (len(part), 2)
    assert np.array_equal(perm, operm) and np.array_equal(partptr, optr) and np.array_equal(where, owhere)
    assert np.array_equal(np.sort(perm), np.arange(len(part)))                       # a permutation
    assert np.array_equal(perm[partptr[where[:, 0]] + where[:, 1]], np.arange(len(part)))
    for c in range(P):
        assert (np.diff(perm[partptr[c]:partptr[c + 1]]) > 0).all()                  # ascending id inside a cluster
    return partptr


def test_random_partitions_are_balanced_and_seeded():
    from grapes_amd.modules.cluster import make_partition
    for N, P in ((1000, 37), (37, 37), (50, 1), (101, 10)):
        a, b, c = make_partition(N, P, "random", 5), make_partition(N, P, "random", 5), make_partition(N, P, "random", 6)
        sizes = np.diff(_valid_tables(a.numpy(), P))
        assert sizes.max() - sizes.min() <= 1 and sizes.sum() == N
        assert torch.equal(a, b) and (P == 1 or not torch.equal(a, c))


def test_range_and_given_partitions_are_valid():
    from grapes_amd.modules.cluster import make_partition, partition_tables
    for N, P in ((1000, 37), (10, 3), (7, 7)):
        part = make_partition(N, P, "range")
        assert np.array_equal(part.numpy(), CO.range_partition(N, P)) and (np.diff(part.numpy()) >= 0).all()
        sizes = np.diff(_valid_tables(part.numpy(), P))
        assert sizes.max() - sizes.min() <= 1
    given = np.random.default_rng(2).integers(0, 6, 80)
    given[given == 4] = 5                                                            # cluster 4 is empty
    ptr = _valid_tables(given, 6)
    assert ptr[5] == ptr[4]
    for bad in ([0, 1, 6], [0, -1, 2]):
        with pytest.raises(ValueError, match=r"cluster id outside \[0, 6\)"):
            partition_tables(torch.tensor(bad), 6)
    with pytest.raises(ValueError, match="integer tensor"):
        partition_tables(torch.zeros(4), 2)
    with pytest.raises(ValueError, match="not built"):
        make_partition(10, 2, "metis")
    with pytest.raises(ValueError, match="num_parts is 1 .. num_nodes"):
        make_partition(10, 11, "range")


# ---------------------------------------------------------------------------------------------------- the command line
_DEFAULTS = dict(dataset="cora", num_parts=32, batch_size=4, partition="random", partition_file=None, diag_lambda=0.0, hidden_dim=256,
                 num_layers=2, lr=1e-3, max_epoch=100, eval_frequency=1, dropout=0.0, runs=1, seed=None)
_SET_ARGV = ["--dataset", "reddit", "--num_parts", "1500", "--batch_size", "20", "--partition", "file", "--partition_file", "p.npy",
             "--diag_lambda", "0.25", "--hidden_dim", "128", "--num_layers", "3", "--lr", "0.005", "--max_epoch", "30",
             "--eval_frequency", "5", "--dropout", "0.5", "--runs", "3", "--seed", "7"]
_SET = dict(dataset="reddit", num_parts=1500, batch_size=20, partition="file", partition_file="p.npy", diag_lambda=0.25, hidden_dim=128,
            num_layers=3, lr=0.005, max_epoch=30, eval_frequency=5, dropout=0.5, runs=3, seed=7)


@pytest.mark.parametrize("argv,want", [(["--dataset", "cora"], _DEFAULTS), (_SET_ARGV, _SET)], ids=["defaults", "set"])
def test_parsed_namespace(argv, want):
    from grapes_amd import clustergcn
    got = vars(clustergcn.parse_args(argv))
    assert got == want
    assert all(type(got[k]) is type(want[k]) for k in want)


_AT_LEAST = "--num_parts, --batch_size, --hidden_dim, --num_layers and --eval_frequency are at least 1"
_FILE = "--partition file goes with --partition_file x.npy, and --partition_file with --partition file"


@pytest.mark.parametrize("argv,exc,message", [
    ([], SystemExit, "--dataset is required"),
    (["--dataset", "cora", "--num_parts", "0"], ValueError, _AT_LEAST),
    (["--dataset", "cora", "--num_layers", "0"], ValueError, _AT_LEAST),
    (["--dataset", "cora", "--num_parts", "8", "--batch_size", "9"], ValueError, "--batch_size counts clusters: at most --num_parts (8)"),
    (["--dataset", "cora", "--partition", "file"], ValueError, _FILE),
    (["--dataset", "cora", "--partition", "range", "--partition_file", "p.npy"], ValueError, _FILE),
])
def test_refusals(argv, exc, message):
    from grapes_amd import clustergcn
    with pytest.raises(exc) as e:
        clustergcn.parse_args(argv)
    assert str(e.value) == message


def test_unknown_flags_and_partition_files(tmp_path):
    from grapes_amd import clustergcn
    with pytest.raises(SystemExit):
        clustergcn.parse_args(["--dataset", "cora", "--partition", "metis"])
    with pytest.raises(SystemExit):
        clustergcn.parse_args(["--dataset", "cora", "--fanouts", "5,5"])
    np.save(tmp_path / "p.npy", np.array([0, 2, 1], dtype=np.int32))
    assert clustergcn.load_partition(str(tmp_path / "p.npy")).tolist() == [0, 2, 1]
    np.save(tmp_path / "f.npy", np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="an integer array"):
        clustergcn.load_partition(str(tmp_path / "f.npy"))


def test_host_tensors_are_refused(built_lib):
    from grapes_amd import ops
    from grapes_amd.modules.gcn import ClusterGCN, ClusterGCNConv
    i32 = torch.int32
    rowptr, col = torch.tensor([0, 2, 3, 3]), torch.tensor([1, 2, 0], dtype=i32)
    perm, partptr = torch.tensor([0, 1, 2], dtype=i32), torch.tensor([0, 2, 3], dtype=i32)
    where, stamp = torch.tensor([[0, 0], [0, 1], [1, 0]], dtype=i32), torch.zeros((2, 2), dtype=i32)
    with pytest.raises(built_lib.GrapesHipError):
        ops.cluster_batch(rowptr, col, 3, perm, partptr, where, torch.tensor([0], dtype=i32), stamp, 1, 3, 8)
    with pytest.raises(built_lib.GrapesHipError):
        ops.cluster_aggregate_fwd(torch.zeros(3, 4), None)
    with pytest.raises(built_lib.GrapesHipError):
        ops.cluster_aggregate_bwd(torch.zeros(3, 4), None)
    with pytest.raises(built_lib.GrapesHipError):
        ClusterGCNConv(4, 4)(torch.zeros(3, 4), torch.zeros((2, 0), dtype=torch.int64))
    with pytest.raises(built_lib.GrapesHipError):
        ClusterGCN(4, [4, 2])(torch.zeros(3, 4), torch.zeros((2, 0), dtype=torch.int64))
    assert ops.CLUSTER_MAX_BATCH_PARTS >= 8192


def test_layers_refuse_what_is_not_built():
    from grapes_amd.modules.gcn import ClusterGCN, ClusterGCNConv
    with pytest.raises(NotImplementedError, match="add_self_loops=False is not built"):
        ClusterGCNConv(8, 8, add_self_loops=False)
    with pytest.raises(ValueError, match="is not built"):
        ClusterGCNConv(258, 258)
    conv = ClusterGCNConv(100, 256, diag_lambda=0.5)
    assert sorted(conv.state_dict()) == ["lin_out.bias", "lin_out.weight", "lin_root.weight"]
    assert conv.default_form() == "aggregate" and ClusterGCNConv(256, 100).default_form() == "transform"
    assert sorted(ClusterGCNConv(8, 4, bias=False).state_dict()) == ["lin_out.weight", "lin_root.weight"]
    m = ClusterGCN(8, [16, 4], diag_lambda=0.25)
    assert len(m.convs) == 2 and all(c.diag_lambda == 0.25 for c in m.convs)
    assert sorted(m.state_dict())[:3] == ["convs.0.lin_out.bias", "convs.0.lin_out.weight", "convs.0.lin_root.weight"]
