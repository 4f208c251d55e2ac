"""CPU checks of the GraphSAINT driver's flags, the loader's refusals and the numpy oracle of tests/saint_oracle.py."""
import numpy as np
import pytest

from tests import saint_oracle as O


def test_flag_defaults_match_graphsaint_py():
    from grapes_amd.graphsaint import parse_args
    a = parse_args(["--dataset", "cora"])
    assert (a.hidden_dim, a.runs, a.lr, a.max_epoch, a.embed_nodes, a.node_emb_dim) == (256, 1, 0.01, 50, False, 64)
    assert (a.batch_size, a.walk_length, a.num_steps, a.engine, a.large_graph, a.e_cap) == (256, 2, 1, "graph", "auto", None)
    assert a.use_normalization is False


def test_embed_nodes_false_is_false_and_use_normalization_accepted():
    from grapes_amd.graphsaint import parse_args
    assert parse_args(["--dataset", "cora", "--embed_nodes", "False"]).embed_nodes is False
    assert parse_args(["--dataset", "cora", "--embed_nodes", "True"]).embed_nodes is True
    assert parse_args(["--dataset", "cora", "--use_normalization"]).use_normalization is True


def test_sample_coverage_is_refused():
    from grapes_amd.modules.saint import GraphSAINTRandomWalkSampler
    with pytest.raises(NotImplementedError):
        GraphSAINTRandomWalkSampler(object(), batch_size=4, walk_length=2, sample_coverage=100)


# 6 nodes: 0 <-> 1, 1 <-> 2, 2 -> 3 (directed), 3 has a stored self-loop, 4 -> 3, 5 isolated
ROWPTR = np.array([0, 1, 3, 5, 6, 7, 7])
COL = np.array([1, 0, 2, 1, 3, 3, 3])


def test_oracle_walk_by_hand():
    roots = [0, 5, 2, 3, 4]
    u = np.array([[0.0, 0.75], [0.5, 0.5], [0.5, 0.0], [0.9, 0.1], [0.2, 0.99]], dtype=np.float32)
    w = O.walk(ROWPTR, COL, roots, u, 2)
    # 0 -> 1 (deg 1); 1: deg 2, u .75 -> index 1 -> 2
    # 5 isolated: stays;  2: deg 2, u .5 -> index 1 -> 3; 3: self-loop -> 3
    # 3 -> 3 -> 3;  4 -> 3 -> 3
    assert w.tolist() == [[0, 1, 2], [5, 5, 5], [2, 3, 3], [3, 3, 3], [4, 3, 3]]
    assert O.node_set(w).tolist() == [0, 1, 2, 3, 4, 5]


def test_oracle_induced_subgraph_by_hand():
    src, dst = O.induced_subgraph(ROWPTR, COL, np.array([1, 2, 3, 5]))
    # local ids: 1->0, 2->1, 3->2, 5->3; row 1: (1,0)x (1,2) ; row 2: (2,1) (2,3); row 3: (3,3); row 5: none
    assert list(zip(src.tolist(), dst.tolist())) == [(0, 1), (1, 0), (1, 2), (2, 2)]


def test_oracle_long_row_stays_in_range():
    """Rows past 2^24 entries: fp32(deg) may round up, but at the largest 24-bit uniform u = 1 - 2^-24 the fp32 product still
    truncates below deg (it rounds to at most fp32(deg) - ulp), so the deg - 1 clamp is a guard that does not fire there."""
    u = np.float32(1.0 - 2.0 ** -24)
    for deg in (2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 5, 2 ** 31 + 7):
        k = int(u * np.float32(deg))
        assert deg - 1 - k <= 2 ** (int(np.log2(deg)) - 23) and k <= deg - 1
    deg = 2 ** 24 + 3
    rowptr = np.array([0, deg])
    col = np.arange(deg, dtype=np.int64) % 7
    assert O.walk(rowptr, col, [0], [[u]], 1)[0, 1] == col[min(int(u * np.float32(deg)), deg - 1)]
