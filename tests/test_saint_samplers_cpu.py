"""CPU checks of the GraphSAINT node and edge samplers: the numpy oracle of tests/saint_samplers_oracle.py on hand-sized graphs,
the constructors' refusals, the driver's --sampler flag and the C-ABI tables for the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import portable_math as pm
from tests import saint_samplers_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# directed, 6 nodes: 0 <-> 1, 1 <-> 2, 2 -> 3, 3 has a stored self-loop, 4 -> 3, 5 isolated (an empty row)
ROWPTR = np.array([0, 1, 3, 5, 6, 7, 7])
COL = np.array([1, 0, 2, 1, 3, 3, 3])
# colcount = [1, 2, 1, 3, 0, 0], rowcount = [1, 2, 2, 1, 1, 0]
# entries (r, c): (0,1) (1,0) (1,2) (2,1) (2,3) (3,3) (4,3);  w = colcount[r] + rowcount[c]
W_HAND = [1 + 2, 2 + 1, 2 + 2, 1 + 2, 1 + 1, 3 + 1, 0 + 1]


def _csr(src, dst, n):
    order = np.lexsort((dst, src))
    src, dst = np.asarray(src)[order], np.asarray(dst)[order]
    keep = np.ones(len(src), bool)
    keep[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    src, dst = src[keep], dst[keep]
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, src + 1, 1)
    return np.cumsum(indptr), dst.astype(np.int64)


def _long_row_graph(symmetric):
    """Node 0 stores 150 entries (three 64-entry blocks: 64 + 64 + 22), among them a self-loop; node 200 is isolated."""
    n = 201
    s = [0] * 150
    d = list(range(0, 150))
    s += [160, 161, 161, 170]
    d += [161, 160, 162, 3]
    if symmetric:
        s, d = s + d, d + s
    return _csr(np.array(s), np.array(d), n)


def test_philox_words_agree_with_the_shared_restatement():
    for seed, off, n in ((0, 0, 8), (77, 5, 1001), (2 ** 63 + 12345, 2 ** 33 + 7, 64)):
        w = S.philox_words(seed, off, n)
        assert w.dtype == np.uint32 and len(w) == n
        assert np.array_equal((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), pm.philox_uniform(seed, off, n))
    # word i of (seed, off) is word i - 4 of (seed, off + 1)
    assert np.array_equal(S.philox_words(9, 3, 12)[4:], S.philox_words(9, 4, 8))


def test_draw_values_are_mulhi64():
    w = S.philox_words(5, 2, 6)
    for total in (1, 7, 2 ** 31 + 11, 2 ** 40 + 3):
        t = S.draw_values(5, 2, 3, total)
        for b in range(3):
            word = (int(w[2 * b]) << 32) | int(w[2 * b + 1])
            assert int(t[b]) == (word * total) >> 64 and 0 <= int(t[b]) < total
    assert [S.offset_advance(B) for B in (1, 2, 3, 4, 256, 257)] == [1, 1, 2, 2, 128, 129]


def test_weights_by_hand():
    assert S.colcount(COL, 6).tolist() == [1, 2, 1, 3, 0, 0]
    assert S.entry_rows(ROWPTR).tolist() == [0, 1, 1, 2, 2, 3, 4]
    assert S.entry_weights(ROWPTR, COL).tolist() == W_HAND
    cc, blockw, roww = S.weight_table(ROWPTR, COL)
    assert cc.dtype == np.int32 and cc.tolist() == [1, 2, 1, 3, 0, 0]
    assert roww.tolist() == [0, 3, 10, 15, 19, 20, 20]
    # every row has one block; row r's slot is (rowptr[r] >> 6) + r = r; the empty row 5 owns none
    assert blockw.tolist() == [3, 7, 5, 4, 1, 0]


def test_symmetric_graph_weight_is_degree_sum():
    indptr, indices = _long_row_graph(True)
    deg = np.diff(indptr)
    assert np.array_equal(S.colcount(indices, len(deg)), deg)
    assert np.array_equal(S.entry_weights(indptr, indices), deg[S.entry_rows(indptr)] + deg[indices])


def test_node_draw_by_hand():
    t = np.arange(7)
    e, ids = S.node_draw(ROWPTR, t)
    assert e.tolist() == list(range(7)) and ids.tolist() == [0, 1, 1, 2, 2, 3, 4]      # the empty row 5 is never drawn
    # an empty row in the middle
    e, ids = S.node_draw(np.array([0, 2, 2, 2, 5]), np.arange(5))
    assert ids.tolist() == [0, 0, 3, 3, 3]


def test_edge_draw_by_hand_and_boundaries():
    cum = np.cumsum(W_HAND)                               # 3 6 10 13 15 19 20
    total = int(cum[-1])
    t = np.arange(total)
    e, ids = S.edge_draw(ROWPTR, COL, t)
    assert e.tolist() == sum(([i] * w for i, w in enumerate(W_HAND)), [])
    assert e[0] == 0 and e[total - 1] == 6
    for i in range(7):                                    # each entry's first and last value
        lo = int(cum[i]) - W_HAND[i]
        assert e[lo] == i and e[int(cum[i]) - 1] == i and (lo == 0 or e[lo - 1] == i - 1)
    rows, cols = S.entry_rows(ROWPTR), COL
    assert ids.reshape(-1, 2).tolist() == [[int(rows[i]), int(cols[i])] for i in e]
    table = S.weight_table(ROWPTR, COL)
    assert [S.edge_entry_by_table(ROWPTR, COL, table, int(v)) for v in t] == e.tolist()


def test_zero_weight_entries_are_never_drawn():
    # 0 -> 1, 0 -> 2, 2 -> 0: entry (0, 1) has colcount[0] = 1; entry (2, 0): colcount[2] + rowcount[0] = 1 + 2.
    # 3 -> 4: colcount[3] = 0 and rowcount[4] = 0: weight 0
    indptr, indices = _csr(np.array([0, 0, 2, 3]), np.array([1, 2, 0, 4]), 5)
    w = S.entry_weights(indptr, indices)
    assert w.tolist() == [1 + 0, 1 + 1, 1 + 2, 0]
    total = int(w.sum())
    e, ids = S.edge_draw(indptr, indices, np.arange(total))
    assert 3 not in e.tolist() and set(e.tolist()) == {0, 1, 2}
    assert np.bincount(e, minlength=4).tolist() == w.tolist()
    # a zero-weight entry in front of and between positive ones
    indptr, indices = _csr(np.array([3, 0, 0, 2]), np.array([4, 1, 2, 0]), 5)       # CSR order: (0,1) (0,2) (2,0) (3,4)
    indptr2, indices2 = _csr(np.array([0, 1, 1, 3]), np.array([4, 2, 3, 1]), 5)     # (0,4): weight 0 comes first
    w2 = S.entry_weights(indptr2, indices2)
    assert w2[0] == 0 and w2.sum() > 0
    e2, _ = S.edge_draw(indptr2, indices2, np.arange(int(w2.sum())))
    assert np.bincount(e2, minlength=4).tolist() == w2.tolist()
    # only weight-0 entries: total 0
    indptr3, indices3 = _csr(np.array([0]), np.array([1]), 2)
    assert S.entry_weights(indptr3, indices3).sum() == 0 and S.weight_table(indptr3, indices3)[2][-1] == 0


@pytest.mark.parametrize("symmetric", [False, True])
def test_long_row_every_block_and_every_boundary(symmetric):
    indptr, indices = _long_row_graph(symmetric)
    n = len(indptr) - 1
    assert indptr[1] - indptr[0] == 150 and 0 in indices[indptr[0]:indptr[1]]            # three blocks, a stored self-loop
    assert indptr[201] == indptr[200]                                                       # an empty row
    w = S.entry_weights(indptr, indices)
    cc, blockw, roww = table = S.weight_table(indptr, indices)
    assert len(blockw) == (len(indices) >> 6) + n
    # node 0's slots: 0, 1, 2; its blocks' prefixes
    assert blockw[:3].tolist() == [int(w[:64].sum()), int(w[:128].sum()), int(w[:150].sum())]
    assert roww[1] == blockw[2] and roww[-1] == w.sum()
    assert np.diff(roww).tolist() == [int(w[indptr[r]:indptr[r + 1]].sum()) for r in range(n)]
    cum = np.cumsum(w)
    total = int(cum[-1])
    # t = 0, t = total - 1, and both sides of every entry boundary inside the long row (so: of every block boundary) and beyond
    pos = w > 0
    firsts = (cum - w)[pos]
    t = np.unique(np.concatenate([[0, total - 1], firsts, cum[pos] - 1]))
    e, ids = S.edge_draw(indptr, indices, t)
    assert np.all(w[e] > 0) and np.all(cum[e] > t) and np.all(cum[e] - w[e] <= t)
    assert {0, 63, 64, 127, 128, 149} <= set(e.tolist())                                     # the chosen entry in each block
    assert [S.edge_entry_by_table(indptr, indices, table, int(v)) for v in t] == e.tolist()
    rows = S.entry_rows(indptr)
    assert np.array_equal(ids.reshape(-1, 2), np.stack([rows[e], indices[e]], 1))
    # the node sampler on the same graph
    en, idn = S.node_draw(indptr, np.arange(len(indices)))
    assert np.array_equal(idn, rows)
    # node set and induced subgraph of an edge batch
    ns = S.node_set(ids[:16])
    assert np.array_equal(ns, np.unique(ids[:16]))
    src, dst = S.induced_subgraph(indptr, indices, ns)
    got = set(zip(ns[src].tolist(), ns[dst].tolist()))
    assert got == {(int(r), int(c)) for r, c in zip(rows, indices) if r in set(ns.tolist()) and c in set(ns.tolist())}


def test_import_and_refusals():
    from grapes_amd import ops
    from grapes_amd.modules.saint import (GraphSAINTEdgeSampler, GraphSAINTNodeSampler, GraphSAINTRandomWalkSampler,
                                          _SaintSampler, make_sampler)
    for cls in (GraphSAINTNodeSampler, GraphSAINTEdgeSampler, GraphSAINTRandomWalkSampler):
        assert issubclass(cls, _SaintSampler)
    for cls in (GraphSAINTNodeSampler, GraphSAINTEdgeSampler):
        with pytest.raises(NotImplementedError):
            cls(object(), batch_size=4, sample_coverage=100)
        with pytest.raises(TypeError):
            cls(object(), batch_size=4, walk_length=2)                        # there is no walk_length
    with pytest.raises(ValueError):
        GraphSAINTNodeSampler(object(), batch_size=ops.SAINT_MAX_IDS + 1)
    with pytest.raises(ValueError):
        GraphSAINTEdgeSampler(object(), batch_size=ops.SAINT_MAX_IDS // 2 + 1)
    with pytest.raises(ValueError):
        make_sampler("walk", object(), 4)
    with pytest.raises(NotImplementedError):
        make_sampler("edge", object(), 4, sample_coverage=1)


def test_graph_without_entries_is_refused():
    """Total weight 0 where it needs no GPU: a graph without a stored entry (a DeviceGraph shell on host tensors)."""
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.saint import GraphSAINTEdgeSampler, GraphSAINTNodeSampler
    g = DeviceGraph.__new__(DeviceGraph)
    g.rowptr, g.col, g.num_nodes, g.device = torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 3, torch.device("cpu")
    for cls in (GraphSAINTEdgeSampler, GraphSAINTNodeSampler):
        with pytest.raises(ValueError):
            cls(g, batch_size=4)


def test_cli_sampler_flag():
    from grapes_amd.graphsaint import parse_args
    assert parse_args(["--dataset", "cora"]).sampler == "rw"
    for k in ("rw", "node", "edge"):
        assert parse_args(["--dataset", "cora", "--sampler", k]).sampler == k
    with pytest.raises(SystemExit):
        parse_args(["--dataset", "cora", "--sampler", "walk"])


def test_header_and_ctypes_tables_agree_for_the_new_entry_points():
    from grapes_amd import _lib
    src = open(os.path.join(ROOT, "include", "grapes_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("grapes_saint_edge_weights", "grapes_saint_draw_nodes"):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert "#define GRAPES_ABI_VERSION 304" in src
