"""ShaDow-GNN without a GPU: the C surface, the host oracle (tests/shadow_oracle.py) against the definitions it restates — the wide
Philox against the 64-bit-counter one, Floyd's rule by exact enumeration, the ego-net against a breadth-first ball — and the driver's
arguments and refusals."""
import ctypes
import itertools
import os
import re
from collections import Counter, deque

import numpy as np
import pytest
import torch

from tests import labor_oracle as LO
from tests import shadow_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"grapes_shadow_sample": 26, "grapes_shadow_sample_workspace_bytes": 3, "grapes_segment_mean_fwd": 8,
                "grapes_segment_mean_bwd": 8}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    from grapes_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.DIAG_LIB_PATH):
        ge.build()
    return _lib


def test_header_table_makefile_and_both_libraries_carry_the_entry_points(built_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grapes_hip.h")).read(), flags=re.S)
    prod, diag = ctypes.CDLL(built_lib.LIB_PATH), ctypes.CDLL(built_lib.DIAG_LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in grapes_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert name in built_lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert len(built_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(prod, name) and hasattr(diag, name), f"{name} is not exported"
    assert built_lib.load().grapes_abi_version() == 304
    makefile = open(os.path.join(ROOT, "grapes_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS := (.*)$", makefile, flags=re.M).group(1).split()
    assert "build/shadow_kernels.o" in objs


def test_workspace_and_argument_checks_are_host_calls(built_lib):
    """The cap is checked before any launch and needs no device."""
    from grapes_amd import ops
    lib = built_lib.load()
    wb = lib.grapes_shadow_sample_workspace_bytes
    assert wb(4, 2, 10) >= (2 * 4 * 111 + 3 * 4 + 1) * 4 and wb(4, 2, 10) < wb(400, 2, 10) < wb(400, 2, 25)
    assert wb(4, 2, 32) == 0 and wb(4, 2, 31) > 0 and wb(4, 1, 65) == 0 and wb(4, 0, 5) == 0 and wb(4097, 1, 5) == 0
    one = ctypes.c_void_p(16)                                            # a non-NULL aligned address that is never read

    def call(m=4, depth=2, fanout=10, n_cap=8, e_cap=8, ws=one):
        return lib.grapes_shadow_sample(one, one, 10, one, m, None, depth, fanout, None, 0, 0, None, n_cap, e_cap, one, one, one, one,
                                        one, one, None, one, one, ws, None, None)
    assert call(depth=2, fanout=32) == -1                                # C = 1057
    assert call(fanout=65, depth=1) == -1 and call(fanout=-1) == -1 and call(fanout=0) == -1 and call(depth=0) == -1
    assert call(m=0) == -1 and call(m=4097) == -1 and call(n_cap=0) == -1 and call(e_cap=0) == -1
    assert call(ws=ctypes.c_void_p(18)) == -2
    assert lib.grapes_segment_mean_fwd(one, one, 3, 10, 1025, one, None, None) == -1
    assert lib.grapes_segment_mean_bwd(one, one, 0, 10, 8, one, None, None) == -1
    assert ops.shadow_cap(2, 10) == 111 and ops.shadow_cap(2, 31) == 993 and ops.shadow_cap(1, 64) == 65 and ops.shadow_cap(3, 5) == 156
    for depth, k in ((2, 32), (1, 65), (2, -1), (0, 3), (11, 2)):
        with pytest.raises(ValueError):
            ops.shadow_cap(depth, k)


# ---------------------------------------------------------------------------------------------------- Philox and Floyd's rule
def test_the_wide_philox_with_a_zero_high_half_is_the_64_bit_counter_one():
    for seed, ctr in ((0, 0), (12345678901234, 17), (2 ** 63 + 5, 2 ** 33 + 1), (2 ** 64 - 1, 2 ** 64 - 1)):
        assert SO.philox4x32_10_wide(ctr, 0, seed) == [int(w) for w in LO.philox4x32_10([ctr], seed)[0]]
    a, b = SO.philox4x32_10_wide(5, 0, 9), SO.philox4x32_10_wide(5, 1, 9)
    assert a != b and SO.philox4x32_10_wide(5, 1 << 32, 9) not in (a, b)       # both halves of the high word reach the output
    # the words of a row: word s & 3 of the call at (v << 4) | (s >> 2), high half off + b depth + h - 1
    w = SO.row_words(7, 100, 3, 2, 2, 41, 10)
    assert w[6] == SO.philox4x32_10_wide((41 << 4) | 1, 100 + 3 * 2 + 1, 7)[2] and len(w) == 10


def test_floyds_rule_is_uniform_by_exact_enumeration():
    """d = 6, k = 3: over every (t_0, t_1, t_2) in [0..3] x [0..4] x [0..5] — each t_s reached through a word that maps to it — each of
    the 20 subsets appears exactly 6 times."""
    d, k = 6, 3
    seen = Counter()
    for ts in itertools.product(range(4), range(5), range(6)):
        words = [-((-t << 32) // (d - k + s + 1)) for s, t in enumerate(ts)]      # the smallest word with (w (j + 1)) >> 32 == t
        assert all(0 <= w < 2 ** 32 and (w * (d - k + s + 1)) >> 32 == t for s, (w, t) in enumerate(zip(words, ts)))
        seen[frozenset(SO.floyd(d, k, words))] += 1
    assert len(seen) == 20 and set(seen.values()) == {6}
    # all zeros: the collision branch at every step but the first
    assert SO.floyd(300, 5, [0] * 5) == {0, 296, 297, 298, 299}
    assert SO.floyd(300, 1, [2 ** 32 - 1]) == {299}


def _bfs_ball(indptr, indices, root, depth):
    dist, q = {root: 0}, deque([root])
    while q:
        v = q.popleft()
        if dist[v] == depth:
            continue
        for c in indices[indptr[v]:indptr[v + 1]]:
            if int(c) not in dist:
                dist[int(c)] = dist[v] + 1
                q.append(int(c))
    return sorted(dist)


def test_with_the_fanout_at_the_maximum_degree_the_ego_net_is_the_exact_ball():
    ip, ix = SO.random_graph(60, 3, 5)
    k = int(np.diff(ip).max())
    assert 1 <= k <= 6
    roots = [0, 17, 59, 17]
    for depth in (1, 2, 3):
        ob = SO.sample(ip, ix, roots, depth, k, seed=3)
        assert ob.philox_offset == len(roots) * depth and not ob.bad_index
        for b, root in enumerate(roots):
            members = ob.n_id[ob.ptr[b]:ob.ptr[b + 1]].tolist()
            assert members == _bfs_ball(ip, ix, root, depth)
            assert ob.n_id[ob.root_n_id[b]] == root and (ob.batch[ob.ptr[b]:ob.ptr[b + 1]] == b).all()
            # the induced entries: every stored entry between two members, in order
            want = [(u, int(c), p) for u in members for p, c in zip(range(ip[u], ip[u + 1]), ix[ip[u]:ip[u + 1]]) if int(c) in members]
            sel = (ob.edge_index[1] >= ob.ptr[b]) & (ob.edge_index[1] < ob.ptr[b + 1])
            got = [(int(ob.n_id[d]), int(ob.n_id[s]), int(p)) for s, d, p in zip(ob.edge_index[0][sel], ob.edge_index[1][sel], ob.e_id[sel])]
            assert got == want
        assert np.array_equal(ix[ob.e_id], ob.n_id[ob.edge_index[0]])
    bad = SO.sample(ip, ix, [3, 60, -1], 1, 2)
    assert bad.bad_index and bad.root_n_id.tolist()[1:] == [-1, -1] and bad.ptr[1] == bad.ptr[2] == bad.ptr[3]


def test_segment_mean_oracle():
    h = np.arange(12, dtype=np.float64).reshape(6, 2)
    ptr = [0, 0, 1, 4, 6]
    assert np.array_equal(SO.segment_mean64(h, ptr), [[0, 0], [0, 1], [4, 5], [9, 10]])
    g = np.array([[9., 9.], [1., 2.], [3., 6.], [4., 8.]])
    assert np.array_equal(SO.segment_mean_bwd64(g, ptr, 6), [[1, 2], [1, 2], [1, 2], [1, 2], [2, 4], [2, 4]])


# ---------------------------------------------------------------------------------------------------- the driver
_DEFAULTS = {'dataset': 'cora', 'batch_size': 512, 'hidden_dim': 256, 'num_layers': 3, 'lr': 0.001, 'max_epoch': 100,
             'eval_frequency': 1, 'dropout': 0.0, 'runs': 1, 'seed': None, 'depth': 2, 'num_neighbors': 10, 'conv': 'sage', 'pool': True}
_SET_ARGV = ["--dataset", "arxiv", "--batch_size", "128", "--hidden_dim", "64", "--num_layers", "5", "--lr", "0.01", "--max_epoch", "5",
             "--eval_frequency", "2", "--dropout", "0.1", "--runs", "2", "--seed", "7", "--depth", "3", "--num_neighbors", "5",
             "--conv", "gcn", "--pool", "false"]
_SET = {'dataset': 'arxiv', 'batch_size': 128, 'hidden_dim': 64, 'num_layers': 5, 'lr': 0.01, 'max_epoch': 5, 'eval_frequency': 2,
        'dropout': 0.1, 'runs': 2, 'seed': 7, 'depth': 3, 'num_neighbors': 5, 'conv': 'gcn', 'pool': False}


@pytest.mark.parametrize("argv,want", [(["--dataset", "cora"], _DEFAULTS), (_SET_ARGV, _SET)], ids=["defaults", "set"])
def test_parsed_namespace(argv, want):
    from grapes_amd import shadow
    got = vars(shadow.parse_args(argv))
    assert got == want
    assert all(type(got[k]) is type(want[k]) for k in want)


_CAP = "shadow_sample: depth 2 with num_neighbors 32 exceeds the ego-net cap: 1 + k + ... + k^depth must be at most 1024"
_K = "shadow_sample: num_neighbors = {} is not built (1 .. 64; -1, every neighbour, would leave the ego-net unbounded)"


@pytest.mark.parametrize("argv,exc,message", [
    ([], SystemExit, "--dataset is required"),
    (["--dataset", "cora", "--depth", "2", "--num_neighbors", "32"], ValueError, _CAP),
    (["--dataset", "cora", "--depth", "1", "--num_neighbors", "65"], ValueError, _K.format(65)),
    (["--dataset", "cora", "--num_neighbors", "-1"], ValueError, _K.format(-1)),
    (["--dataset", "cora", "--depth", "0"], ValueError, "shadow_sample: depth = 0 is not built (depth >= 1)"),
    (["--dataset", "cora", "--batch_size", "5000"], ValueError,
     "--eval_frequency, --hidden_dim and --num_layers are at least 1, --batch_size is 1 .. 4096"),
    (["--dataset", "cora", "--num_layers", "0"], ValueError,
     "--eval_frequency, --hidden_dim and --num_layers are at least 1, --batch_size is 1 .. 4096"),
])
def test_refusals(argv, exc, message):
    from grapes_amd import shadow
    with pytest.raises(exc) as e:
        shadow.parse_args(argv)
    assert str(e.value) == message


def test_the_flags_of_the_other_drivers_are_as_they_were():
    from grapes_amd import graphsage, shadow
    with pytest.raises(SystemExit):
        graphsage.parse_args(["--dataset", "cora", "--depth", "2"])
    with pytest.raises(SystemExit):
        shadow.parse_args(["--dataset", "cora", "--fanouts", "10,10"])
    with pytest.raises(SystemExit):
        shadow.parse_args(["--dataset", "cora", "--conv", "gat"])


def test_host_tensors_are_refused(built_lib):
    from grapes_amd import ops
    rowptr, col = torch.tensor([0, 2, 3, 3]), torch.tensor([1, 2, 0], dtype=torch.int32)
    roots = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(built_lib.GrapesHipError):
        ops.shadow_sample(rowptr, col, 3, roots, 2, 2, e_cap=16)
    with pytest.raises(built_lib.GrapesHipError):
        ops.segment_mean_fwd(torch.zeros(3, 4), torch.tensor([0, 3], dtype=torch.int32))
    with pytest.raises(built_lib.GrapesHipError):
        ops.segment_mean_bwd(torch.zeros(1, 4), torch.tensor([0, 3], dtype=torch.int32), 3)


def test_sampler_model_and_trainer_refuse_what_is_not_built():
    """The argument checks come before the graph is touched."""
    from grapes_amd.modules.shadow import ShaDow, ShaDowKHopSampler
    from grapes_amd.shadow import ShadowTrainer
    with pytest.raises(ValueError, match="exceeds the ego-net cap"):
        ShaDowKHopSampler(None, 2, 32)
    with pytest.raises(ValueError, match="num_neighbors = -1 is not built"):
        ShaDowKHopSampler(None, 2, -1)
    with pytest.raises(ValueError, match="n_cap and e_cap are at least 1"):
        ShaDowKHopSampler(None, 2, 5, e_cap=0)
    with pytest.raises(NotImplementedError, match="conv='gat' is not built"):
        ShaDow(8, 16, 4, 2, conv="gat")
    with pytest.raises(ValueError, match="num_layers and hidden_dim are at least 1"):
        ShaDow(8, 16, 4, 0)
    m = ShaDow(8, 16, 4, 3, conv="sage", pool=True)
    assert len(m.body.convs) == 3 and m.head.weight.shape == (4, 32) and ShaDow(8, 16, 4, 2, conv="gcn", pool=False).head.weight.shape == (4, 16)
    with pytest.raises(ValueError, match="node features with a gradient are not built"):
        ShadowTrainer(None, torch.zeros(3, 8, requires_grad=True), None, m, None)
