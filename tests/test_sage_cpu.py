"""GraphSAGE without a GPU: the C surface, the host oracle's selection rule (tests/sage_oracle.py) against its definition, the
closed-form backward of the mean / sum gather against fp64 autograd, the modules' refusals and the driver's arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import sage_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("grapes_sage_sample_layer", "grapes_sage_sample_layer_workspace_bytes", "grapes_rootsum_aggregate_fwd",
                "grapes_rootsum_aggregate_bwd", "grapes_rootsum_aggregate_workspace_bytes")
UNIFORM_SEED = 2                       # the seed tests/test_sage_gpu.py fixes for its uniformity check


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
    assert int(re.search(r"#define\s+GRAPES_ABI_VERSION\s+(\d+)", header).group(1)) == 304


def test_workspaces_are_host_calls_that_grow(built_lib):
    lib = built_lib.load()
    sizes = [lib.grapes_sage_sample_layer_workspace_bytes(m) for m in (1, 64, 4096)]
    assert sizes[0] > 0 and sizes[0] < sizes[1] < sizes[2] and sizes[2] >= 12 * 4096
    assert lib.grapes_rootsum_aggregate_workspace_bytes(0, 0, 64) < lib.grapes_rootsum_aggregate_workspace_bytes(100, 0, 64) \
        < lib.grapes_rootsum_aggregate_workspace_bytes(100, 10, 64)


def test_entry_points_refuse_bad_arguments_on_the_host(built_lib):
    """Argument checks run before any launch: they need no device."""
    lib = built_lib.load()
    one = ctypes.c_void_p(16)                                            # a non-NULL, 16-byte aligned address that is never read
    for fanout in (0, 65, -1):
        assert lib.grapes_sage_sample_layer(one, one, 10, one, 4, None, fanout, None, 0, 0, 0, None, 16, one, one, None, one, one,
                                            None, None) == -1
    assert lib.grapes_sage_sample_layer(one, one, 10, one, 4, None, 3, None, 0, 0, 0, None, 0, one, one, None, one, one, None,
                                        None) == -1                      # e_cap 0
    for f in (0, 1025, 260 + 1):                                         # no width, too wide, wide and not a multiple of 4
        assert lib.grapes_rootsum_aggregate_fwd(one, 2048, None, 0, None, None, one, one, 0.0, 0, 1, 0, ctypes.c_void_p(32), 2048, None,
                                                0, 4, None, f, None, None, 0, None, None, None) == -1
    assert lib.grapes_rootsum_aggregate_fwd(one, 64, None, 0, None, None, one, one, 0.0, 0, 1, 0, one, 64, None, 0, 4, None, 64, None,
                                            None, 0, None, None, None) == -1   # out aliases src
    for scale in (3, -1):                                                # not one of GRAPES_ROOTSUM_SCALE_*
        assert lib.grapes_rootsum_aggregate_fwd(one, 64, None, 0, None, None, one, one, 0.0, 0, scale, 0, ctypes.c_void_p(32), 64, None,
                                                0, 4, None, 64, None, None, 0, None, None, None) == -1
        assert lib.grapes_rootsum_aggregate_bwd(one, 64, None, 0, None, one, one, one, 0.0, 0, scale, None, 0, ctypes.c_void_p(32), 64,
                                                None, 0, None, 4, None, 64, None, None, 0, one, None, None) == -1


# ---------------------------------------------------------------------------------------------------- the selection rule
def test_selection_keeps_min_deg_k_ascending_and_ties_go_to_the_lower_position():
    rng = np.random.default_rng(1)
    for deg in (0, 1, 2, 3, 4, 63, 64, 65, 129, 1000):
        keys = rng.integers(0, 2 ** 32, deg, dtype=np.uint64).astype(np.uint32)
        for k in (1, 3, 64):
            t = SO.select_row(keys, k)
            assert len(t) == min(deg, k) and (np.diff(t) > 0).all()
            if deg > k:                                                  # the definition: the k smallest keys (these are distinct)
                assert set(t) == set(np.argsort(keys, kind="stable")[:k])
    same = np.full(200, 7, np.uint32)
    assert np.array_equal(SO.select_row(same, 3), [0, 1, 2])             # every key equal: the first k positions
    keys = np.full(130, 9, np.uint32)
    keys[[5, 64, 100]] = 1                                               # three below, then ties on both sides of entry 63 / 64
    assert np.array_equal(SO.select_row(keys, 5), [0, 1, 5, 64, 100])
    keys = np.full(130, 9, np.uint32)
    keys[62:66] = 4
    assert np.array_equal(SO.select_row(keys, 3), [62, 63, 64]) and np.array_equal(SO.select_row(keys, 5), [0, 62, 63, 64, 65])


def test_layer_positions_follow_the_rows_in_list_order_and_a_repeated_row_draws_independently():
    ip, ix = SO.degree_graph([0, 1, 2, 3, 4, 63, 64, 65, 128, 129, 1000], 1200, 1)
    rows = np.array([10, 3, 3, 0, 9, 3])
    src, dst, pos, total = SO.sample_layer(ip, ix, rows, 2, seed=5, offset=7)
    assert total == 1000 + 3 + 3 + 0 + 129 + 3 and len(src) == 2 * 5
    assert np.array_equal(dst, np.repeat([10, 3, 3, 9, 3], 2)) and np.array_equal(ix[pos], src)
    words = SO.stream_keys(5, 7, total)
    p = 0
    picks = []
    for i in rows:
        deg = int(ip[i + 1] - ip[i])
        picks.append(tuple(SO.select_row(words[p:p + deg], 2)))
        p += deg
    assert len({picks[1], picks[2], picks[5]}) > 1                       # row 3, listed three times: not one draw repeated
    assert SO.offset_advance(total) == (total + 3) // 4 and SO.offset_advance(0) == 0
    # given keys replace the stream, a row id outside the graph is an empty row
    k = np.arange(total, dtype=np.uint32)[::-1].copy()
    s2, d2, p2, _ = SO.sample_layer(ip, ix, rows, 2, keys=k)
    assert np.array_equal(p2[:2] - ip[10], [998, 999])                   # descending keys: the last two positions
    s3, d3, _, t3 = SO.sample_layer(ip, ix, np.array([3, 1200, 4]), 64)
    assert t3 == 7 and np.array_equal(np.unique(d3), [3, 4])


def test_oracle_uniformity_for_the_gpu_tests_seed():
    """One degree-10 row listed 4096 times at fanout 3: every neighbour's inclusion count within 6 sigma of 4096 * 0.3 = 1228.8,
    sigma = sqrt(4096 * 0.3 * 0.7) = 29.3, i.e. +-176 — checked here for the oracle alone, for the seed the GPU test fixes."""
    ip, ix = SO.csr_from_rows([list(range(1, 11))] + [[] for _ in range(10)])
    src, _, _, total = SO.sample_layer(ip, ix, np.zeros(4096, np.int64), 3, seed=UNIFORM_SEED, offset=0)
    counts = np.bincount(src, minlength=11)[1:]
    assert total == 40960 and counts.sum() == 3 * 4096
    assert np.abs(counts - 1228.8).max() <= 176.0, counts


def test_batch_construction():
    ip, ix = SO.degree_graph([3, 5, 0, 2, 7, 1, 4, 4], 40, 3)
    b = SO.sample(ip, ix, [4, 1, 2], [3, 2], seed=9)
    L0, L1 = b.layers
    assert np.array_equal(L0.prev, [4, 1, 2]) and np.array_equal(L0.after, np.union1d([4, 1, 2], L0.src))
    assert np.array_equal(L1.prev, L0.after) and np.array_equal(b.node_idx, L1.after)
    assert np.array_equal(np.bincount(L0.dst, minlength=5)[[4, 1, 2]], [3, 3, 0])
    assert np.array_equal(b.node_idx[b.local_targets], [4, 1, 2])
    for ei, L in zip(b.edge_index, b.layers):
        assert np.array_equal(b.node_idx[ei[0]], L.src) and np.array_equal(b.node_idx[ei[1]], L.dst)
    assert b.philox_offset == SO.offset_advance(L0.deg_sum) + SO.offset_advance(L1.deg_sum)
    full = SO.sample(ip, ix, [4, 1, 2], [-1, 2], seed=9)
    assert len(full.layers[0].src) == 7 + 5 + 0 and full.philox_offset == SO.offset_advance(full.layers[1].deg_sum)


# ---------------------------------------------------------------------------------------------------- the maths
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("n", [1, 37])
def test_closed_form_backward_of_the_gather_against_autograd(aggr, n):
    ei = SO.conv_graph(n, 11)
    rng = np.random.default_rng(12)
    x = torch.as_tensor(rng.standard_normal((n, 5))).requires_grad_(True)
    g = rng.standard_normal((n, 5))
    SO.aggregate64(x, ei, n, aggr).backward(torch.as_tensor(g))
    want = SO.mean_sum_backward_closed_form(g, ei, n, aggr)
    assert np.allclose(x.grad.numpy(), want, rtol=1e-12, atol=1e-13)
    if n > 1:
        deg = np.bincount(ei[1], minlength=n)
        assert deg[0] == 0 and deg[3] >= 200 and ((ei[0] == 5) & (ei[1] == 5)).sum() == 2
        agg = SO.aggregate64(x.detach(), ei, n, aggr).numpy()
        assert (agg[0] == 0).all()                                       # the empty row aggregates to 0, mean included


def test_both_operand_forms_are_the_same_map():
    """mean / sum are linear: W_l aggr(x) + W_r x = aggr-gather of (x W_lᵀ) + x W_rᵀ — what lets SAGEConv choose by width."""
    n, fi, fo = 37, 6, 4
    ei = SO.conv_graph(n, 13)
    rng = np.random.default_rng(14)
    x, wl, wr, b = (torch.as_tensor(rng.standard_normal(s)) for s in ((n, fi), (fo, fi), (fo, fi), (fo,)))
    for aggr in ("mean", "sum"):
        a = SO.sage_conv64(x, ei, wl, b, wr, aggr)
        t = SO.aggregate64(x @ wl.T, ei, n, aggr) + x @ wr.T + b
        assert torch.allclose(a, t, rtol=1e-12, atol=1e-12)


def test_adam_first_step_is_the_sign_step():
    p, g = np.array([0.5, -0.25, 1.0]), np.array([0.3, -2.0, 0.0])
    w = torch.nn.Parameter(torch.tensor(p))
    w.grad = torch.tensor(g)
    torch.optim.Adam([w], lr=1e-3).step()
    assert np.allclose(w.detach().numpy(), SO.adam_first_step64(p, g), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- modules and drivers
def test_modules_state_dict_dispatch_and_refusals():
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules.gcn import SAGE, SAGEConv, classifier_layers, classifier_needs_loops
    c = SAGEConv(100, 256)
    assert sorted(c.state_dict()) == ["lin_l.bias", "lin_l.weight", "lin_r.weight"]
    assert tuple(c.lin_l.weight.shape) == (256, 100) and tuple(c.lin_r.weight.shape) == (256, 100)
    assert sorted(SAGEConv(8, 4, root_weight=False, bias=False).state_dict()) == ["lin_l.weight"]
    # the dispatch rule: aggregate-first when in < out and in is a gather width, else transform-first
    assert c.default_form() == "aggregate" and SAGEConv(256, 100).default_form() == "transform"
    assert SAGEConv(64, 64).default_form() == "transform" and SAGEConv(1, 1).default_form() == "transform"
    assert SAGEConv(300, 47).default_form() == "transform" and SAGEConv(300, 47).form_ok("aggregate")
    assert not SAGEConv(301, 47).form_ok("aggregate") and not SAGEConv(47, 1).form_ok("aggregate")
    assert SAGEConv(260, 4).form_ok("aggregate") and SAGEConv(260, 4).default_form() == "transform"
    with pytest.raises(ValueError, match="not built"):
        SAGEConv(258, 2000)                                              # neither form: 258 > 256 is no multiple of 4, 2000 > 1024
    assert SAGEConv(100, 2000).default_form() == "aggregate"             # a wide output needs the aggregate-first form
    with pytest.raises(ValueError, match="not built"):
        SAGEConv(2000, 1100)
    for kw in ({"aggr": "max"}, {"aggr": "lstm"}, {"normalize": True}, {"project": True}):
        with pytest.raises(NotImplementedError):
            SAGEConv(4, 4, **kw)
    m = SAGE(10, [16, 16, 3], dropout=0.5, aggr="sum")
    assert len(m.convs) == 3 and classifier_layers(m) is m.convs and classifier_needs_loops(m)
    assert [(l.in_channels, l.out_channels, l.aggr) for l in m.convs] == [(10, 16, "sum"), (16, 16, "sum"), (16, 3, "sum")]
    assert "convs.2.lin_r.weight" in m.state_dict()
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(GrapesHipError, match="no CPU path"):
        SAGEConv(4, 3)(torch.randn(2, 4), ei)
    with pytest.raises(GrapesHipError, match="no CPU path"):
        SAGE(4, [4, 3])(torch.randn(2, 4), ei)


def test_fanouts_are_checked_before_any_device_work():
    from grapes_amd.modules.sage import NeighborSampler, check_fanouts
    assert check_fanouts([25, 10]) == [25, 10] and check_fanouts((-1, 64, 1)) == [-1, 64, 1]
    for bad in ([0], [65], [25, -2], []):
        with pytest.raises(ValueError):
            check_fanouts(bad)
        with pytest.raises(ValueError):
            NeighborSampler(object(), bad)


def test_cli_arguments_and_refusals():
    from grapes_amd import graphsage, main
    a = graphsage.parse_args(["--dataset", "cora"])
    assert (a.fanouts, a.aggr, a.batch_size, a.hidden_dim, a.num_layers, a.lr) == ([25, 10], "mean", 512, 256, 2, 1e-3)
    assert a.dropout == 0.0 and a.runs == 1 and a.seed is None and a.eval_frequency == 1 and a.max_epoch == 100
    b = graphsage.parse_args(["--dataset", "cora", "--fanouts", "25,10", "--aggr", "mean", "--hidden_dim", "256", "--batch_size",
                              "512", "--lr", "1e-3", "--max_epoch", "100", "--dropout", "0", "--runs", "1", "--seed", "3"])
    assert b.fanouts == [25, 10] and b.seed == 3
    c = graphsage.parse_args(["--dataset", "cora", "--fanouts", "5,-1,64", "--aggr", "sum", "--num_layers", "3"])
    assert c.fanouts == [5, -1, 64] and c.aggr == "sum" and c.num_layers == 3
    with pytest.raises(SystemExit):
        graphsage.parse_args(["--dataset", "cora", "--aggr", "max"])
    with pytest.raises(SystemExit):
        graphsage.parse_args([])
    for fan in ("0,5", "65", "10,x"):
        with pytest.raises((ValueError, SystemExit)):
            graphsage.parse_args(["--dataset", "cora", "--fanouts", fan])
    with pytest.raises(ValueError, match="one entry per layer"):
        graphsage.parse_args(["--dataset", "cora", "--fanouts", "25,10", "--num_layers", "3"])
    with pytest.raises(ValueError):
        graphsage.parse_args(["--dataset", "cora", "--batch_size", "5000"])
    with pytest.raises(ValueError):
        main.parse_args(["--classifier", "sage"])                        # the GRAPES driver still refuses the name
