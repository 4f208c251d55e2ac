"""The label-propagation partitioner without a GPU: tests/partition_oracle.py against brute force (a dense count matrix, one full
sort), the invariants of a run, the quality on the planted graph, the refusals, the --partition lp parsing and the entry points."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import partition_oracle as PO

ENTRY_POINTS = {"grapes_partition_propose_workspace_bytes": 2, "grapes_partition_propose": 10, "grapes_partition_admit_workspace_bytes": 2,
                "grapes_partition_admit": 11, "grapes_partition_cut_workspace_bytes": 1, "grapes_partition_cut": 9}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    from grapes_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.DIAG_LIB_PATH):
        ge.build()
    return _lib


def test_both_libraries_carry_the_entry_points_with_their_argument_counts(built_lib):
    import ctypes
    prod, diag = ctypes.CDLL(built_lib.LIB_PATH), ctypes.CDLL(built_lib.DIAG_LIB_PATH)
    for name, n_args in ENTRY_POINTS.items():
        assert name in built_lib.SIGNATURES and hasattr(prod, name) and hasattr(diag, name)
        assert len(built_lib.SIGNATURES[name][1]) == n_args
    header = open(os.path.join(os.path.dirname(built_lib.__file__), "..", "include", "grapes_hip.h")).read()
    for name, n_args in ENTRY_POINTS.items():
        decl = header.split(f" {name}(")[1].split(");")[0]
        assert decl.count(",") + 1 == n_args
    lib = built_lib.load()
    assert lib.grapes_abi_version() == 304
    assert lib.grapes_partition_propose_workspace_bytes(1000, 10) >= 4 * 1000
    assert lib.grapes_partition_admit_workspace_bytes(1000, 10) >= 8 * 1000 + 8 * 10 + 4 * 41
    assert lib.grapes_partition_cut_workspace_bytes(1000) >= 4 * 1000 + 8 * 64


def _small_graphs():
    g1 = PO.planted(120, 5, 3, 1, seed=1, hub=7, hub_degree=90, dups=40, loops=9)
    g2 = PO.planted(60, 60, 1, 2, seed=2)
    ties = PO.csr([[1, 2, 3, 4], [0], [0], [0], [0], [5, 5, 0, 0]])         # row 0: four labels once each; row 5: loops, a duplicate
    return {"hub_dups_loops": (g1[0], g1[1], PO.balanced_random(120, 7, 3), 7),
            "one_per_group": (g2[0], g2[1], PO.balanced_random(60, 60, 4), 60),
            "ties": (ties[0], ties[1], np.array([2, 3, 1, 2, 0, 0]), 4)}


@pytest.mark.parametrize("name", list(_small_graphs()))
def test_propose_against_the_dense_count_matrix(name):
    ip, ix, part, P = _small_graphs()[name]
    want, gain, status = PO.propose(ip, ix, part, P)
    dw, dg = PO.propose_dense(ip, ix, part, P)
    assert status == 0 and np.array_equal(want, dw) and np.array_equal(gain, dg)
    assert ((want >= 0) == (gain >= 1)).all() and (want != part).all()
    if name == "ties":
        assert want[0] == -1 and gain[0] == 0                               # cur = 2 is among the labels at the maximum: 0 stays
        assert want[5] == 2 and gain[5] == 2                                # loops dropped, the duplicate counts twice


def test_propose_ties_without_cur_take_the_smallest_label():
    ip, ix = PO.csr([[1, 2, 3, 4], [0], [0], [0], [0]])
    want, gain, _ = PO.propose(ip, ix, [0, 3, 1, 3, 1], 4)
    assert want[0] == 1 and gain[0] == 2                                    # labels 1 and 3 twice each, cur = 0 never


@pytest.mark.parametrize("name", list(_small_graphs()))
@pytest.mark.parametrize("slack", [0, 1, 3, 1000])
def test_admit_against_a_full_sort(name, slack):
    ip, ix, part, P = _small_graphs()[name]
    want, gain, _ = PO.propose(ip, ix, part, P)
    size = np.bincount(part, minlength=P)
    cap = int(size.max()) + slack
    a = PO.admit(want, gain, part, size, cap)
    b = PO.admit_by_full_sort(want, gain, part, size, cap)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[1].max() <= cap and a[1].sum() == len(part) and np.array_equal(a[1], np.bincount(a[0], minlength=P))
    assert a[2] == (a[0] != part).sum()
    if slack == 1000:
        assert a[2] == (want >= 0).sum()


def test_admit_prefers_the_gain_then_the_smaller_id():
    want, gain = np.array([1, 1, 1, 1, -1, -1]), np.array([1, 3, 1, 2, 0, 0])
    part, size, moved = PO.admit(want, gain, [0, 0, 0, 0, 1, 1], [4, 2], 4)
    assert moved == 2 and part.tolist() == [0, 1, 0, 1, 1, 1] and size.tolist() == [2, 4]
    part, size, moved = PO.admit(want, gain, [0, 0, 0, 0, 1, 1], [4, 2], 5)
    assert moved == 3 and part.tolist() == [1, 1, 0, 1, 1, 1]               # gains 3, 2, then the smaller id of the two with gain 1
    assert PO.admit(want, gain, [0, 0, 0, 0, 1, 1], [4, 2], 2)[2] == 0       # free = 0


@pytest.fixture(scope="module")
def planted_4000():
    ip, ix, group = PO.planted(4000, 16, 4, 1, seed=11)
    start = PO.balanced_random(4000, 16, 12)
    trace = []
    part, info = PO.refine(ip, ix, start, 16, PO.default_cap(4000, 16), 30, trace=trace)
    return ip, ix, group, start, part, info, trace


def test_sizes_stay_below_cap_and_the_smallest_cut_round_is_returned(planted_4000):
    ip, ix, _, start, part, info, trace = planted_4000
    cap = PO.default_cap(4000, 16)
    assert cap == 250 + 25 and len(trace) == len(info["moved"])
    for p, size in trace:
        assert size.max() <= cap and size.sum() == 4000 and np.array_equal(size, np.bincount(p, minlength=16))
    cuts = info["cuts"]
    assert cuts[0] == PO.cut(ip, ix, start, 16) and info["round"] == int(np.argmin(cuts)) and min(cuts) <= cuts[0]
    assert PO.cut(ip, ix, part, 16) == cuts[info["round"]]
    assert np.array_equal(part, trace[info["round"] - 1][0] if info["round"] else start)
    assert info["max_size"] == np.bincount(part, minlength=16).max() <= cap


def test_the_planted_graph_loses_at_least_four_tenths_of_its_cut(planted_4000):
    ip, ix, group, _, _, info, _ = planted_4000
    ratio = info["cuts"][info["round"]] / info["cuts"][0]
    print(f"planted 4000 / 16: cut {info['cuts'][0]} -> {info['cuts'][info['round']]} of {len(ix)} entries "
          f"(ratio {ratio:.3f}, start fraction {info['cuts'][0] / len(ix):.3f}, round {info['round']}, planted "
          f"{PO.cut(ip, ix, group, 16) / len(ix):.3f})")
    assert ratio < 0.6


def test_a_cap_below_the_largest_starting_cluster_is_refused():
    from grapes_amd.modules.cluster import default_cap, make_partition, refine_partition
    ip, ix, _ = PO.planted(200, 4, 3, 1, seed=5)
    start = np.arange(200) % 4
    start[:10] = 0                                                          # cluster 0 holds 57 nodes
    with pytest.raises(ValueError, match="cap is below the largest starting cluster"):
        PO.refine(ip, ix, start, 4, 56, 5)
    PO.refine(ip, ix, start, 4, 57, 1)
    host = SimpleNamespace(num_nodes=200, nnz=len(ix), device=torch.device("cpu"))
    with pytest.raises(ValueError, match=r"cap 56 is below the start's largest cluster \(57\)"):
        refine_partition(host, torch.from_numpy(start), 4, cap=56)
    with pytest.raises(ValueError, match="below the start's largest cluster"):
        refine_partition(host, torch.from_numpy(start), 4, imbalance=0.1)   # the default cap: 50 + 5
    with pytest.raises(ValueError, match=r"cluster id outside \[0, 3\)"):
        refine_partition(host, torch.from_numpy(start), 3)
    with pytest.raises(ValueError, match="integer tensor"):
        refine_partition(host, torch.zeros(200), 4)
    assert default_cap(4000, 16, 0.1) == PO.default_cap(4000, 16) == 275
    assert default_cap(6000, 100, 0.1) == 66 and default_cap(10, 3, 0.0) == 4 and default_cap(1001, 10, 0.25) == 101 + 25
    with pytest.raises(ValueError, match="'lp' refines an assignment over a graph: ClusterData"):
        make_partition(10, 2, "lp")
    with pytest.raises(ValueError, match="not built"):
        make_partition(10, 2, "metis")


@pytest.mark.parametrize("value,want", [("random", ("random", None, None)), ("file", ("file", None, None)), ("lp", ("lp", 30, 0.1)),
                                        ("lp:5", ("lp", 5, 0.1)), ("lp:0", ("lp", 0, 0.1)), ("lp:12:0.25", ("lp", 12, 0.25)),
                                        ("lp:7:0", ("lp", 7, 0.0))])
def test_partition_values_parse(value, want):
    from grapes_amd import clustergcn
    assert clustergcn.parse_partition(value) == want
    args = clustergcn.parse_args(["--dataset", "cora", "--partition", value] + (["--partition_file", "p.npy"] if value == "file" else []))
    assert args.partition == value                                          # kept as given: parsed after parse_args


@pytest.mark.parametrize("value", ["metis", "lp:", "lp:x", "lp:-1", "lp:5:-0.1", "lp:5:x", "lp:5:0.1:2", "lp5", "LP", "lp:5:inf", ""])
def test_other_partition_values_are_argparse_errors(value):
    from grapes_amd import clustergcn
    with pytest.raises(ValueError):
        clustergcn.parse_partition(value)
    with pytest.raises(SystemExit):
        clustergcn.parse_args(["--dataset", "cora", "--partition", value])


def test_lp_does_not_take_a_partition_file_and_the_tool_parses():
    from grapes_amd import clustergcn, partition
    with pytest.raises(ValueError, match="--partition file goes with --partition_file"):
        clustergcn.parse_args(["--dataset", "cora", "--partition", "lp:5", "--partition_file", "p.npy"])
    got = vars(partition.parse_args(["--dataset", "cora", "--num_parts", "8", "--out", "p.npy"]))
    assert got == dict(dataset="cora", num_parts=8, rounds=30, imbalance=0.1, start="random", seed=None, out="p.npy")
    with pytest.raises(SystemExit):
        partition.parse_args(["--dataset", "cora", "--num_parts", "8", "--out", "p.npy", "--start", "lp"])
    with pytest.raises(ValueError, match="at least"):
        partition.parse_args(["--dataset", "cora", "--num_parts", "0", "--out", "p.npy"])
    info = dict(cuts=[100, 60, 40, 45], moved=[30, 20, 10], round=2, max_size=9, cap=11)
    assert clustergcn.partition_report(info) == ("Partition: label propagation, cut 100 -> 40 (round 2 of 3 run; largest cluster 9, "
                                                 "cap 11)")


def test_host_tensors_are_refused(built_lib):
    from grapes_amd import ops
    i32 = torch.int32
    rowptr, col, part = torch.tensor([0, 2, 3, 3]), torch.tensor([1, 2, 0], dtype=i32), torch.tensor([0, 1, 0], dtype=i32)
    with pytest.raises(built_lib.GrapesHipError):
        ops.partition_propose(rowptr, col, 3, part, 2)
    with pytest.raises(built_lib.GrapesHipError):
        ops.partition_cut(rowptr, col, 3, part, 2)
    with pytest.raises(built_lib.GrapesHipError):
        ops.partition_admit(part, part, part, torch.tensor([2, 1], dtype=i32), 3)
