"""The label-propagation partitioner on the MI355X against tests/partition_oracle.py, every integer output bit for bit: proposals over
rows on either side of the kernels' limits (64 | 65 entries: one wavefront in registers | an LDS table; 2048 | 2049: the table | the
P-sized slabs), 1 .. 5 000 distinct labels, forced ties, stored loops and duplicates, P = 1, P = N and an empty cluster; admissions
below, at and above the free room, the radix select over one large bucket; the cut; refine_partition, ClusterData(method="lp") under
ClusterLoader, the status word and the command lines.

Left out: a cut above 2^31.  The cut counts stored entries, so it needs a graph of more than 2^31 entries, which the entry points
refuse (fewer than 2^31 entries is their contract)."""
import numpy as np
import pytest
import torch

from tests import cluster_oracle as CO
from tests import partition_oracle as PO

pytestmark = pytest.mark.gpu

BAD = 4


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _propose(ops, ip, ix, part, P):
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    want, gain = ops.partition_propose(_dev(ip, np.int64), _dev(ix, np.int32), len(ip) - 1, _dev(part, np.int32), P, status=status)
    return _np(want).astype(np.int64), _np(gain).astype(np.int64), int(status.item())


def _check_propose(ops, ip, ix, part, P, expect_status=0):
    want, gain, status = _propose(ops, ip, ix, part, P)
    ow, og, ostatus = PO.propose(ip, ix, part, P)
    assert status == ostatus == expect_status
    assert np.array_equal(want, ow) and np.array_equal(gain, og)
    return ow, og


def _rows_of(degrees, n, seed, tail_degree=3):
    """Row i < len(degrees) holds degrees[i] random columns, every later row tail_degree."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n, d).tolist() for d in list(degrees) + [tail_degree] * (n - len(degrees))]


# ---------------------------------------------------------------------------------------------------- the proposal
_LIMIT_DEGREES = [0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1000, 2047, 2048, 2049, 2050, 3000, 4097]


@pytest.mark.parametrize("P", [1, 2, 7, 64, 65, 700, 3000])
def test_rows_on_either_side_of_every_limit(P):
    """Random labels over P clusters; P = 700 and 3 000 give the long rows hundreds to thousands of distinct labels."""
    ops = _ops()
    n = 3000
    ip, ix = PO.csr(_rows_of(_LIMIT_DEGREES, n, seed=P))
    part = np.random.default_rng(P + 1).integers(0, P, n)
    want, _ = _check_propose(ops, ip, ix, part, P)
    assert P == 1 or (want[3:len(_LIMIT_DEGREES)] >= 0).sum() >= 5          # (the long rows do propose)


@pytest.mark.parametrize("deg,distinct", [(64, 1), (64, 64), (65, 1), (65, 65), (200, 64), (200, 65), (2048, 1), (2048, 2048), (2049, 1),
                                          (2049, 2049), (5000, 1), (5000, 2100), (5000, 5000), (70000, 300)])
def test_a_row_with_a_given_number_of_distinct_labels(deg, distinct):
    """Row 0 stores deg entries over `distinct` columns whose labels all differ (part[v] = v, P = N).  2 100 and 5 000 labels are
    more than the LDS table takes; the 5 000-entry hub appears with all labels distinct and with all of them equal."""
    ops = _ops()
    n = max(distinct + 2, 100)
    cols = 1 + (np.arange(deg) * 7919) % distinct                          # every one of the `distinct` columns, interleaved
    rows = [cols.tolist()] + [[0] for _ in range(n - 1)]
    ip, ix = PO.csr(rows)
    part = np.arange(n)
    want, gain = _check_propose(ops, ip, ix, part, n)
    assert len(np.unique(cols)) == distinct and want[0] == cols.min() == 1
    assert gain[0] == np.bincount(cols).max()
    part[0] = 1                                                             # cur is now the smallest label of the row
    want, gain = _check_propose(ops, ip, ix, part, n)
    first = np.bincount(cols)[1]
    assert (want[0] == -1) == (first == np.bincount(cols).max())


@pytest.mark.parametrize("half", [2, 32, 33, 65, 1000, 1024, 2500])
def test_forced_ties(half):
    """Row 0 stores `half` entries of label 5 and `half` of label 3 (rows of 4 .. 5 000 entries: all three kernels): with cur among
    the labels at the maximum v stays; without, the smallest label wins with gain = half - count[cur]."""
    ops = _ops()
    n = 2 * half + 10
    a, b = np.arange(1, half + 1), np.arange(half + 1, 2 * half + 1)
    row0 = np.stack([a, b], 1).reshape(-1).tolist() + [2 * half + 1]        # interleaved, and one entry of a third label
    ip, ix = PO.csr([row0] + [[0] for _ in range(n - 1)])
    part = np.zeros(n, dtype=np.int64)
    part[a], part[b], part[2 * half + 1] = 5, 3, 6
    for cur, want0, gain0 in ((5, -1, 0), (3, -1, 0), (6, 3, half - 1), (0, 3, half), (7, 3, half)):
        part[0] = cur
        want, gain = _check_propose(ops, ip, ix, part, 8)
        assert want[0] == want0 and gain[0] == gain0


def test_hand_rows_loops_duplicates_and_an_empty_cluster():
    ops = _ops()
    ip, ix = PO.csr([[1, 2, 3, 4], [0], [0], [0], [0], [5, 5, 0, 0], [], [7], [6, 6, 7, 6]])
    part = [2, 3, 1, 2, 0, 0, 4, 4, 0]                                      # P = 6: cluster 5 holds no node
    want, gain = _check_propose(ops, ip, ix, part, 6)
    assert want.tolist() == [-1, 2, 2, -1, 2, 2, -1, -1, 4] and gain.tolist() == [0, 1, 1, 0, 1, 2, 0, 0, 4]
    for seed, P in ((1, 7), (2, 120), (3, 1)):
        ip, ix, _ = PO.planted(120, 5, 3, 1, seed=seed, hub=7, hub_degree=3000, dups=300, loops=40)
        part = np.random.default_rng(seed).integers(0, P, 120) if P < 120 else np.arange(120)
        _check_propose(ops, ip, ix, part, P)
    ip, ix = PO.csr([[0] * 70, [1] * 3000, [0, 1]])                        # rows of nothing but stored loops, short and long
    want, _ = _check_propose(ops, ip, ix, [0, 1, 1], 2)
    assert want.tolist() == [-1, -1, -1]


def test_bad_columns_and_labels_raise_through_the_status_word():
    ops = _ops()
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.cluster import refine_partition
    rows = _rows_of([5, 70, 2100], 50, seed=1)
    for r in rows[:3]:
        r[1], r[-1] = 50, -2                                                # a column at N and a negative one in every kind of row
    ip, ix = PO.csr(rows)
    part = np.arange(50) % 5
    want, _ = _check_propose(ops, ip, ix, part, 5, expect_status=BAD)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cut = ops.partition_cut(_dev(ip, np.int64), _dev(ix, np.int32), 50, _dev(part, np.int32), 5, status=status)
    assert int(cut.item()) == PO.cut(ip, ix, part, 5) and int(status.item()) == BAD
    with pytest.raises(GrapesHipError, match="refine_partition: .*index"):
        refine_partition(DeviceGraph(_dev(ip, np.int64), _dev(ix, np.int32), 50), torch.as_tensor(part), 5)
    ip, ix = PO.csr(_rows_of([5, 70, 2100], 50, seed=2))
    for bad in (5, -1):
        part = np.arange(50) % 5
        part[[3, 17]] = bad                                                 # a label outside [0, P): a neighbour's, and a node's own
        _check_propose(ops, ip, ix, part, 5, expect_status=BAD)
    status.zero_()
    part = _dev(np.arange(50) % 5, np.int32)
    want = torch.full((50,), -1, dtype=torch.int32, device="cuda")
    want[4], want[9] = 5, 2                                                 # a destination at P; a proposal with gain 0
    size = torch.full((5,), 10, dtype=torch.int32, device="cuda")
    moved = ops.partition_admit(want, torch.zeros_like(want), part, size, 20, status=status)
    assert int(moved.item()) == 0 and int(status.item()) == BAD and size.tolist() == [10] * 5


# ---------------------------------------------------------------------------------------------------- the admission
def _check_admit(ops, want, gain, part, P, cap):
    size = np.bincount(part, minlength=P)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_part, d_size = _dev(part, np.int32), _dev(size, np.int32)
    moved = ops.partition_admit(_dev(want, np.int32), _dev(gain, np.int32), d_part, d_size, cap, status=status)
    opart, osize, omoved = PO.admit(want, gain, part, size, cap)
    assert int(status.item()) == 0 and int(moved.item()) == omoved
    assert np.array_equal(_np(d_part), opart) and np.array_equal(_np(d_size), osize)
    return opart, osize, omoved


def _proposals(n, part, dest_of, gains, seed):
    """want / gain: node v proposes to dest_of[part[v]] listed in `dest_of` (a dict cluster -> (destination, how many of its nodes))."""
    rng = np.random.default_rng(seed)
    want, gain = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for c, (dest, k) in dest_of.items():
        v = rng.permutation(np.nonzero(part == c)[0])[:k]
        want[v], gain[v] = dest, rng.choice(gains, len(v))
    return want, gain


@pytest.mark.parametrize("gains", [[1], [1, 2, 3], [1, 70000, 2 ** 30]], ids=["equal", "mixed", "wide"])
def test_buckets_below_at_and_above_the_free_room(gains):
    """Four clusters of 100 nodes, cap 110: cluster 1 gets 5 proposers, cluster 2 exactly 10, cluster 3 thirty (mixed gains straddle
    the cut-off), cluster 0 none; then the same with no room at all."""
    ops = _ops()
    n, P = 400, 4
    part = np.arange(n) % P
    want, gain = _proposals(n, part, {0: (1, 5), 1: (2, 10), 2: (3, 30)}, gains, seed=len(gains))
    _, size, moved = _check_admit(ops, want, gain, part, P, 110)
    assert moved == 25 and size.tolist() == [95, 95, 100, 110]
    assert _check_admit(ops, want, gain, part, P, 100)[2] == 0              # free = 0 everywhere
    assert _check_admit(ops, want, gain, part, P, 90)[2] == 0               # cap below the sizes: free = 0, not negative
    assert _check_admit(ops, want, gain, part, P, 101)[2] == 3


def test_twenty_thousand_equal_proposers_for_seven_places():
    ops = _ops()
    n = 20050
    part = np.zeros(n, dtype=np.int64)
    part[:50] = 1
    want, gain = np.where(part == 0, 1, -1), np.where(part == 0, 1, 0)
    opart, size, moved = _check_admit(ops, want, gain, part, 2, 57)
    assert moved == 7 and np.nonzero(opart != part)[0].tolist() == list(range(50, 57)) and size.tolist() == [19993, 57]


@pytest.mark.parametrize("free", [1, 255, 4000, 14999])
def test_two_clusters_and_every_node_of_one_proposing(free):
    """P = 2, 30 000 nodes, all 15 000 of cluster 0 propose with gains 1 .. 5: one bucket, the select reaches the low digits."""
    ops = _ops()
    n = 30000
    part = np.random.default_rng(7).permutation(n) % 2
    want, gain = _proposals(n, part, {0: (1, 15000)}, [1, 2, 3, 4, 5], seed=8)
    assert _check_admit(ops, want, gain, part, 2, 15000 + free)[2] == free


def test_many_destinations_with_full_buckets():
    """1 000 clusters of 20, every node proposing to the next cluster with room for 3: a thousand listed buckets."""
    ops = _ops()
    n, P = 20000, 1000
    part = np.arange(n) % P
    rng = np.random.default_rng(9)
    want, gain = (part + 1) % P, rng.integers(1, 4, n)
    assert _check_admit(ops, want, gain, part, P, 23)[2] == 3 * P


# ---------------------------------------------------------------------------------------------------- the cut
def test_cut_against_the_oracle():
    ops = _ops()
    cases = [PO.planted(500, 8, 3, 1, seed=1, hub=11, hub_degree=5000, dups=200, loops=30)[:2],
             PO.csr(_rows_of(_LIMIT_DEGREES + [1023, 1024, 1025], 3000, seed=4)),
             PO.csr([[], [1, 1], [0]])]
    for ip, ix in cases:
        n = len(ip) - 1
        for P in (1, 2, min(9, n), n):
            part = np.random.default_rng(P).integers(0, P, n)
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            cut = ops.partition_cut(_dev(ip, np.int64), _dev(ix, np.int32), n, _dev(part, np.int32), P, status=status)
            assert cut.dtype == torch.int64 and int(cut.item()) == PO.cut(ip, ix, part, P) and int(status.item()) == 0
            assert P > 1 or int(cut.item()) == 0


# ---------------------------------------------------------------------------------------------------- the driver and its users
@pytest.fixture(scope="module")
def planted_4000():
    ip, ix, _ = PO.planted(4000, 16, 4, 1, seed=11)
    start = PO.balanced_random(4000, 16, 12)
    return ip, ix, start, PO.refine(ip, ix, start, 16, PO.default_cap(4000, 16), 10)


def test_refine_partition_equals_the_oracle_twice(planted_4000):
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.cluster import refine_partition
    ip, ix, start, (opart, oinfo) = planted_4000
    g = DeviceGraph.from_csr(ip, ix)
    runs = [refine_partition(g, torch.from_numpy(start), 16, rounds=10) for _ in range(2)]
    for part, info in runs:
        assert part.dtype == torch.int32 and part.is_cuda and np.array_equal(_np(part), opart)
        assert info["cap"] == 275 and {k: info[k] for k in oinfo} == oinfo
    assert oinfo["cuts"][oinfo["round"]] < 0.75 * oinfo["cuts"][0] and len(oinfo["moved"]) == 10
    part, info = refine_partition(g, torch.from_numpy(start), 16, rounds=0)
    assert np.array_equal(_np(part), start) and info["round"] == 0 and info["moved"] == [] and info["cuts"] == oinfo["cuts"][:1]
    part, info = refine_partition(g, torch.from_numpy(start), 16, rounds=10, cap=250)      # no room anywhere: the first round moves nothing
    assert np.array_equal(_np(part), start) and info["moved"] == [0] and info["round"] == 0


def test_cluster_data_lp_feeds_the_loader(planted_4000):
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.cluster import ClusterData, ClusterLoader, make_partition
    ip, ix, _, _ = planted_4000
    g = DeviceGraph.from_csr(ip, ix)
    cd = ClusterData(g, 16, method="lp", seed=5, lp_start="random", lp_rounds=10)
    start = make_partition(4000, 16, "random", 5).numpy()
    opart, oinfo = PO.refine(ip, ix, start, 16, PO.default_cap(4000, 16), 10)
    assert np.array_equal(_np(cd.part), opart) and {k: cd.lp_info[k] for k in oinfo} == oinfo
    assert ClusterData(g, 16, method="random", seed=5).lp_info is None
    clusters = [3, 11, 0, 7]
    b = ClusterLoader(cd, 4, seed=1).batch(clusters)
    ob = CO.batch(ip, ix, opart, 16, clusters)
    assert b.num_nodes == ob.n and np.array_equal(_np(b.node_idx), ob.node_idx) and np.array_equal(_np(b.edge_index), ob.edge_index)
    assert np.array_equal(_np(b.e_id), ob.e_id) and np.array_equal(_np(b.rowptr), ob.rowptr)
    before = ClusterLoader(ClusterData(g, 16, method="random", seed=5), 4, seed=1).batch(clusters)
    assert b.edge_index.shape[1] > before.edge_index.shape[1] == CO.batch(ip, ix, start, 16, clusters).e
    polished = ClusterData(g, 16, part=torch.from_numpy(opart), method="lp", lp_rounds=3)  # a given part is refined too
    assert polished.lp_info["cuts"][0] == oinfo["cuts"][oinfo["round"]]
    assert polished.lp_info["cuts"][polished.lp_info["round"]] <= polished.lp_info["cuts"][0]


def test_cli_two_epochs_on_a_refined_partition(capsys, tmp_path):
    _ops()
    from grapes_amd import clustergcn, partition
    argv = ["--dataset", "cora", "--num_parts", "16", "--batch_size", "4", "--partition", "lp:5", "--max_epoch", "2",
            "--hidden_dim", "32", "--seed", "1"]
    v = clustergcn.main(argv)
    out = capsys.readouterr().out
    assert out.count("Epoch: ") == 2 and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0
    line = [s for s in out.splitlines() if s.startswith("Partition: label propagation, cut ")]
    assert len(line) == 1
    a, b = (int(x) for x in line[0].split("cut ")[1].split(" (")[0].split(" -> "))
    assert b <= a
    path = tmp_path / "part.npy"
    part, info = partition.main(["--dataset", "cora", "--num_parts", "16", "--rounds", "5", "--seed", "1", "--out", str(path)])
    assert capsys.readouterr().out.strip() == line[0]                      # the same start, rounds and rule: the same three numbers
    saved = np.load(path)
    assert saved.dtype == np.int32 and np.array_equal(saved, _np(part)) and saved.min() >= 0 and saved.max() < 16
    assert np.array_equal(clustergcn.load_partition(str(path)).numpy(), saved)
