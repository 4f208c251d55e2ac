"""Cluster-GCN on the MI355X against tests/cluster_oracle.py: every integer output of the cluster-union batch bit for bit (cptr, node_idx,
the local row pointers through n_cap, the edge lists, e_id, the counts) over hand graphs, a hub row cut over many work items, a random
graph with uneven clusters, capacities, bad cluster lists, stale membership across calls and across the serial's wrap, a node set past
grapes_saint_subgraph's limit and a cluster list past one scan tile; the aggregation kernels and ClusterGCNConv against fp64, judged by
the project's measure (sage_oracle.rel_err) at the tolerances tests/test_sage_gpu.py applies, 1e-5 and 1e-4; one trainer step against
fp64 rebuilt from the oracle's batch; evaluate; and the command line."""
import numpy as np
import pytest
import torch

from tests import cluster_oracle as CO
from tests import sage_oracle as SGO

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4                                           # tests/test_sage_gpu.py's
F32, F64 = np.float32, np.float64
MARK, FMARK = -7, -123.0
EDGE, NODE, BAD = 1, 2, 4                                                # the status bits


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(4321)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


class _Tables:
    """The graph and its partition tables on the device, with one membership table and its serial (as ClusterLoader keeps them)."""

    def __init__(self, ip, ix, part, P):
        self.ip, self.ix, self.part, self.P, self.N = ip, ix, list(part), P, len(ip) - 1
        perm, partptr, where = CO.partition_tables(part, P)
        i32 = lambda a: _dev(np.asarray(a, dtype=np.int32))
        self.d = (_dev(np.asarray(ip, dtype=np.int64)), i32(ix), i32(perm), i32(partptr), i32(where))
        self.stamp = torch.zeros((P, 2), dtype=torch.int32, device="cuda")
        self.serial = 0

    def run(self, ops, clusters, n_cap, e_cap, pad=5, item_cap=None):
        """The device call into buffers `pad` entries longer than their capacities, filled with MARK -> (outputs as numpy, status)."""
        q = len(clusters)
        mk = lambda shape, dt=torch.int32: torch.full(shape if isinstance(shape, tuple) else (shape,), MARK, dtype=dt, device="cuda")
        out = (mk(q + 1 + pad), mk(n_cap + pad), mk(n_cap + 1 + pad), mk((2, e_cap + pad)), mk(e_cap + pad, torch.int64), mk(1), mk(1))
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.serial += 1
        rowptr, col, perm, partptr, where = self.d
        ops.cluster_batch(rowptr, col, self.N, perm, partptr, where, _dev(np.asarray(clusters, dtype=np.int32)), self.stamp, self.serial,
                          n_cap, e_cap, item_cap=item_cap, status=status, out=out)
        return [_np(t) for t in out], int(status.item())

    def oracle(self, clusters, **kw):
        return CO.batch(self.ip, self.ix, self.part, self.P, clusters, **kw)

    def check(self, ops, clusters, n_cap=None, e_cap=None, expect_status=0):
        """A call with the given capacities (None: exactly what the batch needs) against the oracle under the same ones."""
        room = self.oracle(clusters)
        nc = max(room.n, 1) if n_cap is None else n_cap
        ec = max(room.e, 1) if e_cap is None else e_cap
        ob = self.oracle(clusters, n_cap=nc, e_cap=ec)
        got, status = self.run(ops, clusters, nc, ec)
        assert status == ob.status == expect_status
        _same(got, ob, len(clusters), nc, ec)
        return ob


def _same(got, ob, q, n_cap, e_cap):
    """Every integer output against the oracle's batch ob, and the guard values behind the capacities."""
    cptr, node_idx, rowptr_l, ei, e_id, d_n, d_e = got
    assert int(d_n[0]) == ob.n and int(d_e[0]) == ob.e
    assert np.array_equal(cptr[:q + 1], ob.cptr) and (cptr[q + 1:] == MARK).all()
    assert np.array_equal(node_idx[:ob.n], ob.node_idx) and (node_idx[ob.n:] == MARK).all()
    assert np.array_equal(rowptr_l[:n_cap + 1], ob.rowptr_full) and (rowptr_l[n_cap + 1:] == MARK).all()
    assert np.array_equal(ei[:, :ob.e], ob.edge_index) and np.array_equal(e_id[:ob.e], ob.e_id)
    assert (ei[:, ob.e:] == MARK).all() and (e_id[ob.e:] == MARK).all()


# ---------------------------------------------------------------------------------------------------- hand graphs
def _star(leaves, P):
    """Node 0 is the hub with `leaves` entries; every leaf stores the hub.  Cluster 0 = the hub and the leaves 1 .. 9; the other
    leaves go round the clusters 1 .. P - 1."""
    ip, ix = CO.csr([list(range(1, leaves + 1))] + [[0] for _ in range(leaves)])
    part = [0] * 10 + [1 + (v % (P - 1)) for v in range(10, leaves + 1)]
    return (ip, ix), part, P


_HAND = {
    "path": (CO.csr([[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]), [0, 1, 0, 2, 1, 2], 3),
    "isolated_nodes": (CO.csr([[1], [0], [], [], [5], [4], []]), [0, 1, 1, 0, 2, 0, 2], 3),
    "duplicates_and_loops": (CO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0]]), [1, 0, 1, 2], 3),
    "empty_cluster": (CO.csr([[1, 2], [0], [0, 3], [2]]), [0, 2, 2, 3], 4),                       # cluster 1 holds no node
    "one_cluster": (CO.csr([[1, 2, 0], [0], [0, 1, 1]]), [0, 0, 0], 1),
    "star": _star(300, 7),          # a row longer than a wavefront, than GRAPES_LONG_ROW and than one work item
}


@pytest.mark.parametrize("name", list(_HAND))
def test_hand_graphs(name):
    ops = _ops()
    (ip, ix), part, P = _HAND[name]
    T = _Tables(ip, ix, part, P)
    lists = [[c] for c in range(P)] + [list(range(P)), list(range(P))[::-1]]
    if name == "empty_cluster":
        lists += [[0, 2], [1, 3], [3, 1, 0]]                              # the empty cluster unchosen, chosen, chosen in the middle
    if name == "star":
        lists += [[0, 2, 5], [5, 0], [3, 1, 4]]                           # the hub with its leaves' clusters partly chosen; leaves alone
    for clusters in lists:
        ob = T.check(ops, clusters)
        assert ob.n == sum(part.count(c) for c in clusters)
    if name == "star":
        assert T.oracle([0, 2, 5]).e == 2 * (sum(part.count(c) for c in (0, 2, 5)) - 1) and T.oracle([3, 1, 4]).e == 0
    whole = T.oracle(list(range(P)))
    assert whole.e == len(ix) and np.array_equal(np.sort(whole.e_id), np.arange(len(ix)))


def test_a_row_of_many_items_straddles_e_cap():
    """A hub of 1 000 entries = 16 work items whose kept entries (about half) straddle e_cap: the first e_cap edges exactly."""
    ops = _ops()
    (ip, ix), part, P = _star(1000, 5)
    T = _Tables(ip, ix, part, P)
    full = T.oracle([0, 1, 3])
    hub_kept = int(full.rowptr[1] - full.rowptr[0])
    assert 400 < hub_kept < 600 and full.node_idx[0] == 0
    for e_cap in (hub_kept // 2, hub_kept // 2 + 37, 64, 65, hub_kept, hub_kept + 3):
        ob = T.check(ops, [0, 1, 3], e_cap=e_cap, expect_status=EDGE)
        assert ob.e == e_cap and np.array_equal(ob.edge_index, full.edge_index[:, :e_cap])
    T.check(ops, [0, 1, 3], e_cap=full.e)
    few = T.oracle([0, 1, 3], n_cap=full.n, e_cap=full.e, item_cap=5)    # room for 5 work items only: the hub's first 320 entries
    got, status = T.run(ops, [0, 1, 3], full.n, full.e, item_cap=5)
    assert status == few.status == EDGE and few.e < hub_kept
    _same(got, few, 3, full.n, full.e)


_R = {}


def _random():
    """N = 2 000, about 8 entries per row (duplicates, loops, stored order random), P = 37 clusters of uneven sizes."""
    if "t" not in _R:
        ip, ix = CO.random_graph(2000, 8, 31)
        part = np.random.default_rng(32).integers(0, 37, 2000) ** 2 // 37        # uneven: the low clusters are larger
        _R["t"] = _Tables(ip, ix, part.tolist(), 37)
    return _R["t"]


def test_random_graph_and_capacities():
    ops = _ops()
    T = _random()
    sizes = np.bincount(T.part, minlength=37)
    assert sizes.max() > 3 * max(sizes.min(), 1)
    clusters = [20, 3, 36, 0, 11]
    full = T.check(ops, clusters)
    assert full.n > 300 and full.e > 100
    T.check(ops, clusters, n_cap=full.n + 9, e_cap=full.e + 4)           # room to spare: rowptr_l = e through n_cap
    cut = T.check(ops, clusters, e_cap=full.e - 1, expect_status=EDGE)
    assert cut.e == full.e - 1 and np.array_equal(cut.edge_index, full.edge_index[:, :-1])
    over = T.check(ops, clusters, n_cap=full.n - 1, expect_status=NODE)
    assert over.n == 0 and over.e == 0
    T.check(ops, clusters[::-1])


def test_bad_cluster_lists_give_an_empty_batch_and_the_next_call_is_exact():
    ops = _ops()
    T = _random()
    good = [5, 9, 2]
    room = T.oracle(good)
    for bad in ([5, -1, 2], [5, 37, 2], [5, 9, 5], [7, 7], [-1], [2, 9, 5, 9, 2]):
        ob = T.check(ops, bad, n_cap=room.n, e_cap=room.e, expect_status=BAD)
        assert ob.n == 0 and ob.e == 0 and not ob.cptr.any() and not ob.rowptr_full.any()
        T.check(ops, good)                                               # the same tables, the stamps of the refused call still in them
    T.check(ops, [9])


def test_a_bad_column_is_reported_and_dropped():
    ops = _ops()
    ip, ix = CO.csr([[1, 9, 2], [0, -3], [0, 2]])
    T = _Tables(ip, ix, [0, 1, 0], 2)
    ob = T.check(ops, [0, 1], expect_status=BAD)
    assert ob.node_idx.tolist() == [0, 2, 1] and ob.e_id.tolist() == [0, 2, 5, 6, 3]           # entries 1 (column 9) and 4 (-3) dropped


# ---------------------------------------------------------------------------------------------------- the loader
def _loader(T, batch_size, **kw):
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.cluster import ClusterData, ClusterLoader
    cd = ClusterData(DeviceGraph.from_csr(T.ip, T.ix), T.P, part=torch.as_tensor(T.part))
    assert np.array_equal(_np(cd.perm), CO.partition_tables(T.part, T.P)[0])
    return ClusterLoader(cd, batch_size, seed=3, **kw)


def _batch_is(b, ob):
    assert b.num_nodes == ob.n and b.edge_index.dtype == torch.int32 and tuple(b.edge_index.shape) == (2, ob.e)
    assert np.array_equal(_np(b.node_idx), ob.node_idx) and np.array_equal(_np(b.cptr), ob.cptr)
    assert np.array_equal(_np(b.rowptr), ob.rowptr) and np.array_equal(_np(b.edge_index), ob.edge_index)
    assert np.array_equal(_np(b.e_id), ob.e_id)


def test_stale_membership_across_calls_and_across_the_serial_wrap():
    _ops()
    T = _random()
    L = _loader(T, 4)
    lists = [[1, 2, 3], [10, 11, 12], [11, 3, 20, 10], [11, 3, 20, 10], [4]]      # disjoint, overlapping, identical
    for clusters in lists:
        _batch_is(L.batch(clusters), T.oracle(clusters))
    assert L.serial == len(lists)
    L.serial = 2 ** 31 - 2                                               # the next call takes the last serial, the one after wraps
    for clusters in lists:
        _batch_is(L.batch(torch.tensor(clusters)), T.oracle(clusters))
    assert L.serial == len(lists) - 1
    L.check()
    assert len(L) == 10 and L.n_cap == int(np.sort(np.bincount(T.part, minlength=37))[-4:].sum())
    seen = []
    for b in L:                                                          # one pass: every cluster once, the last batch short
        assert 1 <= b.clusters.numel() <= 4
        _batch_is(b, T.oracle(_np(b.clusters).tolist()))
        seen += _np(b.clusters).tolist()
    assert sorted(seen) == list(range(37))
    L.check()


def test_loader_grows_its_edge_buffer_and_reports_what_it_cannot_fix():
    _ops()
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules import cluster as MC
    T = _random()
    L = _loader(T, 37)
    L._e_hint = 16                                                       # far too small: doubled until the batch fits
    everything = list(range(37))
    _batch_is(L.batch(everything), T.oracle(everything))
    L.check()
    assert L._e_hint >= MC._E_FLOOR
    fixed = _loader(T, 3, e_cap=10)
    b = fixed.batch([0, 1, 2])
    assert b.edge_index.shape[1] == 10
    with pytest.raises(GrapesHipError, match="cluster loader: edge buffer overflow"):
        fixed.check()
    fixed.batch([0, 0])
    with pytest.raises(GrapesHipError, match="cluster loader: index out of range"):
        fixed.check()
    small = _loader(T, 3, n_cap=5)
    assert small.batch([0, 1]).num_nodes == 0
    with pytest.raises(GrapesHipError, match="node buffer overflow"):
        small.check()
    with pytest.raises(ValueError, match="batch_size is 1 .. 37"):
        _loader(T, 38)


def test_past_the_old_node_limit():
    """n = 20 000 rows: more than the 16 384 ids grapes_saint_subgraph sorts in LDS."""
    ops = _ops()
    N = 40000
    rng = np.random.default_rng(41)
    ip = np.arange(0, 4 * N + 1, 4, dtype=np.int64)
    ix = rng.integers(0, N, 4 * N).astype(np.int32)
    T = _Tables(ip, ix, CO.range_partition(N, 4).tolist(), 4)
    ob = T.check(ops, [3, 1])
    assert ob.n == 20000 > ops.SAINT_MAX_IDS and 30000 < ob.e < 50000


def test_past_one_scan_tile():
    """N = P = 5 000 singleton clusters, q = 4 500: the one-workgroup scan of the sizes takes two tiles of 4 096."""
    ops = _ops()
    N = 5000
    ip, ix = CO.random_graph(N, 5, 43)
    T = _Tables(ip, ix, list(range(N)), N)
    clusters = np.random.default_rng(44).permutation(N)[:4500].tolist()
    ob = T.check(ops, clusters)
    assert ob.n == 4500 and np.array_equal(ob.node_idx, clusters) and ob.e > 10000
    assert ops.CLUSTER_MAX_BATCH_PARTS >= 8192
    T.check(ops, clusters[:4096] + [clusters[0]], n_cap=4500, e_cap=ob.e, expect_status=BAD)      # the duplicate sits in the second tile


def test_two_runs_of_the_batch_give_the_same_bits():
    ops = _ops()
    T = _random()
    a, sa = T.run(ops, [8, 1, 30, 16], 900, 4000)
    b, sb = T.run(ops, [8, 1, 30, 16], 900, 4000)
    assert sa == sb == 0 and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- the aggregation, the layer
_CG = {}


def _cgraph():
    """An edge list [2, e] (row 0 the sources) over 320 nodes: node 0 is isolated (no entry in or out), node 3 is the hub of a 300-leaf
    star (300 entries in, 300 out), (1, 4) is stored twice, the loop (5, 5) twice and (2, 2) once, and 600 random entries go elsewhere."""
    if "g" not in _CG:
        _ops()
        rng = np.random.default_rng(20)
        n = 320
        leaves = list(range(10, 310))
        src = leaves + [3] * 300 + [1, 1, 5, 5, 2]
        dst = [3] * 300 + leaves + [4, 4, 5, 5, 2]
        for _ in range(600):
            src.append(int(rng.integers(1, n))); dst.append(int(rng.integers(1, n)))
        ei = np.array([src, dst], dtype=np.int64)
        _CG["g"] = (n, ei, _dev(ei.astype(np.int32)))
    return _CG["g"]


def _conv_reference(x, ei, wo, b, wr, lam, relu, gate, gout):
    """fp64: the forward with a true ReLU, and the gradients of sum(out * gout) with the ReLU replaced by the device's gates."""
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=F64))
    fwd = CO.conv64(t(x), ei, t(wo), t(b), t(wr), lam, relu=relu).numpy()
    leaves = [t(a).requires_grad_(True) for a in (x, wo, b, wr)]
    out = CO.conv64(leaves[0], ei, leaves[1], leaves[2], leaves[3], lam, gate=gate if relu else None)
    (out * t(gout)).sum().backward()
    return fwd, [l.grad.numpy() for l in leaves]


def _run_conv(f, lam, relu, form, long_rows):
    from grapes_amd.modules.gcn import ClusterGCNConv
    n, ei, ei_d = _cgraph()
    rng = np.random.default_rng(1000 * f + 7)
    torch.manual_seed(1000 * f + 7)                                      # the same weights whatever the form
    conv = ClusterGCNConv(f, f, diag_lambda=lam).cuda()
    with torch.no_grad():
        conv.lin_out.bias.copy_(_dev((rng.standard_normal(f) * 0.5).astype(F32)))
    x32 = rng.standard_normal((n, f)).astype(F32)
    gout = rng.standard_normal((n, f)).astype(F32)
    x = _dev(x32).requires_grad_(True)
    out = conv(x, ei_d, relu=relu, _form=form, _long_rows=long_rows)
    out.backward(_dev(gout))
    fwd, grads = _conv_reference(x32, ei, _np(conv.lin_out.weight), _np(conv.lin_out.bias), _np(conv.lin_root.weight), lam, relu,
                                 _np(out) > 0, gout)
    what = f"f={f} lambda={lam} relu={relu} {form} long={long_rows}"
    errs = {"out": SGO.rel_err(_np(out), fwd), "dx": SGO.rel_err(_np(x.grad), grads[0]),
            "dW_out": SGO.rel_err(_np(conv.lin_out.weight.grad), grads[1]), "db": SGO.rel_err(_np(conv.lin_out.bias.grad), grads[2]),
            "dW_root": SGO.rel_err(_np(conv.lin_root.weight.grad), grads[3])}
    print(f"[cluster] {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.isfinite(out).all()
    assert errs.pop("out") <= ACT_TOL, what
    assert all(v <= GRAD_TOL for v in errs.values()), (what, errs)
    return _np(out), _np(x.grad)


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("f", [7, 64, 260])
def test_clustergcnconv_both_forms_against_fp64(f, lam):
    _ops()
    for relu in (False, True):
        outs = [_run_conv(f, lam, relu, form, long_rows) for form in ("transform", "aggregate") for long_rows in (True, False)]
        for o, _ in outs[1:]:
            assert SGO.rel_err(o, outs[0][0]) <= 2 * ACT_TOL             # all within ACT_TOL of one reference
    a, b = _run_conv(f, lam, True, "transform", True), _run_conv(f, lam, True, "transform", True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])     # fixed order: two runs give the same bits


def test_aggregate_entry_points_strided_blocks_sage_identity_and_refusals():
    """ops.cluster_aggregate_fwd / _bwd on column blocks of wider matrices against fp64; diag_lambda = 0 against
    ops.sage_aggregate_fwd(mean, loops = ones), the second witness; two runs of the backward give the same bits."""
    ops = _ops()
    n, ei, ei_d = _cgraph()
    f = 12
    src_i, dst_i = ei_d[0].contiguous(), ei_d[1].contiguous()
    rng = np.random.default_rng(7)
    wide = rng.standard_normal((n, 3 * f)).astype(F32)                    # dout = columns [0, f), src = [f, 2 f), add = [2 f, 3 f)
    bias = rng.standard_normal(f).astype(F32)
    w_d = _dev(wide)
    x64 = torch.as_tensor(wide[:, f:2 * f].astype(F64))
    prep = ops.PreparedGraph(src_i, dst_i, n)
    s = 1.0 / CO.degrees(ei, n)
    ns, nd = CO._noloop(ei)
    for lam in (0.0, 0.5):
        for long_rows in (True, False):
            out = torch.full((n, 2 * f), FMARK, device="cuda")
            ops.cluster_aggregate_fwd(w_d[:, f:2 * f], prep, lam, add=w_d[:, 2 * f:], bias=_dev(bias), relu=True, out=out[:, f:],
                                      copy_out=out[:, :f], long_rows=long_rows)
            ref = (CO.propagate64(x64, ei, n, lam).numpy() + wide[:, 2 * f:] + bias).clip(min=0)
            got = _np(out)
            assert SGO.rel_err(got[:, f:], ref) <= ACT_TOL and np.array_equal(got[:, :f], wide[:, f:2 * f])
            dh = torch.full((n, 2 * f), FMARK, device="cuda")
            _, _, dbias = ops.cluster_aggregate_bwd(w_d[:, :f], prep, lam, relu_out=out[:, f:], add=w_d[:, 2 * f:], dsrc=dh[:, :f],
                                                    dadd=dh[:, f:], want_bias=True, long_rows=long_rows)
            g = wide[:, :f].astype(F64) * (got[:, f:] > 0)
            want = (1.0 + lam) * s[:, None] * g + wide[:, 2 * f:]
            np.add.at(want, ns, s[nd][:, None] * g[nd])
            gh = _np(dh)
            assert SGO.rel_err(gh[:, :f], want) <= GRAD_TOL and SGO.rel_err(gh[:, f:], g) <= ACT_TOL
            assert SGO.rel_err(_np(dbias), g.sum(0)) <= GRAD_TOL
            again = ops.cluster_aggregate_bwd(w_d[:, :f], prep, lam, relu_out=out[:, f:], add=w_d[:, 2 * f:], want_bias=True,
                                              long_rows=long_rows)
            assert torch.equal(again[0], dh[:, :f]) and torch.equal(again[2], dbias)
    prep.loops = torch.ones(n, dtype=torch.int32, device="cuda")          # SAGE's mean over the row and ONE loop per node
    for long_rows in (True, False):
        for relu in (False, True):
            c = ops.cluster_aggregate_fwd(w_d[:, f:2 * f], prep, 0.0, add=w_d[:, 2 * f:], bias=_dev(bias), relu=relu, long_rows=long_rows)
            sg = ops.sage_aggregate_fwd(w_d[:, f:2 * f], prep, "mean", add=w_d[:, 2 * f:], bias=_dev(bias), relu=relu, long_rows=long_rows)
            assert SGO.rel_err(_np(c), _np(sg).astype(F64)) <= ACT_TOL
    with pytest.raises(ValueError, match="not built"):
        ops.cluster_aggregate_fwd(torch.zeros(n, 258, device="cuda"), prep)
    with pytest.raises(ValueError, match="not built"):
        ops.cluster_aggregate_bwd(torch.zeros(n, 258, device="cuda"), prep)
    from grapes_amd.modules.gcn import ClusterGCNConv
    with pytest.raises(ValueError, match="not built"):
        ClusterGCNConv(258, 258)
    with pytest.raises(ValueError, match="not built"):
        ClusterGCNConv(258, 16).cuda()(torch.zeros(n, 258, device="cuda"), ei_d, _form="aggregate")


def test_state_dict_keys():
    _ops()
    from grapes_amd.modules.gcn import ClusterGCN, ClusterGCNConv
    conv = ClusterGCNConv(12, 20, diag_lambda=0.5).cuda()
    assert list(conv.state_dict()) == ["lin_out.weight", "lin_out.bias", "lin_root.weight"]
    assert conv.lin_out.weight.shape == (20, 12) and conv.lin_root.weight.shape == (20, 12) and conv.lin_out.bias.shape == (20,)
    m = ClusterGCN(12, [20, 4])
    assert list(m.state_dict()) == [f"convs.{i}.{k}" for i in (0, 1) for k in ("lin_out.weight", "lin_out.bias", "lin_root.weight")]
    m2 = ClusterGCN(12, [20, 4])
    m2.load_state_dict(m.state_dict())


# ---------------------------------------------------------------------------------------------------- trainer, evaluate, CLI
def _params(model):
    return [tuple(_np(p).astype(F64) for p in (c.lin_out.weight, c.lin_out.bias, c.lin_root.weight)) for c in model.convs]


def _entries(ip, ix):
    """The CSR's entries as an edge list [2, nnz]: row 0 the neighbours (sources), row 1 the rows (targets)."""
    return np.array([np.asarray(ix, dtype=np.int64), np.repeat(np.arange(len(ip) - 1), np.diff(ip))])


def test_trainer_step_against_fp64():
    """One ClusterTrainer.step with Adam, judged as tests/test_sage_gpu.py judges SageTrainer's: the loss and the gradients against
    fp64 on the device's ReLU gates, rebuilt from the ORACLE's batch; the parameters against Adam's first step where the gradient's
    sign is certain."""
    _ops()
    from grapes_amd.clustergcn import ClusterTrainer
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.cluster import ClusterData
    from grapes_amd.modules.gcn import ClusterGCN, ClusterGCNConv
    from tests import ladies_oracle as LO
    n, F, H, C, P, lr, lam = 256, 32, 16, 4, 8, 1e-3, 0.5
    ip, ix = LO.random_symmetric(n, 8, 51, loops=6)
    rng = np.random.default_rng(52)
    part = rng.integers(0, P, n)
    x32 = rng.standard_normal((n, F)).astype(F32)
    labels = rng.integers(0, C, n)
    train = rng.random(n) < 0.5
    model = ClusterGCN(F, [H, C], diag_lambda=lam).cuda()
    p0 = _params(model)
    cd = ClusterData(DeviceGraph.from_csr(ip, ix), P, part=torch.as_tensor(part))
    tr = ClusterTrainer(cd, _dev(x32), _dev(labels), _dev(train), model, torch.optim.Adam(model.parameters(), lr=lr), batch_size=3, seed=8)
    clusters = [6, 1, 4]
    loss, b = tr.step(clusters)
    ob = CO.batch(ip, ix, part.tolist(), P, clusters)
    _batch_is(b, ob)
    xb = x32[ob.node_idx]
    with torch.no_grad():                                                # the device's ReLU gates of the hidden layer, from p0
        c0 = ClusterGCNConv(F, H, diag_lambda=lam).cuda()
        c0.load_state_dict({"lin_out.weight": _dev(p0[0][0].astype(F32)), "lin_out.bias": _dev(p0[0][1].astype(F32)),
                            "lin_root.weight": _dev(p0[0][2].astype(F32))})
        gate = _np(c0(_dev(xb), b.edge_index, relu=True) > 0)
    rows = np.nonzero(train[ob.node_idx])[0]
    assert 10 < len(rows) < ob.n
    l64, grads, _ = CO.train_step64(xb, p0, ob.edge_index, rows, labels[ob.node_idx[rows]], lam, gates=[gate])
    assert abs(float(loss) - l64) <= ACT_TOL * max(1.0, abs(l64))
    names = ("lin_out.weight", "lin_out.bias", "lin_root.weight")
    for li, conv in enumerate(model.convs):
        for name, before, g64 in zip(names, p0[li], grads[li]):
            mod, attr = name.split(".")
            p = getattr(getattr(conv, mod), attr)
            err = SGO.rel_err(_np(p.grad), g64)
            step = _np(p).astype(F64) - before
            sure = np.abs(g64) > 2 * GRAD_TOL * max(1.0, float(np.abs(g64).max()))
            ref = SGO.adam_first_step64(before, g64, lr=lr)
            perr = SGO.rel_err(_np(p)[sure], ref[sure]) if sure.any() else 0.0
            print(f"[cluster] step convs.{li}.{name}: grad err {err:.2e}, {int(sure.sum())}/{sure.size} sure elements, param err {perr:.2e}")
            assert err <= GRAD_TOL and perr <= GRAD_TOL
            assert sure.any() and np.abs(step).max() <= lr * (1 + 1e-3) + 1e-7 and np.abs(step).max() > 0


def test_evaluate_is_the_exact_full_graph_forward_and_an_epoch_runs():
    _ops()
    from grapes_amd.clustergcn import ClusterTrainer
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.cluster import ClusterData
    from grapes_amd.modules.gcn import ClusterGCN
    from tests import ladies_oracle as LO
    n, F, H, C, lam = 50, 12, 8, 3, 0.25
    ip, ix = LO.random_symmetric(n, 5, 61, loops=3)
    rng = np.random.default_rng(62)
    x32 = rng.standard_normal((n, F)).astype(F32)
    y = rng.integers(0, C, n)
    model = ClusterGCN(F, [H, C], diag_lambda=lam).cuda()
    g = DeviceGraph.from_csr(ip, ix)
    cd = ClusterData(g, 5, method="range")
    train = torch.zeros(n, dtype=torch.bool, device="cuda"); train[::2] = True
    tr = ClusterTrainer(cd, _dev(x32), _dev(y), train, model, torch.optim.Adam(model.parameters(), lr=1e-2), batch_size=2, seed=1)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=F64))
    z64 = CO.forward64(t(x32), [tuple(t(p) for p in layer) for layer in _params(model)], _entries(ip, ix), lam).numpy()
    with torch.no_grad():
        z = _np(model(_dev(x32), g))
    assert SGO.rel_err(z, z64) <= ACT_TOL
    margin = np.sort(z64, 1)
    assert (margin[:, -1] - margin[:, -2]).min() > 1e-4                  # no near-tie: the argmax is the fp64 one
    mask = np.zeros(n, dtype=bool); mask[1::2] = True
    val, test = tr.evaluate((_dev(mask), _dev(~mask)))
    pred = z64.argmax(1)
    assert val == pytest.approx((pred[mask] == y[mask]).mean(), abs=1e-6) and test == pytest.approx((pred[~mask] == y[~mask]).mean(), abs=1e-6)
    assert model.training
    losses = [tr.epoch() for _ in range(3)]
    assert all(np.isfinite(losses)) and tr.loader.serial == 3 * len(tr.loader) == 9
    tr.check()


@pytest.mark.parametrize("partition", ["random", "range", "file"])
def test_cli_two_epochs(partition, capsys, tmp_path):
    _ops()
    from grapes_amd import clustergcn
    argv = ["--dataset", "cora", "--num_parts", "16", "--batch_size", "4", "--partition", partition, "--max_epoch", "2",
            "--hidden_dim", "32", "--diag_lambda", "0.1", "--seed", "1"]
    if partition == "file":
        path = tmp_path / "part.npy"
        np.save(path, (np.arange(2708) % 16).astype(np.int32))
        argv += ["--partition_file", str(path)]
    v = clustergcn.main(argv)
    out = capsys.readouterr().out
    assert out.count("Epoch: ") == 2 and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0
    assert clustergcn.main(argv) == v                                    # one seed, one accuracy
