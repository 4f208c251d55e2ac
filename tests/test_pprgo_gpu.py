"""PPRGo on the MI355X against tests/pprgo_oracle.py.  ops.pprgo_topk: every integer bit for bit with guard values behind m K — hand
graphs, the hub graph of the push rule's table, the edge of the touched-set capacity, batch sizes, a device count below m, repeated and
bad roots, dead slots — and against ops.shadow_ppr_sample on the device.  ops.pprgo_batch: every integer on hand-made slot tables.
ops.pprgo_aggregate_fwd / _bwd against fp64 at the derived bound |err| <= gamma_{c + 1} sum |w z| (c terms; any order, with or
without fma).  The sampler's weights and cache, one trainer step, the power iteration, both evaluate modes and the command line."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pprgo_oracle as GO
from tests import sage_oracle as SG
from tests import shadow_oracle as SO
from tests import shadow_ppr_oracle as PO

pytestmark = pytest.mark.gpu

MARK = -7
EDGE, NODE, BAD = 1, 2, 4                                                # the status bits
ONE, T = 1 << 30, 4096
PAIRS = [(0.25, 2 ** -10), (0.25, 2 ** -12), (0.25, 2 ** -14), (0.5, 2 ** -16), (0.15, 2 ** -20)]
FAR = 1 << 30                                                            # what a dead slot holds where nothing may read it


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _mk(*shape, dt=torch.int32):
    return torch.full(shape, MARK, dtype=dt, device="cuda")


# ---------------------------------------------------------------------------------------------------- topk
def _topk_run(ops, ip, ix, roots, k, aq, thr, max_rounds, live=None, pad=5):
    """The device call into flat buffers `pad` entries longer than m K (and m), filled with MARK -> (outputs as numpy, status)."""
    m, K = len(roots), k + 1
    out = (_mk(m * K + pad), _mk(m * K + pad), _mk(m + pad), _mk(m + pad), _mk(m + pad))
    status = _status()
    d_m = None if live is None else _dev(np.array([live], dtype=np.int32))
    ops.pprgo_topk(_dev(ip), _dev(ix), len(ip) - 1, _dev(np.asarray(roots, dtype=np.int32)), k, aq, thr, max_rounds, d_m=d_m, status=status,
                   out=out)
    return [_np(t) for t in out], int(status.item())


def _topk_same(got, ot, m, K):
    nbr, score, cnt, rounds, stop = got
    assert np.array_equal(nbr[:m * K].reshape(m, K), ot.nbr) and np.array_equal(score[:m * K].reshape(m, K), ot.score)
    assert np.array_equal(cnt[:m], ot.cnt) and np.array_equal(rounds[:m], ot.rounds) and np.array_equal(stop[:m], ot.stop)
    assert all((a[n:] == MARK).all() for a, n in ((nbr, m * K), (score, m * K), (cnt, m), (rounds, m), (stop, m)))


def _topk_check(ops, ip, ix, roots, k, alpha=0.25, eps=2 ** -14, max_rounds=32, live=None, expect_status=0, pushes=None):
    aq, thr = PO.fixed(alpha, eps)
    ot = GO.topk(ip, ix, roots, k, aq, thr, max_rounds, live=live, pushes=pushes)
    got, status = _topk_run(ops, ip, ix, roots, k, aq, thr, max_rounds, live=live)
    assert status == expect_status == (BAD if ot.bad_index else 0)
    _topk_same(got, ot, len(roots), k + 1)
    return ot


def _star(leaves):
    """Node 0 is the centre with `leaves` entries; every leaf stores the centre."""
    return SO.csr([list(range(1, leaves + 1))] + [[0] for _ in range(leaves)])


_HAND = {
    "path": (SO.csr([[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]), [0, 2, 5]),
    "clique": (SO.csr([[u for u in range(9) if u != v] for v in range(9)]), [0, 4, 8]),
    "star_300": (_star(300), [0, 5, 300]),
    "loops_and_duplicates": (SO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0]]), [0, 1, 2, 3]),
    "isolated_root": (SO.csr([[1], [0], [], [3, 3]]), [2, 3, 0]),
    "directed_with_an_empty_row": (SO.csr([[1, 2], [2], [], [0, 2, 2]]), [0, 3, 1, 2]),
}


@pytest.mark.parametrize("name", list(_HAND))
def test_topk_hand_graphs(name):
    ops = _ops()
    (ip, ix), roots = _HAND[name]
    for alpha, eps, k in ((0.25, 2 ** -14, 1), (0.25, 2 ** -14, 5), (0.5, 2 ** -20, 200), (0.15, 2 ** -6, 1023)):
        ot = _topk_check(ops, ip, ix, roots, k, alpha, eps)
        if k == 1023:                                                    # fewer than k candidates: dead slots hold (root, 0)
            assert (ot.cnt < k + 1).all()
        if name == "star_300" and eps <= 2 ** -14:                       # every leaf ties: the k smallest ids win, in id order
            assert ot.nbr[0, :ot.cnt[0]].tolist() == list(range(0, min(k, 300) + 1))
        if name == "isolated_root":
            assert ot.cnt[0] == 1 and ot.score[0, 0] == ONE and (ot.nbr[0] == 2).all() and ot.rounds[0] == 1


_HUB = 7
_G = {}


def _hub_graph():
    """N = 3000, about 8 entries per row, row 7 with 2500: the graph of the push rule's table."""
    if "hub" not in _G:
        _G["hub"] = SO.random_graph(3000, 8, 1, hub=_HUB, hub_degree=2500)
    return _G["hub"]


def _hub_roots():
    ip, ix = _hub_graph()
    return [0, _HUB, int(ix[ip[_HUB]]), 100, 1234, 2999]


@pytest.mark.parametrize("alpha,eps", PAIRS)
def test_topk_hub_graph(alpha, eps):
    ops = _ops()
    ip, ix = _hub_graph()
    pushes = {}
    for k in (1, 32, 200, 1023):
        ot = _topk_check(ops, ip, ix, _hub_roots(), k, alpha, eps, pushes=pushes)
        if (alpha, eps) == (0.25, 2 ** -14):
            assert ot.stop.tolist() == [0, 2, 0, 0, 0, 0]
        if k == 1023 and eps <= 2 ** -12:
            assert ot.cnt.max() >= 600
        if eps == 2 ** -10:
            assert ot.cnt[1] == 1 and ot.rounds[1] == 0                  # the hub root never pushes


def test_topk_stops_at_max_rounds():
    ops = _ops()
    ip, ix = _hub_graph()
    ot = _topk_check(ops, ip, ix, _hub_roots(), 200, 0.25, 2 ** -14, max_rounds=2)
    assert ot.stop.tolist() == [1, 2, 1, 1, 1, 1] and ot.rounds.tolist() == [2, 1, 2, 2, 2, 2]


def test_topk_capacity_edge():
    ops = _ops()
    ip, ix = _star(T - 1)                                                 # |S| + sum deg = 1 + 4095 = T: the round runs
    for k in (5, 1023):
        ot = _topk_check(ops, ip, ix, [0], k)
        assert (ot.rounds[0], ot.stop[0]) == (1, 2) and ot.nbr[0].tolist() == list(range(k + 1)) and ot.cnt[0] == k + 1
    ip, ix = _star(T)                                                     # 1 + 4096 > T: stop 2 at round 0, the root alone
    ot = _topk_check(ops, ip, ix, [0, 1], 1023)
    assert (ot.rounds[0], ot.stop[0], ot.cnt[0]) == (0, 2, 1) and ot.score[0, 0] == ONE >> 2
    ip, ix = _star(5000)                                                  # a leaf root: one round, then the centre's row is too long
    ot = _topk_check(ops, ip, ix, [17], 1023)
    assert (ot.rounds[0], ot.stop[0]) == (1, 2) and ot.nbr[0, :2].tolist() == [17, 0] and ot.cnt[0] == 2


def _many_roots(B, seed=2):
    rng = np.random.default_rng(seed)
    head = _hub_roots() + [3, 3]                                          # a root listed twice
    return (head + rng.integers(0, 3000, max(B - len(head), 0)).tolist())[:B] if B > 1 else [3]


@pytest.mark.parametrize("B", [1, 7, 300])
def test_topk_batch_sizes_and_a_device_count_below_m(B):
    ops = _ops()
    ip, ix = _hub_graph()
    pushes = {}
    _topk_check(ops, ip, ix, _many_roots(B), 32, 0.25, 2 ** -12, pushes=pushes)
    if B > 1:
        ot = _topk_check(ops, ip, ix, _many_roots(B), 32, 0.25, 2 ** -12, live=B - 3, pushes=pushes)
        assert (ot.cnt[B - 3:] == 0).all() and (ot.nbr[B - 3:] == -1).all()


def test_topk_bad_roots_repeated_roots_and_two_calls():
    ops = _ops()
    ip, ix = _hub_graph()
    roots = [1234, 3000, 1234, -1, _HUB, 2 ** 31 - 1, _HUB]
    ot = _topk_check(ops, ip, ix, roots, 200, expect_status=BAD)
    assert ot.cnt[[1, 3, 5]].tolist() == [0, 0, 0] and np.array_equal(ot.nbr[0], ot.nbr[2]) and np.array_equal(ot.score[4], ot.score[6])
    aq, thr = PO.fixed(0.25, 2 ** -14)
    first, s1 = _topk_run(ops, ip, ix, roots, 200, aq, thr, 32)
    again, s2 = _topk_run(ops, ip, ix, roots, 200, aq, thr, 32)
    assert s1 == s2 == BAD and all(np.array_equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("k", [32, 1023])
def test_topk_against_the_ego_net_sampler_on_the_device(k):
    ops = _ops()
    ip, ix = _hub_graph()
    roots = _many_roots(12)
    aq, thr = PO.fixed(0.25, 2 ** -12)
    r = _dev(np.asarray(roots, dtype=np.int32))
    nbr, score, cnt, rounds, stop = (_np(t) for t in ops.pprgo_topk(_dev(ip), _dev(ix), 3000, r, k, aq, thr, 32))
    n_id, ptr, _, _, _, _, _, _, sc, rd, st = (None if t is None else _np(t) for t in ops.shadow_ppr_sample(
        _dev(ip), _dev(ix), 3000, r, k, aq, thr, 32, e_cap=1 << 20, want_e_id=False))
    assert np.array_equal(rounds, rd) and np.array_equal(stop, st) and np.array_equal(cnt, np.diff(ptr))
    for b in range(len(roots)):
        order = np.argsort(nbr[b, :cnt[b]])
        assert np.array_equal(nbr[b, :cnt[b]][order], n_id[ptr[b]:ptr[b + 1]]) and np.array_equal(score[b, :cnt[b]][order], sc[ptr[b]:ptr[b + 1]])


# ---------------------------------------------------------------------------------------------------- batch
def _batch_run(ops, nbr, cnt, N, n_cap, e_cap, scratch=None, pad=5):
    m, K = nbr.shape
    scratch = ops.pprgo_scratch(N, "cuda") if scratch is None else scratch
    out = (_mk(n_cap + pad), _mk(m * K + pad), _mk(n_cap + 1 + pad), _mk(e_cap + pad), _mk(3 + pad))
    status = _status()
    ops.pprgo_batch(_dev(nbr.astype(np.int32)), _dev(cnt.astype(np.int32)), N, scratch, n_cap=n_cap, e_cap=e_cap, status=status, out=out)
    got = [_np(t) for t in out]
    assert (got[4][3:] == MARK).all()
    got = got[:4] + [got[4][0:1], got[4][1:2], got[4][2:3]]
    assert not bool(scratch[0].any())                                     # the bitmap is zero again
    return got, int(status.item())


def _batch_check(ops, nbr, cnt, N, scratch=None, expect_status=0):
    ob = GO.batch(nbr, cnt, N)
    m, K = nbr.shape
    got, status = _batch_run(ops, nbr, cnt, N, max(ob.n, 1), max(ob.e, 1), scratch)
    node_idx, loc, tptr, tslot, d_n, d_e, seg_max = got
    assert status == expect_status == (BAD if ob.bad_index else 0) and int(d_n[0]) == ob.n and int(d_e[0]) == ob.e
    assert int(seg_max[0]) == (int(np.diff(ob.tptr).max()) if ob.n else 0)
    assert np.array_equal(node_idx[:ob.n], ob.node_idx) and np.array_equal(loc[:m * K].reshape(m, K), ob.loc)
    assert np.array_equal(tptr[:ob.n + 1], ob.tptr) and np.array_equal(tslot[:ob.e], ob.tslot)
    assert (node_idx[max(ob.n, 1):] == MARK).all() and (loc[m * K:] == MARK).all() and (tptr[max(ob.n, 1) + 1:] == MARK).all()
    assert (tslot[max(ob.e, 1):] == MARK).all()
    return ob


def _segments_table():
    """65 roots of 5 slots over N = 203 (203 % 64 != 0): sources listed by 1, 63, 64 and 65 roots, ids 0 and N - 1 among them."""
    N, m, K = 203, 65, 5
    nbr = np.full((m, K), FAR, dtype=np.int64)
    for b in range(m):
        row = [100 + b, N - 1]                                            # its own node (a segment of 1), and node N - 1 in all 65 lists
        if b < 64:
            row.append(0)                                                 # node 0 in 64
        if b < 63:
            row.append(50)                                                # node 50 in 63
        nbr[b, :len(row)] = row
    cnt = (nbr != FAR).sum(1)
    return nbr, cnt, N


def test_batch_segment_lengths_around_a_wavefront():
    ops = _ops()
    nbr, cnt, N = _segments_table()
    ob = _batch_check(ops, nbr, cnt, N)
    assert sorted(set(np.diff(ob.tptr).tolist())) == [1, 63, 64, 65] and ob.node_idx[0] == 0 and ob.node_idx[-1] == N - 1


def test_batch_one_source_in_all_of_4096_lists():
    ops = _ops()
    m, N = 4096, 5001
    nbr = np.stack([np.arange(1, m + 1), np.zeros(m, dtype=np.int64), np.full(m, FAR)], axis=1)
    nbr[::7, 1], nbr[::7, 2] = 4500, 0                                    # the hub is not always in the same slot
    cnt = np.where(np.arange(m) % 7 == 0, 3, 2)
    ob = _batch_check(ops, nbr, cnt, N)
    assert ob.tptr[1] - ob.tptr[0] == 4096 and ob.n == 4098


def test_batch_ragged_counts_one_node_and_reused_scratch():
    ops = _ops()
    scratch = ops.pprgo_scratch(130, "cuda")
    scratch[1].fill_(12345)                                               # node_map may hold anything
    rng = np.random.default_rng(11)
    nbr = np.stack([rng.permutation(130)[:9] for _ in range(23)])
    nbr[0, :2], cnt = [0, 129], rng.integers(0, 10, 23)
    cnt[:4] = [9, 0, 1, 0]
    dead = np.arange(9)[None, :] >= cnt[:, None]
    nbr = np.where(dead, FAR, nbr)
    nbr[5, 0] = 77                                                        # (a live slot 0 that the dead slots of its row repeat)
    for _ in range(2):                                                    # two calls in a row on the same scratch
        ob = _batch_check(ops, nbr, cnt, 130, scratch)
    assert ob.node_idx[0] == 0 and ob.node_idx[-1] == 129 and (ob.loc[1] == -1).all() and (ob.loc[2] == ob.loc[2, 0]).all()
    one = _batch_check(ops, np.array([[5, FAR], [5, FAR], [5, FAR]]), np.array([1, 1, 1]), 130, scratch)
    assert one.n == 1 and one.tslot.tolist() == [0, 2, 4] and (one.loc == 0).all()
    none = _batch_check(ops, np.array([[5, 6]]), np.array([0]), 130, scratch)
    assert none.n == 0 and none.e == 0
    bad = _batch_check(ops, np.array([[5, 130, 6], [-1, 5, 6]]), np.array([3, 2]), 130, scratch, expect_status=BAD)
    assert bad.loc.tolist() == [[0, -1, 1], [-1, 0, -1]] and bad.e == 3


def test_batch_capacities_one_below_the_need():
    ops = _ops()
    nbr, cnt, N = _segments_table()
    ob = GO.batch(nbr, cnt, N)
    (node_idx, loc, tptr, tslot, d_n, d_e, _), status = _batch_run(ops, nbr, cnt, N, ob.n, ob.e - 1)
    assert status == EDGE and int(d_n[0]) == ob.n and int(d_e[0]) == ob.e - 1
    assert np.array_equal(node_idx[:ob.n], ob.node_idx) and np.array_equal(loc[:loc.size - 5].reshape(ob.loc.shape), ob.loc)
    assert np.array_equal(tptr[:ob.n + 1], np.minimum(ob.tptr, ob.e - 1)) and (tslot[ob.e - 1:] == MARK).all()
    last = ob.tptr[ob.n - 1]                                              # the last source's segment lost one entry, whichever came last
    assert np.array_equal(tslot[:last], ob.tslot[:last]) and set(tslot[last:ob.e - 1].tolist()) < set(ob.tslot[last:].tolist())
    (node_idx, loc, tptr, tslot, d_n, d_e, _), status = _batch_run(ops, nbr, cnt, N, ob.n - 1, ob.e)
    assert status & NODE and int(d_n[0]) == ob.n - 1
    assert np.array_equal(node_idx[:ob.n - 1], ob.node_idx[:ob.n - 1]) and (node_idx[ob.n - 1:] == MARK).all()
    assert (tptr[ob.n:] == MARK).all() and (tslot[ob.e:] == MARK).all() and int(d_e[0]) == ob.e - 65      # node N - 1 was dropped


# ---------------------------------------------------------------------------------------------------- aggregate
def _table(rng, m, K, pool, ragged=True):
    nbr = np.stack([rng.permutation(pool)[:K] for _ in range(m)])
    cnt = rng.integers(0, K + 1, m) if ragged else np.full(m, K)
    cnt[0], cnt[-1] = K, K                                                # full rows too; ragged ones include 0 and 1 now and then
    if m > 3:
        cnt[1], cnt[2] = 0, 1
    return nbr, cnt


def _gather_case(ops, rng, m, K, F, nbr=None, cnt=None, N=None):
    """Forward and backward on one table against fp64 at gamma_{c + 1} sum |w z|; dead slots hold NaN weights and loc = 2^30, the
    rows of z nothing names are NaN; two runs give the same bits.  Returns the two largest ratios err / bound."""
    if nbr is None:
        N = max(K + 7, 150)
        nbr, cnt = _table(rng, m, K, N)
    ob = GO.batch(nbr, cnt, N)
    live = np.arange(K)[None, :] < cnt[:, None]
    w = np.where(live, rng.standard_normal((m, K)), np.nan).astype(np.float32)
    loc = np.where(live, ob.loc, FAR).astype(np.int32)
    z = rng.standard_normal((ob.n + 2, F)).astype(np.float32)
    z[ob.n:] = np.nan                                                     # two rows that no slot names
    g = rng.standard_normal((m, F)).astype(np.float32)
    dw, dloc, dcnt, dz_, dg = _dev(w), _dev(loc), _dev(cnt.astype(np.int32)), _dev(z), _dev(g)
    status = _status()
    out = ops.pprgo_aggregate_fwd(dz_, dw, dloc, dcnt, status=status)
    out2 = ops.pprgo_aggregate_fwd(dz_, dw, dloc, dcnt, status=status)
    dz = ops.pprgo_aggregate_bwd(dg, dw, _dev(ob.tptr), _dev(ob.tslot), ob.n, ob.e, status=status)
    dz2 = ops.pprgo_aggregate_bwd(dg, dw, _dev(ob.tptr), _dev(ob.tslot), ob.n, ob.e, status=status)
    assert int(status.item()) == 0 and torch.equal(out, out2) and torch.equal(dz, dz2)
    assert out.shape == (m, F) and dz.shape == (ob.n, F) and torch.isfinite(out).all() and torch.isfinite(dz).all()
    w0 = np.where(live, w, 0.0)
    ref, mag = GO.aggregate_fwd(z[:ob.n], w0, ob.loc, cnt)
    bound = GO.gamma(cnt + 1)[:, None] * mag
    err = np.abs(_np(out).astype(np.float64) - ref)
    assert (err <= bound).all(), (m, K, F, float((err - bound).max()))
    rref, rmag = GO.aggregate_bwd(g, w0, ob.tptr, ob.tslot, K)
    rbound = GO.gamma(np.diff(ob.tptr) + 1)[:, None] * rmag
    rerr = np.abs(_np(dz).astype(np.float64) - rref)
    assert (rerr <= rbound).all(), (m, K, F, float((rerr - rbound).max()))
    assert (_np(out)[cnt == 0] == 0).all()
    ratio = lambda e, b: float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    return ratio(err, bound), ratio(rerr, rbound)


@pytest.mark.parametrize("F", [1, 3, 4, 47, 64, 100, 256, 260, 1024])
def test_aggregate_against_fp64(F):
    ops = _ops()
    rng = np.random.default_rng(100 + F)
    for K in (2, 33, 64, 65, 66, 201, 1024):
        rf, rb = _gather_case(ops, rng, 37, K, F)
        print(f"[pprgo] F {F} K {K}: forward err / bound {rf:.3f}, backward {rb:.3f}")


@pytest.mark.parametrize("F", [3, 64])
def test_aggregate_long_source_segments(F):
    """The backward's chunked segments: 63 / 64 / 65 entries around the threshold, and one source in all of 4096 lists."""
    ops = _ops()
    rng = np.random.default_rng(200 + F)
    nbr, cnt, N = _segments_table()
    _gather_case(ops, rng, 65, 5, F, nbr, cnt, N)
    m = 4096
    nbr = np.stack([np.arange(1, m + 1), np.zeros(m, dtype=np.int64)], axis=1)
    rf, rb = _gather_case(ops, rng, m, 2, F, nbr, np.full(m, 2), m + 1)
    print(f"[pprgo] F {F}, a 4096-long segment: forward err / bound {rf:.3f}, backward {rb:.3f}")


# ---------------------------------------------------------------------------------------------------- the Python layer
def _planted():
    if "planted" not in _G:
        _G["planted"] = PO.planted_graph(600, 6, 0)
    return _G["planted"]


@pytest.mark.parametrize("norm", ["row", "sym", "col"])
def test_the_samplers_batch_weights_and_cache(norm):
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.pprgo import PPRGoSampler
    ip, ix = _hub_graph()
    roots = _many_roots(40)
    k, alpha, eps = 32, 0.25, 2 ** -12
    s = PPRGoSampler(DeviceGraph.from_csr(ip, ix), k=k, alpha=alpha, eps=eps, max_rounds=32, normalization=norm)
    ot = GO.topk(ip, ix, roots, k, *PO.fixed(alpha, eps), 32)
    ob = GO.batch(ot.nbr, ot.cnt, 3000)
    w64 = GO.weights(ip, roots, ot.nbr, ot.score, ot.cnt, norm)

    def same(b):
        assert b.num_nodes == ob.n and b.num_slots == ob.e and np.array_equal(_np(b.node_idx), ob.node_idx)
        assert b.item_cap == (0 if np.diff(ob.tptr).max() <= 64 else ob.e // 64)
        assert np.array_equal(_np(b.nbr), ot.nbr) and np.array_equal(_np(b.cnt), ot.cnt) and np.array_equal(_np(b.loc), ob.loc)
        assert b.score.dtype == torch.uint32 and np.array_equal(_np(b.score.view(torch.int32)), ot.score)
        assert np.array_equal(_np(b.tptr), ob.tptr) and np.array_equal(_np(b.tslot), ob.tslot)
        assert np.array_equal(_np(b.targets), roots) and np.array_equal(_np(b.local_targets), np.arange(40))
        assert np.array_equal(_np(b.rounds), ot.rounds) and np.array_equal(_np(b.stop), ot.stop)
        w = _np(b.weight)
        assert b.weight.dtype == torch.float32 and w.shape == ot.nbr.shape
        if norm == "row":
            assert np.array_equal(w, ot.score.astype(np.float32) * np.float32(2 ** -30))
        else:                                                             # at most five roundings, with room for a 1-ulp sqrt
            assert (np.abs(w.astype(np.float64) - w64) <= 8 * GO.U * np.abs(w64)).all()
        assert (w[np.arange(k + 1)[None, :] >= ot.cnt[:, None]] == 0).all()
    first = s.sample(_dev(np.asarray(roots)))
    s.check()
    same(first)
    s.precompute(_dev(np.unique(np.asarray(roots + [11, 12]))))
    cached = s.sample(_dev(np.asarray(roots)))
    s.check()
    same(cached)
    assert all(torch.equal(getattr(first, f), getattr(cached, f)) for f in ("weight", "loc", "tslot", "nbr", "node_idx"))
    mixed = s.sample(_dev(np.asarray(roots[:5] + [2000])))                # a root outside the table: the whole batch is pushed
    assert np.array_equal(_np(mixed.nbr)[:5], ot.nbr[:5])
    s.check()


def test_the_sampler_raises_on_a_bad_root():
    _ops()
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.pprgo import PPRGoSampler
    ip, ix = _hub_graph()
    s = PPRGoSampler(DeviceGraph.from_csr(ip, ix), k=8)
    s.sample(_dev(np.array([3, 3000])))
    with pytest.raises(GrapesHipError, match="PPRGo sampler: index out of range"):
        s.check()
    s.check()                                                             # cleared


def test_one_trainer_step_runs_the_model_over_the_oracles_batch():
    """Nothing is drawn and the kernels are the same: the step's logits are the model's over the oracle's batch, bit for bit (SGD with
    lr = 0 keeps the parameters).  The gradients are judged against fp64 autograd over the oracle's batch on the device's ReLU gates,
    by tests/test_sage_gpu.py's measure and tolerance."""
    ops = _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.pprgo import PPRGo
    from grapes_amd.pprgo import PPRGoTrainer
    torch.manual_seed(4321)
    n, F, H, C, B, k = 600, 16, 32, 5, 24, 50
    ip, ix = _planted()
    rng = np.random.default_rng(52)
    x32 = rng.standard_normal((n, F)).astype(np.float32)
    x, labels = _dev(x32), rng.integers(0, C, n)
    model = PPRGo(F, [H, C]).cuda()
    alpha, eps = 0.25, 2 ** -12
    tr = PPRGoTrainer(DeviceGraph.from_csr(ip, ix), x, _dev(labels), model, torch.optim.SGD(model.parameters(), lr=0.0), k=k, alpha=alpha,
                      eps=eps, max_rounds=32, batch_size=B)
    roots = rng.permutation(n)[:B]
    seen = {}
    forward = tr._forward
    tr._forward = lambda xb, b: seen.setdefault("logits", forward(xb, b))
    loss, b = tr.step(_dev(roots))
    ot = GO.topk(ip, ix, roots, k, *PO.fixed(alpha, eps), 32)
    ob = GO.batch(ot.nbr, ot.cnt, n)
    w32 = ot.score.astype(np.float32) * np.float32(2 ** -30)
    oracle_batch = SimpleNamespace(node_idx=_dev(ob.node_idx), num_nodes=ob.n, weight=_dev(w32), loc=_dev(ob.loc), cnt=_dev(ot.cnt),
                                   tptr=_dev(ob.tptr), tslot=_dev(ob.tslot))
    with torch.no_grad():
        xb = ops.gather_rows(x, oracle_batch.node_idx)
        want = model(xb, oracle_batch)
        gate = _np(model.lins[0](xb) > 0)
    got = seen["logits"].detach()
    assert got.shape == (B, C) and torch.equal(got, want) and np.isfinite(float(loss))
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in model.parameters())
    W = [torch.as_tensor(_np(l.weight).astype(np.float64)).requires_grad_(True) for l in model.lins]
    h = (torch.as_tensor(x32[ob.node_idx].astype(np.float64)) @ W[0].T) * torch.as_tensor(gate.astype(np.float64))
    z = h @ W[1].T
    live = torch.as_tensor((np.arange(k + 1)[None, :] < ot.cnt[:, None]).astype(np.float64))
    logits = ((torch.as_tensor(w32.astype(np.float64)) * live)[:, :, None] * z[torch.as_tensor(np.maximum(ob.loc, 0).astype(np.int64))]).sum(1)
    l64 = SG.loss64(logits, np.arange(B), labels[roots])
    l64.backward()
    assert abs(float(loss) - float(l64.detach())) <= 1e-5 * max(1.0, abs(float(l64.detach())))
    for lin, w in zip(model.lins, W):
        err = SG.rel_err(_np(lin.weight.grad), w.grad.numpy())
        print(f"[pprgo] step grad err {err:.2e}")
        assert err <= 1e-4
    val, test = tr.evaluate((_dev(np.arange(n) < 50), _dev(np.arange(n) >= 550)), inference="ppr")
    assert 0.0 <= val <= 1.0 and 0.0 <= test <= 1.0 and model.training
    pv, pt = tr.evaluate((_dev(np.arange(n) < 50), _dev(np.arange(n) >= 550)))           # the default: power iteration
    assert 0.0 <= pv <= 1.0 and 0.0 <= pt <= 1.0 and tr.evaluate((_dev(np.arange(n) < 50),), inference="power")[0] == pv and model.training


@pytest.mark.parametrize("norm", ["row", "sym", "col"])
def test_propagate_against_dense_fp64(norm):
    """Every row of the planted graph holds 5 entries and no loop, so S is row-stochastic under all three normalisations and |Q| never
    exceeds ||Z||_inf: a round adds at most gamma_12 ||Z||_inf of rounding (the mean: 4 additions and a scaling; two scale_rows by
    factors that carry a square root's and a reciprocal's rounding; the blend: two products and a sum), and the error carried in
    shrinks by (1 - alpha), so nprop rounds stay inside nprop gamma_12 ||Z||_inf."""
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.pprgo import PPRGo
    ip, ix = _planted()
    A = GO.dense_adjacency(ip, ix)
    assert (A.sum(1) == 5).all() and (np.diag(A) == 0).all()
    Z = np.random.default_rng(9).standard_normal((600, 7)).astype(np.float32)
    alpha, nprop = 0.25, 4
    got = _np(PPRGo.propagate(_dev(Z), DeviceGraph.from_csr(ip, ix), alpha, nprop, norm)).astype(np.float64)
    want = GO.power_iteration(GO.transition(A, norm), Z.astype(np.float64), alpha, nprop)
    err = np.abs(got - want).max()
    print(f"[pprgo] propagate {norm}: err {err:.2e}, bound {nprop * GO.gamma(12) * np.abs(Z).max():.2e}")
    assert err <= nprop * GO.gamma(12) * np.abs(Z).max()
    assert np.array_equal(_np(PPRGo.propagate(_dev(Z), DeviceGraph.from_csr(ip, ix), alpha, 0, norm)), Z)


def test_cli_three_epochs_lower_the_loss(capsys):
    _ops()
    from grapes_amd import pprgo
    v = pprgo.main(["--dataset", "cora", "--max_epoch", "3", "--hidden_dim", "32", "--seed", "1"])
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"Loss: ([0-9.]+)", out)]
    assert out.count("Epoch: ") == 3 and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[2] < losses[0]
