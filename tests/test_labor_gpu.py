"""LABOR on the MI355X against tests/labor_oracle.py: the kept sets bit for bit (Philox words and given per-node keys, every branch
of the kernels: rows around the fanout and around the 64-entry chunk, row counts around the workgroup and scan boundaries), forced
ties, the shared variates, overflow and bad ids, the importance iterations against fp64, the batch, the two routes of the trainer
and the command line.  Logits and gradients are judged by the project's measure (sage_oracle.rel_err) at 1e-5 and 1e-4."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import labor_oracle as LO
from tests import sage_oracle as SO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_TOL, GRAD_TOL = 1e-5, 1e-4
F32, F64 = np.float32, np.float64
MARK, FMARK = -7, 12345.0
N = 200
CHUNK = 64


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


def _keys(words):
    return _dev(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32))


_GRAPHS = {}


def _graph(n=N, seed=11, **kw):
    _ops()
    key = (n, seed, tuple(sorted(kw.items())))
    if key not in _GRAPHS:
        ip, ix, deg = LO.hand_graph(n, seed, **kw)
        _GRAPHS[key] = (ip, ix, deg, _dev(ip), _dev(ix))
    return _GRAPHS[key]


def _rows(m, seed=3):
    """m list rows: the special rows first in a shuffled order (the longest early, so that later offsets are large), then random ones —
    past 200 rows a node is listed twice, and decides twice alike."""
    rng = np.random.default_rng(seed)
    if m == 1:
        return np.array([14])                                            # the row of three chunks and one entry
    head = rng.permutation(len(LO.SPECIAL_DEGREES) + 1)
    return np.concatenate([head, rng.integers(0, N, max(m - len(head), 0))])[:m]


def _sample(ops, rows, fanout, graph=None, d_m=None, **kw):
    ip, ix, deg, rp, col = graph or _graph()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    if "e_cap" not in kw:                                                # the entry count of the rows that exist
        kw["deg_sum"] = int(sum(deg[s] for s in rows if 0 <= s < len(deg)))
    src, dst, pos, w, d_e = ops.labor_sample_layer(rp, col, len(ip) - 1, _dev(np.asarray(rows, dtype=np.int32)), fanout, status=status,
                                                   d_m=None if d_m is None else _dev(np.array([d_m], dtype=np.int32)), **kw)
    e = int(d_e.item())
    return _np(src)[:e].astype(np.int64), _np(dst)[:e].astype(np.int64), _np(pos)[:e], _np(w)[:e], int(status.item())


def _same(got, want, what):
    for g, w, name in zip(got[:3], want[:3], ("src", "dst", "pos")):
        assert np.array_equal(g, w), (what, name)
    assert len(got[0]) == len(want[0]), what                             # d_e
    assert np.allclose(got[3], want[4], rtol=1e-6, atol=0), (what, "weight")


# ------------------------------------------------------------------------------------------------------------ the kept sets
SCAN_TILE = 4096                       # the values one tile of the single-workgroup scans holds (1024 threads x 4)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 4500])
@pytest.mark.parametrize("k", [1, 3, 64])
def test_kept_sets_on_the_philox_words(k, m):
    """m = 1, 255, 256, 257 cross the workgroup boundaries of the per-item kernels; 4500 rows (and their work items) need a second
    tile in both scans."""
    ops = _ops()
    ip, ix, deg, _, _ = _graph()
    rows = _rows(m)
    assert m < SCAN_TILE or int(np.ceil(deg[rows] / CHUNK).sum()) > SCAN_TILE
    base = (1 << 33) + 5 if m == 256 else 7
    words = LO.node_words(77, base, N)
    want = LO.sample_layer(ip, ix, rows, k, words)
    got = _sample(ops, rows, k, philox_seed=77, philox_base=base)
    assert got[4] == 0
    _same(got, want, f"k={k} m={m}")
    assert np.array_equal(ix[got[2]], got[0])                            # edge_pos indexes col back to edge_src
    if m > 1:                                                            # LABOR-0: 1 / kept_s on every entry of a row, exactly
        first = rows[0]
        sel = got[1] == first
        if sel.any():
            n_first = int(sel.sum()) // int((rows == first).sum())
            assert (got[3][sel] == F32(1.0) / F32(n_first)).all()
    if k < 64 and m > 1:
        assert not np.array_equal(_sample(ops, rows, k, philox_seed=78, philox_base=base)[0], got[0])     # another key, other words


@pytest.mark.parametrize("k", [1, 3, 64])
def test_kept_sets_with_given_keys_a_device_row_count_and_every_special_row(k):
    ops = _ops()
    ip, ix, deg, _, _ = _graph()
    rows = _rows(257)
    keys = np.random.default_rng(5 + k).integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    _same(_sample(ops, rows, k, keys=_keys(keys)), LO.sample_layer(ip, ix, rows, k, keys), f"keys k={k}")
    # d_m smaller than m: the rows past it write nothing
    _same(_sample(ops, rows, k, keys=_keys(keys), d_m=100), LO.sample_layer(ip, ix, rows[:100], k, keys), f"d_m k={k}")
    # every special row alone — 0, 1, k, k + 1, 63, 64, 65, 127 .. 129, 192, 193 entries, duplicates and loops — one launch each
    for s in range(len(LO.SPECIAL_DEGREES) + 1):
        got, want = _sample(ops, [s], k, keys=_keys(keys)), LO.sample_layer(ip, ix, [s], k, keys)
        _same(got, want, f"row {s} k={k}")
        assert deg[s] > k or len(got[0]) == deg[s]


def test_forced_ties_zero_keys_and_all_ones_keys():
    ops = _ops()
    ip, ix, deg, _, _ = _graph()
    rows = _rows(64)
    k, d = 3, 64                                                         # r d == k << 32 at r = 3 2^26, on the rows of 64 entries
    tie = (k << 32) // d
    assert tie * d == k << 32
    for word, kept_on_64 in ((tie, 0), (tie - 1, 64)):
        keys = np.full(N, word, dtype=np.uint32)
        got = _sample(ops, rows, k, keys=_keys(keys))
        _same(got, LO.sample_layer(ip, ix, rows, k, keys), f"tie word {word}")
        for s in (7, 15, 16):                                            # the rows of exactly 64 entries
            assert int((got[1] == s).sum()) == kept_on_64 * int((rows == s).sum())
    zero = _sample(ops, rows, k, keys=_keys(np.zeros(N, dtype=np.uint32)))
    assert len(zero[0]) == int(deg[rows].sum())                          # all-zero keys keep everything
    ones = _sample(ops, rows, k, keys=_keys(np.full(N, 0xFFFFFFFF, dtype=np.uint32)))
    assert len(ones[0]) == int(deg[rows][deg[rows] <= k].sum())          # all-ones keys keep only the rows with d <= k
    assert set(ones[1].tolist()) == {int(s) for s in rows if 0 < deg[s] <= k}


def test_rows_that_share_a_vertex_decide_alike_at_equal_thresholds():
    ops = _ops()
    ip, ix, deg, _, _ = _graph()
    rows, k = np.arange(N), 3
    src, dst, pos, w, status = _sample(ops, rows, k, philox_seed=9, philox_base=0)
    assert status == 0
    kept = set(zip(dst.tolist(), src.tolist()))
    pairs = both = 0
    seen = {}
    for s in rows:
        if deg[s] <= k:
            continue
        for t in set(ix[ip[s]:ip[s + 1]].tolist()):
            decision = (s, t) in kept
            prior = seen.setdefault((int(deg[s]), t), decision)          # same degree = same threshold
            assert prior == decision, (s, t)
            pairs += 1
            both += int(decision)
    assert pairs > 500 and 0 < both < pairs
    # duplicates of one entry are kept or dropped together: the kept count of (s, t) is 0 or its multiplicity
    for s in (17,):
        nb = ix[ip[s]:ip[s + 1]]
        for t in set(nb.tolist()):
            assert int(((dst == s) & (src == t)).sum()) in (0, int((nb == t).sum()))


def test_overflow_item_overflow_and_bad_ids():
    ops = _ops()
    ip, ix, deg, rp, col = _graph()
    rows = _rows(64)
    keys = np.random.default_rng(8).integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    want = LO.sample_layer(ip, ix, rows, 3, keys)
    count = len(want[0])
    cap = count - 1
    out = (torch.full((count,), MARK, dtype=torch.int32, device="cuda"), torch.full((count,), MARK, dtype=torch.int32, device="cuda"),
           torch.full((count,), MARK, dtype=torch.int64, device="cuda"), torch.full((count,), FMARK, dtype=torch.float32, device="cuda"),
           torch.zeros(1, dtype=torch.int32, device="cuda"))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.labor_sample_layer(rp, col, N, _dev(rows.astype(np.int32)), 3, e_cap=cap, keys=_keys(keys), deg_sum=int(deg[rows].sum()),
                           status=status, out=out)
    assert int(status.item()) == 1 and int(out[4].item()) == cap
    assert np.array_equal(_np(out[0])[:cap], want[0][:cap]) and np.array_equal(_np(out[2])[:cap], want[2][:cap])
    assert int(out[0][cap]) == MARK and int(out[1][cap]) == MARK and int(out[2][cap]) == MARK and float(out[3][cap]) == FMARK
    # one work item too few: the overflow bit again
    items = int(np.ceil(deg[rows] / CHUNK).sum())
    got = _sample(ops, rows, 3, keys=_keys(keys), e_cap=count, item_cap=items)
    assert got[4] == 0 and np.array_equal(got[0], want[0])
    assert _sample(ops, rows, 3, keys=_keys(keys), e_cap=count, item_cap=items - 1)[4] == 1
    # a column outside [0, N) is reported and never kept; a bad row id is an empty row
    bad_ix = ix.copy()
    a = int(ip[13])                                                      # in the row of 192 entries
    bad_ix[a + 70] = N + 5
    bad_ix[a + 71] = -1
    g = (ip, bad_ix, deg, rp, _dev(bad_ix))
    got = _sample(ops, [13, 3], 64, graph=g, keys=_keys(np.zeros(N, dtype=np.uint32)))
    assert got[4] == 4 and len(got[0]) == 192 + 3 - 2 and (got[0] >= 0).all() and (got[0] < N).all()
    got = _sample(ops, [3, N + 1, -2, 4], 64, keys=_keys(keys))
    assert got[4] == 4
    _same(got, LO.sample_layer(ip, ix, [3, 4], 64, keys), "bad rows")


# ------------------------------------------------------------------------------------------------------------ the importance iterations
N_I = 300


def _igraph():
    return _graph(N_I, 12, special=(500, 0, 1, 3, 4, 40), max_deg=20)


def _irows():
    return np.concatenate([[0], 1 + np.random.default_rng(5).permutation(N_I - 1)[:119]])


def _rel(a, ref):
    return float((np.abs(np.asarray(a, dtype=F64) - ref) / np.abs(ref)).max())


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_importance_against_fp64_then_the_kept_set_given_the_kernels_own_c_and_pi(iters):
    ops = _ops()
    ip, ix, deg, rp, col = _igraph()
    rows, k = _irows(), 3
    d_rows = _dev(rows.astype(np.int32))
    scratch = ops.labor_scratch(N_I, "cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    c, pi = ops.labor_importance(rp, col, N_I, d_rows, k, iters, scratch, status=status)
    c2, pi2 = ops.labor_importance(rp, col, N_I, d_rows, k, iters, scratch, status=status)
    assert int(status.item()) == 0 and not bool(scratch.any())           # the N-sized table is zero again
    touched = np.zeros(N_I, dtype=bool)
    for s in rows:
        touched[ix[ip[s]:ip[s + 1]]] = True
    c, pi = _np(c), _np(pi)
    assert np.array_equal(c, _np(c2)) and np.array_equal(pi[touched], _np(pi2)[touched])         # two runs, the same bits
    c64, pi64 = LO.importance(ip, ix, rows, k, iters, N_I)
    c32, pi32 = LO.importance(ip, ix, rows, k, iters, N_I, dtype=F32)
    big = deg[rows] > k
    assert big.sum() > 50 and (c[~big] == 0).all() and deg[rows[0]] == 500
    own = max(_rel(c32[big], c64[big]), _rel(pi32[touched], pi64[touched]))
    err = max(_rel(c[big], c64[big]), _rel(pi[touched], pi64[touched]))
    print(f"[labor] importance iters={iters}: the oracle's sorted solve in fp32 NumPy is within {own:.3e} of fp64, the kernel {err:.3e}")
    # The bound is 4 x the error of the oracle's own algorithm in fp32 on these inputs (the kernel's sums run in another order).
    # Recorded on the CPU for the oracle: 8.92e-07 (iters 1), 9.31e-07 (iters 2), 3.78e-06 (iters 3); for the kernel on an MI355X:
    # 9.64e-08 (iters 1), 1.52e-07 (iters 2), 2.03e-07 (iters 3).
    assert err <= 4 * own
    # the kept set GIVEN the kernel's own fp32 c and pi: bit for bit; the weights to 1e-6
    words = LO.node_words(31, 9, N_I)
    want = LO.sample_layer(ip, ix, rows, k, words, c, pi)
    src, dst, pos, w, d_e = ops.labor_sample_layer(rp, col, N_I, d_rows, k, philox_seed=31, philox_base=9, c=_dev(c), pi=_dev(pi),
                                                   deg_sum=int(deg[rows].sum()), status=status)
    e = int(d_e.item())
    assert int(status.item()) == 0 and e == len(want[0]) and 0 < e < int(deg[rows].sum())
    assert np.array_equal(_np(src)[:e], want[0]) and np.array_equal(_np(dst)[:e], want[1]) and np.array_equal(_np(pos)[:e], want[2])
    assert np.allclose(_np(w)[:e], want[4], rtol=1e-6, atol=0)
    assert (want[3] < 1).any() and (want[3] == 1).any()                  # saturated and unsaturated entries both occur
    again = ops.labor_sample_layer(rp, col, N_I, d_rows, k, philox_seed=31, philox_base=9, c=_dev(c), pi=_dev(pi),
                                   deg_sum=int(deg[rows].sum()), status=status)
    assert np.array_equal(_np(again[3])[:e], _np(w)[:e])                 # the weights too are the same bits


def test_zero_iterations_give_k_over_d():
    ops = _ops()
    ip, ix, deg, rp, col = _igraph()
    rows = _irows()
    c, pi = ops.labor_importance(rp, col, N_I, _dev(rows.astype(np.int32)), 3, 0, ops.labor_scratch(N_I, "cuda"))
    big = deg[rows] > 3
    assert np.allclose(_np(c)[big], 3.0 / deg[rows][big], rtol=1e-6, atol=0) and (_np(c)[~big] == 0).all()
    for s in rows:
        assert (_np(pi)[ix[ip[s]:ip[s + 1]]] == 1).all()


# ------------------------------------------------------------------------------------------------------------ the sampler
def _device_graph(ip, ix):
    from grapes_amd.graph import DeviceGraph
    return DeviceGraph.from_csr(ip, ix)


def _check_batch(b, ob, what):
    assert np.array_equal(_np(b.node_idx), ob.node_idx) and np.array_equal(_np(b.local_targets), ob.local_targets), what
    assert b.num_nodes == len(ob.node_idx)
    for d, (L, R) in enumerate(zip(b.layers, ob.layers)):
        assert np.array_equal(_np(L.prev), R.prev) and np.array_equal(_np(L.after), R.after), (what, d)
        assert np.array_equal(_np(L.edge_src), R.src) and np.array_equal(_np(L.edge_dst), R.dst), (what, d)
        assert np.array_equal(_np(b.edge_index[d]), ob.edge_index[d]), (what, d)
        assert np.allclose(_np(b.edge_weight[d]), R.w, rtol=1e-6, atol=0), (what, d)


@pytest.mark.parametrize("fanouts", [[3, 2], [-1, 2]])
def test_sampler_batches_layer_dependency_and_the_offset(fanouts):
    _ops()
    from grapes_amd.modules.labor import LaborSampler
    ip, ix, deg, _, _ = _graph()
    g = _device_graph(ip, ix)
    targets = np.random.default_rng(100).permutation(N)[:64]
    per_layer = (N + 3) // 4
    edges = {}
    for dep in (False, True):
        s = LaborSampler(g, fanouts, layer_dependency=dep, seed=21)
        b = s.sample(_dev(targets))
        s.check()
        ob = LO.sample(ip, ix, targets, fanouts, seed=21, layer_dependency=dep)
        _check_batch(b, ob, f"dep={dep}")
        assert b.uniform and s.philox_offset == 2 * per_layer == ob.philox_offset            # advances alike in both settings
        assert (b.layers[0].edge_pos is None) == (fanouts[0] == -1)
        for t in (g.bits, g.prev_bits):
            assert not bool(t.any())                                     # the graph's bitmaps are zero at rest again
        b2 = s.sample(_dev(targets))                                     # the second batch draws from the advanced offset
        _check_batch(b2, LO.sample(ip, ix, targets, fanouts, seed=21, philox_offset=ob.philox_offset, layer_dependency=dep), "second")
        assert s.philox_offset == 4 * per_layer
        edges[dep] = (_np(b.layers[1].edge_src), _np(b.layers[1].edge_dst), ob)
    # with layer_dependency the two layers read identical words, without it different ones
    assert np.array_equal(edges[True][2].layers[0].words, edges[True][2].layers[1].words)
    assert not np.array_equal(edges[False][2].layers[0].words, edges[False][2].layers[1].words)
    assert not (np.array_equal(edges[True][0], edges[False][0]) and np.array_equal(edges[True][1], edges[False][1]))
    # given per-node keys for layer 0
    keys = np.random.default_rng(2).integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    bk = LaborSampler(g, fanouts, seed=21).sample(_dev(targets), keys=[_keys(keys)])
    _check_batch(bk, LO.sample(ip, ix, targets, fanouts, seed=21, keys=[keys]), "keys")


def test_shared_variates_reduce_the_vertices_of_a_layer():
    """A condition, not a measurement.  Fanout 3, 64 targets, seed 0 on the 200-node graph: the oracle's first layer has 89 distinct
    sources under the shared variates against 119 under independent per-entry variates at the same thresholds (both counted on the
    CPU when the seed was chosen); the sampler's count is the oracle's, by bit-exactness."""
    _ops()
    from grapes_amd.modules.labor import LaborSampler
    ip, ix, deg, _, _ = _graph()
    targets = np.random.default_rng(100).permutation(N)[:64]
    shared = len(set(LO.sample_layer(ip, ix, targets, 3, LO.node_words(0, 0, N))[0].tolist()))
    independent = LO.independent_source_count(ip, ix, targets, 3, 0)
    assert (shared, independent) == (89, 119) and shared < independent
    b = LaborSampler(_device_graph(ip, ix), [3], seed=0).sample(_dev(targets))
    assert len(set(_np(b.layers[0].edge_src).tolist())) <= shared


def test_importance_batch_against_the_oracle_given_the_kernels_c_and_pi():
    _ops()
    from grapes_amd.modules.labor import LaborSampler
    ip, ix, deg, _, _ = _igraph()
    g = _device_graph(ip, ix)
    targets = _irows()[:40]
    s = LaborSampler(g, [3, 2], importance_iters=2, seed=4)
    b = s.sample(_dev(targets))
    s.check()
    assert not b.uniform and not bool(s.scratch.any())
    cpi = [(_np(L.c), _np(L.pi)) for L in b.layers]
    _check_batch(b, LO.sample(ip, ix, targets, [3, 2], seed=4, cpi=cpi), "importance")
    c64, _ = LO.importance(ip, ix, targets, 3, 2, N_I)
    big = deg[targets] > 3
    assert _rel(cpi[0][0][big], c64[big]) < 1e-4                         # (the layer's c is the importance kernel's, loosely)


# ------------------------------------------------------------------------------------------------------------ the trainer
def _params(model):
    return [(_np(c.lin_l.weight).copy(), _np(c.lin_l.bias).copy(), _np(c.lin_r.weight).copy()) for c in model.convs]


def _train_graph(n=256):
    from tests import ladies_oracle as LAD
    ip, ix = LAD.random_symmetric(n, 8, 51, loops=6)
    return ip, ix, _device_graph(ip, ix)


def test_uniform_batch_weighted_route_equals_the_sage_route():
    _ops()
    from grapes_amd.labor import LaborTrainer
    from grapes_amd.modules.gcn import SAGE
    from grapes_amd.target_batch import _GatherX, _TargetLoss
    n, F, H, C = 256, 32, 16, 4
    ip, ix, g = _train_graph(n)
    rng = np.random.default_rng(52)
    x, y = _dev(rng.standard_normal((n, F)).astype(F32)), _dev(rng.integers(0, C, n))
    model = SAGE(F, [H, C]).cuda()
    tr = LaborTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=1e-3), fanouts=[5, 3], seed=8)
    b = tr.sampler.sample(_dev(rng.permutation(n)[:32]))
    tr.sampler.check()
    assert b.uniform
    results = []
    for weighted in (False, True):
        model.zero_grad()
        xb = _GatherX.apply(x, b.node_idx, None, None, False)
        z = tr._forward(xb, b, weighted=weighted)
        _TargetLoss.apply(z, b.local_targets, b.targets, y).backward()
        results.append((_np(z), [_np(p.grad).copy() for p in model.parameters()]))
    (z0, g0), (z1, g1) = results
    assert SO.rel_err(z1, z0) <= 1e-5
    for a, ref in zip(g1, g0):
        assert np.abs(ref).max() > 0 and SO.rel_err(a, ref) <= 1e-5


def _weighted_step64(x32, params32, edge_index, weights, local_targets, labels, gates):
    """One step of the weighted route restated in fp64 autograd: act(sum_e w_e x_src W_lᵀ + b + x W_rᵀ), SAGE's routing."""
    x = torch.as_tensor(np.asarray(x32, dtype=F64))
    params = [tuple(torch.as_tensor(np.asarray(p, dtype=F64)).requires_grad_(True) for p in layer) for layer in params32]
    L = len(params)
    for i, (w_l, b_l, w_r) in enumerate(params):
        last = i == L - 1
        q = 0 if last else -(i + 1)
        src, dst = (torch.as_tensor(np.asarray(r, dtype=np.int64)) for r in edge_index[q])
        agg = torch.zeros_like(x).index_add_(0, dst, x[src] * torch.as_tensor(np.asarray(weights[q], dtype=F64))[:, None])
        x = agg @ w_l.T + b_l + x @ w_r.T
        if not last:
            x = x * torch.as_tensor(np.asarray(gates[i], dtype=F64))
    loss = SO.loss64(x, local_targets, labels)
    loss.backward()
    return float(loss.detach()), [tuple(p.grad.numpy() for p in layer) for layer in params], x.detach().numpy()


def test_importance_step_against_fp64():
    """One LaborTrainer.step with importance_iters = 2 and Adam, judged as tests/test_sage_gpu.py judges SageTrainer's: the loss and the
    gradients against fp64 autograd on the device's ReLU gates at 1e-5 / 1e-4, the parameters against the fp64 Adam step where the
    gradient's sign is sure."""
    _ops()
    from grapes_amd.labor import LaborTrainer, weighted_sage
    from grapes_amd.ladies import weighted_structures
    from grapes_amd.modules.gcn import SAGE
    n, F, H, C, B, lr = 256, 32, 16, 4, 32, 1e-3
    ip, ix, g = _train_graph(n)
    rng = np.random.default_rng(52)
    x32 = rng.standard_normal((n, F)).astype(F32)
    labels = rng.integers(0, C, n)
    model = SAGE(F, [H, C]).cuda()
    p0 = _params(model)
    tr = LaborTrainer(g, _dev(x32), _dev(labels), model, torch.optim.Adam(model.parameters(), lr=lr), fanouts=[5, 3],
                      importance_iters=2, seed=8)
    targets = rng.permutation(n)[:B]
    loss, b = tr.step(_dev(targets))
    assert not b.uniform
    node_idx, ei, w = _np(b.node_idx), [_np(e) for e in b.edge_index], [_np(v) for v in b.edge_weight]
    for e, v in zip(ei, w):                                              # Hajek: the weights of every row with an entry sum to 1
        sums = np.bincount(e[1], weights=v.astype(F64), minlength=len(node_idx))
        assert np.allclose(sums[np.unique(e[1])], 1.0, atol=1e-5) and len(v) == e.shape[1]
    xb = x32[node_idx]
    with torch.no_grad():                                                # the device's ReLU gates of the hidden layer, from p0
        m0 = SAGE(F, [H, C]).cuda()
        for conv, (wl, bl, wr) in zip(m0.convs, p0):
            conv.load_state_dict({"lin_l.weight": _dev(wl), "lin_l.bias": _dev(bl), "lin_r.weight": _dev(wr)})
        m0.convs = m0.convs[:1]
        ws = weighted_structures([b.edge_index[-1]], b.num_nodes)
        pre = weighted_sage(m0, _dev(xb), ws, [b.edge_weight[-1]])       # one layer = the last: no ReLU applied
        gate = _np(pre > 0)
    l64, grads, _ = _weighted_step64(xb, p0, ei, w, _np(b.local_targets), labels[targets], [gate])
    assert abs(float(loss) - l64) <= ACT_TOL * max(1.0, abs(l64))
    names = ("lin_l.weight", "lin_l.bias", "lin_r.weight")
    for li, conv in enumerate(model.convs):
        for name, before, g64 in zip(names, p0[li], grads[li]):
            mod, attr = name.split(".")
            p = getattr(getattr(conv, mod), attr)
            err = SO.rel_err(_np(p.grad), g64)
            sure = np.abs(g64) > 2 * GRAD_TOL * max(1.0, float(np.abs(g64).max()))
            ref = SO.adam_first_step64(before, g64, lr=lr)
            perr = SO.rel_err(_np(p)[sure], ref[sure]) if sure.any() else 0.0
            print(f"[labor] step convs.{li}.{name}: grad err {err:.2e}, {int(sure.sum())}/{sure.size} sure elements, param err {perr:.2e}")
            assert err <= GRAD_TOL and perr <= GRAD_TOL and sure.any()


def test_training_lowers_the_loss_and_evaluates():
    _ops()
    from grapes_amd.graphsage import build_model
    from grapes_amd.labor import LaborTrainer
    from tests import ladies_oracle as LAD
    n, F, C = 512, 16, 4
    rng = np.random.default_rng(61)
    y = rng.integers(0, C, n)
    same = [(a, b) for a, b in rng.integers(0, n, (6000, 2)) if y[a] == y[b] and a != b][:1200]     # edges inside the classes
    s, d = np.array([a for a, b in same] + [b for a, b in same]), np.array([b for a, b in same] + [a for a, b in same])
    ip, ix = LAD.csr_from_edges(s, d, n)
    x = (np.eye(C)[y] @ rng.standard_normal((C, F)) * 2.0 + 0.3 * rng.standard_normal((n, F))).astype(F32)
    g = _device_graph(ip, ix)
    train = _dev(np.arange(0, n, 2))
    mask = torch.zeros(n, dtype=torch.bool, device="cuda"); mask[1::2] = True
    for iters in (0, 1):
        model = build_model(F, 16, C, 2, 0.0, "mean", "cuda")
        tr = LaborTrainer(g, _dev(x), _dev(y), model, torch.optim.Adam(model.parameters(), lr=2e-2), fanouts=[4, 3],
                          importance_iters=iters, seed=6)
        losses = [tr.epoch(train, 128) for _ in range(4)]
        print(f"[labor] importance_iters={iters} epoch losses", np.round(losses, 4))
        assert all(np.isfinite(losses)) and losses[-1] < losses[0]
        val, test = tr.evaluate((mask, ~mask))
        assert np.isfinite(val) and np.isfinite(test) and 0.0 <= val <= 1.0 and 0.0 <= test <= 1.0
    with pytest.raises(ValueError, match="fanouts"):
        LaborTrainer(g, _dev(x), _dev(y), model, None, fanouts=[4])
    with pytest.raises(ValueError, match="aggr='mean'"):
        LaborTrainer(g, _dev(x), _dev(y), build_model(F, 16, C, 2, 0.0, "sum", "cuda"), None, fanouts=[4, 3])


def test_cli_two_epochs_in_a_fresh_process():
    _ops()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "grapes_amd.labor", "--dataset", "cora", "--max_epoch", "2"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.count("Epoch: ") == 2
    acc = [ln for ln in run.stdout.splitlines() if ln.startswith("Acc: ")]
    assert len(acc) == 1
    value = float(acc[0].split()[1])
    assert np.isfinite(value) and 0.0 <= value <= 100.0
