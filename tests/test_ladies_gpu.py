"""LADIES / FastGCN on the MI355X (grapes_amd/csrc/ladies_kernels.hip, modules/ladies.py, ladies.py) against the fp64 oracle of
tests/ladies_oracle.py.

Tolerances.  An importance pi_j is a sum of t_j positive fp32 terms, each with a few roundings (a division, a square): relative error
<= (t_j + 8) 2^-24 in any summation order; logit = logf(pi) - C adds logf's and the subtraction's roundings:
|d| <= (t_j + 8) 2^-24 + 4 * 2^-24 |logit|.  A layer weight is a quotient over a sum of t_i positive terms: relative error
<= (t_i + 8) 2^-24.  The trainer's logits and gradients are judged by the project's element-wise criterion (oracle/accuracy.py) as
tests/test_wgcn_gpu.py judges its WGCN_UNNORMALIZED layers, the reference chained through both layers; the scalar loss — a mean of B
row losses, each a few fp32 operations on logits that the criterion holds to fp32 accuracy — by
|d| <= (B + 8) 2^-24 (mean |row loss| + max |logit magnitude|).  Every graph has at most 4 096 nodes, but the one of the row list
past one scan tile (5 000)."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc
from tests import gcnconv_modes_oracle as MO
from tests import ladies_oracle as LO

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
SENTINEL = -12345.5


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


def _bitmap(ids, n):
    words = np.zeros((n + 63) // 64, np.uint64)
    for v in np.asarray(ids, dtype=np.int64):
        words[v >> 6] |= np.uint64(1) << np.uint64(v & 63)
    return _dev(words.view(np.int64))


def _transpose(indptr, indices, n):
    rows = np.repeat(np.arange(n), np.diff(indptr))
    return LO.csr_from_edges(np.asarray(indices, dtype=np.int64), rows, n)


class _Case:
    """One graph on the device with its transpose (the graph itself when symmetric) and a prev set."""

    def __init__(self, indptr, indices, n, prev, symmetric=True):
        self.indptr, self.indices, self.n = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32), n
        self.prev = None if prev is None else np.asarray(prev, dtype=np.int64)
        self.rowptr, self.col = _dev(self.indptr), _dev(self.indices)
        if symmetric:
            self.rowptr_t, self.col_t = self.rowptr, self.col
        else:
            tp, ti = _transpose(self.indptr, self.indices, n)
            self.rowptr_t, self.col_t = _dev(tp), _dev(ti)


def _star(hub_in_prev):
    n = 2001                                                             # hub 0, leaves 1 .. 2000
    s = np.concatenate([np.zeros(2000, np.int64), np.arange(1, 2001)])
    d = np.concatenate([np.arange(1, 2001), np.zeros(2000, np.int64)])
    indptr, indices = LO.csr_from_edges(s, d, n)
    prev = np.random.default_rng(2).permutation(np.arange(1, 2001))[:1500]
    return _Case(indptr, indices, n, np.concatenate([prev, [0]]) if hub_in_prev else prev)


def _cases():
    out = {}
    ip, ix = LO.random_symmetric(64, 8, 11)
    assert np.diff(ip).max() <= 8
    out["a_random64"] = _Case(ip, ix, 64, np.random.default_rng(1).permutation(64)[:16])
    out["b_star"] = _star(False)
    out["b_star_hub_in_prev"] = _star(True)
    ip, ix = LO.random_symmetric(63, 6, 12)                              # node 63 is isolated
    ip = np.concatenate([ip, ip[-1:]])
    out["c_isolated"] = _Case(ip, ix, 64, [63, 5, 40, 2])
    ip, ix = LO.random_symmetric(100, 6, 13, loops=10)
    loops = [i for i in range(100) if i in ix[ip[i]:ip[i + 1]]]
    assert len(loops) == 10
    out["d_loops"] = _Case(ip, ix, 100, loops[:5] + [i for i in range(100) if i not in loops][:20])
    rng = np.random.default_rng(14)
    ip, ix = LO.csr_from_edges(rng.integers(0, 80, 400), rng.integers(0, 80, 400), 80)
    out["e_directed"] = _Case(ip, ix, 80, rng.permutation(80)[:20], symmetric=False)
    ip, ix = LO.random_symmetric(300, 8, 15)
    out["g_prev1"] = _Case(ip, ix, 300, [int(np.argmax(np.diff(ip)))])
    ip, ix = LO.random_symmetric(5000, 6, 16)                            # 4 500 rows: past one tile (4 096) of a row-list prefix
    out["h_two_tiles"] = _Case(ip, ix, 5000, np.random.default_rng(3).permutation(5000)[:4500])
    return out


_CASES = {}


def _case(name):
    _ops()
    if not _CASES:
        _CASES.update(_cases())
    return _CASES[name]


PREV_CASES = ["a_random64", "b_star", "b_star_hub_in_prev", "c_isolated", "d_loops", "e_directed", "g_prev1"]


def _check_importance(pi, logit, ref_pi, terms, m, what):
    pi, logit = _np(pi).astype(F64), _np(logit).astype(F64)
    rel = np.abs(pi - ref_pi) / ref_pi
    tol = (terms + 8) * U
    ref_l = LO.logits64(ref_pi, m)
    dl = np.abs(logit - ref_l)
    tol_l = tol + 4 * U * np.abs(ref_l)
    print(f"[ladies] {what}: pi worst err/tol {np.max(rel / tol):.3f}, logit worst err/tol {np.max(dl / tol_l):.3f}, "
          f"max terms {int(terms.max())}")
    assert (rel <= tol).all(), what
    assert (dl <= tol_l).all(), what
    assert (logit <= -20.0 + 1e-3).all(), what


def _importance(ops, c, ids=None, **kw):
    m = len(c.prev)
    return ops.ladies_importance(c.rowptr, c.rowptr_t, c.col_t, c.n, ids=None if ids is None else _dev(np.asarray(ids, np.int32)),
                                 prev_bits=_bitmap(c.prev, c.n), m=m, **kw)


# ------------------------------------------------------------------------------------------------------------ importance
@pytest.mark.parametrize("name", PREV_CASES)
def test_importance_over_the_candidates(name):
    ops, c = _ops(), _case(name)
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    ref, t = LO.importance(c.indptr, c.indices, c.n, c.prev)
    assert (t[cand] > 0).all()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    table = torch.full((c.n,), SENTINEL, device="cuda")
    pi, logit = _importance(ops, c, cand, pi_table=table, status=status)
    _check_importance(pi, logit, ref[cand], t[cand], len(c.prev), name)
    assert int(status.item()) == 0
    tb = _np(table)
    other = np.setdiff1d(np.arange(c.n), cand)
    assert np.array_equal(tb[cand], _np(pi)) and (tb[other] == SENTINEL).all()       # only candidates are written
    if name == "c_isolated":
        assert _np(pi)[list(cand).index(63)] == 1.0
    if name.startswith("b_star"):
        assert t[0] >= 1500                                              # the hub's column walk: many trips of 64


def test_importance_is_the_same_twice():
    ops, c = _ops(), _case("b_star_hub_in_prev")
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    a, b = _importance(ops, c, cand), _importance(ops, c, cand)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_importance_over_every_row_without_bitmap_or_ids():
    ops = _ops()
    for name in ("a_random64", "e_directed", "d_loops", "b_star"):
        c = _case(name)
        ref, t = LO.importance(c.indptr, c.indices, c.n)
        pi, logit = ops.ladies_importance(c.rowptr, c.rowptr_t, c.col_t, c.n)
        assert pi.numel() == c.n
        _check_importance(pi, logit, ref, t, c.n, name + " (FastGCN)")


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_importance_candidate_counts(count):
    ops, c = _ops(), _case("g_prev1")
    ip, ix = c.indptr, c.indices
    prev = np.random.default_rng(count).permutation(c.n)[:150]
    cc = _Case(ip, ix, c.n, prev)
    cand = LO.candidates(ip, ix, prev)
    assert len(cand) >= 257
    ids = cand[:count]
    ref, t = LO.importance(ip, ix, c.n, prev)
    pi, logit = _importance(ops, cc, ids)
    assert pi.numel() == count
    _check_importance(pi, logit, ref[ids], t[ids], 150, f"{count} candidates")


def test_importance_live_count_on_the_device():
    ops, c = _ops(), _case("a_random64")
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    live, cap = len(cand) - 7, len(cand)
    ref, t = LO.importance(c.indptr, c.indices, c.n, c.prev)
    out = (torch.full((cap,), SENTINEL, device="cuda"), torch.full((cap,), SENTINEL, device="cuda"))
    d_n = torch.tensor([live], dtype=torch.int32, device="cuda")
    d_m = torch.tensor([len(c.prev)], dtype=torch.int32, device="cuda")
    pi, logit = ops.ladies_importance(c.rowptr, c.rowptr_t, c.col_t, c.n, ids=_dev(cand.astype(np.int32)), d_n=d_n,
                                      prev_bits=_bitmap(c.prev, c.n), m=c.n, d_m=d_m, out=out)
    _check_importance(pi[:live], logit[:live], ref[cand[:live]], t[cand[:live]], len(c.prev), "device counts")
    assert bool((pi[live:] == SENTINEL).all()) and bool((logit[live:] == SENTINEL).all())


def test_importance_reports_a_bad_id():
    ops, c = _ops(), _case("a_random64")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    pi, logit = _importance(ops, c, [3, 64, -1], status=status)
    assert int(status.item()) == 4 and float(pi[1]) == 0.0 and float(pi[2]) == 0.0 and float(pi[0]) > 0.0


# ------------------------------------------------------------------------------------------------------------ layer kernel
def _device_table(ops, c, cand):
    table = torch.zeros(c.n, device="cuda")
    if c.prev is None:
        ops.ladies_importance(c.rowptr, c.rowptr_t, c.col_t, c.n, pi_table=table)
    else:
        _importance(ops, c, cand, pi_table=table)
    return table


def _check_layer(got, c, rows, after, table, what):
    src, dst, w, d_e = got
    e = int(d_e.item())
    rs, rd, rw, rt = LO.layer_entries(c.indptr, c.indices, c.n, rows, after, _np(table).astype(F64))
    assert e == len(rs), what
    assert np.array_equal(_np(src[:e]), rs) and np.array_equal(_np(dst[:e]), rd), what
    rel = np.abs(_np(w[:e]).astype(F64) - rw) / rw
    tol = (rt + 8) * U
    print(f"[ladies] {what}: {e} entries, weight worst err/tol {np.max(rel / tol) if e else 0.0:.3f}")
    assert (rel <= tol).all(), what
    return e


@pytest.mark.parametrize("name", PREV_CASES + ["h_two_tiles"])
def test_layer_entries_and_weights(name):
    ops, c = _ops(), _case(name)
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    table = _device_table(ops, c, cand)
    rng = np.random.default_rng(7)
    after = np.union1d(rng.permutation(cand)[:max(1, len(cand) // 3)], c.prev[:3])
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = _dev(c.prev.astype(np.int32))
    need = len(LO.layer_entries(c.indptr, c.indices, c.n, c.prev, after, _np(table).astype(F64))[0])
    e_cap = need if name == "h_two_tiles" else need + 5                  # (the two-tile case: the capacity exact)
    got = ops.ladies_layer(c.rowptr, c.col, c.n, rows, _bitmap(after, c.n), table, e_cap, status=status)
    assert _check_layer(got, c, c.prev, after, table, name) == need and int(status.item()) == 0
    again = ops.ladies_layer(c.rowptr, c.col, c.n, rows, _bitmap(after, c.n), table, e_cap)
    assert all(torch.equal(a[:need], b[:need]) for a, b in zip(got[:3], again[:3]))


def test_fastgcn_layer_with_empty_rows():
    ops, c = _ops(), _case("a_random64")
    cc = _Case(c.indptr, c.indices, c.n, None)
    table = _device_table(ops, cc, None)
    rows, after = np.array([40, 3, 17, 22, 9, 60]), np.array([3, 5, 61])
    nb = [set(c.indices[c.indptr[i]:c.indptr[i + 1]]) | {i} for i in rows]
    assert any(not (s & set(after)) for s in nb) and any(s & set(after) for s in nb)
    got = ops.ladies_layer(c.rowptr, c.col, c.n, _dev(rows.astype(np.int32)), _bitmap(after, c.n), table, 64)
    _check_layer(got, c, rows, after, table, "FastGCN layer, empty rows")
    d_m = torch.tensor([2], dtype=torch.int32, device="cuda")            # the live row count on the device
    got = ops.ladies_layer(c.rowptr, c.col, c.n, _dev(rows.astype(np.int32)), _bitmap(after, c.n), table, 64, d_m=d_m)
    _check_layer(got, c, rows[:2], after, table, "FastGCN layer, two live rows")


def test_layer_overflow_writes_nothing_past_e_cap():
    ops = _ops()
    for name in ("d_loops", "h_two_tiles"):                              # (the second: the count one above e_cap behind a tile boundary)
        c = _case(name)
        cand = LO.candidates(c.indptr, c.indices, c.prev)
        table = _device_table(ops, c, cand)
        rs, rd, rw, _ = LO.layer_entries(c.indptr, c.indices, c.n, c.prev, cand, _np(table).astype(F64))
        e_cap, guard = len(rs) - 1, 64
        bufs = (torch.full((e_cap + guard,), -7, dtype=torch.int32, device="cuda"),
                torch.full((e_cap + guard,), -7, dtype=torch.int32, device="cuda"), torch.full((e_cap + guard,), SENTINEL, device="cuda"))
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = (bufs[0][:e_cap], bufs[1][:e_cap], bufs[2][:e_cap], torch.zeros(1, dtype=torch.int32, device="cuda"))
        src, dst, w, d_e = ops.ladies_layer(c.rowptr, c.col, c.n, _dev(c.prev.astype(np.int32)), _bitmap(cand, c.n), table, e_cap,
                                            status=status, out=out)
        assert int(status.item()) & 1 and int(d_e.item()) == e_cap, name
        assert bool((bufs[0][e_cap:] == -7).all()) and bool((bufs[1][e_cap:] == -7).all()) and bool((bufs[2][e_cap:] == SENTINEL).all())
        assert np.array_equal(_np(src), rs[:e_cap]) and np.array_equal(_np(dst), rd[:e_cap]), name


# ------------------------------------------------------------------------------------------------------------ whole sampler
_GRAPHS = {}


def _graph(name):
    _ops()
    from grapes_amd.graph import DeviceGraph
    if name not in _GRAPHS:
        if name == "hand":
            ip, ix, n = LO.hand_graph()
        else:
            n = 300
            ip, ix = LO.random_symmetric(n, 8, 21, loops=12)
        _GRAPHS[name] = (ip, ix, n, DeviceGraph.from_csr(ip, ix))
    return _GRAPHS[name]


def _compare_batch(b, ob, what):
    assert len(b.layers) == len(ob.layers)
    for d, (L, R) in enumerate(zip(b.layers, ob.layers)):
        assert np.array_equal(_np(L.prev), R.prev), (what, d)
        if L.candidates is not None:
            assert np.array_equal(_np(L.candidates), R.candidates), (what, d)
        assert np.array_equal(_np(L.after), R.after), (what, d)
        assert np.array_equal(_np(L.edge_src), R.src) and np.array_equal(_np(L.edge_dst), R.dst), (what, d)
        rel = np.abs(_np(L.weight).astype(F64) - R.w) / R.w
        tol = (R.row_terms + 8) * U
        print(f"[ladies] {what} layer {d}: {len(R.w)} entries, weight worst err/tol {np.max(rel / tol) if len(rel) else 0.0:.3f}")
        assert (rel <= tol).all(), (what, d)
    assert np.array_equal(_np(b.node_idx), ob.node_idx), what
    assert np.array_equal(_np(b.local_targets), ob.local_targets), what
    for ei, oe in zip(b.edge_index, ob.edge_index):
        assert np.array_equal(_np(ei), oe), what


@pytest.mark.parametrize("kind", ["ladies", "fastgcn"])
@pytest.mark.parametrize("layers,samp_num,graph", [(2, 4, "random"), (3, 4, "random"), (2, 64, "random"), (3, 64, "random"),
                                                   (2, 64, "hand"), (3, 4, "hand")])
def test_sampler_against_the_oracle(kind, layers, samp_num, graph):
    from grapes_amd.modules.ladies import LayerWiseSampler
    ip, ix, n, g = _graph(graph)
    rng = np.random.default_rng(31 + layers)
    targets = np.array([5, 2, 11]) if graph == "hand" else rng.permutation(n)[:24]
    u = [rng.random(n).astype(F32) for _ in range(layers)]
    s = LayerWiseSampler(g, samp_num, layers, kind=kind, seed=5)
    b = s.sample(_dev(targets), uniforms=[_dev(v) for v in u])
    s.check()
    ob = LO.sample(ip, ix, n, targets, samp_num, layers, kind=kind, uniforms=u, logits=[_np(L.logit) for L in b.layers])
    _compare_batch(b, ob, f"{kind} L={layers} s={samp_num} {graph}")
    if graph == "hand" and samp_num == 64:
        assert all(len(R.sampled) == len(R.candidates) for R in ob.layers)       # keep-all
    for t in (g.bits, g.prev_bits, g.mult):
        assert not bool(t.any())                                         # the graph's scratch is zero at rest again


@pytest.mark.parametrize("kind", ["ladies", "fastgcn"])
def test_one_seed_gives_the_same_batches(kind):
    from grapes_amd.modules.ladies import LayerWiseSampler
    ip, ix, n, g = _graph("random")
    targets = _dev(np.random.default_rng(41).permutation(n)[:16])
    runs = []
    for _ in range(2):
        s = LayerWiseSampler(g, 4, 2, kind=kind, seed=77)
        runs.append([s.sample(targets), s.sample(targets)])
    for a, b in zip(*runs):
        assert torch.equal(a.node_idx, b.node_idx)
        for x, y in zip(a.edge_index + a.edge_weight, b.edge_index + b.edge_weight):
            assert torch.equal(x, y)
    other = LayerWiseSampler(g, 4, 2, kind=kind, seed=78).sample(targets)
    assert not torch.equal(other.layers[0].sampled, runs[0][0].layers[0].sampled)


def test_a_grapes_hop_after_sampling_is_what_a_fresh_graph_gives():
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.ladies import LayerWiseSampler
    from grapes_amd.step import GrapesTrainer
    ip, ix, n, g = _graph("random")
    targets = _dev(np.random.default_rng(43).permutation(n)[:16])
    for kind in ("ladies", "fastgcn"):
        LayerWiseSampler(g, 4, 3, kind=kind, seed=3).sample(targets)
    X = torch.zeros(n, 4, device="cuda")
    inject = lambda hop, bn: torch.sin(bn.to(torch.float32) * 0.37 + hop)
    outs = []
    for graph in (g, DeviceGraph.from_csr(ip, ix)):
        gen = torch.Generator(device="cuda"); gen.manual_seed(9)
        uni = [torch.rand(n, device="cuda", generator=gen) for _ in range(2)]
        tr = GrapesTrainer(graph, X, None, None, None, None, sampling_hops=2, num_samples=8)
        outs.append(tr.step(targets, uniforms_fn=lambda hop, nn: uni[hop][:nn].contiguous(), inject_logits_fn=inject, trace=True))
    a, b = outs
    assert torch.equal(a["all_nodes"], b["all_nodes"])
    for x, y in zip(a["edge_indices"], b["edge_indices"]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ trainer
def _judge(got, ref3, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite outputs"
    return acc.assert_fp32_accuracy(got, torch.as_tensor(ref3[0]), torch.as_tensor(ref3[1]), torch.as_tensor(ref3[2]), what)


def _loss_parts(z3, local_targets, labels):
    """From the logits' triple (ref, mag, base): the loss in fp64, d loss / d logits as a triple, the mean |row loss| and the largest
    logit magnitude among the targets' rows."""
    B = len(local_targets)
    out = []
    for z, dt in ((z3[0], F64), (z3[2], F32)):
        zt = z[local_targets].astype(dt)
        if labels.ndim == 1:
            mx = zt.max(1, keepdims=True)
            lse = (mx + np.log(np.exp(zt - mx).sum(1, keepdims=True, dtype=dt))).astype(dt)
            rows = (lse[:, 0] - zt[np.arange(B), labels]).astype(dt)
            d = (np.exp(zt - lse).astype(dt) - np.eye(zt.shape[1], dtype=dt)[labels]) / dt(B)
        else:
            y = labels.astype(dt)
            rows = (np.maximum(zt, 0) - zt * y + np.log1p(np.exp(-np.abs(zt)))).astype(dt).mean(1)
            d = ((dt(1) / (dt(1) + np.exp(-zt))).astype(dt) - y) / dt(B * zt.shape[1])
        full = np.zeros(z.shape, dt)
        full[local_targets] = d
        out.append((rows, full))
    (rows64, d64), (_, d32) = out
    return float(rows64.mean()), (d64, np.abs(d64), d32), float(np.abs(rows64).mean()), float(z3[1][local_targets].max())


@pytest.mark.parametrize("kind,multilabel", [("ladies", False), ("ladies", True), ("fastgcn", False)])
def test_trainer_step_against_fp64(kind, multilabel):
    ops = _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.ladies import LadiesTrainer, weighted_structures
    from grapes_amd.modules.gcn import GCN, _WeightedGCNConvFn
    n, F, H, C, B = 256, 32, 16, 4, 32
    ip, ix = LO.random_symmetric(n, 8, 51, loops=6)
    g = DeviceGraph.from_csr(ip, ix)
    rng = np.random.default_rng(52)
    x32 = rng.standard_normal((n, F)).astype(F32)
    labels = (rng.random((n, C)) < 0.4).astype(F32) if multilabel else rng.integers(0, C, n)
    model = GCN(F, [H, C]).cuda()
    with torch.no_grad():
        for layer in model.gcn_layers:
            layer.bias.copy_(_dev((rng.standard_normal(layer.out_channels) * 0.1).astype(F32)))
    W1, b1, W2, b2 = (_np(p).copy() for p in (model.gcn_layers[0].lin.weight, model.gcn_layers[0].bias,
                                              model.gcn_layers[1].lin.weight, model.gcn_layers[1].bias))
    tr = LadiesTrainer(g, _dev(x32), _dev(labels), model, torch.optim.Adam(model.parameters(), lr=1e-3), samp_num=24, kind=kind, seed=8)
    targets = rng.permutation(n)[:B]
    loss, b = tr.step(_dev(targets))
    nb = b.num_nodes
    ei, ew = [_np(t).astype(np.int64) for t in b.edge_index], [_np(t) for t in b.edge_weight]
    xb = x32[_np(b.node_idx)]
    lt, y_t = _np(b.local_targets).astype(np.int64), labels[targets]
    with torch.no_grad():                                                # the device's ReLU gates of the hidden layer
        ws = weighted_structures(b.edge_index, nb)
        gate = _np(_WeightedGCNConvFn.apply(_dev(xb), _dev(W1), _dev(b1), b.edge_weight[-1], ws[-1], True, ops.WGCN_UNNORMALIZED, 1.0) > 0)
    # the fp64 oracle on the device's batch, and the same thing chained as (reference, magnitude, fp32 baseline) triples
    l64, dW, db, z64 = LO.train_step64(xb, [W1, W2], [b1, b2], ei, ew, lt, y_t, gates=[gate])
    P1 = MO.ModeProblem(ei[-1][0], ei[-1][1], ew[-1], nb, normalize=False)
    P0 = MO.ModeProblem(ei[0][0], ei[0][1], ew[0], nb, normalize=False)
    x3 = (xb.astype(F64), np.abs(xb.astype(F64)), xb)
    h3 = P1.chain_forward(x3, W1, b1, gate=gate)
    z3 = P0.chain_forward(h3, W2, b2)
    assert np.allclose(z3[0], z64, rtol=1e-11, atol=1e-12)
    lref, d3, row_mag, z_mag = _loss_parts(z3, lt, y_t)
    assert np.isclose(lref, l64, rtol=1e-12)
    back2 = P0.chain_backward(d3, h3, W2)
    g64 = gate.astype(F64)
    back1 = P1.chain_backward(tuple(v * g64.astype(v.dtype) for v in back2["dx"]), x3, W1)
    for got, want in ((back1["dW"][0], dW[0]), (back1["db"][0], db[0]), (back2["dW"][0], dW[1]), (back2["db"][0], db[1])):
        assert np.allclose(got, want, rtol=1e-10, atol=1e-13)
    what = f"{kind} {'BCE' if multilabel else 'CE'}"
    bound = (B + 8) * U * (row_mag + z_mag)
    print(f"[ladies] {what}: loss {float(loss):.7f} fp64 {l64:.7f} |d| / bound {abs(float(loss) - l64) / bound:.3f}")
    assert abs(float(loss) - l64) <= bound
    _judge(model.gcn_layers[0].lin.weight.grad, back1["dW"], what + " dW1")
    _judge(model.gcn_layers[0].bias.grad, back1["db"], what + " db1")
    _judge(model.gcn_layers[1].lin.weight.grad, back2["dW"], what + " dW2")
    _judge(model.gcn_layers[1].bias.grad, back2["db"], what + " db2")
    assert not np.array_equal(_np(model.gcn_layers[1].lin.weight), W2)   # Adam stepped


@pytest.mark.parametrize("kind", ["ladies", "fastgcn"])
def test_training_lowers_the_loss_and_evaluates(kind):
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.ladies import LadiesTrainer, build_model
    n, F, C = 512, 16, 4
    rng = np.random.default_rng(61)
    y = rng.integers(0, C, n)
    same = [(a, b) for a, b in rng.integers(0, n, (6000, 2)) if y[a] == y[b] and a != b][:1200]     # edges inside the classes
    s, d = np.array([a for a, b in same] + [b for a, b in same]), np.array([b for a, b in same] + [a for a, b in same])
    ip, ix = LO.csr_from_edges(s, d, n)
    x = (np.eye(C)[y] @ rng.standard_normal((C, F)) * 2.0 + 0.3 * rng.standard_normal((n, F))).astype(F32)
    g = DeviceGraph.from_csr(ip, ix)
    model = build_model(F, 16, C, 2, 0.0, "cuda")
    tr = LadiesTrainer(g, _dev(x), _dev(y), model, torch.optim.Adam(model.parameters(), lr=2e-2), samp_num=64, kind=kind, seed=6)
    train = _dev(np.arange(0, n, 2))
    losses = [tr.epoch(train, 128) for _ in range(5)]
    print(f"[ladies] {kind} epoch losses", np.round(losses, 4))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    mask = torch.zeros(n, dtype=torch.bool, device="cuda"); mask[1::2] = True
    val, test = tr.evaluate((mask, ~mask))
    assert np.isfinite(val) and np.isfinite(test) and 0.0 <= val <= 1.0 and 0.0 <= test <= 1.0
    yl = _dev((np.eye(C)[y]).astype(F32))                                # the multi-label metric
    f1, = LadiesTrainer(g, _dev(x), yl, model, torch.optim.Adam(model.parameters(), lr=1e-3), samp_num=64, kind=kind, seed=6).evaluate((mask,))
    assert np.isfinite(f1) and 0.0 <= f1 <= 1.0


@pytest.mark.parametrize("kind", ["ladies", "fastgcn"])
def test_cli_two_epochs(kind, capsys):
    _ops()
    from grapes_amd import ladies
    v = ladies.main(["--dataset", "cora", "--sampler", kind, "--max_epoch", "2", "--hidden_dim", "32", "--seed", "1"])
    out = capsys.readouterr().out
    assert out.count("Epoch: ") == 2 and "Acc: " in out and 0.0 <= v <= 1.0
