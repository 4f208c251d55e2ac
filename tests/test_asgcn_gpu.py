"""AS-GCN on the MI355X (grapes_amd/csrc/asgcn_kernels.hip, modules/asgcn.py, asgcn.py) against the fp64 oracle of
tests/asgcn_oracle.py.  Graphs and cases are those of tests/test_ladies_gpu.py.

Tolerances, U = 2^-24.  c_j is a sum of t_j positive fp32 terms with a division each: relative error <= (t_j + 8) U.  a_j is an
F-term dot product plus the bias: |d| <= (F + 8) U (sum_f |x_jf w_f| + |b_g|).  g = max(a, 0) + 1 moves by no more than a does, plus
one rounding; q = c g and logq = logf(q) compose the two, logf adding 4 U |logq|.  The shift is exact: logit is the fp32 expression
(logq - max logq) - 20 of the device's own logq, bit for bit.  A layer weight: relative error <= (row entries + 8) U of the fp64
weight formed from the device's q.  V, dw, T and the step's gradients are judged by oracle/accuracy.py's element-wise criterion
against (reference, magnitude, fp32 baseline) triples; the bounds of the scalar losses are written where they are used."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc
from tests import asgcn_oracle as AO
from tests import gcnconv_modes_oracle as MO
from tests import ladies_oracle as LO
from tests import test_ladies_gpu as TL

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
SENTINEL = -12345.5
_dev, _np, _ops = TL._dev, TL._np, TL._ops


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(4321)


def _features(n, F, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, F)).astype(F32), (rng.standard_normal(F) * 0.5).astype(F32), np.array([0.1], F32)


def _importance(ops, c, ids, x, w_g, b_g, **kw):
    return ops.asgcn_importance(c.rowptr, c.rowptr_t, c.col_t, c.n, x if torch.is_tensor(x) else _dev(x), _dev(w_g), _dev(b_g),
                                ids=None if ids is None else _dev(np.asarray(ids, np.int32)), prev_bits=TL._bitmap(c.prev, c.n),
                                m=len(c.prev), **kw)


def _check_importance(got, c, prev, ids, x, w_g, b_g, what):
    """The five outputs over the candidates ids against the oracle; returns the share of candidates left out of the g comparison."""
    F = x.shape[1]
    ref = AO.importance(c.indptr, c.indices, c.n, prev, x, w_g, b_g)
    ids = np.asarray(ids, dtype=np.int64)
    cd, ad, qd, lqd, lgd = (_np(t) for t in got)
    rc, ra, rg, rq, rl, t, am = (v[ids] for v in (ref.c, ref.a, ref.g, ref.q, ref.logq, ref.terms, ref.a_mag))
    assert (t > 0).all() and (rc > 0).all(), what
    eps_c = (t + 8) * U
    rel_c = np.abs(cd.astype(F64) - rc) / rc
    tol_a = (F + 8) * U * am
    err_a = np.abs(ad.astype(F64) - ra)
    tol_g = tol_a + U * rg
    tol_q = rc * tol_g + rq * eps_c + rc * eps_c * tol_g + U * rq
    err_q = np.abs(qd.astype(F64) - rq)
    rel_q = tol_q / rq
    assert (rel_q < 0.5).all(), what
    tol_l = -np.log1p(-rel_q) + 4 * U * np.abs(rl)
    err_l = np.abs(lqd.astype(F64) - rl)
    unsure = np.abs(ra) < tol_a                                          # the sign of a is not decided within its bound
    share = float(unsure.mean())
    keep = ~unsure
    print(f"[asgcn] {what}: F {F}, {len(ids)} candidates, worst err/tol c {np.max(rel_c / eps_c):.3f} a {np.max(err_a / tol_a):.3f} "
          f"q {np.max(err_q / tol_q):.3f} logq {np.max(err_l / tol_l):.3f}, max terms {int(t.max())}, left out {share:.4f}")
    assert (rel_c <= eps_c).all() and (err_a <= tol_a).all(), what
    assert share <= 0.01, what
    assert (err_q[keep] <= tol_q[keep]).all() and (err_l[keep] <= tol_l[keep]).all(), what
    want = AO.shifted_logits32(lqd)
    assert np.array_equal(lgd.view(np.uint32), want.view(np.uint32)), what           # the shift: exactly two roundings
    assert lgd.max() == F32(-20.0), what
    return share


# ------------------------------------------------------------------------------------------------------------ importance
WIDTHS = (1, 3, 4, 64, 260)


@pytest.mark.parametrize("name", TL.PREV_CASES)
def test_importance_over_the_candidates(name):
    ops, c = _ops(), TL._case(name)
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    for F in WIDTHS:
        x, w_g, b_g = _features(c.n, F, 100 + F)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        qt, at = torch.full((c.n,), SENTINEL, device="cuda"), torch.full((c.n,), SENTINEL, device="cuda")
        got = _importance(ops, c, cand, x, w_g, b_g, q_table=qt, a_table=at, status=status)
        _check_importance(got, c, c.prev, cand, x, w_g, b_g, f"{name}")
        assert int(status.item()) == 0
        other = np.setdiff1d(np.arange(c.n), cand)
        for tb, col in ((_np(qt), got[2]), (_np(at), got[1])):           # only candidates are written
            assert np.array_equal(tb[cand], _np(col)) and (tb[other] == SENTINEL).all()
    if name.startswith("b_star"):
        assert AO.column_mass(c.indptr, c.indices, c.n, c.prev)[1][0] >= 1500      # the hub's column walk: many trips of 64


def test_importance_reads_rows_of_a_wider_matrix():
    """x as a column slice of a wider matrix: row stride 8 with F = 4 (16-byte loads) and row stride 5 with F = 3 (scalar loads)."""
    ops, c = _ops(), TL._case("a_random64")
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    for F, wide in ((4, 8), (3, 5), (4, 6)):
        xw = np.random.default_rng(F + wide).standard_normal((c.n, wide)).astype(F32)
        _, w_g, b_g = _features(c.n, F, 7)
        got = _importance(ops, c, cand, _dev(xw)[:, :F], w_g, b_g)
        _check_importance(got, c, c.prev, cand, xw[:, :F], w_g, b_g, f"stride {wide}")


def test_importance_is_the_same_twice():
    ops, c = _ops(), TL._case("b_star_hub_in_prev")
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    x, w_g, b_g = _features(c.n, 64, 5)
    a, b = _importance(ops, c, cand, x, w_g, b_g), _importance(ops, c, cand, x, w_g, b_g)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_importance_candidate_counts(count):
    ops, c = _ops(), TL._case("g_prev1")
    prev = np.random.default_rng(count).permutation(c.n)[:150]
    cc = TL._Case(c.indptr, c.indices, c.n, prev)
    cand = LO.candidates(c.indptr, c.indices, prev)
    assert len(cand) >= 257
    x, w_g, b_g = _features(c.n, 4, count)
    got = _importance(ops, cc, cand[:count], x, w_g, b_g)
    assert all(t.numel() == count for t in got)
    _check_importance(got, cc, prev, cand[:count], x, w_g, b_g, f"{count} candidates")


def test_importance_live_count_on_the_device():
    ops, c = _ops(), TL._case("a_random64")
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    live, cap = len(cand) - 7, len(cand)
    x, w_g, b_g = _features(c.n, 3, 9)
    out = tuple(torch.full((cap,), SENTINEL, device="cuda") for _ in range(5))
    d_n = torch.tensor([live], dtype=torch.int32, device="cuda")
    got = _importance(ops, c, cand, x, w_g, b_g, d_n=d_n, out=out)
    _check_importance(tuple(t[:live] for t in got), c, c.prev, cand[:live], x, w_g, b_g, "device count")
    assert all(bool((t[live:] == SENTINEL).all()) for t in got)


def test_importance_reports_a_bad_id():
    ops, c = _ops(), TL._case("a_random64")
    x, w_g, b_g = _features(c.n, 4, 9)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cm, a, q, logq, logit = _importance(ops, c, [3, 64, -1], x, w_g, b_g, status=status)
    assert int(status.item()) == 4 and float(q[1]) == 0.0 and float(q[2]) == 0.0 and float(q[0]) > 0.0
    assert float(logit[1]) == -np.inf and float(logit[2]) == -np.inf and float(logit[0]) == -20.0


def test_the_sign_of_a_on_exact_integers():
    """Integer-valued x, w_g and b_g: the dot product is exact in fp32 whatever its order.  a = 0, a < 0 and a > 0 are all present, and
    g is exactly 1, 1 and a + 1: q is the fp32 product of the device's c and that g, bit for bit."""
    ops, c = _ops(), TL._case("a_random64")
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    for F in (3, 8):
        rng = np.random.default_rng(F)
        x = rng.integers(-3, 4, (c.n, F)).astype(F32)
        w_g, b_g = rng.integers(-2, 3, F).astype(F32), np.array([1.0], F32)
        x[cand[0]] = 0.0; x[cand[0], 0] = 1.0; w_g[0] = -1.0            # a = -1 + 1 = 0 exactly
        a64 = x.astype(F64) @ w_g.astype(F64) + 1.0
        assert (a64[cand] == 0).any() and (a64[cand] < 0).any() and (a64[cand] > 0).any()
        cm, a, q, logq, logit = (_np(t) for t in _importance(ops, c, cand, x, w_g, b_g))
        assert np.array_equal(a.astype(F64), a64[cand])
        g = np.where(a64[cand] > 0, a64[cand] + 1.0, 1.0).astype(F32)
        assert np.array_equal(q.view(np.uint32), (cm * g).astype(F32).view(np.uint32))


def test_zero_parameters_give_the_column_mass():
    ops, c = _ops(), TL._case("d_loops")
    cand = LO.candidates(c.indptr, c.indices, c.prev)
    x = _features(c.n, 4, 3)[0]
    cm, a, q, logq, logit = _importance(ops, c, cand, x, np.zeros(4, F32), np.zeros(1, F32))
    assert torch.equal(cm.view(torch.int32), q.view(torch.int32)) and not bool(a.any())


# ------------------------------------------------------------------------------------------------------------ whole sampler
_GRAPHS = {}


def _graph(name):
    _ops()
    from grapes_amd.graph import DeviceGraph
    if name not in _GRAPHS:
        if name == "hand":
            ip, ix, n = LO.hand_graph()
        else:
            n = 256
            ip, ix = LO.random_symmetric(n, 8, 21, loops=12)
        x = np.random.default_rng(22).standard_normal((n, 8)).astype(F32)
        _GRAPHS[name] = (ip, ix, n, DeviceGraph.from_csr(ip, ix), x)
    return _GRAPHS[name]


def _sampler(g, samp_num, layers, F, seed, w_seed=3):
    from grapes_amd.modules.asgcn import AdaptiveSampler
    s = AdaptiveSampler(g, samp_num, layers, F, seed=seed)
    with torch.no_grad():
        s.w_g.copy_(_dev((np.random.default_rng(w_seed).standard_normal(F) * 0.5).astype(F32)))
        s.b_g.fill_(0.1)
    return s


@pytest.mark.parametrize("layers,samp_num,graph", [(2, 4, "random"), (3, 4, "random"), (2, 64, "random"), (3, 64, "random"),
                                                   (2, 64, "hand")])
def test_sampler_against_the_oracle(layers, samp_num, graph):
    ip, ix, n, g, x = _graph(graph)
    rng = np.random.default_rng(31 + layers)
    targets = np.array([5, 2, 11]) if graph == "hand" else rng.permutation(n)[:24]
    u = [rng.random(n).astype(F32) for _ in range(layers)]
    s = _sampler(g, samp_num, layers, x.shape[1], 5)
    b = s.sample(_dev(targets), _dev(x), uniforms=[_dev(v) for v in u])
    s.check()
    q_tables = []
    for L in b.layers:
        t = np.zeros(n)
        t[_np(L.candidates)] = _np(L.q).astype(F64)
        q_tables.append(t)
    ob = AO.sample(ip, ix, n, targets, samp_num, layers, x, _np(s.w_g), _np(s.b_g), uniforms=u, logits=[_np(L.logit) for L in b.layers],
                   q_tables=q_tables)
    what = f"asgcn L={layers} s={samp_num} {graph}"
    for d, (L, R) in enumerate(zip(b.layers, ob.layers)):
        assert np.array_equal(_np(L.prev), R.prev) and np.array_equal(_np(L.candidates), R.candidates), (what, d)
        assert np.array_equal(_np(L.sampled), np.sort(R.sampled)) and np.array_equal(_np(L.after), R.after), (what, d)
        assert np.array_equal(_np(L.edge_src), R.src) and np.array_equal(_np(L.edge_dst), R.dst), (what, d)
        rel = np.abs(_np(L.weight).astype(F64) - R.w) / R.w
        tol = (R.row_terms + 8) * U
        print(f"[asgcn] {what} layer {d}: {len(R.w)} entries, weight worst err/tol {np.max(rel / tol):.3f}")
        assert (rel <= tol).all(), (what, d)
        _check_importance((L.c, L.a, L.q, L.logq, L.logit), SimpleList(indptr=ip, indices=ix, n=n), R.prev, R.candidates, x, _np(s.w_g),
                          _np(s.b_g), f"{what} layer {d}")
    assert np.array_equal(_np(b.node_idx), ob.node_idx) and np.array_equal(_np(b.local_targets), ob.local_targets), what
    for ei, oe, lp, op in zip(b.edge_index, ob.edge_index, b.local_prev, ob.local_prev):
        assert np.array_equal(_np(ei), oe) and np.array_equal(_np(lp), op), what
    a_all = x.astype(F64) @ _np(s.w_g).astype(F64) + 0.1
    assert np.allclose(_np(b.a), a_all[ob.node_idx], rtol=0, atol=1e-5)
    if graph == "hand":
        assert all(len(R.sampled) == len(R.candidates) for R in ob.layers)       # keep-all
        assert s.philox_offset == 0                                              # ... which advances no stream
    for t in (g.bits, g.prev_bits, g.mult):
        assert not bool(t.any())                                         # the graph's scratch is zero at rest again


def test_one_seed_gives_the_same_batches():
    ip, ix, n, g, x = _graph("random")
    targets, xd = _dev(np.random.default_rng(41).permutation(n)[:16]), _dev(x)
    runs = []
    for _ in range(2):
        s = _sampler(g, 4, 2, x.shape[1], 77)
        runs.append([s.sample(targets, xd), s.sample(targets, xd)])
    for a, b in zip(*runs):
        assert torch.equal(a.node_idx, b.node_idx)
        for p, q in zip(a.edge_index + a.edge_weight, b.edge_index + b.edge_weight):
            assert torch.equal(p, q)
    other = _sampler(g, 4, 2, x.shape[1], 78).sample(targets, xd)
    assert not torch.equal(other.layers[0].sampled, runs[0][0].layers[0].sampled)


def test_a_grapes_hop_after_sampling_is_what_a_fresh_graph_gives():
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.step import GrapesTrainer
    ip, ix, n, g, x = _graph("random")
    targets = _dev(np.random.default_rng(43).permutation(n)[:16])
    _sampler(g, 4, 3, x.shape[1], 3).sample(targets, _dev(x))
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
    for p, q in zip(a["edge_indices"], b["edge_indices"]):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------------------ entry lists
ROW_LENGTHS = (0, 1, 63, 64, 65, 330, 1, 7, 0, 64, 2)


def _entry_list(seed, n_local=400, lengths=ROW_LENGTHS):
    """A layer's entry list as ladies_layer writes it: rows = distinct local ids in a shuffled order, each with lengths[r] entries,
    sources ascending and distinct within a row, positive weights that sum to 1 per row (fp32)."""
    rng = np.random.default_rng(seed)
    rows = rng.permutation(n_local)[:len(lengths)]
    src, dst, w = [], [], []
    for r, L in zip(rows, lengths):
        if L == 0:
            continue
        src.append(np.sort(rng.permutation(n_local)[:L])); dst.append(np.full(L, r))
        v = rng.random(L) ** 3 + 1e-3                                     # weights of very different sizes
        w.append(v / v.sum())
    return SimpleList(src=np.concatenate(src).astype(np.int32), dst=np.concatenate(dst).astype(np.int32),
                      w=np.concatenate(w).astype(F32), rows=rows.astype(np.int32), n_local=n_local, lengths=np.array(lengths))


class SimpleList:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def dev(self):
        return _dev(self.src), _dev(self.dst), _dev(self.w), _dev(self.rows)


def _triple(ref, mag, base):
    return torch.as_tensor(np.asarray(ref, dtype=F64)), torch.as_tensor(np.asarray(mag, dtype=F64)), torch.as_tensor(np.asarray(base, dtype=F32))


@pytest.mark.parametrize("C", [1, 3, 7, 47, 256, 100, 512, 1024])      # (100, 512 and 1024: two, eight and sixteen channels per lane)
def test_variance_against_fp64(C):
    ops = _ops()
    E = _entry_list(60 + C)
    assert {0, 1, 63, 64, 65}.issubset(set(E.lengths)) and E.lengths.max() >= 300
    H = np.random.default_rng(C).standard_normal((E.n_local, C)).astype(F32)
    ref = AO.variance(E.src, E.dst, E.w, E.rows, H.astype(F64), H)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    src, dst, w, rows = E.dev()
    V, lvar, dw = ops.asgcn_variance(src, dst, w, rows, _dev(H), status=status)
    assert int(status.item()) == 0
    acc.assert_fp32_accuracy(V.cpu(), *_triple(ref.V, ref.V_mag, ref.V32), f"V, C = {C}")
    acc.assert_fp32_accuracy(dw.cpu(), *_triple(ref.dw, ref.dw_mag, ref.dw32), f"dw, C = {C}")
    Vd, m = _np(V).astype(F64), len(E.rows)
    one = E.lengths == 1                                                 # one entry: w = 1, the two terms cancel
    assert (np.abs(ref.V[one]) <= 1e-12 * ref.V_mag[one]).all() and (np.abs(Vd[one]) <= (C + 9) * U * ref.V_mag[one]).all()
    assert (Vd[E.lengths == 0] == 0).all()
    assert (Vd >= -(E.lengths + C + 8) * U * ref.V_mag).all()
    fixed = float(np.sum(Vd)) / m
    assert abs(float(lvar) - fixed) <= (m + 8) * U * np.abs(Vd).sum() / m
    again = ops.asgcn_variance(src, dst, w, rows, _dev(H))
    assert torch.equal(again[0], V) and torch.equal(again[1], lvar) and torch.equal(again[2], dw)


def test_variance_and_logq_bwd_report_bad_ids_without_reading_them():
    ops = _ops()
    E = _entry_list(5, lengths=(3, 2, 4))
    H = _dev(np.ones((E.n_local, 4), F32))
    for bad_src, bad_dst in ((True, False), (False, True)):
        src, dst = E.src.copy(), E.dst.copy()
        if bad_src:
            src[1] = E.n_local + 5
        if bad_dst:
            dst[3:5] = [i for i in range(E.n_local) if i not in E.rows][0]        # a target that is none of the rows
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        V, lvar, dw = ops.asgcn_variance(_dev(src), _dev(dst), _dev(E.w), _dev(E.rows), H, status=status)
        assert int(status.item()) == 4 and bool(torch.isfinite(V).all()) and bool(torch.isfinite(lvar).all())
        status.zero_()
        T = ops.asgcn_logq_bwd(_dev(src), _dev(dst), _dev(E.w), _dev(np.ones(len(src), F32)), _dev(E.rows), E.n_local, status=status)
        assert bool(torch.isfinite(T).all()) and int(status.item()) == 4


def test_logq_bwd_against_fp64():
    ops = _ops()
    A, B = _entry_list(71), _entry_list(72, lengths=(5, 64, 200, 0, 1))
    refs, out = [], None
    for E, seed in ((A, 1), (B, 2)):
        G = (np.random.default_rng(seed).standard_normal(len(E.src)) * np.random.default_rng(seed + 9).choice([1e-3, 1.0, 30.0], len(E.src))).astype(F32)
        T3 = AO.logq_bwd(E.src, E.dst, E.w, (G.astype(F64), np.abs(G.astype(F64)), G), E.rows, E.n_local)
        src, dst, w, rows = E.dev()
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        T = ops.asgcn_logq_bwd(src, dst, w, _dev(G), rows, E.n_local, status=status)
        assert int(status.item()) == 0
        acc.assert_fp32_accuracy(T.cpu(), *_triple(*T3[:3]), f"T, {len(E.src)} entries")
        total = abs(float(_np(T).astype(F64).sum()))
        print(f"[asgcn] |sum T| / bound {total / ((len(E.src) + 8) * U * T3[3]):.3f}")
        assert total <= (len(E.src) + 8) * U * T3[3]
        assert torch.equal(ops.asgcn_logq_bwd(src, dst, w, _dev(G), rows, E.n_local), T)          # two runs, the same bits
        out = ops.asgcn_logq_bwd(src, dst, w, _dev(G), rows, E.n_local, out=out)                  # += across layers
        refs.append(T3)
    base = (refs[0][2] + refs[1][2]).astype(F32)
    acc.assert_fp32_accuracy(out.cpu(), *_triple(refs[0][0] + refs[1][0], refs[0][1] + refs[1][1], base), "T over two layers")


# ------------------------------------------------------------------------------------------------------------ trainer
def _step_problem(multilabel):
    n, F, H, C, B = 256, 32, 16, 4, 32
    ip, ix = LO.random_symmetric(n, 8, 51, loops=6)
    rng = np.random.default_rng(52)
    x32 = rng.standard_normal((n, F)).astype(F32)
    labels = (rng.random((n, C)) < 0.4).astype(F32) if multilabel else rng.integers(0, C, n)
    b1, b2 = (rng.standard_normal(H) * 0.1).astype(F32), (rng.standard_normal(C) * 0.1).astype(F32)
    targets = rng.permutation(n)[:B]
    return SimpleList(n=n, F=F, H=H, C=C, B=B, ip=ip, ix=ix, x32=x32, labels=labels, b1=b1, b2=b2, targets=targets)


def _trainer(P, var_coef, train_sampler=True, state=None):
    from grapes_amd.asgcn import AsgcnTrainer
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    g = DeviceGraph.from_csr(P.ip, P.ix)
    model = GCN(P.F, [P.H, P.C]).cuda()
    if state is not None:
        model.load_state_dict(state)
    else:
        with torch.no_grad():
            model.gcn_layers[0].bias.copy_(_dev(P.b1)); model.gcn_layers[1].bias.copy_(_dev(P.b2))
    s = _sampler(g, 24, 2, P.F, 8, w_seed=53)
    if not train_sampler:
        for p in s.parameters():
            p.requires_grad_(False)
    params = list(model.parameters()) + [p for p in s.parameters() if p.requires_grad]
    return AsgcnTrainer(g, _dev(P.x32), _dev(P.labels), model, s, torch.optim.Adam(params, lr=1e-3), var_coef=var_coef), model, s


@pytest.mark.parametrize("multilabel", [False, True])
@pytest.mark.parametrize("var_coef", [0.0, 0.5])
def test_trainer_step_against_fp64(multilabel, var_coef):
    """The oracle runs on the device's batch (entries, fp32 weights, the kernel's a), its ReLU gates and its [a > 0] masks.
    L_c: |d| <= (B + 8) U (mean |row loss| + max |logit magnitude|), as tests/test_ladies_gpu.py.  L_var: V is quadratic in H, whose
    entries carry the fp32 error of two GEMMs and two aggregations — relative to their magnitudes at most k U with
    k = F + H + 2 (longest row) + 16 terms — so |d| <= (2 k + longest row + C + m + 8) U mean_i (s_i sum_j w_ij^2 |Hmag_j|^2 +
    |sum_j w_ij Hmag_j|^2) with Hmag the magnitude of H."""
    ops = _ops()
    from grapes_amd.ladies import weighted_structures
    from grapes_amd.modules.gcn import _WeightedGCNConvFn
    P = _step_problem(multilabel)
    tr, model, s = _trainer(P, var_coef)
    W1, b1, W2, b2 = (_np(p).copy() for p in (model.gcn_layers[0].lin.weight, model.gcn_layers[0].bias,
                                              model.gcn_layers[1].lin.weight, model.gcn_layers[1].bias))
    wg0 = _np(s.w_g).copy()
    loss, b = tr.step(_dev(P.targets))
    tr.check()
    nb = b.num_nodes
    ei, ew = [_np(t).astype(np.int64) for t in b.edge_index], [_np(t) for t in b.edge_weight]
    lp = [_np(t).astype(np.int64) for t in b.local_prev]
    xb = P.x32[_np(b.node_idx)]
    lt, y_t = _np(b.local_targets).astype(np.int64), P.labels[P.targets]
    a_dev = _np(b.a)
    with torch.no_grad():                                                # the device's ReLU gates of the hidden layer
        ws = weighted_structures(b.edge_index, nb)
        gate = _np(_WeightedGCNConvFn.apply(_dev(xb), _dev(W1), _dev(b1), b.edge_weight[-1], ws[-1], True, ops.WGCN_UNNORMALIZED, 1.0) > 0)
    # the chain of (reference, magnitude, fp32 baseline) triples, the weights taken as the device's fp32 values
    P1 = MO.ModeProblem(ei[-1][0], ei[-1][1], ew[-1], nb, normalize=False)
    P0 = MO.ModeProblem(ei[0][0], ei[0][1], ew[0], nb, normalize=False)
    x3 = (xb.astype(F64), np.abs(xb.astype(F64)), xb)
    h3 = P1.chain_forward(x3, W1, b1, gate=gate)
    z3 = P0.chain_forward(h3, W2, b2)
    lref, d3, row_mag, z_mag = TL._loss_parts(z3, lt, y_t)
    back2 = P0.chain_backward(d3, h3, W2)
    g64 = gate.astype(F64)
    dh3 = tuple(v * g64.astype(v.dtype) for v in back2["dx"])
    back1 = P1.chain_backward(dh3, x3, W1)
    l64, dW, db, z64 = LO.train_step64(xb, [W1, W2], [b1, b2], ei, ew, lt, y_t, gates=[gate])
    assert np.allclose(z3[0], z64, rtol=1e-11, atol=1e-12) and np.isclose(lref, l64, rtol=1e-12)
    for got, want in ((back1["dW"][0], dW[0]), (back2["dW"][0], dW[1])):
        assert np.allclose(got, want, rtol=1e-10, atol=1e-13)
    what = f"asgcn {'BCE' if multilabel else 'CE'} lambda {var_coef}"
    bound = (P.B + 8) * U * (row_mag + z_mag)
    print(f"[asgcn] {what}: L_c {float(b.loss_c):.7f} fp64 {l64:.7f} |d| / bound {abs(float(b.loss_c) - l64) / bound:.3f}")
    assert abs(float(b.loss_c) - l64) <= bound
    # H of the layer that writes the logits, and L_var
    contract = lambda t3, W: (t3[0] @ W.astype(F64).T, t3[1] @ np.abs(W.astype(F64)).T,
                              acc.fp32_contract(np.ascontiguousarray(np.asarray(t3[2], dtype=F32).T), W.T.copy()).numpy())
    H3 = contract(h3, W2)
    var = AO.variance(ei[0][0], ei[0][1], ew[0], lp[0], H3[0], H3[2])
    vmag = AO.variance(ei[0][0], ei[0][1], ew[0], lp[0], H3[1]).V_mag
    rows_len = np.bincount(ei[0][1], minlength=nb)[lp[0]]
    longest = max(int(np.bincount(e[1]).max()) for e in ei)
    k = P.F + P.H + 2 * longest + 16
    vbound = (2 * k + longest + P.C + len(lp[0]) + 8) * U * float(vmag.mean())
    print(f"[asgcn] {what}: L_var {float(b.loss_var):.7f} fp64 {var.L_var:.7f} |d| / bound {abs(float(b.loss_var) - var.L_var) / vbound:.3f}")
    assert (rows_len > 0).all() and abs(float(b.loss_var) - var.L_var) <= vbound
    assert abs(float(loss) - (float(b.loss_c) + var_coef * float(b.loss_var))) <= 4 * U * (abs(float(b.loss_c)) + abs(float(b.loss_var)))
    # the classifier's gradients
    TL._judge(model.gcn_layers[0].lin.weight.grad, back1["dW"], what + " dW1")
    TL._judge(model.gcn_layers[0].bias.grad, back1["db"], what + " db1")
    TL._judge(model.gcn_layers[1].lin.weight.grad, back2["dW"], what + " dW2")
    TL._judge(model.gcn_layers[1].bias.grad, back2["db"], what + " db2")
    # G = d L / d w per layer, T, and the sampler's gradients
    G0 = [np.asarray(t) for t in P0.weight_grad(d3[0], H3[0], d3[1], H3[1], d3[2], H3[2])]
    G0 = (G0[0] + var_coef * var.dw, G0[1] + var_coef * var.dw_mag, (G0[2] + F32(var_coef) * var.dw32).astype(F32))
    X3 = contract(x3, W1)
    G1 = tuple(np.asarray(t) for t in P1.weight_grad(dh3[0], X3[0], dh3[1], X3[1], dh3[2], X3[2]))
    T3 = [AO.logq_bwd(ei[d][0], ei[d][1], ew[d], G, lp[d], nb)[:3] for d, G in ((0, G0), (1, G1))]
    sg = AO.sampler_grads(T3, a_dev, xb)
    assert (a_dev > 0).any() and (a_dev <= 0).any() and np.abs(sg["da"][0]).max() > 0
    TL._judge(torch.cat([s.w_g.grad, s.b_g.grad]), tuple(np.concatenate([p, q]) for p, q in zip(sg["dw_g"], sg["db_g"])),
              what + " dw_g and db_g")
    # the closed form is the gradient: autograd through the sampler's weights in fp64 on the same batch and masks
    c_local, v = [], []
    for L in b.layers:
        t = np.ones(P.n)
        t[_np(L.candidates)] = _np(L.c).astype(F64)
        c_local.append(t[_np(b.node_idx)])
        v.append(AO.entry_v(P.ip, P.ix, _np(L.edge_src), _np(L.edge_dst)))
    full = AO.train_step64(xb, [W1, W2], [b1, b2], wg0, np.array([0.1], F32), ei, c_local, v, lp, lt, y_t, var_coef, gates=[gate],
                           mask=(a_dev > 0))
    # (the reference above takes the device's fp32 weights as given, autograd forms them in fp64: each is within (longest row + 8) U
    # of the other, and a term of these sums holds up to four factors that depend on them — w in T, in Gbar, and through G and H)
    close = 4 * (longest + 8) * U * sg["dw_g"][1]
    print(f"[asgcn] {what}: closed form against fp64 autograd, worst |d| / bound {np.max(np.abs(sg['dw_g'][0] - full.dw_g) / close):.3f}")
    assert (np.abs(sg["dw_g"][0] - full.dw_g) <= close).all()
    assert not np.array_equal(_np(s.w_g), wg0)                           # Adam moved w_g


def test_the_variance_term_leaves_the_classifier_gradients_alone():
    """H is detached in L_var: with lambda = 0 and a sampler whose parameters need no gradient, the classifier's gradients are those of
    the lambda = 0.5 run, bit for bit (the same seed and parameters draw the same batch)."""
    _ops()
    P = _step_problem(False)
    tr_a, model_a, s_a = _trainer(P, 0.5)
    state = {k: v.clone() for k, v in model_a.state_dict().items()}
    tr_b, model_b, s_b = _trainer(P, 0.0, train_sampler=False, state=state)
    _, ba = tr_a.step(_dev(P.targets))
    _, bb = tr_b.step(_dev(P.targets))
    assert torch.equal(ba.node_idx, bb.node_idx) and all(torch.equal(p, q) for p, q in zip(ba.edge_weight, bb.edge_weight))
    for pa, pb in zip(model_a.parameters(), model_b.parameters()):
        assert torch.equal(pa.grad, pb.grad)
    assert s_a.w_g.grad is not None and s_b.w_g.grad is None
    assert torch.equal(ba.loss_c, bb.loss_c) and torch.equal(ba.loss_var, bb.loss_var)


def test_training_lowers_the_loss_and_evaluates():
    _ops()
    from grapes_amd.asgcn import AsgcnTrainer
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.ladies import build_model
    from grapes_amd.modules.asgcn import AdaptiveSampler
    n, F, C = 512, 16, 4
    rng = np.random.default_rng(61)
    y = rng.integers(0, C, n)
    same = [(a, b) for a, b in rng.integers(0, n, (6000, 2)) if y[a] == y[b] and a != b][:1200]     # edges inside the classes
    s, d = np.array([a for a, b in same] + [b for a, b in same]), np.array([b for a, b in same] + [a for a, b in same])
    ip, ix = LO.csr_from_edges(s, d, n)
    x = (np.eye(C)[y] @ rng.standard_normal((C, F)) * 2.0 + 0.3 * rng.standard_normal((n, F))).astype(F32)
    g = DeviceGraph.from_csr(ip, ix)
    model = build_model(F, 16, C, 2, 0.0, "cuda")
    sampler = AdaptiveSampler(g, 64, 2, F, seed=6)
    opt = torch.optim.Adam(list(model.parameters()) + list(sampler.parameters()), lr=2e-2)
    tr = AsgcnTrainer(g, _dev(x), _dev(y), model, sampler, opt, var_coef=0.5)
    train = _dev(np.arange(0, n, 2))
    losses = [tr.epoch(train, 128) for _ in range(5)]
    print("[asgcn] epoch losses", np.round(losses, 4))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    mask = torch.zeros(n, dtype=torch.bool, device="cuda"); mask[1::2] = True
    val, test = tr.evaluate((mask, ~mask))
    assert np.isfinite(val) and np.isfinite(test) and 0.0 <= val <= 1.0 and 0.0 <= test <= 1.0
    for k in range(30 - 10):                                             # 30 steps in all
        _, b = tr.step(train[(k % 2) * 128:(k % 2) * 128 + 128])
    tr.check()
    assert np.isfinite(float(b.loss_var)) and np.isfinite(float(b.loss_c))
    assert bool(torch.isfinite(sampler.w_g).all()) and bool(torch.isfinite(sampler.b_g).all())


def test_cli_two_epochs(capsys):
    _ops()
    from grapes_amd import asgcn
    v = asgcn.main(["--dataset", "cora", "--max_epoch", "2", "--hidden_dim", "32", "--seed", "1"])
    out = capsys.readouterr().out
    assert out.count("Epoch: ") == 2 and "Acc: " in out and 0.0 <= v <= 1.0
