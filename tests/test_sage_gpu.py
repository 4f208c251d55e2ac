"""GraphSAGE on the MI355X (grapes_amd/csrc/sage_kernels.hip, modules/gcn.py SAGEConv / SAGE, modules/sage.py, graphsage.py) against
the host oracle of tests/sage_oracle.py.

Sampled sets and edge lists are bit-exact: the selection is integer arithmetic on Philox words (or given keys).  Activations and
gradients are judged by the project's measure (gat_oracle.rel_err: max |a - ref| / max(1, max |ref|)) at its tolerances, 1e-5 and
1e-4, against fp64; the backward of a fused ReLU is compared on the device's own gates (out > 0), so a pre-activation within fp32
rounding of 0 cannot flip a whole gradient row.  Every graph has at most 1 200 nodes, but the one of the row list past one scan
tile (5 000)."""
import numpy as np
import pytest
import torch

from tests import sage_oracle as SO

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4
F32, F64 = np.float32, np.float64
MARK = -7
FMARK = 12345.0
UNIFORM_SEED = 2                       # tests/test_sage_cpu.py checks that the oracle alone meets the 6 sigma band for this seed


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


# ------------------------------------------------------------------------------------------------------------ the sampler
N_S = 1200
_SGRAPH = {}


def _degrees(k):
    return [0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, 128, 129, 1000]


def _sgraph(k):
    """The hand graph for fanout k: rows 0 .. 10 have the degrees 0, 1, k - 1, k, k + 1, 63, 64, 65, 128, 129 and 1000."""
    _ops()
    if k not in _SGRAPH:
        ip, ix = SO.degree_graph(_degrees(k), N_S, 100 + k)
        _SGRAPH[k] = (ip, ix, _dev(ip), _dev(ix))
    return _SGRAPH[k]


def _sample(ops, k, rows, fanout, e_cap=None, **kw):
    ip, ix, rp, col = _sgraph(k)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    src, dst, pos, d_e = ops.sage_sample_layer(rp, col, N_S, _dev(np.asarray(rows, dtype=np.int32)), fanout, e_cap=e_cap, status=status,
                                               **kw)
    e = int(d_e.item())
    return _np(src)[:e].astype(np.int64), _np(dst)[:e].astype(np.int64), _np(pos)[:e], int(status.item())


def _same(got, want, what):
    for g, w, name in zip(got, want, ("src", "dst", "pos")):
        assert np.array_equal(g, w), (what, name)


ROWS = np.array([10, 4, 0, 7, 1, 9, 3, 6, 2, 8, 5])                      # every degree, the hub first (the largest offsets)


@pytest.mark.parametrize("offset", [0, (1 << 33) + 5])
@pytest.mark.parametrize("k", [1, 3, 64])
def test_sampler_on_the_philox_stream(k, offset):
    ops = _ops()
    ip, ix, _, _ = _sgraph(k)
    want = SO.sample_layer(ip, ix, ROWS, k, seed=77, offset=offset)
    got = _sample(ops, k, ROWS, k, philox_seed=77, philox_offset=offset)
    assert got[3] == 0 and len(got[0]) == sum(min(d, k) for d in _degrees(k))
    _same(got, want, f"k={k} offset={offset}")
    assert np.array_equal(ix[got[2]], got[0])                            # edge_pos indexes col back to edge_src
    again = _sample(ops, k, ROWS, k, philox_seed=77, philox_offset=offset)
    _same(again, got, "two calls on one stream")
    other = _sample(ops, k, ROWS, k, philox_seed=78, philox_offset=offset)
    assert not np.array_equal(other[0], got[0])


@pytest.mark.parametrize("k", [1, 3, 64])
def test_sampler_with_given_keys_and_forced_ties(k):
    ops = _ops()
    ip, ix, _, _ = _sgraph(k)
    total = int(sum(_degrees(k)))
    rng = np.random.default_rng(5 + k)
    cases = {"random": rng.integers(0, 2 ** 32, total, dtype=np.uint64).astype(np.uint32),
             "all equal": np.full(total, 0x80000000, np.uint32),
             "few values": rng.integers(0, 3, total).astype(np.uint32) << 30}
    ties = np.full(total, 9, np.uint32)                                  # rows of ROWS' order: the hub's entries are positions 0 .. 999
    ties[60:68] = 4                                                      # equal keys on both sides of entry 63 / 64 of the hub
    ties[1000 + (k + 1) + 0 + 62:1000 + (k + 1) + 0 + 66] = 4            # ... and of row 7 (degree 65), third in ROWS after rows 10, 4, 0
    cases["ties around 63 / 64"] = ties
    for name, words in cases.items():
        want = SO.sample_layer(ip, ix, ROWS, k, keys=words)
        got = _sample(ops, k, ROWS, k, keys=_keys(words), deg_sum=total)
        assert got[3] == 0
        _same(got, want, f"k={k} {name}")
    got = _sample(ops, k, ROWS, k, keys=_keys(cases["all equal"]), deg_sum=total)
    hub = got[2][got[1] == 10] - ip[10]
    assert np.array_equal(hub, np.arange(k))                             # all keys equal: the first k positions
    got = _sample(ops, k, ROWS, k, keys=_keys(ties), deg_sum=total)
    hub = got[2][got[1] == 10] - ip[10]
    assert np.array_equal(hub, sorted((list(range(60, 68)) + list(range(0, 60)))[:k]))   # the eight 4s first, then the 9s from position 0


def test_a_row_listed_twice_draws_independently_and_a_short_key_list_is_reported():
    ops = _ops()
    ip, ix, _, _ = _sgraph(3)
    rows = np.array([8, 10, 8, 8, 10])
    want = SO.sample_layer(ip, ix, rows, 3, seed=11, offset=0)
    got = _sample(ops, 3, rows, 3, philox_seed=11)
    _same(got, want, "repeated rows")
    picks = [tuple(got[2][3 * j:3 * j + 3]) for j in range(5)]
    assert len({picks[0], picks[2], picks[3]}) > 1 and picks[1] != picks[4]
    short = _sample(ops, 3, rows, 3, keys=_keys(np.zeros(100, np.uint32)))
    assert short[3] & 4                                                  # a stream position past the key list


def test_device_row_count_offset_advance_and_untouched_tails():
    ops = _ops()
    ip, ix, rp, col = _sgraph(3)
    rows = _dev(ROWS.astype(np.int32))
    d_m = torch.tensor([5], dtype=torch.int32, device="cuda")
    d_off = torch.tensor([40], dtype=torch.int64, device="cuda")
    cap = 3 * len(ROWS)
    out = (torch.full((cap,), MARK, dtype=torch.int32, device="cuda"), torch.full((cap,), MARK, dtype=torch.int32, device="cuda"),
           torch.full((cap,), MARK, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.sage_sample_layer(rp, col, N_S, rows, 3, e_cap=cap, philox_seed=3, philox_offset=999, d_philox_offset=d_off, d_m=d_m,
                          status=status, out=out)
    want = SO.sample_layer(ip, ix, ROWS[:5], 3, seed=3, offset=40)       # the device offset wins over the host value
    e = int(out[3].item())
    assert e == len(want[0]) and int(status.item()) == 0
    _same([_np(t)[:e] for t in out[:3]], want, "d_m = 5")
    for t in out[:3]:
        assert bool((t[e:] == MARK).all())                               # the rows past d_m wrote nothing
    assert int(d_off.item()) == 40 + SO.offset_advance(want[3])
    ops.sage_sample_layer(rp, col, N_S, rows, 3, e_cap=cap, philox_seed=3, d_philox_offset=d_off, d_m=d_m, status=status, out=out)
    nxt = SO.sample_layer(ip, ix, ROWS[:5], 3, seed=3, offset=40 + SO.offset_advance(want[3]))
    _same([_np(t)[:e] for t in out[:3]], nxt, "the advanced offset")


def test_a_row_list_past_one_scan_tile():
    """4 500 list rows over a sparse graph of 5 000 nodes: sage_scan_k's two prefixes carry their totals from one tile of 4 096 rows
    into the next.  The 1 000-entry hub is listed first, so every later stream position is large, and 300 rows are listed twice.  On
    the Philox stream, then with a live count on the device below m (behind the tile boundary)."""
    ops = _ops()
    n, k, m = 5000, 3, 4500
    rng = np.random.default_rng(31)
    ip, ix = SO.degree_graph([1000] + rng.integers(0, 7, n - 1).tolist(), n, 32)
    rows = np.concatenate([[0], rng.permutation(np.arange(1, n))[:m - 301], np.zeros(300, np.int64)])
    rows[-300:] = rows[1:301]
    assert len(rows) == m and (np.diff(ip)[rows[4096:]] > k).any()
    rp, col, d_rows = _dev(ip), _dev(ix), _dev(rows.astype(np.int32))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for live in (m, 4200):
        want = SO.sample_layer(ip, ix, rows[:live], k, seed=21, offset=7)
        d_m = None if live == m else torch.tensor([live], dtype=torch.int32, device="cuda")
        src, dst, pos, d_e = ops.sage_sample_layer(rp, col, n, d_rows, k, philox_seed=21, philox_offset=7, d_m=d_m, status=status)
        e = int(d_e.item())
        assert e == len(want[0]) and int(status.item()) == 0
        _same([_np(t)[:e] for t in (src, dst, pos)], want, f"4 500 rows, {live} live")


def test_overflow_and_bad_row_id():
    ops = _ops()
    ip, ix, rp, col = _sgraph(3)
    want = SO.sample_layer(ip, ix, ROWS, 3, seed=9, offset=0)
    full = len(want[0])
    cap = full - 5
    out = (torch.full((full,), MARK, dtype=torch.int32, device="cuda"), torch.full((full,), MARK, dtype=torch.int32, device="cuda"),
           torch.full((full,), MARK, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.sage_sample_layer(rp, col, N_S, _dev(ROWS.astype(np.int32)), 3, e_cap=cap, philox_seed=9, status=status, out=out)
    assert int(status.item()) == 1 and int(out[3].item()) == cap
    _same([_np(t)[:cap] for t in out[:3]], [w[:cap] for w in want[:3]], "overflow: the head is the list's head")
    for t in out[:3]:
        assert bool((t[cap:] == MARK).all())                             # nothing past e_cap
    rows = np.array([4, N_S, 6, -1, 5])
    got = _sample(ops, 3, rows, 3, philox_seed=9)
    assert got[3] == 4
    _same(got, SO.sample_layer(ip, ix, rows, 3, seed=9, offset=0, num_nodes=N_S), "a row id of N is an empty row")
    with pytest.raises(ValueError):
        ops.sage_sample_layer(rp, col, N_S, _dev(ROWS.astype(np.int32)), 65)
    with pytest.raises(ValueError):
        ops.sage_sample_layer(rp, col, N_S, _dev(ROWS.astype(np.int32)), 3, deg_sum=2 ** 31)


def test_uniformity_under_a_fixed_seed():
    """One degree-10 row listed 4096 times at fanout 3: every neighbour's inclusion count is within 6 sigma of 4096 * 0.3 = 1228.8,
    sigma = sqrt(4096 * 0.3 * 0.7) = 29.3, i.e. +-176 (and equals the oracle's)."""
    ops = _ops()
    ip, ix = SO.csr_from_rows([list(range(1, 11))] + [[] for _ in range(10)])
    rows = np.zeros(4096, np.int32)
    src, dst, pos, d_e = ops.sage_sample_layer(_dev(ip), _dev(ix), 11, _dev(rows), 3, philox_seed=UNIFORM_SEED)
    assert int(d_e.item()) == 3 * 4096
    counts = np.bincount(_np(src), minlength=11)[1:]
    want = SO.sample_layer(ip, ix, rows, 3, seed=UNIFORM_SEED, offset=0)
    print("[sage] inclusion counts", counts, "worst |d| =", np.abs(counts - 1228.8).max())
    assert np.abs(counts - 1228.8).max() <= 176.0
    assert np.array_equal(_np(src), want[0])


# ------------------------------------------------------------------------------------------------------------ aggregation, SAGEConv
SHAPES = [(1, 1), (5, 3), (100, 256), (300, 47), (64, 64), (260, 4)]
_CGRAPH = {}


def _cgraph(n):
    _ops()
    if n not in _CGRAPH:
        ei = SO.conv_graph(n, 20 + n)
        _CGRAPH[n] = (ei, _dev(ei.astype(np.int32)))
    return _CGRAPH[n]


def _conv_reference(x, ei, wl, b, wr, aggr, relu, gate, gout):
    """fp64: the forward with a true ReLU, and the gradients of sum(out * gout) with the ReLU replaced by the device's gates."""
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=F64))
    fwd = SO.sage_conv64(t(x), ei, t(wl), t(b), t(wr), aggr, relu=relu).numpy()
    leaves = [None if a is None else t(a).requires_grad_(True) for a in (x, wl, b, wr)]
    out = SO.sage_conv64(leaves[0], ei, leaves[1], leaves[2], leaves[3], aggr, gate=gate if relu else None)
    (out * t(gout)).sum().backward()
    return fwd, [None if l is None else l.grad.numpy() for l in leaves]


def _run_conv(n, fi, fo, aggr, relu, form, root=True, bias=True, long_rows=None, seed=0):
    from grapes_amd.modules.gcn import SAGEConv
    ei, ei_d = _cgraph(n)
    rng = np.random.default_rng(1000 * fi + fo + seed)
    torch.manual_seed(1000 * fi + fo + seed)                             # the same weights whatever the form
    conv = SAGEConv(fi, fo, aggr=aggr, root_weight=root, bias=bias).cuda()
    if bias:
        with torch.no_grad():
            conv.lin_l.bias.copy_(_dev((rng.standard_normal(fo) * 0.5).astype(F32)))
    x32 = rng.standard_normal((n, fi)).astype(F32)
    gout = rng.standard_normal((n, fo)).astype(F32)
    x = _dev(x32).requires_grad_(True)
    out = conv(x, ei_d, relu=relu, _form=form, _long_rows=long_rows)
    out.backward(_dev(gout))
    wl, wr = _np(conv.lin_l.weight), _np(conv.lin_r.weight) if root else None
    b = _np(conv.lin_l.bias) if bias else None
    fwd, grads = _conv_reference(x32, ei, wl, b, wr, aggr, relu, _np(out) > 0, gout)
    what = f"n={n} {fi}->{fo} {aggr} relu={relu} {form} root={root} bias={bias} long={long_rows}"
    errs = {"out": SO.rel_err(_np(out), fwd), "dx": SO.rel_err(_np(x.grad), grads[0]),
            "dW_l": SO.rel_err(_np(conv.lin_l.weight.grad), grads[1])}
    if bias:
        errs["db"] = SO.rel_err(_np(conv.lin_l.bias.grad), grads[2])
    if root:
        errs["dW_r"] = SO.rel_err(_np(conv.lin_r.weight.grad), grads[3])
    print(f"[sage] {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.isfinite(out).all()
    assert errs.pop("out") <= ACT_TOL, what
    assert all(v <= GRAD_TOL for v in errs.values()), (what, errs)
    return _np(out)


@pytest.mark.parametrize("fi,fo", SHAPES)
@pytest.mark.parametrize("n", [1, 37])
def test_sageconv_both_forms_against_fp64(n, fi, fo):
    _ops()
    from grapes_amd.modules.gcn import SAGEConv
    probe = SAGEConv(fi, fo)
    forms = [f for f in ("transform", "aggregate") if probe.form_ok(f)]
    assert "transform" in forms and (("aggregate" in forms) == (fo >= 2))   # every listed shape runs transform-first
    assert probe.default_form() == ("aggregate" if (fi, fo) == (100, 256) else "transform")   # the dispatch rule on these shapes
    for aggr in ("mean", "sum"):
        for relu in (False, True):
            outs = [_run_conv(n, fi, fo, aggr, relu, form) for form in forms]
            if len(outs) == 2:
                assert SO.rel_err(outs[0], outs[1]) <= 2 * ACT_TOL        # both within ACT_TOL of one reference
    default = _run_conv(n, fi, fo, "mean", True, None)
    assert np.array_equal(default, _run_conv(n, fi, fo, "mean", True, probe.default_form()))   # the default IS that form, bit for bit


@pytest.mark.parametrize("form", ["transform", "aggregate"])
def test_sageconv_options_and_long_row_items(form):
    _ops()
    for aggr in ("mean", "sum"):
        _run_conv(37, 12, 20, aggr, True, form, root=False)
        _run_conv(37, 12, 20, aggr, False, form, bias=False)
        _run_conv(37, 12, 20, aggr, True, form, root=False, bias=False)
        a = _run_conv(37, 64, 64, aggr, True, form, long_rows=True)       # the hub's 200 entries as 4 work items + a combine
        b = _run_conv(37, 64, 64, aggr, True, form, long_rows=False)      # ... and by one group of lanes
        assert SO.rel_err(a, b) <= 2 * ACT_TOL
        _run_conv(37, 5, 7, aggr, True, form, long_rows=True)            # scalar columns through the items
    from grapes_amd.modules.gcn import SAGEConv
    with pytest.raises(ValueError, match="not built"):
        SAGEConv(47, 1).cuda()(torch.zeros(37, 47, device="cuda"), _cgraph(37)[1], _form="aggregate")


def test_aggregate_entry_points_strided_blocks_and_device_row_count():
    """ops.sage_aggregate_fwd / _bwd on column blocks of wider matrices, and with d_n below the allocated rows: rows past it stay
    untouched."""
    ops = _ops()
    n, m, f = 48, 37, 12
    ei, _ = _cgraph(37)                                                   # entries among the first 37 nodes only
    src, dst = (_dev(ei[k].astype(np.int32)) for k in (0, 1))
    rng = np.random.default_rng(7)
    wide = rng.standard_normal((n, 3 * f)).astype(F32)                    # src = columns [f, 2 f), add = columns [2 f, 3 f)
    bias = rng.standard_normal(f).astype(F32)
    wide_d = _dev(wide)
    x64 = torch.as_tensor(wide[:m, f:2 * f].astype(F64))
    for live in (None, m):
        d_n = None if live is None else torch.tensor([m], dtype=torch.int32, device="cuda")
        rows = n if live is not None else m
        prep = ops.gcn2_attach_loops(ops.PreparedGraph(src, dst, rows, d_n=d_n), src, dst)
        w_d = wide_d[:rows]
        for aggr in ("mean", "sum"):
            out = torch.full((rows, 2 * f), FMARK, device="cuda")
            ops.sage_aggregate_fwd(w_d[:, f:2 * f], prep, aggr, add=w_d[:, 2 * f:], bias=_dev(bias), relu=True, out=out[:, f:],
                                   copy_out=out[:, :f])
            ref = (SO.aggregate64(x64, ei, m, aggr).numpy() + wide[:m, 2 * f:] + bias).clip(min=0)
            got = _np(out)
            assert SO.rel_err(got[:m, f:], ref) <= ACT_TOL and np.array_equal(got[:m, :f], wide[:m, f:2 * f])
            assert (got[m:] == FMARK).all()
            # backward: dout = columns [0, f) of a wide matrix, gated by the forward's output
            dh = torch.full((rows, 2 * f), FMARK, device="cuda")
            dsrc, dadd, dbias = ops.sage_aggregate_bwd(w_d[:, :f], prep, aggr, relu_out=out[:, f:], add=w_d[:, 2 * f:],
                                                       dsrc=dh[:, :f], dadd=dh[:, f:], want_bias=True)
            g = wide[:m, :f].astype(F64) * (got[:m, f:] > 0)
            want = SO.mean_sum_backward_closed_form(g, ei, m, aggr) + wide[:m, 2 * f:]
            gh = _np(dh)
            assert SO.rel_err(gh[:m, :f], want) <= GRAD_TOL and SO.rel_err(gh[:m, f:], g) <= ACT_TOL
            assert SO.rel_err(_np(dbias), g.sum(0)) <= GRAD_TOL
            assert (gh[m:] == FMARK).all()
            again = ops.sage_aggregate_bwd(w_d[:, :f], prep, aggr, relu_out=out[:, f:], add=w_d[:, 2 * f:], want_bias=True)
            assert torch.equal(again[0][:m], dh[:m, :f]) and torch.equal(again[2], dbias)     # fixed order: the same bits
    with pytest.raises(ValueError, match="not built"):
        ops.sage_aggregate_fwd(torch.zeros(37, 257, device="cuda"), prep, "mean")
    with pytest.raises(NotImplementedError):
        ops.sage_aggregate_fwd(torch.zeros(37, 8, device="cuda"), prep, "max")


# ------------------------------------------------------------------------------------------------------------ model, trainer, CLI
def _graph40():
    _ops()
    from grapes_amd.graph import DeviceGraph
    from tests import ladies_oracle as LO
    if "g40" not in _CGRAPH:
        ip, ix = LO.random_symmetric(40, 6, 33, loops=3)
        _CGRAPH["g40"] = (ip, ix, DeviceGraph.from_csr(ip, ix))
    return _CGRAPH["g40"]


def _params(model):
    return [(_np(c.lin_l.weight).copy(), _np(c.lin_l.bias).copy(), _np(c.lin_r.weight).copy()) for c in model.convs]


@pytest.mark.parametrize("fanouts", [[3, 2], [-1, 2]])
def test_neighbor_sampler_batch_and_model_against_the_oracle(fanouts):
    _ops()
    from grapes_amd.target_batch import _TargetLoss
    from grapes_amd.modules.gcn import SAGE
    from grapes_amd.modules.sage import NeighborSampler
    ip, ix, g = _graph40()
    targets = np.array([7, 31, 2, 18, 5])
    s = NeighborSampler(g, fanouts, seed=21)
    b = s.sample(_dev(targets))
    s.check()
    ob = SO.sample(ip, ix, targets, fanouts, seed=21)
    assert np.array_equal(_np(b.node_idx), ob.node_idx) and np.array_equal(_np(b.local_targets), ob.local_targets)
    assert b.num_nodes == len(ob.node_idx) and s.philox_offset == ob.philox_offset
    for d, (L, R) in enumerate(zip(b.layers, ob.layers)):
        assert np.array_equal(_np(L.prev), R.prev) and np.array_equal(_np(L.after), R.after), d
        assert np.array_equal(_np(L.edge_src), R.src) and np.array_equal(_np(L.edge_dst), R.dst), d
        assert np.array_equal(_np(b.edge_index[d]), ob.edge_index[d]), d
    for t in (g.bits, g.prev_bits):
        assert not bool(t.any())                                         # the graph's bitmaps are zero at rest again
    b2 = s.sample(_dev(targets))                                         # the stream has advanced: the oracle from that offset
    ob2 = SO.sample_layer(ip, ix, targets, fanouts[0], seed=21, offset=ob.philox_offset) if fanouts[0] != -1 else None
    if ob2 is not None:
        assert np.array_equal(_np(b2.layers[0].edge_src), ob2[0])
    # given keys
    k0 = np.random.default_rng(2).integers(0, 2 ** 32, int(ob.layers[0].deg_sum), dtype=np.uint64).astype(np.uint32)
    if fanouts[0] != -1:
        bk = NeighborSampler(g, fanouts, seed=21).sample(_dev(targets), keys=[_keys(k0)])
        assert np.array_equal(_np(bk.layers[0].edge_src), SO.sample_layer(ip, ix, targets, fanouts[0], keys=k0)[0])
    # SAGE logits and loss on the batch
    F, H, C = 9, 8, 4
    rng = np.random.default_rng(3)
    x32 = rng.standard_normal((40, F)).astype(F32)
    y = rng.integers(0, C, 40)
    for aggr in ("mean", "sum"):
        model = SAGE(F, [H, C], aggr=aggr).cuda()
        xb = x32[ob.node_idx]
        out = model(_dev(xb), b.edge_index)
        loss = _TargetLoss.apply(out, b.local_targets, b.targets, _dev(y))
        l64, _, z64 = SO.train_step64(xb, _params(model), ob.edge_index, ob.local_targets, y[targets], aggr)
        assert SO.rel_err(_np(out), z64) <= ACT_TOL
        assert abs(float(loss.detach()) - l64) <= ACT_TOL * max(1.0, abs(l64))
        whole = model(_dev(x32), g)                                      # one graph for every layer: the DeviceGraph as stored
        ei_all = np.stack([ix.astype(np.int64), np.repeat(np.arange(40), np.diff(ip))])
        zw = SO.sage_forward64(torch.as_tensor(x32.astype(F64)), [tuple(torch.as_tensor(p.astype(F64)) for p in layer)
                                                                  for layer in _params(model)], ei_all, aggr).numpy()
        assert SO.rel_err(_np(whole), zw) <= ACT_TOL


def test_trainer_step_against_fp64():
    """One SageTrainer.step with Adam.  The gradients are judged against fp64 on the device's ReLU gates (as tests/test_ladies_gpu.py
    judges its step by the gradients).  Adam's first step is p - lr g / (|g| + eps): where |g| exceeds twice what GRAD_TOL lets the
    device's gradient differ by, its sign — the whole step — is fixed, and there the parameters are held to the fp64 step; elsewhere
    a gradient within tolerance may step the other way, so those elements are only held to |step| <= lr."""
    _ops()
    from grapes_amd.graphsage import SageTrainer
    from grapes_amd.modules.gcn import SAGE, SAGEConv
    from tests import ladies_oracle as LO
    from grapes_amd.graph import DeviceGraph
    n, F, H, C, B, lr = 256, 32, 16, 4, 32, 1e-3
    ip, ix = LO.random_symmetric(n, 8, 51, loops=6)
    g = DeviceGraph.from_csr(ip, ix)
    rng = np.random.default_rng(52)
    x32 = rng.standard_normal((n, F)).astype(F32)
    labels = rng.integers(0, C, n)
    model = SAGE(F, [H, C]).cuda()
    p0 = _params(model)
    tr = SageTrainer(g, _dev(x32), _dev(labels), model, torch.optim.Adam(model.parameters(), lr=lr), fanouts=[5, 3], seed=8)
    targets = rng.permutation(n)[:B]
    loss, b = tr.step(_dev(targets))
    ob = SO.sample(ip, ix, targets, [5, 3], seed=8)
    assert np.array_equal(_np(b.node_idx), ob.node_idx)
    for ei, oe in zip(b.edge_index, ob.edge_index):
        assert np.array_equal(_np(ei), oe)
    xb = x32[ob.node_idx]
    with torch.no_grad():                                                # the device's ReLU gates of the hidden layer, from p0
        c0 = SAGEConv(F, H).cuda()
        c0.load_state_dict({"lin_l.weight": _dev(p0[0][0]), "lin_l.bias": _dev(p0[0][1]), "lin_r.weight": _dev(p0[0][2])})
        gate = _np(c0(_dev(xb), b.edge_index[-1], relu=True) > 0)
    l64, grads, _ = SO.train_step64(xb, p0, ob.edge_index, ob.local_targets, labels[targets], "mean", gates=[gate])
    assert abs(float(loss) - l64) <= ACT_TOL * max(1.0, abs(l64))
    names = ("lin_l.weight", "lin_l.bias", "lin_r.weight")
    for li, conv in enumerate(model.convs):
        for name, before, g64 in zip(names, p0[li], grads[li]):
            mod, attr = name.split(".")
            p = getattr(getattr(conv, mod), attr)
            err = SO.rel_err(_np(p.grad), g64)
            step = _np(p).astype(F64) - before
            sure = np.abs(g64) > 2 * GRAD_TOL * max(1.0, float(np.abs(g64).max()))
            ref = SO.adam_first_step64(before, g64, lr=lr)
            perr = SO.rel_err(_np(p)[sure], ref[sure]) if sure.any() else 0.0
            print(f"[sage] step convs.{li}.{name}: grad err {err:.2e}, {int(sure.sum())}/{sure.size} sure elements, param err {perr:.2e}")
            assert err <= GRAD_TOL and perr <= GRAD_TOL
            assert sure.any() and np.abs(step).max() <= lr * (1 + 1e-3) + 1e-7 and np.abs(step).max() > 0


def test_training_lowers_the_loss_and_evaluates():
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.graphsage import SageTrainer, build_model
    from tests import ladies_oracle as LO
    n, F, C = 512, 16, 4
    rng = np.random.default_rng(61)
    y = rng.integers(0, C, n)
    same = [(a, b) for a, b in rng.integers(0, n, (6000, 2)) if y[a] == y[b] and a != b][:1200]     # edges inside the classes
    s, d = np.array([a for a, b in same] + [b for a, b in same]), np.array([b for a, b in same] + [a for a, b in same])
    ip, ix = LO.csr_from_edges(s, d, n)
    x = (np.eye(C)[y] @ rng.standard_normal((C, F)) * 2.0 + 0.3 * rng.standard_normal((n, F))).astype(F32)
    g = DeviceGraph.from_csr(ip, ix)
    model = build_model(F, 16, C, 2, 0.0, "mean", "cuda")
    tr = SageTrainer(g, _dev(x), _dev(y), model, torch.optim.Adam(model.parameters(), lr=2e-2), fanouts=[4, 3], seed=6)
    train = _dev(np.arange(0, n, 2))
    losses = [tr.epoch(train, 128) for _ in range(4)]
    print("[sage] epoch losses", np.round(losses, 4))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    mask = torch.zeros(n, dtype=torch.bool, device="cuda"); mask[1::2] = True
    val, test = tr.evaluate((mask, ~mask))
    assert np.isfinite(val) and np.isfinite(test) and 0.0 <= val <= 1.0 and 0.0 <= test <= 1.0
    with pytest.raises(ValueError, match="fanouts"):
        SageTrainer(g, _dev(x), _dev(y), model, None, fanouts=[4])


def test_cli_two_epochs_twice(capsys):
    _ops()
    from grapes_amd import graphsage
    argv = ["--dataset", "cora", "--fanouts", "5,5", "--max_epoch", "2", "--hidden_dim", "32", "--seed", "1"]
    v = graphsage.main(argv)
    out = capsys.readouterr().out
    assert out.count("Epoch: ") == 2 and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0
    assert graphsage.main(argv) == v                                     # one seed, one accuracy
