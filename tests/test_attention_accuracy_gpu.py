"""Element-wise accuracy of the GAT aggregation kernels (grapes_amd/csrc/gat_kernels.hip) against fp64: ops.gat_scores,
ops.gat_aggregate_fwd and ops.gat_aggregate_bwd called directly on graphs built by ops.PreparedGraph, each output judged relative
to the fp64 sum of |terms| of ITS OWN terms (oracle/accuracy.py, "attention aggregation").  Two conditions per output tensor
(assert_attention_accuracy): max and rms of that error within MAX_FACTOR = 6 / RMS_FACTOR = 3 of a host fp32 baseline (a two-pass
softmax whose sums run sequentially in CSR order, self-loop first), and a hard cap per output, (L_r + 14 + 2 S_r) 2^-24 mag for
the forward (derived at accuracy.gat_forward_sums) and the sums of its parts' caps for the gradients (derived at
accuracy.gat_backward_reference).  Every row tensor is judged on all rows together and on the row groups L <= 5, 30..33, 62..65,
95..129, 191..321 and the hubs one by one.  tests/test_attention_accuracy_cpu.py shows on the same problems that a faithful
emulation of the forward passes and that an accumulator left unscaled, a lost lane, a lost self-loop, a chunk merged with weight 1
and an ignored chunk do not.

Data (accuracy.attention_case): rows of 0-5, 8, 9, 15-17, 24, 30-33, 62-65, 95-97, 127-129, 191-193, 200, 257, 321, 1000 entries
and hubs of 5000-20000 (20000 entries = 313 chunks: gat_fwd_combine_k's second trip over the chunk maxima), on the graph and on
its transpose, so that the named lengths are rows of the by-target CSR (forward, ds_dst) and of the by-source CSR (dh, ds_src);
kinds normal, mixed (rows at 10^[-4, 4]), zeros, striped; the scores s_src / s_dst are multiples of 2^-7 (every sum exact, none
on LeakyReLU's kink) in the regimes narrow, wide_asc / wide_desc / wide_rand (a spread of 50 and more with the maximum in a row's
last batch, first batch, anywhere) and ties.  Capacity rows past the device-side count are NaN in every operand, the CSR past its
live extent names a NaN row, the forward's `out` is prefilled with a marker that must survive past the live rows.  The references
take the DEVICE's rowptr / csr arrays and, for the backward, the device forward's fp32 `out`; alpha is recomputed in fp64 from
the scores, never from row_ms.  row_ms itself: the maximum bit for bit the fp32 maximum of the fp32 scores, the log-sum within
(L + 14 + 2 S + 2 lse) 2^-24 of fp64.

Cases (the instantiation of ROW_LAUNCH each width reaches):
  float4  4, 128 <4, 32, 1>;  132, 256 <4, 64, 1>;  260, 1024 <4, 64, 4>
  scalar  1, 32 (unaligned view) <1, 32, 1>;  33, 64 (unaligned view) <1, 64, 1>;  65, 253 <1, 64, 4>
  small (1537 rows: every row by one group, up to 6001 entries in 188 batches), large (2641 rows: rows above 64 entries as chunk
  items + combine), rows9k (gat_bwd_params_k with 141 partial blocks, gat_bwd_params_final_k's second trip), each with its
  transpose.  Every width on `normal` (test_every_width); one float4 and one scalar width per (kind, regime), all six
  instantiations on every kind (test_kinds_and_regimes).

GATv2 (grapes_amd/csrc/gatv2_kernels.hip; ops.gatv2_aggregate_fwd / _bwd): x_l an even and x_r an odd multiple of 2^-7 (every
z = x_l[j] + x_r[i] exact, none on the kink), att ~ N(0,1) 0.3; kinds normal, zeros, striped (no `mixed`: the score depends on x_l);
the head layouts of V2_SHAPES, concat and head mean, negative_slope 0.2 and 0; the small graph with its hub cut to 700 entries and
the large one, GATv2 splitting rows above 64 entries on both.  out (and agg for the head mean), row_ms, dx_l, dx_r, datt, dbias;
the forward cap is (L + 14 + 30 S) 2^-24 mag, S including the score's own sum |att| |LeakyReLU z| (accuracy.Gatv2Weights).  The
kernel's score is not the baseline's bit for bit, so row_ms is judged as the pair maximum + log-sum against fp64.

A row group may be one row of one column; there the baseline's error is not taken below its rms over the whole tensor
(accuracy.assert_attention_accuracy says why).  What is not checked: the outputs the entry points allocate themselves (row_ms, agg,
the gradients) cannot be prefilled, so only the forward's `out` carries a marker past the device-side row count; every operand's
capacity rows are NaN, which a kernel that read them would spread into live rows.

Measured on the MI355X, worst over the cases: max / rms ratio to the fp32 baseline over all rows of a tensor, worst ratio within a
row group, worst fraction of the hard cap:
  GAT    out     2.24 / 1.50, group 3.02, cap 0.40      row_ms  maximum bit-exact, log-sum at 0.25 of its bound
         dh      2.47 / 2.38, group 5.00, cap 0.27      dbias   1.30 / 1.06, cap 0.001
         da_src  3.31 / 2.90, cap 0.004                 da_dst  2.20 / 2.86, cap 0.001
         s_src, s_dst (gat_scores)  1.24 / 0.95, cap 0.24
  GATv2  out     1.27 / 1.01, group 2.34, cap 0.58      agg     1.19 / 0.99, group 1.85, cap 0.14     row_ms  0.21 of its bounds
         dx_l    1.91 / 1.58, group 3.54, cap 0.16      dx_r    1.67 / 1.30, group 2.47, cap 0.12
         datt    0.36 / 0.35, cap < 0.001               dbias   2.00 / 1.62, cap 0.001
The rms ratios near RMS_FACTOR belong to tensors of one to four outputs (da_src at f = 1: 2.90; da_dst at f = 33: 2.86, both
below the criterion's FLOOR of 2^-30 in the baseline), where the baseline's error is a single draw of 0.05 - 0.1 u and the kernel's
0.2 - 0.3 u.  dh's 5.00 is the max ratio of the rows of up to 5 entries on the small graph's transpose (zeros, ties, f = 260): 8 u of
mag on an output whose ds_dst term comes from a long by-target row, at 0.27 of its cap.  No output exceeds a
factor or a cap, and no kernel defect was found.  The module takes 60 s there.
"""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc

pytestmark = pytest.mark.gpu

MARKER = -12345.5
VEC_WIDTHS, SCALAR_WIDTHS = (4, 128, 132, 256, 260, 1024), (1, 32, 33, 64, 65, 253)
REDUCED_VEC, REDUCED_SCALAR = (4, 132, 260), (1, 33, 65)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a, unaligned=False):
    """a on the device; unaligned: at an address that is 4 mod 16 (f % 4 == 0 then still takes the scalar kernels)."""
    a = np.ascontiguousarray(a)
    if not unaligned:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    off = next(o for o in range(1, 5) if (buf.data_ptr() + 4 * o) % 16 == 4)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


class _Graph:
    """One built graph and its arrays read back: rt / cs (by target), rs / cd (by source); live rows n of cap."""

    def __init__(self, ops, size, transpose, hub_cap=None):
        p = acc.attention_case(size, "normal", 4, transpose=transpose, hub_cap=hub_cap)
        n, cap = p["n"], p["cap"]
        self.n, self.cap = n, cap
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        self.prep = prep = ops.PreparedGraph(_dev(p["src"]), _dev(p["dst"]), cap, d_n=d_n, status=self.status)
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0
        self.rt = prep.rowptr_t[:n + 1].cpu().numpy().astype(np.int64)
        self.rs = prep.rowptr_s[:n + 1].cpu().numpy().astype(np.int64)
        self.cs = prep.csr_src.cpu().numpy()[:self.rt[-1]]
        self.cd = prep.csr_dst.cpu().numpy()[:self.rs[-1]]
        self.lens, self.lens_s = np.diff(self.rt), np.diff(self.rs)
        assert np.array_equal(self.lens, p["lens"]) and np.array_equal(self.lens_s, p["lens_s"]), "the build's rows do not have the prescribed entry counts"
        named = self.lens_s if transpose else self.lens
        assert set(acc.ATT_ROW_LENGTHS) <= set(named.tolist())
        h_rt, h_cs, h_rs, h_cd, _ = acc.host_csr(p["src"], p["dst"], n)
        for rp, col, h_col in ((self.rt, self.cs, h_cs), (self.rs, self.cd, h_cd)):
            rows = np.repeat(np.arange(n), np.diff(rp))
            assert np.array_equal(col[np.lexsort((col, rows))], h_col), "the build's rows do not hold the prescribed entries"
        prep.csr_src[int(self.rt[-1]):] = cap - 1           # the CSR past its live extent names a NaN row
        prep.csr_dst[int(self.rs[-1]):] = cap - 1
        if cap > 2048:
            assert int(prep.n_items_t.item()) > 0 and int(prep.n_items_s.item()) > 0    # rows above 64 entries became chunk items


_GRAPHS, _WEIGHTS = {}, {}


def _graph(ops, size, transpose, hub_cap=None):
    key = (size, transpose, hub_cap)
    if key not in _GRAPHS:
        _GRAPHS[key] = _Graph(ops, size, transpose, hub_cap)
    return _GRAPHS[key]


def _weights(g, size, transpose, regime):
    """(GatWeights over the device's by-target CSR, s_src, s_dst on the device) — they do not depend on kind or width."""
    key = (size, transpose, regime)
    if key not in _WEIGHTS:
        s_src, s_dst = acc.attention_scores(g.n, g.cap, regime)
        _WEIGHTS[key] = (acc.GatWeights(g.rt, g.cs, s_src, s_dst, g.n), _dev(s_src), _dev(s_dst))
    return _WEIGHTS[key]


def _attention_vectors(f, seed):
    rng = np.random.default_rng(4242 + seed)
    return ((rng.standard_normal(f) * 0.3).astype(np.float32), (rng.standard_normal(f) * 0.3).astype(np.float32))


def _forward(ops, g, w, s_src, s_dst, p, h, f, what, combos):
    """gat_aggregate_fwd for every (bias, relu) of combos from one set of reference sums -> {(bias, relu): (out, row_ms)}."""
    sums = acc.gat_forward_sums(w, p["h"])
    K = torch.from_numpy(w.K())[:, None]
    bias = _dev(p["bias"])
    res = {}
    for with_bias, relu in combos:
        tag = f"{what} b{int(with_bias)}r{int(relu)}"
        out = torch.full((g.cap, f), MARKER, device="cuda")
        o2, row_ms = ops.gat_aggregate_fwd(h, s_src, s_dst, g.prep, bias if with_bias else None, relu, out=out)
        assert o2 is out
        again = torch.full((g.cap, f), MARKER, device="cuda")
        _, ms2 = ops.gat_aggregate_fwd(h, s_src, s_dst, g.prep, bias if with_bias else None, relu, out=again)
        got = out[:g.n].cpu()
        assert bool(torch.isfinite(got).all()), f"{tag}: non-finite outputs in live rows"
        assert torch.equal(out, again) and torch.equal(row_ms[:g.n], ms2[:g.n]), f"{tag}: two runs differ"
        assert bool((out[g.n:] == MARKER).all()), f"{tag}: rows past the live count were written"
        ref, mag, base = acc.aggregate_finish(sums, p["bias"] if with_bias else None, relu)
        acc.assert_attention_accuracy(got, ref, mag, base, K * mag, g.lens, "out " + tag)
        x = acc.gat_row_ms_excess(w, row_ms[:g.n].cpu().numpy())
        print(f"[row_ms] row_ms {tag}: maximum bit-exact, log-sum at {x:.3f} of its bound")
        assert x <= 1.0, f"row_ms {tag}: log-sum at x{x:.3f} of its bound"
        res[(with_bias, relu)] = (out, row_ms)
    return res


def _backward(ops, g, w, s_src, s_dst, p, h, f, what, fwd, with_bias, relu, seed):
    out, row_ms = fwd[(with_bias, relu)]
    a_src, a_dst = _attention_vectors(f, seed)
    dout, bias = _dev(p["dout"]), _dev(p["bias"]) if with_bias else None
    args = (dout, out, h, s_src, s_dst, row_ms, _dev(a_src), _dev(a_dst), g.prep)
    got = ops.gat_aggregate_bwd(*args, bias=bias, relu=relu)
    again = ops.gat_aggregate_bwd(*args, bias=bias, relu=relu)
    ref = acc.gat_backward_reference(w, g.rs, g.cd, p["h"], p["dout"], out[:g.n].cpu().numpy(), a_src, a_dst,
                                     p["bias"] if with_bias else None, relu)
    tag = f"{what} b{int(with_bias)}r{int(relu)}"
    for name, t, t2 in zip(("dh", "da_src", "da_dst", "dbias"), got, again):
        live = t[:g.n] if name == "dh" else t
        assert torch.equal(live, t2[:g.n] if name == "dh" else t2), f"{name} {tag}: two runs differ"
        assert bool(torch.isfinite(live).all()), f"{name} {tag}: non-finite outputs"
        acc.assert_attention_accuracy(live.cpu(), *ref[name], g.lens_s if name == "dh" else None, f"{name} {tag}")


def _status(g):
    torch.cuda.synchronize()
    assert int(g.status.item()) == 0


# ------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("kind", acc.ATT_KINDS)
def test_scores_against_fp64(kind):
    """ops.gat_scores on its own: s_src = H a_src and s_dst = H a_dst against fp64 (matmul_reference: each output relative to its
    own sum of |h||a|, cap (f + 4) 2^-24 mag), every width, with a device-side row count; rows past it are not written."""
    ops = _ops()
    g = _graph(ops, "small", False)
    d_n = g.prep.d_n
    for f in VEC_WIDTHS + SCALAR_WIDTHS:
        p = acc.attention_case("small", kind, f)
        un = f in (32, 64)
        a_src, a_dst = _attention_vectors(f, f)
        s_src, s_dst = ops.gat_scores(_dev(p["h"], un), _dev(a_src), _dev(a_dst), d_n=d_n)
        ref = acc.matmul_reference(p["h"][:g.n], np.stack([a_src, a_dst], 1))
        for c, (name, s) in enumerate((("s_src", s_src), ("s_dst", s_dst))):
            got = s[:g.n].cpu()
            assert bool(torch.isfinite(got).all())
            acc.assert_aggregate_accuracy(got, ref[0][:, c], ref[1][:, c], ref[2][:, c], float(f), f"{name} {kind} f={f}")


# ------------------------------------------------------------------------------------------------- forward and backward
@pytest.mark.parametrize("width", VEC_WIDTHS + SCALAR_WIDTHS)
@pytest.mark.parametrize("size,regime", [("small", "wide_rand"), ("large", "wide_rand"), ("large", "narrow")])
def test_every_width(size, regime, width):
    """Forward (bias x ReLU) and backward (with both, with neither) at every width of ROW_LAUNCH on `normal` data: the small graph
    (every row by one group: a 6000-entry row in 95 or 188 batches) and the large one (work items) under a wide regime, where
    every batch and every chunk rescales, and the large one under the narrow regime."""
    ops = _ops()
    f = width
    g = _graph(ops, size, False)
    w, s_src, s_dst = _weights(g, size, False, regime)
    p = acc.attention_case(size, "normal", f)
    h = _dev(p["h"], f in (32, 64))
    what = f"{size} T0 normal {regime} f={f}"
    fwd = _forward(ops, g, w, s_src, s_dst, p, h, f, what, ((True, True), (False, False), (True, False), (False, True)))
    _backward(ops, g, w, s_src, s_dst, p, h, f, what, fwd, True, True, f)
    if f <= 260:
        _backward(ops, g, w, s_src, s_dst, p, h, f, what, fwd, False, False, f + 1)
    _status(g)


@pytest.mark.parametrize("regime", acc.ATT_REGIMES)
@pytest.mark.parametrize("kind", acc.ATT_KINDS)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("size", ["small", "large"])
def test_kinds_and_regimes(size, transpose, kind, regime):
    """All four kinds under every score regime on the small and the large graph and their transposes: one float4 and one scalar
    width per case, chosen so that every kind meets all six instantiations; the forward with bias x ReLU, the backward with bias
    and ReLU at the float4 width and with neither at the scalar one."""
    ops = _ops()
    g = _graph(ops, size, transpose)
    w, s_src, s_dst = _weights(g, size, transpose, regime)
    k = acc.ATT_REGIMES.index(regime) + int(transpose)
    for f, with_bias in ((REDUCED_VEC[k % 3], True), (REDUCED_SCALAR[(k + 1) % 3], False)):
        p = acc.attention_case(size, kind, f, transpose=transpose)
        h = _dev(p["h"])
        what = f"{size} T{int(transpose)} {kind} {regime} f={f}"
        fwd = _forward(ops, g, w, s_src, s_dst, p, h, f, what, ((True, True), (False, False), (True, False), (False, True)))
        _backward(ops, g, w, s_src, s_dst, p, h, f, what, fwd, with_bias, with_bias, f)
    _status(g)


@pytest.mark.parametrize("width,transpose", [(64, False), (65, True), (128, True), (132, False)])
def test_nine_thousand_rows(width, transpose):
    """rows9k (9023 allocated rows, 9000 live): gat_bwd_params_k in 141 partial blocks of 64 rows at both column-tile widths on
    either side of their edges (CW = 64 | 128 at f = 64 / 65, 128 | 256 at 128 / 132) — gat_bwd_params_final_k's lanes take a second
    and third partial — and the forward and the row gradients over a 5000-entry hub in work items."""
    ops = _ops()
    f = width
    g = _graph(ops, "rows9k", transpose)
    assert g.n > 64 * 64
    w, s_src, s_dst = _weights(g, "rows9k", transpose, "narrow")
    p = acc.attention_case("rows9k", "normal", f, transpose=transpose)
    h = _dev(p["h"])
    what = f"rows9k T{int(transpose)} normal narrow f={f}"
    fwd = _forward(ops, g, w, s_src, s_dst, p, h, f, what, ((True, True),))
    _backward(ops, g, w, s_src, s_dst, p, h, f, what, fwd, True, True, f)
    _status(g)


# -------------------------------------------------------------------------------------------------------------- GATv2
# (heads, channels, concat): (1, 5) scalar <1, 32, 1>; (3, 7) head mean, scalar, heads that are no power of two: the masked head_sum;
# (6, 8), (4, 16) <4, 32, 1> with 2 and 4 lanes a head; (16, 4) one float4 a head; (8, 32) <4, 64, 1>; (2, 128) head mean, a head
# over 32 lanes; (8, 64) <4, 64, 4>, (16, 64) F = 1024; (3, 20) float4 with C / 4 = 5 lanes a head: the masked head_sum;
# (1, 256) a head as wide as the group
V2_SHAPES = [(1, 5, True), (3, 7, False), (6, 8, True), (4, 16, True), (16, 4, True), (8, 32, True), (2, 128, False), (8, 64, True),
             (16, 64, True), (3, 20, True), (1, 256, True)]
V2_HUB_CAP = 700        # the small graph's hub for GATv2, which splits long rows on every graph: 11 work items


def _gatv2(ops, g, size, transpose, hub_cap, kind, heads, c, concat, slope, what):
    """gatv2_aggregate_fwd with bias and ReLU and with neither, gatv2_aggregate_bwd after the first; every output under both
    conditions, two runs bit-identical."""
    f = heads * c
    W = f if concat else c
    p = acc.attention_case(size, kind, f, transpose=transpose, hub_cap=hub_cap)
    v = acc.gatv2_inputs(p, heads, c)
    w = acc.Gatv2Weights(g.rt, g.cs, v["x_l"], v["x_r"], v["att"], heads, slope, g.n)
    x_l, x_r, att = _dev(v["x_l"]), _dev(v["x_r"]), _dev(v["att"])
    n = g.n
    assert int(g.prep.n_items_t.item()) > 0 and int(g.prep.n_items_s.item()) > 0
    for with_bias, relu in ((True, True), (False, False)):
        tag = f"{what} b{int(with_bias)}r{int(relu)}"
        bias_np = np.ascontiguousarray(v["bias"][:W]) if with_bias else None
        bias = _dev(bias_np) if with_bias else None
        out, agg, row_ms = ops.gatv2_aggregate_fwd(x_l, x_r, att, g.prep, heads, concat, slope, bias, relu)
        out2, agg2, ms2 = ops.gatv2_aggregate_fwd(x_l, x_r, att, g.prep, heads, concat, slope, bias, relu)
        assert torch.equal(out[:n], out2[:n]) and torch.equal(row_ms[:n], ms2[:n]), f"{tag}: two runs differ"
        assert bool(torch.isfinite(out[:n]).all()), f"{tag}: non-finite outputs in live rows"
        ref = acc.gatv2_forward_reference(w, bias_np, relu, concat)
        acc.assert_attention_accuracy(out[:n].cpu(), *ref["out"], g.lens, "out " + tag)
        if not concat:
            assert torch.equal(agg[:n], agg2[:n])
            acc.assert_attention_accuracy(agg[:n].cpu(), *ref["agg"], g.lens, "agg " + tag)
        x = acc.gatv2_row_ms_excess(w, row_ms[:n].cpu().numpy())
        print(f"[row_ms] row_ms {tag}: maximum and log-sum at {x:.3f} of their bounds")
        assert x <= 1.0, f"row_ms {tag}: at x{x:.3f} of its bound"
        if not with_bias:
            continue
        dout = _dev(np.ascontiguousarray(v["dout"][:, :W]))
        args = (dout, out, agg, x_l, x_r, att, row_ms, g.prep, heads, concat, slope)
        got = ops.gatv2_aggregate_bwd(*args, bias=bias, relu=relu)
        again = ops.gatv2_aggregate_bwd(*args, bias=bias, relu=relu)
        bref = acc.gatv2_backward_reference(w, g.rs, g.cd, v["dout"], out[:n].cpu().numpy(), None if concat else agg[:n].cpu().numpy(),
                                            bias_np, relu, concat)
        for name, t, t2 in zip(("dx_l", "dx_r", "datt", "dbias"), got, again):
            rows = name in ("dx_l", "dx_r")
            live, live2 = (t[:n], t2[:n]) if rows else (t, t2)
            assert torch.equal(live, live2), f"{name} {tag}: two runs differ"
            assert bool(torch.isfinite(live).all()), f"{name} {tag}: non-finite outputs"
            lens = g.lens_s if name == "dx_l" else (g.lens if name == "dx_r" else None)
            acc.assert_attention_accuracy(live.cpu(), *bref[name], lens, f"{name} {tag}")
    _status(g)


@pytest.mark.parametrize("heads,c,concat,size", [s + (size,) for s in V2_SHAPES for size in ("small", "large")
                                                 if not (s[0] * s[1] == 1024 and size == "large")])
def test_gatv2_shapes(heads, c, concat, size):
    """Every head layout on `normal` data, negative_slope 0.2: the small graph with its hub cut to 700 entries and the large one
    (hubs of 5000 and 20000), GATv2 splitting rows above 64 entries on both; the graph or its transpose, alternating over the
    shapes.  F = 1024 on the small graph only (its fp64 reference takes seconds there, half a minute on the large one)."""
    ops = _ops()
    transpose = (V2_SHAPES.index((heads, c, concat)) + (size == "large")) % 2 == 1
    hub_cap = V2_HUB_CAP if size == "small" else None
    g = _graph(ops, size, transpose, hub_cap)
    _gatv2(ops, g, size, transpose, hub_cap, "normal", heads, c, concat, 0.2,
           f"v2 {size} T{int(transpose)} normal {heads}x{c}{'' if concat else 'm'} s=0.2")


@pytest.mark.parametrize("heads,c,concat", [(3, 7, False), (4, 16, True), (3, 20, True), (8, 32, True)])
@pytest.mark.parametrize("kind,slope", [("zeros", 0.2), ("striped", 0.2), ("normal", 0.0), ("striped", 0.0)])
def test_gatv2_kinds_and_slope(kind, slope, heads, c, concat):
    """The zeros and striped kinds and negative_slope = 0 (LeakyReLU's negative side exactly 0, its derivative 0) on the large
    graph's transpose and the small graph."""
    ops = _ops()
    for size, transpose, hub_cap in (("large", True, None), ("small", False, V2_HUB_CAP)):
        g = _graph(ops, size, transpose, hub_cap)
        _gatv2(ops, g, size, transpose, hub_cap, kind, heads, c, concat, slope,
               f"v2 {size} T{int(transpose)} {kind} {heads}x{c}{'' if concat else 'm'} s={slope}")
