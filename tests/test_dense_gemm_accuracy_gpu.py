"""Element-wise accuracy of the plain fp32 dense GEMM entry points of grapes_amd/csrc/gemm_kernels.hip against fp64
(oracle/accuracy.py, the dense section): grapes_linear_fwd, grapes_linear_fwd_row_scaled, grapes_linear_bias_act_fwd,
grapes_linear_bwd_input, grapes_linear_bwd_weight and the deferred slab path (grapes_linear_bwd_weight_slabs[_and_input] +
grapes_slab_reduce_sets), each through grapes_amd.ops.

Every output is judged relative to its own fp64 sum of |a||b| under two conditions (accuracy.dense_accuracy): the
project's factors RMS_FACTOR = 3 / MAX_FACTOR = 6 against a fixed-order fp32 baseline (one sequential chain in k order for the
forward forms and the input gradient, fp32_contract for the weight gradients), and the hard cap (L + 4) 2^-24 mag (L + 5 with a
row scale), which admits no exception.  Where mag == 0 the output must be exactly 0.

Every case: the output buffer is prefilled with a sentinel and carries two rows past the host count — rows past the DEVICE-side
count must keep it; operand rows past the live count are NaN; live outputs must be finite.  The shapes (accuracy.DENSE_CASES,
shared with tests/test_dense_gemm_accuracy_cpu.py) are the smallest that reach each branch, and DenseCase.check_route asserts
with Python mirrors of skinny_ok / dw_small_ok / vec / mt < 8 that each is on the intended side of every boundary; the kernel a
case reaches is the first part of its id and is named in each test's docstring.

Not here: the bf16x3 arm of grapes_linear_bias_act_fwd (n >= 2048 and wsplit_ok: tests/test_split_dw_accuracy_gpu.py), and
gemm_wstat_f32_k / gemm_wstat2_f32_k, which the product library cannot reach: wsplit_ok accepts every shape wstat_ok does, and
the switch that turns the bf16x3 kernel off (GRAPES_GEMM_SPLIT=0) is a diagnosis setting.

Measured on the MI355X, worst over an entry point's cases and kinds (max / rms ratio to the baseline; fraction of the hard cap):
  grapes_linear_fwd               1.30 / 1.32   0.32     (gemv_rows_k: 1029x8x1 mixed the max, 4x103x1 normal the rms)
  grapes_linear_fwd_row_scaled    1.00 / 1.00   0.21
  grapes_linear_bias_act_fwd      1.20 / 1.00   0.25
  grapes_linear_bwd_input         1.11 / 1.00   0.39
  grapes_linear_bwd_weight        1.07 / 1.00   0.28
  deferred slab path              1.00 / 0.99   0.21
No output exceeds a factor (no known-excess table), the hard cap holds everywhere, and no sentinel past a device-side count was
overwritten.  The module takes 5 s on the MI355X (83 tests; tests/test_spmm_accuracy_gpu.py 23 s, tests/test_tsplit_accuracy_gpu.py
30 s), so every shape runs on all three kinds."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
SEED = 20
_worst = {}


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a, off=False):
    """The array on the device; off: as a contiguous view 4 bytes past a 16-byte boundary (the kernels' scalar load paths)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _out(rows, cols, prior=None):
    """(whole buffer [rows + 2, cols], the [rows, cols] view handed to the entry point), sentinel-filled (or holding prior)."""
    buf = torch.full((rows + 2, cols), SENTINEL, device="cuda")
    if prior is not None:
        buf[:rows] = torch.from_numpy(prior).cuda()
    return buf, buf[:rows]


def _problem(c, kind):
    return acc.dense_problem(c.rows, c.f_in, c.f_out, kind, seed=SEED + c.rows + c.f_in, n_pad=c.pad)


def _d_n(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _judge(group, buf, live, ref5, what, emulate=None):
    """Sentinel past the live rows, finite live outputs, then both accuracy conditions on the live part.  On an excess over the
    factors the message carries the CPU emulation of the kernel's order on the same data (emulate: () -> tensor)."""
    ref, mag, base, L, extra = ref5
    host = buf.cpu()
    assert bool((host[live:] == SENTINEL).all()), f"{what}: rows past the device-side count were written"
    got = host[:live]
    assert bool(torch.isfinite(got).all()), f"{what}: a live output is not finite"
    got = got.reshape(ref.shape)
    a, cap = acc.dense_accuracy(got, ref, mag, base, L, extra)
    print(f"[cap] {what}: worst |err| / ((L + {extra}) u mag) = {cap:.3f}")
    print(f"[accuracy] {what}: {a}")
    w = _worst.setdefault(group, [0.0, 0.0, 0.0])
    w[:] = [max(w[0], a.max_ratio), max(w[1], a.rms_ratio), max(w[2], cap)]
    assert cap <= 1.0, f"{what}: an output exceeds the (L + {extra}) 2^-24 mag bound by x{cap:.3f}"
    if not a.ok():
        emu = ""
        if emulate is not None:
            e = emulate()
            if e is not None:
                emu = f"; CPU emulation of the kernel's order on the same data: {acc.Accuracy(e.reshape(ref.shape), ref, mag, base)}"
        raise AssertionError(f"{what}: {a}{emu}")


def _report(group):
    w = _worst.get(group)
    if w:
        print(f"[worst] {group}: max x{w[0]:.2f}, rms x{w[1]:.2f}, {w[2]:.3f} of the hard cap")


def _ids(group):
    return [pytest.param(c, id=c.id) for c in acc.DENSE_CASES[group]]


def _fwd_like(c, call, bias_relu=((False, False),)):
    ops = _ops()
    c.check_route()
    for kind in c.kinds:
        p = _problem(c, kind)
        n = p["n"]
        x, w = _dev(p["x"], c.unaligned == "x"), _dev(p["w"], c.unaligned == "w")
        d_n = _d_n(n)
        for bias, relu in bias_relu:
            buf, out = _out(c.cap, c.f_out)
            call(ops, p, x, w, d_n, out, bias, relu)
            ref5 = acc.dense_case_refs(c, p, bias, relu)["out"]
            _judge(c.entry, buf, n, ref5, f"{c.entry} {c.id} {kind}" + (f" bias={bias} relu={relu}" if c.entry == "bias_act" else ""),
                   lambda: acc.dense_case_emulation(c, p, bias, relu, fma=True)["out"])
    _report(c.entry)


# ------------------------------------------------------------------------------------------------- grapes_linear_fwd
@pytest.mark.parametrize("c", _ids("fwd"))
def test_linear_fwd(c):
    """grapes_linear_fwd.  gemv-*: gemv_rows_k (f_out = 1; f_in 260 takes a second trip of the float4 loop, the off_x view and
    f_in % 4 != 0 the scalar loop, 32773 rows the stride loop past the 8192 x 4-row grid).  skinny-*: gemm_skinny_f32_k<false>
    (host rows <= 4096, K <= 256; K 1 .. 5 and 13 leave quarters of the K split empty or ragged, 255 / 256 fill it; off_x / off_w
    take the scalar operand loads).  tiled-*: gemm_mfma_f32_k<false, false> (130x260x130 vector loads, 17 K-steps, mt = 2;
    129x1433x7 scalar loads, 90 K-steps; 1030x272x136 mt = 9, the XCD-aware block map with idle padded blocks; 4100 rows with
    K = 16 / 20 / 48 one, two (ragged) and three K-steps; 100 live rows in a capacity of 4200: dispatch follows the host count and
    most blocks return at m0 >= M)."""
    _fwd_like(c, lambda ops, p, x, w, d_n, out, bias, relu: ops.linear_fwd(x, w, d_n=d_n, out=out))


# -------------------------------------------------------------------------------------- grapes_linear_fwd_row_scaled
@pytest.mark.parametrize("c", _ids("fwd_row_scaled"))
def test_linear_fwd_row_scaled(c):
    """grapes_linear_fwd_row_scaled.  skinny-*: gemm_skinny_f32_k<false> + scale_rows_few_k; tiled-*: gemm_mfma_f32_k<false,
    false> with the out_scale epilogue.  The row scale mixes signs and magnitudes 10^[-6, 6]; the cap is (K + 5) 2^-24 mag."""
    _fwd_like(c, lambda ops, p, x, w, d_n, out, bias, relu: ops.linear_fwd_row_scaled(x, w, _dev(p["row_scale"]), d_n=d_n, out=out))


# ---------------------------------------------------------------------------------------- grapes_linear_bias_act_fwd
@pytest.mark.parametrize("c", _ids("bias_act"))
def test_linear_bias_act_fwd(c):
    """grapes_linear_bias_act_fwd, the arms this family owns, bias on/off x ReLU on/off.  skinny-*: gemm_skinny_f32_k<false> with
    its bias / ReLU epilogue (2047 rows: one below the bf16x3 kernel's threshold); tiled-*: gemm_mfma_f32_k<false, false> with
    GemmEx's (f_out = 72 is no multiple of 32, K = 260 is above 192: neither is a bf16x3 shape)."""
    _fwd_like(c, lambda ops, p, x, w, d_n, out, bias, relu: ops.linear_bias_act_fwd(x, w, _dev(p["bias"]) if bias else None, relu,
                                                                                   d_n=d_n, out=out),
              bias_relu=[(b, r) for b in (False, True) for r in (False, True)])


# ------------------------------------------------------------------------------------------- grapes_linear_bwd_input
@pytest.mark.parametrize("c", _ids("bwd_input"))
def test_linear_bwd_input(c):
    """grapes_linear_bwd_input, dx = dh w.  outer-*: outer_rows_k (f_out = 1; 8200 x 257 is past 8192 x 256 elements: the stride
    loop).  skinny-*: gemm_skinny_f32_k<true> (K = f_out; f_in % 4 == 0 loads the k-major B tile by float4, else by floats).
    tiled-*: gemm_mfma_f32_k<false, true> (4100x130x20 and 129x103x262 scalar loads, 130x100x260 vector loads)."""
    ops = _ops()
    c.check_route()
    for kind in c.kinds:
        p = _problem(c, kind)
        buf, out = _out(c.cap, c.f_in)
        ops.linear_bwd_input(_dev(p["dh_in"]), _dev(p["w_in"]), d_n=_d_n(p["n"]), out=out)
        _judge("bwd_input", buf, p["n"], acc.dense_case_refs(c, p)["dx"], f"bwd_input {c.id} {kind}",
               lambda: acc.dense_case_emulation(c, p, fma=True)["dx"])
    _report("bwd_input")


# ------------------------------------------------------------------------------------------ grapes_linear_bwd_weight
@pytest.mark.parametrize("c", _ids("bwd_weight"))
def test_linear_bwd_weight(c):
    """grapes_linear_bwd_weight, fresh and accumulated onto a prior of mixed sign (mag gains |prior|).  colsum-*: the weighted
    column sum behind f_out = 1.  dw_small-*: gemm_dw_small_k + slab_reduce_k (1 .. 32 slabs of 128 rows, the last one ragged or
    empty; tiles around 32 x 64).  split_k-*: gemm_mfma_f32_k<true, true> in split-K form + slab_reduce_k (4100x20x8 the chunk
    floor of 16: 257 live slabs of 512, reduce quarters of 65 / 65 / 65 / 62 in the 16-, 4- and 1-wide loops; 8200x20x8 chunks of
    18: a second K-step of 2 rows; 4097x260x130 six tiles, 85 slabs, scalar loads; 4100x103x7 scalar loads; 100 live rows in a
    capacity of 4200: 7 live slabs, the other blocks return)."""
    ops = _ops()
    c.check_route()
    for kind in c.kinds:
        p = _problem(c, kind)
        n = p["n"]
        dh, x, d_n = _dev(p["dh"]), _dev(p["x_dw"]), _d_n(n)
        for accumulate in (False, True):
            buf, dw = _out(c.f_out, c.f_in, p["prior_dw"] if accumulate else None)
            ops.linear_bwd_weight(dh, x, d_n=d_n, out=dw, accumulate=accumulate)
            _judge("bwd_weight", buf, c.f_out, acc.dense_case_refs(c, p, accumulate=accumulate)["dw"],
                   f"bwd_weight {c.id} {kind} acc={accumulate}",
                   lambda: (acc.dense_case_emulation(c, p, accumulate=accumulate, fma=True) or {"dw": None})["dw"])
    _report("bwd_weight")


# ------------------------------------------------------------------------------------------------ deferred slab path
def _slab_layer(ops, defer, form, p, d_n, accumulate, w_pair=None, own_dx=False):
    """Adds one layer to the DeferredSlabs; -> {output: (whole buffer, live rows, (ref, mag, base, L, extra), emulation)}"""
    n, fo, fi = p["n"], p["dh"].shape[1], p["x_dw"].shape[1]
    dh, x = _dev(p["dh"]), _dev(p["x_dw"])
    buf, dw = _out(fo, fi, p["prior_dw"] if accumulate else None)
    prior = p["prior_dw"] if accumulate else None
    res = {}
    gate = p["gate"] if form == "gated" else None
    if form == "dw":
        ops.linear_bwd_weight(dh, x, d_n=d_n, out=dw, accumulate=accumulate, defer=defer)
    elif form == "gated":
        bbuf, db = _out(1, fo, p["prior_db"][None] if accumulate else None)
        ops.linear_bwd_weight_gated(dh, x, gate=_dev(p["gate"]), d_n=d_n, dw=dw, dbias=db.view(-1), accumulate=accumulate, defer=defer)
        r = acc.dense_dw_reference(p["dh"][:n], p["x_dw"][:n], p["gate"][:n], prior, p["prior_db"] if accumulate else None)
        res["db"] = (bbuf, 1, r["db"] + (n, 4),
                     lambda: acc.emulate_dw_small(p["dh"], p["x_dw"], n, p["gate"], p["prior_db"] if accumulate else None, fma=True, want="db"))
    else:
        w = _dev(w_pair)
        if own_dx:          # the same launch through DeferredSlabs.try_add, so that dx is a sentinel-filled buffer of the test's
            xbuf, dx = _out(p["cap"], fi)
            assert defer.try_add(dh, None, x, d_n, dw, None, accumulate, w=w, dx=dx)
            live = n
        else:
            dx = ops.linear_bwd_weight_and_input(dh, x, w, d_n=d_n, out=dw, accumulate=accumulate, defer=defer)
            xbuf, live = torch.cat([dx[:n], torch.full((2, fi), SENTINEL, device="cuda")]), n
        res["dx"] = (xbuf, live, acc.dense_fwd_reference(p["dh"][:n], np.ascontiguousarray(w_pair.T)) + (fo, 4),
                     lambda: acc.emulate_skinny(p["dh"][:n], np.ascontiguousarray(w_pair.T), fma=True))
    assert any(s[2].data_ptr() == dw.data_ptr() for s in defer.sets), f"{form}: the layer did not take the deferred few-row path"
    r = acc.dense_dw_reference(p["dh"][:n], p["x_dw"][:n], gate[:n] if gate is not None else None, prior)
    res["dw"] = (buf, fo, r["dw"] + (n, 4), lambda: acc.emulate_dw_small(p["dh"], p["x_dw"], n, gate, prior, fma=True))
    return res


@pytest.mark.parametrize("rows", acc.SLAB_ROWS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_deferred_slabs_of_three_layers_in_one_reduction(rows, accumulate):
    """ops.DeferredSlabs over three layers of different shapes and one row count: a plain dW (gemm_dw_small_k), a gated dW with its
    dbias (the column sums ride along as an MFMA against ones) and a dW with its layer's dx in the pair launch
    (gemm_dw_small_dx_pair_k: gemm_dw_small_body beside gemm_skinny_body<true>); one flush() sums the four sets
    (slab_reduce_sets_k).  129 rows: two slabs, the second of one row; 1022 rows: eight slabs (capacity rows NaN)."""
    ops = _ops()
    pad = 3
    assert all(acc.dw_small_ok(rows + pad, fo, fi) for fi, fo, _ in acc.SLAB_LAYERS) and acc.skinny_ok(rows + pad, acc.SLAB_LAYERS[2][1])
    for kind in acc.KINDS:
        d_n = _d_n(rows)
        defer = ops.DeferredSlabs()
        outs = []
        for i, (fi, fo, form) in enumerate(acc.SLAB_LAYERS):
            p = acc.dense_problem(rows, fi, fo, kind, seed=SEED + rows + 10 * i, n_pad=pad)
            w_pair = acc.dense_problem(1, fi, fo, "normal", seed=SEED + i)["w"] if form == "pair" else None
            outs.append((form, _slab_layer(ops, defer, form, p, d_n, accumulate, w_pair, own_dx=accumulate)))
        assert len(defer.sets) == 4
        defer.flush()
        for form, res in outs:
            for name, (buf, live, ref5, emu) in res.items():
                _judge("slabs", buf, live, ref5, f"slabs n={rows} {form} {name} {kind} acc={accumulate}", emu)
    _report("slabs")


@pytest.mark.parametrize("accumulate", [False, True])
def test_deferred_slabs_past_eight_sets_flush_inside(accumulate):
    """Nine plain dW layers over the same rows: the ninth try_add finds eight sets waiting and flushes them itself
    (slab_reduce_sets_k with all SR_MAX_SETS sets), the caller's flush() sums the last one."""
    ops = _ops()
    rows, fi, fo, layers = acc.SLAB_MANY
    kinds = [acc.KINDS[i % 3] for i in range(layers)]
    d_n = _d_n(rows)
    defer = ops.DeferredSlabs()
    outs = []
    for i in range(layers):
        p = acc.dense_problem(rows, fi, fo, kinds[i], seed=SEED + 100 + i, n_pad=3)
        outs.append((i, _slab_layer(ops, defer, "dw", p, d_n, accumulate)))
        assert len(defer.sets) == (i % 8) + 1
    defer.flush()
    for i, res in outs:
        buf, live, ref5, emu = res["dw"]
        _judge("slabs", buf, live, ref5, f"slabs n={rows} set {i} of {layers} {kinds[i]} acc={accumulate}", emu)
    _report("slabs")
