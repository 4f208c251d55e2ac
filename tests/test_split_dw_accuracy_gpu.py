"""Element-wise accuracy of the split-bf16 weight-gradient GEMM of the sampler nets (gemm_dw_split_k + slab_reduce_rank1_k)
and of the forward GEMM with the fused 1-wide head, against fp64 (oracle/accuracy.py).  Each output is measured relative to
its own sum |a||b|, and the max and rms of that error must stay within RMS_FACTOR / MAX_FACTOR of a fixed-order fp32 sum's on the
same fp32 operands.  The mask is always the device's own (its gate words decoded, or its activations > 0), so a ReLU that
flips between fp32 and fp64 cannot enter the comparison.  tests/test_accuracy_criterion_cpu.py shows the criterion rejects a
lost or misplaced third bf16 plane, which the norm-wise bounds of the older tests let through."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from oracle import accuracy as acc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def decode_bits(words: torch.Tensor, n: int, H: int) -> np.ndarray:
    """[n, H] bool from gate words: bit 16 h + 4 q + u of word [r][c // 32] is column 32 (c // 32) + 8 q + 4 h + u."""
    w = words[:n].cpu().numpy().astype(np.uint32)
    c = np.arange(H)
    shift = (16 * ((c % 8) // 4) + 4 * ((c % 32) // 8) + c % 4).astype(np.uint32)
    return ((w[:, c // 32] >> shift) & 1).astype(bool)


# Outputs measured above the criterion on the MI355X (the calls' other outputs pass).  Each is held to the criterion only by
# test_known_excesses_over_the_fp32_criterion (strict xfail: it starts to fail once an output comes within the factors).
#  - db1 over several row sets, one of them with mixed magnitudes: rms 3.4x - 4.3x, max 3.3x - 5.6x (and dW2 = <S, w1> + b1 T,
#    which carries T: rms 3.2x in one of the cases).  The CPU emulation of
#    the split arithmetic (tests/test_accuracy_criterion_cpu.py: emulate_split_dw; the three planes of rs added one after the
#    other into one fp32 accumulator) gives 3.6x on the same data, and the fp32 kernel of the activation form at H = 96 (not
#    the split one) shows it as well (3.5x): a property of summing these magnitudes in those orders, not a lost plane.
#  - dW2 of the gate-word form on the 160-column kernel at 37,000 rows of mixed magnitudes: rms 4.2x, max 4.3x, where the CPU
#    emulation of the split gives 1.2x (dW1 and db1 of the same call: within 1x).  Not explained yet.
KNOWN_EXCESS = {"bits multi (137, 2, 5000)": ("db", "dwh"), "bits multi (1, 2, 3, 4000)": ("db",),
                "gated multi n=2500,833 K=64": ("db",), "bits n=37000 K=132": ("dwh",)}
_enforce_known = [False]


def _check(outs, refs, what, names=("dw", "db", "dwh")):
    known = next((v for key, v in KNOWN_EXCESS.items() if what.startswith(key)), ())
    res = {}
    for k in names:
        if k in refs:
            if k in known and not _enforce_known[0]:
                res[k] = acc.Accuracy(outs[k].cpu(), *refs[k])
                print(f"[accuracy, known excess] {what} {k}: {res[k]}")
            else:
                res[k] = acc.assert_fp32_accuracy(outs[k].cpu(), *refs[k], what=f"{what} {k}")
    return res


def _prev(H, K, rng):
    return {"dw": rng.standard_normal((H, K)).astype(np.float32), "db": rng.standard_normal(H).astype(np.float32),
            "dwh": rng.standard_normal(H).astype(np.float32)}


def _bits_segment(ops, n, K, H, kind, seed, layer=None):
    """A row set with NaN rows beyond its live count n (a capacity of at least 2048 rows, where the split kernels apply), and
    the device's gate words of the layer over it."""
    p = acc.layer_problem(n, K, H, kind, seed, n_pad=max(19, 2048 + 19 - n))
    if layer is not None:
        p.update({k: layer[k] for k in ("w", "b", "w2")})
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    x = _dev(p["x"])
    bits, _ = ops.linear_relu_head_fwd_bits(x, _dev(p["w"]), _dev(p["b"]), _dev(p["w2"]).view(1, -1), d_n=d_n)
    mask = decode_bits(bits.words, n, H)
    return p, x, bits, d_n, mask


# ------------------------------------------------------------------------------------------------ gate-word forms
@pytest.mark.parametrize("n,K,H,kind", [(37500, 104, 256, "normal"), (5000, 100, 256, "mixed"), (2500, 64, 96, "zeros"),
                                        (37000, 132, 256, "mixed"), (5000, 128, 256, "zeros"), (3000, 144, 128, "normal"),
                                        # one workgroup (100 rows < DS_MINROWS; a ragged 4-row last chunk), three (300 rows)
                                        (100, 104, 256, "mixed"), (300, 64, 96, "normal"), (150, 132, 256, "normal"),
                                        # the parameter's own layout: K = 101 / 131 in 4-padded operands
                                        (9000, 101, 256, "mixed"), (9000, 131, 256, "normal")])
def test_gate_bit_dw_is_elementwise_as_accurate_as_fp32(n, K, H, kind):
    """linear_bwd_weight_bits_multi, one row set: dW1 (= cv ⊙ S, magnitude |w2| ⊗ maskᵀ|rs x|), db1 and the head's dW2
    (<S, w1> + b1 T) each element-wise against fp64, overwriting and accumulating onto non-zero buffers; rows beyond the live
    count are NaN; the dead unit's dW1 row and db1 entry are exactly 0; in the padded layout the pad columns are exactly 0.
    Measured on the MI355X, worst case over these shapes (max / rms ratio to the fp32 baseline): dW1 1.00 / 1.00,
    db1 1.24 / 1.32, dW2 1.49 / 1.68 — the KNOWN_EXCESS output (dW2 at 37,000 rows on the 160-column kernel) aside."""
    ops = _ops()
    Kp = (K + 3) // 4 * 4
    p, x, bits, d_n, mask = _bits_segment(ops, n, K, H, kind, seed=n + K)
    assert not mask[:, acc.DEAD_UNIT].any() and mask[:, acc.ONE_ROW_UNIT].sum() == 1
    w, b, cv = _dev(p["w"]), _dev(p["b"]), _dev(p["w2"])
    rs = _dev(p["rs"])
    rng = np.random.default_rng(n)
    layouts = (Kp, K) if K != Kp else (K,)
    for cols in layouts:
        for accumulate in (False, True):
            prev = _prev(H, cols, rng)
            dw = _dev(prev["dw"]) if accumulate else torch.full((H, cols), 7.0, device="cuda")
            db = _dev(prev["db"]) if accumulate else torch.full((H,), 7.0, device="cuda")
            dwh = _dev(prev["dwh"]) if accumulate else torch.full((H,), 7.0, device="cuda")
            ops.linear_bwd_weight_bits_multi([bits], [x], [rs], [d_n], cv, w, b, dw, dbias=db, dw_head=dwh, accumulate=accumulate)
            refs = acc.dw_reference([(mask, p["x"][:n, :cols], p["rs"][:n])], p["w2"], p["w"], p["b"],
                                    prev=prev if accumulate else None)
            _check({"dw": dw, "db": db, "dwh": dwh}, refs, f"bits n={n} K={K} cols={cols} acc={accumulate}")
            if not accumulate:
                assert float(dw[acc.DEAD_UNIT].abs().max()) == 0.0 and float(db[acc.DEAD_UNIT]) == 0.0
                if cols > K:
                    assert float(dw[:, K:].abs().max()) == 0.0


@pytest.mark.parametrize("K,H,counts", [(104, 256, (3000, 77, 0, 1500)), (104, 256, (137, 2, 5000)), (64, 96, (0, 4100)),
                                        (132, 256, (20000, 0, 333, 129)), (100, 256, (0, 0)), (144, 128, (1, 2, 3, 4000))])
def test_gate_bit_dw_over_several_row_sets_is_elementwise_as_accurate_as_fp32(K, H, counts):
    """linear_bwd_weight_bits_multi with 1-4 row sets sharing the weights: segment boundaries inside one workgroup's share,
    a row set with no live rows, all row sets empty (every output exactly 0), rows beyond each live count NaN.  Measured
    (max / rms ratio to the fp32 baseline): dW1 1.61 / 1.85, db1 3.96 / 1.19, dW2 3.21 / 2.49 — the KNOWN_EXCESS outputs
    aside."""
    ops = _ops()
    layer = acc.layer_problem(1, K, H, "normal", seed=K + H)
    segs = [_bits_segment(ops, c, K, H, ("normal", "mixed", "zeros")[i % 3], seed=1000 * i + c + K, layer=layer)
            for i, c in enumerate(counts)]
    w, b, cv = _dev(layer["w"]), _dev(layer["b"]), _dev(layer["w2"])
    dw = torch.full((H, K), 5.0, device="cuda"); db = torch.full((H,), 5.0, device="cuda"); dwh = torch.full((H,), 5.0, device="cuda")
    ops.linear_bwd_weight_bits_multi([s[2] for s in segs], [s[1] for s in segs], [_dev(s[0]["rs"]) for s in segs],
                                     [s[3] for s in segs], cv, w, b, dw, dbias=db, dw_head=dwh)
    refs = acc.dw_reference([(s[4], s[0]["x"][:c, :K], s[0]["rs"][:c]) for s, c in zip(segs, counts)], layer["w2"], layer["w"],
                            layer["b"])
    _check({"dw": dw, "db": db, "dwh": dwh}, refs, f"bits multi {counts}")
    if sum(counts) == 0:
        assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0 and float(dwh.abs().max()) == 0.0


@pytest.mark.parametrize("K,Kb,H,counts,nb", [(104, 100, 256, (9000, 3100), 9000), (132, 128, 256, (20000,), 20000),
                                              (64, 64, 96, (700,), 650)])
def test_gate_bit_dw_pair_launch_is_elementwise_as_accurate_as_fp32(K, Kb, H, counts, nb):
    """linear_bwd_weight_bits_pair: layer a over 1-2 row sets and layer b (its own weights, over the leading Kb columns of
    layer a's first row set) in one launch; both problems' dW1, db1 and dW2 element-wise, accumulating onto non-zero buffers.
    Measured (max / rms ratio to the fp32 baseline): dW1 1.28 / 1.07, db1 1.00 / 1.02, dW2 1.88 / 2.50."""
    ops = _ops()
    la = acc.layer_problem(1, K, H, "normal", seed=K)
    lb = acc.layer_problem(1, Kb, H, "normal", seed=Kb + 1)
    segs = [_bits_segment(ops, c, K, H, ("mixed", "normal")[i % 2], seed=c + i, layer=la) for i, c in enumerate(counts)]
    x0 = segs[0][1]
    xb = x0[:, :Kb]
    d_nb = torch.tensor([nb], dtype=torch.int32, device="cuda")
    bits_b, _ = ops.linear_relu_head_fwd_bits(xb, _dev(lb["w"]), _dev(lb["b"]), _dev(lb["w2"]).view(1, -1), d_n=d_nb)
    mask_b = decode_bits(bits_b.words, nb, H)
    rsb = np.random.default_rng(nb).standard_normal(x0.shape[0]).astype(np.float32)
    rng = np.random.default_rng(K + Kb)
    pa, pb = _prev(H, K, rng), _prev(H, Kb, rng)
    oa = {k: _dev(v) for k, v in pa.items()}; ob = {k: _dev(v) for k, v in pb.items()}
    ops.linear_bwd_weight_bits_pair([s[2] for s in segs], [s[1] for s in segs], [_dev(s[0]["rs"]) for s in segs], [s[3] for s in segs],
                                    _dev(la["w2"]), _dev(la["w"]), _dev(la["b"]), oa["dw"], oa["db"], oa["dwh"],
                                    bits_b, xb, _dev(rsb), d_nb, _dev(lb["w2"]), _dev(lb["w"]), _dev(lb["b"]), ob["dw"], ob["db"], ob["dwh"],
                                    accumulate=True)
    ra = acc.dw_reference([(s[4], s[0]["x"][:c, :K], s[0]["rs"][:c]) for s, c in zip(segs, counts)], la["w2"], la["w"], la["b"], prev=pa)
    rb = acc.dw_reference([(mask_b, segs[0][0]["x"][:nb, :Kb], rsb[:nb])], lb["w2"], lb["w"], lb["b"], prev=pb)
    _check(oa, ra, f"pair a {counts}")
    _check(ob, rb, f"pair b {nb}")


# ------------------------------------------------------------------------------------------------ activation forms
def _act_problem(ops, n, K, H, kind, seed):
    p = acc.layer_problem(n, K, H, kind, seed, n_pad=max(29, 2048 + 29 - n))
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    x = _dev(p["x"])
    act = ops.linear_bias_act_fwd(x, _dev(p["w"]), _dev(p["b"]), True, d_n=d_n)
    act[n:] = float("nan")
    return p, x, act, d_n, act[:n].cpu().numpy()


@pytest.mark.parametrize("n,K,H,kind", [(37500, 104, 256, "normal"), (5000, 100, 256, "mixed"), (2500, 64, 96, "zeros"),
                                        (100, 104, 256, "normal"), (4099, 100, 256, "zeros")])
def test_activation_form_dw_is_elementwise_as_accurate_as_fp32(n, K, H, kind):
    """linear_bwd_weight_gated in rank-1 mode (gate = the device's activations; gemm_dw_split_k<false>), its strided form over the
    leading K columns of a wider matrix, and linear_bwd_weight_gated_multi over two row sets: dW1, db1 and dW2 = rsᵀ act
    element-wise against fp64, accumulating onto non-zero buffers.  Measured (max / rms ratio to the fp32 baseline):
    dW1 1.51 / 1.39, db1 1.29 / 1.47, dW2 1.58 / 1.73 — the KNOWN_EXCESS output (db1 of the two-set call at H = 96) aside."""
    ops = _ops()
    p, x, act, d_n, act_np = _act_problem(ops, n, K, H, kind, seed=n + K + 1)
    mask = act_np > 0
    rs, cv = _dev(p["rs"]), _dev(p["w2"])
    rng = np.random.default_rng(n + 7)
    prev = _prev(H, K, rng)
    xs = x[:, :K].contiguous()
    ref = acc.dw_reference([(mask, p["x"][:n, :K], p["rs"][:n])], p["w2"], prev=prev)
    ref["dwh"] = acc.head_reference([(act_np, p["rs"][:n])], prev=prev["dwh"])
    o = {k: _dev(v) for k, v in prev.items()}
    ops.linear_bwd_weight_gated(None, xs, gate=act, d_n=d_n, dw=o["dw"], dbias=o["db"], accumulate=True, row_scale=rs, col_vec=cv,
                                dw_head=o["dwh"])
    _check(o, ref, f"gated n={n} K={K}")
    wide = torch.full((x.shape[0], K + 4), float("nan"), device="cuda"); wide[:, :K] = xs
    o = {k: _dev(v) for k, v in prev.items()}
    assert ops.split_gemm_available(x.shape[0], K, H)
    ops.linear_bwd_weight_gated_strided(wide[:, :K], act, rs, cv, o["dw"], dbias=o["db"], dw_head=o["dwh"], d_n=d_n, accumulate=True)
    _check(o, ref, f"gated strided n={n} K={K}")
    # two row sets (the second: its own rows and a row count below its capacity)
    n2 = max(1, n // 3)
    p2, x2, act2, d_n2, act2_np = _act_problem(ops, n2, K, H, "mixed", seed=n2 + 3)
    o = {k: _dev(v) for k, v in prev.items()}
    ops.linear_bwd_weight_gated_multi([act, act2], [xs, x2[:, :K].contiguous()], [rs, _dev(p2["rs"])], [d_n, d_n2], cv, o["dw"],
                                      dbias=o["db"], dw_head=o["dwh"], accumulate=True)
    ref2 = acc.dw_reference([(mask, p["x"][:n, :K], p["rs"][:n]), (act2_np > 0, p2["x"][:n2, :K], p2["rs"][:n2])], p["w2"], prev=prev)
    ref2["dwh"] = acc.head_reference([(act_np, p["rs"][:n]), (act2_np, p2["rs"][:n2])], prev=prev["dwh"])
    _check(o, ref2, f"gated multi n={n},{n2} K={K}")


_DW_AB_CASES = ((37500, 104, 256, "normal"), (5000, 100, 256, "mixed"), (2500, 64, 256, "zeros"))
_CHILD = textwrap.dedent("""
    import os, sys, numpy as np, torch
    sys.path.insert(0, os.getcwd())
    from grapes_amd import ops
    from oracle import accuracy as acc
    acts = torch.load(sys.argv[1])
    res = {}
    for (n, K, H, kind), act in acts.items():
        p = acc.layer_problem(n, K, H, kind, seed=n + K + 2)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        x = t(p["x"][:, :K]); d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        dw = torch.empty(H, K, device="cuda"); db = torch.empty(H, device="cuda"); dh = torch.empty(H, device="cuda")
        ops.linear_bwd_weight_gated(None, x, gate=act.cuda(), d_n=d_n, dw=dw, dbias=db, row_scale=t(p["rs"]), col_vec=t(p["w2"]),
                                    dw_head=dh)
        res[(n, K, H, kind)] = {"dw": dw.cpu(), "db": db.cpu(), "dwh": dh.cpu()}
    torch.save(res, sys.argv[2])
""")


def test_split_dw_is_as_accurate_as_the_fp32_mfma_dw_kernel(tmp_path):
    """The activation form on both of its kernels (GRAPES_GEMM_SPLIT, a switch of the diagnostic build read once per process,
    hence child processes): gemm_dw_split_k<false> and the fp32-MFMA gemm_dw_rank1_k on the same data and the same gate (this
    process's activations, handed to both), each against fp64.  The split kernel's element-wise max and rms stay within a small
    factor of the fp32 kernel's (both share the slab sums).  Measured, split / fp32-MFMA kernel: dW1 max 1.50 / rms 1.48,
    db1 1.00 / 1.36, dW2 0.97 / 1.06; against the fp32 baseline the split kernel stays within 1.18 / 1.42."""
    ops = _ops()
    acts = {}
    for n, K, H, kind in _DW_AB_CASES:
        p = acc.layer_problem(n, K, H, kind, seed=n + K + 2)
        d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        acts[(n, K, H, kind)] = ops.linear_bias_act_fwd(_dev(p["x"]), _dev(p["w"]), _dev(p["b"]), True, d_n=d_n).cpu()
    torch.save(acts, str(tmp_path / "acts.pt"))
    out = {}
    for flag in ("1", "0"):
        path = str(tmp_path / f"dw{flag}.pt")
        env = dict(os.environ, GRAPES_GEMM_SPLIT=flag, GRAPES_DIAG="1")
        r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "acts.pt"), path], env=env, capture_output=True, text=True,
                           timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        out[flag] = torch.load(path)
    for key, s in out["1"].items():
        f = out["0"][key]
        n, K, H, kind = key
        p = acc.layer_problem(n, K, H, kind, seed=n + K + 2)
        act = acts[key][:n].numpy()
        ref = acc.dw_reference([(act > 0, p["x"][:n, :K], p["rs"][:n])], p["w2"])
        ref["dwh"] = acc.head_reference([(act, p["rs"][:n])])
        for k in ("dw", "db", "dwh"):
            a_s = acc.assert_fp32_accuracy(s[k], *ref[k], what=f"split {key} {k}")
            a_f = acc.assert_fp32_accuracy(f[k], *ref[k], what=f"fp32-MFMA {key} {k}")
            print(f"[split vs fp32-MFMA dW] {key} {k}: max x{a_s.max / max(a_f.max, acc.FLOOR):.2f}, rms x{a_s.rms / max(a_f.rms, acc.FLOOR):.2f}")
            # Both kernels share the row shares and the slab sums and accumulate in fp32; they differ only in the steps inside a
            # workgroup (16-row bf16 MFMAs of three planes against 2-row fp32 MFMAs).  Another order of fp32 additions moves the
            # rms by well under 2x and a single output (the max) by under 3x; a lost third plane moves the rms 15x - 90x
            # (tests/test_accuracy_criterion_cpu.py).
            assert a_s.rms <= 2.0 * a_f.rms + acc.FLOOR and a_s.max <= 3.0 * a_f.max + acc.FLOOR, (key, k, a_s, a_f.max, a_f.rms)
        assert not torch.equal(s["dw"], f["dw"])          # really two kernels


# ------------------------------------------------------------------------------------------------ domain edges
@pytest.mark.parametrize("form", ["bits", "act"])
def test_split_dw_domain_edges(form):
    """The two edges of the split's range (include/grapes_hip.h, beside the split entry points), on both sides of each.
    Large: an rs * x of 3.39e38 still splits (bf16 of it is finite, 3.3895e38) and dW1 meets the criterion; at 3.40e38 the
    bf16 conversion rounds to inf, the lower planes become -inf and NaN, and that output COLUMN of dW1 is NaN for every unit
    (a 0 of the mask times inf is NaN as well) — with the gate-word form's dW2, which is derived from it; db1 and the other
    columns keep the criterion.  Small: rows at 1e-28 meet the criterion; at 1e-35 the planes hold rs * x only to bf16's
    smallest subnormal step (2^-133, rounded to nearest: an error of at most 2^-134 per product) — no longer to 24 bits.  On
    both sides every output is within that resolution (within_split_resolution), as the CPU emulation of the split is on the
    same data (test_accuracy_criterion_cpu.py: test_split_holds_tiny_products_only_to_the_bf16_subnormal_step).  Measured at
    1e-35: max 1.6e-4 / rms 2.0e-6 of |w2| maskᵀ|rs x|."""
    ops = _ops()
    n, K, H = 3000, 104, 256
    p = acc.layer_problem(n, K, H, "normal", seed=77)
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    w, b, cv = _dev(p["w"]), _dev(p["b"]), _dev(p["w2"])
    x_clean = _dev(p["x"])
    if form == "bits":
        bits, _ = ops.linear_relu_head_fwd_bits(x_clean, w, b, cv.view(1, -1), d_n=d_n)
        mask = decode_bits(bits.words, n, H)
    else:
        act = ops.linear_bias_act_fwd(x_clean, w, b, True, d_n=d_n)
        mask = act.cpu().numpy() > 0

    def run(x_np, rs_np):
        o = {k: torch.full(s, 9.0, device="cuda") for k, s in (("dw", (H, K)), ("db", (H,)), ("dwh", (H,)))}
        if form == "bits":
            ops.linear_bwd_weight_bits_multi([bits], [_dev(x_np)], [_dev(rs_np)], [d_n], cv, w, b, o["dw"], dbias=o["db"], dw_head=o["dwh"])
        else:
            ops.linear_bwd_weight_gated(None, _dev(x_np), gate=act, d_n=d_n, dw=o["dw"], dbias=o["db"], row_scale=_dev(rs_np),
                                        col_vec=cv, dw_head=o["dwh"])
        return {k: v.cpu() for k, v in o.items()}

    rs = acc.domain_edge_row_scale(n)
    r0, c0 = 5, 7
    names = ("dw", "db", "dwh") if form == "bits" else ("dw", "db")
    for big, finite in ((3.39e38, True), (3.40e38, False)):
        x = (p["x"] * 1e-3).astype(np.float32); x[r0, c0] = big
        o = run(x, rs)
        ref = acc.dw_reference([(mask, x, rs)], p["w2"], p["w"] if form == "bits" else None, p["b"])
        assert bool(torch.isfinite(ref["dw"][0]).all())
        if finite:
            _check(o, ref, f"{form} {big}", names=names)
        else:
            assert bool(torch.isnan(o["dw"][:, c0]).all())
            others = [c for c in range(K) if c != c0]
            acc.assert_fp32_accuracy(o["dw"][:, others], *(t[:, others] for t in ref["dw"]), what=f"{form} {big} other columns")
            acc.assert_fp32_accuracy(o["db"], *ref["db"], what=f"{form} {big} db")
            if form == "bits":
                assert bool(torch.isnan(o["dwh"]).all())
    for scale, inside in ((1e-28, True), (1e-35, False)):
        x = (p["x"] * scale).astype(np.float32)
        o = run(x, rs)
        ref = acc.dw_reference([(mask, x, rs)], p["w2"])
        a = acc.Accuracy(o["dw"], *ref["dw"])
        print(f"[domain edge {scale}] {form}: {a}")
        assert a.ok() == inside, a
        assert acc.within_split_resolution(o["dw"], ref["dw"], mask, p["w2"])        # on both sides: 2^-134 per product


# ------------------------------------------------------------------------------------------------ fused-head forward
@pytest.mark.parametrize("n,cap,K,N,kind", [(37501, 37600, 104, 256, "normal"), (5000, 5000, 100, 256, "mixed"),
                                            (2100, 4100, 64, 96, "zeros"), (700, 800, 104, 256, "normal"),
                                            (20, 3000, 104, 256, "normal"), (64, 2048, 8, 32, "mixed"),
                                            (3000, 3000, 144, 128, "normal"), (9000, 9000, 132, 256, "mixed")])
def test_fused_head_forward_is_elementwise_as_accurate_as_fp32(n, cap, K, N, kind):
    """linear_bias_act_head_fwd[_strided] and linear_relu_head_fwd_bits[_pair]: head against the fp64 act · w2 of the device's
    own activations (magnitude |act| · |w2|, baseline a fixed-order fp32 sum of the same act), and every activation / gate bit
    against the sign of the fp64 pre-activation wherever |z64| > 4u (|x| |w|ᵀ + |b|) (u = 2^-24).  Rows beyond the live
    count are NaN.  Measured head (max / rms ratio to the fp32 baseline): 0.61 / 1.00 at worst, every form."""
    ops = _ops()
    p = acc.layer_problem(n, K, N, kind, seed=n + N + 5, n_pad=cap - n)
    x, w, b, w2 = _dev(p["x"]), _dev(p["w"]), _dev(p["b"]), _dev(p["w2"]).view(1, -1)
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    x64, w64, b64 = (torch.from_numpy(p[k]).double() for k in ("x", "w", "b"))
    z64 = x64[:n] @ w64.T + b64
    sure = z64.abs() > 4 * 2.0 ** -24 * (x64[:n].abs() @ w64.abs().T + b64.abs())
    want = (z64 > 0)[sure]
    act, head = ops.linear_bias_act_head_fwd(x, w, b, True, w2, d_n=d_n)
    act_np = act[:n].cpu().numpy()
    assert torch.equal(torch.from_numpy(act_np > 0)[sure], want)
    ref = acc.matmul_reference(act_np, p["w2"][:, None])
    acc.assert_fp32_accuracy(head[:n].cpu(), *ref, what="head")
    Kp = x.shape[1]
    if ops.split_gemm_available(cap, Kp, N):
        wide = torch.full((cap, Kp + 4), float("nan"), device="cuda"); wide[:, :Kp] = x
        act_s, head_s = ops.linear_bias_act_head_fwd_strided(wide[:, :Kp], w, b, True, w2, d_n=d_n)
        assert torch.equal(act_s[:n], act[:n])
        acc.assert_fp32_accuracy(head_s[:n].cpu(), *ref, what="strided head")
        bits, head_b = ops.linear_relu_head_fwd_bits(x, w, b, w2, d_n=d_n)
        assert torch.equal(torch.from_numpy(decode_bits(bits.words, n, N)), torch.from_numpy(act_np > 0))
        acc.assert_fp32_accuracy(head_b[:n].cpu(), *ref, what="gate-word head")
        # the pair launch: a second layer over the leading Kp - 4 columns of the same rows
        Kb = Kp - 4
        lb = acc.layer_problem(1, Kb, N, "normal", seed=Kb + 9)
        r = ops.linear_relu_head_fwd_bits_pair(x, w, b, w2, x[:, :Kb], _dev(lb["w"]), _dev(lb["b"]), _dev(lb["w2"]).view(1, -1),
                                               d_n=d_n) if Kb >= 4 else None
        if r is not None:
            assert torch.equal(r[0].words[:n], bits.words[:n])
            acc.assert_fp32_accuracy(r[1][:n].cpu(), *ref, what="pair head a")
            act_b = ops.linear_bias_act_fwd(x[:, :Kb].contiguous(), _dev(lb["w"]), _dev(lb["b"]), True, d_n=d_n)[:n].cpu().numpy()
            assert np.array_equal(decode_bits(r[2].words, n, N), act_b > 0)
            acc.assert_fp32_accuracy(r[3][:n].cpu(), *acc.matmul_reference(act_b, lb["w2"][:, None]), what="pair head b")


@pytest.mark.xfail(strict=True, reason="KNOWN_EXCESS: these outputs exceed the fp32 criterion (see the note at KNOWN_EXCESS)")
@pytest.mark.parametrize("case", ["multi-137", "multi-4000", "gated-multi-96", "bits-37000-wide"])
def test_known_excesses_over_the_fp32_criterion(case):
    """The KNOWN_EXCESS outputs held to the criterion: each case reruns its test with them enforced."""
    _enforce_known[0] = True
    try:
        if case == "multi-137":
            test_gate_bit_dw_over_several_row_sets_is_elementwise_as_accurate_as_fp32(104, 256, (137, 2, 5000))
        elif case == "multi-4000":
            test_gate_bit_dw_over_several_row_sets_is_elementwise_as_accurate_as_fp32(144, 128, (1, 2, 3, 4000))
        elif case == "gated-multi-96":
            test_activation_form_dw_is_elementwise_as_accurate_as_fp32(2500, 64, 96, "zeros")
        else:
            test_gate_bit_dw_is_elementwise_as_accurate_as_fp32(37000, 132, 256, "mixed")
    finally:
        _enforce_known[0] = False
