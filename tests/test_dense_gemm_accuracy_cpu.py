"""The element-wise criterion of oracle/accuracy.py on the plain fp32 dense GEMMs of grapes_amd/csrc/gemm_kernels.hip
(grapes_linear_fwd, _fwd_row_scaled, _bias_act_fwd, _bwd_input, _bwd_weight and the deferred slab path), shown on the CPU on the
very problems and shape table tests/test_dense_gemm_accuracy_gpu.py runs the kernels on (accuracy.DENSE_CASES, dense_problem).

Faithful emulations of the kernels' summation orders — the tiled kernel's one chain over k, the skinny kernel's four k ranges
combined ((q0 + q1) + q2) + q3, gemv_rows_k's lane chains and butterfly, the few-row weight gradient's 128-row slabs in the skinny
order, the split-K chunks of auto_kchunk, and the slab reduction's four contiguous quarters combined (p0 + p1) + (p2 + p3) — stay
inside RMS_FACTOR = 3 / MAX_FACTOR = 6 of the baseline and under the hard cap (L + 4) 2^-24 mag on every (shape, kind), with
separately rounded products and with fused multiply-adds.  That is the evidence that the inputs leave a correct kernel inside
the factors: worst over the table max x1.30 / rms x1.32 (gemv_rows_k's lane chains and butterfly on 8- and 103-term rows), every other group <= x1.20 /
x1.00, and at most 0.39 of the hard cap.

Each seeded defect (DEFECTS) is rejected by at least one of the two conditions, on every kind.

On N(0,1) data the norm-wise bound of tests/test_hip_parity.py (max|got - ref| <= 2e-5 max(1, max|ref|)) rejects the
dropped-slab and shifted-row-scale defects too: a lost 128-row slab moves every output by about sqrt(128), a row scale taken from
the neighbouring row rescales whole rows by up to 10^12, both far above 2e-5 max|ref|
(test_normwise_bound_on_the_same_defects asserts exactly that).  What the norm-wise bound cannot see is what VERDICT.md names: an
error of 1e-4 of a small output that stands beside a large one."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc

ALL_CASES = [c for cases in acc.DENSE_CASES.values() for c in cases]
BY_ID = {f"{c.entry}:{c.id}": c for c in ALL_CASES}
SEED = 20


def _problem(c, kind):
    return acc.dense_problem(c.rows, c.f_in, c.f_out, kind, seed=SEED + c.rows + c.f_in, n_pad=c.pad)


def test_every_shape_is_on_the_intended_side_of_its_dispatch_boundaries():
    ids = list(BY_ID)
    assert len(set(ids)) == len(ALL_CASES)
    for c in ALL_CASES:
        c.check_route()
    assert acc.skinny_ok(4096, 256) and not acc.skinny_ok(4097, 256) and not acc.skinny_ok(4096, 257) and not acc.skinny_ok(1, 0)
    assert acc.dw_nslab(8, 20) == 512 and acc.dw_nslab(130, 260) == 85 and acc.dw_nslab(256, 256) == 128
    assert acc.auto_kchunk(4100, 512) == 16 and acc.auto_kchunk(8200, 512) == 18 and acc.auto_kchunk(4097, 85) == 50
    assert -(-4100 // 16) == 257          # live slabs of (4100, 20, 8): quarters of 65 / 65 / 65 / 62
    assert acc.skinny_quarters(47) == [(0, 12), (12, 24), (24, 36), (36, 47)] and acc.skinny_quarters(5)[1:] == [(4, 5), (5, 5), (5, 5)]


@pytest.mark.parametrize("group", list(acc.DENSE_CASES))
def test_faithful_orders_pass_both_conditions_on_every_shape_and_kind(group):
    worst = [0.0, 0.0, 0.0]
    for c in acc.DENSE_CASES[group]:
        for kind in c.kinds:
            p = _problem(c, kind)
            for accumulate in ((False, True) if c.entry == "bwd_weight" else (False,)):
                opts = [(False, False)] if c.entry != "bias_act" else [(b, r) for b in (False, True) for r in (False, True)]
                for bias, relu in opts:
                    refs = acc.dense_case_refs(c, p, bias, relu, accumulate)
                    for fma in (False, True):
                        emu = acc.dense_case_emulation(c, p, bias, relu, accumulate, fma=fma)
                        if emu is None:
                            continue
                        for k, (ref, mag, base, L, extra) in refs.items():
                            a, cap = acc.dense_accuracy(emu[k], ref, mag, base, L, extra)
                            assert acc.dense_ok(a, cap), f"{c.id} {kind} acc={accumulate} bias={bias} relu={relu} fma={fma}: {a}, cap {cap:.3f}"
                            assert torch.isfinite(emu[k]).all()
                            worst = [max(worst[0], a.max_ratio), max(worst[1], a.rms_ratio), max(worst[2], cap)]
    print(f"[accuracy] {group}: worst faithful emulation max x{worst[0]:.2f}, rms x{worst[1]:.2f}, {worst[2]:.2f} of the hard cap")


def test_zero_outputs_of_the_zeros_kind_are_exactly_zero_and_required_to_be():
    """A zero row of x, a zero row of w and a zero column of dh leave outputs with mag == 0: the reference, the baseline and the
    emulation hold exact zeros there, and a 1e-30 in their place is rejected (elementwise: inf)."""
    c = BY_ID["fwd:skinny-31x47x65"]
    p = _problem(c, "zeros")
    ref, mag, base, L, extra = acc.dense_case_refs(c, p)["out"]
    zero = mag == 0
    assert zero[:, -1].all() and zero.all(1).any() and not zero.all()
    out = acc.dense_case_emulation(c, p)["out"]
    assert (out[zero] == 0).all() and (base[zero] == 0).all()
    bad = out.clone(); bad[zero] = 1e-30
    a, cap = acc.dense_accuracy(bad, ref, mag, base, L, extra)
    assert not acc.dense_ok(a, cap) and a.max == float("inf") and cap == float("inf")
    d = BY_ID["bwd_weight:dw_small-129x65x33"]
    p = _problem(d, "zeros")
    ref, mag, base, L, extra = acc.dense_case_refs(d, p)["dw"]
    assert (mag[33 // 2] == 0).all() and (mag[:, 65 // 2] == 0).all()
    assert (acc.dense_case_emulation(d, p)["dw"][mag == 0] == 0).all()


# defect -> the cases it is seeded on, each on every kind of the case ("overwrite" accumulates onto a prior, the others run fresh)
DEFECTS = {
    "drop_partial_kstep": ["fwd:tiled-130x260x130", "fwd:tiled-129x1433x7", "bwd_input:tiled-129x103x262", "bwd_weight:split_k-8200x20x8"],
    "drop_quad": ["fwd:skinny-31x47x65", "fwd:skinny-33x255x63", "bwd_input:skinny-33x65x47"],
    "drop_last_slab": ["bwd_weight:dw_small-1022x64x32", "bwd_weight:split_k-4100x20x8"],
    "slab_twice": ["bwd_weight:dw_small-1022x64x32", "bwd_weight:split_k-4100x20x8"],
    "read_capacity": ["bwd_weight:dw_small-129x65x33", "bwd_weight:split_k-100x20x8+4100"],
    "bias_twice": ["bias_act:skinny-33x47x65", "bias_act:tiled-130x260x130"],
    "scale_shift": ["fwd_row_scaled:skinny-33x47x65", "fwd_row_scaled:tiled-130x260x130"],
    "overwrite": ["bwd_weight:dw_small-129x65x33", "bwd_weight:split_k-4100x20x8"],
}


def _defective(key, kind, defect):
    c = BY_ID[key]
    p = _problem(c, kind)
    bias, accumulate = defect == "bias_twice", defect == "overwrite"
    refs = acc.dense_case_refs(c, p, bias, False, accumulate)
    emu = acc.dense_case_emulation(c, p, bias, False, accumulate, defect=defect)
    (k, (ref, mag, base, L, extra)), = refs.items()
    return emu[k], ref, mag, base, L, extra


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_seeded_defects_are_rejected(defect):
    for key in DEFECTS[defect]:
        for kind in BY_ID[key].kinds:
            got, ref, mag, base, L, extra = _defective(key, kind, defect)
            a, cap = acc.dense_accuracy(got, ref, mag, base, L, extra)
            print(f"[defect] {defect} {key} {kind}: {a}, {cap:.3g} of the hard cap")
            assert not acc.dense_ok(a, cap), f"{defect} on {key} {kind} passes: {a}, cap {cap:.3f}"
            if defect == "read_capacity":      # the NaN row poisons every output
                assert a.max == float("inf") and cap == float("inf")


def test_normwise_bound_on_the_same_defects():
    """What max|got - ref| <= 2e-5 max(1, max|ref|) makes of the same emulations on N(0,1) data: it accepts the faithful orders,
    and it also rejects a lost slab and a shifted row scale (see the module docstring)."""
    for defect in ("drop_last_slab", "scale_shift"):
        for key in DEFECTS[defect]:
            got, ref, *_ = _defective(key, "normal", defect)
            assert not acc.normwise_ok(got, ref)
            good, ref, *_ = _defective(key, "normal", None)
            assert acc.normwise_ok(good, ref)
