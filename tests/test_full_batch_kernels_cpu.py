"""The oracle of the full-batch training kernels (tests/full_batch_oracle.py) checked against itself, without a GPU: the row-list
transpose and the transposed gather against a dense brute force, the loss reference against fp64 torch autograd, and the criterion
of oracle/accuracy.py shown to separate the two orders a cross-entropy row can be written in on the "shifted" logits the GPU test
uses (tests/test_full_batch_kernels_gpu.py) — which also shows that those inputs leave torch's own fp32 arithmetic, the baseline,
inside the factors."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc
from tests import full_batch_oracle as FB

F32 = np.float32


def _small_graph():
    return FB.kernel_graph(60, seed=4, hub=13, hub_rows=20, long_rows=((30, 40),))


@pytest.mark.parametrize("which", ["all", "third", "one", "empty_rows"])
def test_transpose_and_gather_equal_the_dense_transposed_product(which):
    """(Â restricted to rows)ᵀ dZ on a 60-node graph with stored self-loops and isolated nodes: the rows of the product that are
    sources equal gather_t_ref over rowlist_transpose_ref (g = dinv[rows] ⊙ dZ), every other row is exactly zero."""
    rowptr, col, info = _small_graph()
    n = len(rowptr) - 1
    assert len(info["empty"]) and len(info["loop_only"]) and len(info["hub_rows"]) >= 20
    rng = np.random.default_rng(1)
    rows = {"all": np.arange(n), "third": np.sort(rng.choice(n, n // 3, replace=False)), "one": np.array([30]),
            "empty_rows": np.concatenate([info["empty"], info["loop_only"]])}[which]
    rows = np.sort(rows)
    dinv = FB.host_dinv(rowptr, col)
    srcs, src_off, pos = FB.rowlist_transpose_ref(rowptr, col, n, rows)
    assert np.all(np.diff(srcs) > 0) and src_off[0] == 0 and src_off[-1] == len(pos)
    for j in range(len(srcs)):
        assert np.all(np.diff(pos[src_off[j]:src_off[j + 1]]) > 0)
    if which == "empty_rows":
        assert np.array_equal(srcs, rows) and len(pos) == len(rows)
    dz = rng.standard_normal((len(rows), 5))
    g = dinv[rows].astype(np.float64)[:, None] * dz
    out, mag = FB.gather_t_ref(g, srcs, src_off, pos, dinv)
    A = FB.dense_adjacency(rowptr, col, dinv)
    brute = A[rows].T @ dz
    assert np.allclose(out, brute[srcs], rtol=1e-12, atol=1e-14)
    rest = np.ones(n, bool); rest[srcs] = False
    assert not brute[rest].any()
    assert np.allclose(mag, (A[rows].T @ np.abs(dz))[srcs], rtol=1e-12)
    # the fp32 baseline is the same sum, to fp32 accuracy
    b32, _ = FB.gather_t_ref(g.astype(F32), srcs, src_off, pos, dinv, dtype=np.float32)
    assert b32.dtype == np.float32 and np.all(np.abs(b32 - out) <= 64 * 2.0 ** -24 * mag + 1e-30)


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_loss_reference_equals_fp64_autograd_through_the_mask(multi, p):
    C, M = 11, 97
    z, rows, labels, dinv = FB.loss_problem("normal", M, C, multi, seed=3)
    mask = FB.dropout_mask(FB.N_LOSS, C, p, 5, 17) if p else None
    ref = FB.rowlist_loss_ref(z, C, rows, labels, dinv, p, mask)
    tl, tg, tc = FB.torch_loss_fp64(z, C, rows, labels, dinv, p, mask)
    assert abs(ref["loss"] - tl) <= 1e-13 * abs(tl)
    assert np.allclose(ref["g"], tg, rtol=1e-11, atol=1e-16) and np.allclose(ref["dcol"], tc, rtol=1e-11, atol=1e-16)
    assert np.all(ref["g_mag"] >= np.abs(ref["g"]) * (1 - 1e-12)) and np.all(ref["dcol_mag"] >= np.abs(ref["dcol"]) * (1 - 1e-12))
    assert ref["loss_mag"] >= ref["loss"] * (1 - 1e-12)
    if p:
        assert not ref["g"][~mask[rows]].any() and not ref["g_mag"][~mask[rows]].any()
        assert 0.2 < 1 - mask.mean() < 0.4
    # the fp32 baseline is the same quantity
    base = FB.rowlist_loss_base(z, C, rows, labels, dinv, p, mask)
    assert abs(base["loss"] - ref["loss"]) <= 1e-5 * ref["loss_mag"]
    assert np.all(np.abs(base["g"] - ref["g"]) <= 1e-5 * ref["g_mag"] + 1e-30)
    assert np.all(np.abs(base["dcol"] - ref["dcol"]) <= 1e-4 * ref["dcol_mag"])


@pytest.mark.parametrize("C", [47, 172])
def test_criterion_separates_the_two_cross_entropy_orders_on_shifted_logits(C):
    """ce_rows_f32 in both orders against fp64, the baseline torch's fp32 cross_entropy: on N(0, 1) logits the criterion accepts
    both; with a common offset of +-1000 per row it accepts lsm = (x - m) - log(se) and rejects lse = m + log(se), whose softmax
    carries the rounding of a number of size 1000."""
    M = 257
    seen = {}
    for kind in ("normal", "shifted"):
        z, rows, labels, dinv = FB.loss_problem(kind, M, C, False, seed=C)
        ref = FB.rowlist_loss_ref(z, C, rows, labels, dinv)
        base = FB.rowlist_loss_base(z, C, rows, labels, dinv)
        d32 = dinv[rows.astype(np.int64)][:, None]
        for order in ("shift_first", "add_back"):
            dz, rl = FB.ce_rows_f32(z[:, :C], labels[rows.astype(np.int64)], order)
            a = acc.Accuracy((d32 * dz).astype(F32), ref["g"], ref["g_mag"], base["g"])
            print(f"[accuracy] C={C} {kind} {order}: {a}")
            seen[kind, order] = a
            # the row losses: the single-number convention of the GPU test, 4 * 2^-24 of the loss's magnitude
            loss = float(rl.astype(np.float64).sum() / M)
            seen[kind, order, "loss"] = abs(loss - ref["loss"]) / (2.0 ** -24 * ref["loss_mag"])
    assert seen["normal", "shift_first"].ok() and seen["normal", "add_back"].ok()
    assert seen["shifted", "shift_first"].ok()
    assert not seen["shifted", "add_back"].ok()
    assert seen["shifted", "add_back"].max_ratio > 4 * acc.MAX_FACTOR and \
        seen["shifted", "add_back"].rms_ratio > 10 * acc.RMS_FACTOR              # not a near miss
    assert seen["normal", "shift_first", "loss"] <= 4 and seen["normal", "add_back", "loss"] <= 4
    # (the MEAN loss does not separate the orders: the rows' errors of either sign average out, 0.3 * 2^-24 of its magnitude here;
    # the gradient, judged element by element, is what shows the defect)
    assert seen["shifted", "shift_first", "loss"] <= 4


def test_dropout_mask_is_the_whole_matrix_stream():
    """Row r of the N x width mask is the slice r * width .. of ONE stream: a block's mask does not depend on the block."""
    from oracle import portable_math as pm
    m = FB.dropout_mask(301, 37, 0.3, 77, 123)
    u = pm.philox_uniform(77, 123, 301 * 37)
    assert m.shape == (301, 37) and np.array_equal(m[77:177].reshape(-1), u[77 * 37:177 * 37] >= F32(0.3))
    assert FB.dropout_mask(5, 3, 0.0, 1, 2).all() and not FB.dropout_mask(5, 3, 1.0, 1, 2).any()
    assert FB.dropout_scale(0.0) == 1 and FB.dropout_scale(1.0) == 0
