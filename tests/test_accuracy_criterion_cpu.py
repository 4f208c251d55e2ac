"""The element-wise accuracy criterion (oracle/accuracy.py) has teeth: a CPU emulation of the split-bf16 GEMMs' arithmetic
passes it when faithful and fails it when one plane of the split is lost, misplaced or mispaired — defects that the
norm-wise tolerance of the older parity tests (2e-5 of max|ref|) lets through.  Same shapes and data generators as the
GPU tests (tests/test_split_dw_accuracy_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc

DW_BLOCKS, DS_MINROWS = 256, 128      # gemm_kernels.hip: workgroups, the gate-word form's share floor


def split3(v: torch.Tensor):
    """fp32 -> three fp32 tensors holding bf16 values, h + m + l = v (split3 / split3_pair: round-to-nearest-even
    conversions, as v_cvt_pk_bf16_f32 rounds)."""
    h = v.bfloat16().float()
    r1 = v - h
    m = r1.bfloat16().float()
    return h, m, (r1 - m).bfloat16().float()


def emulate_split_dw(mask, x, rs, cv, defect=None):
    """gemm_dw_split_k<true> + slab_reduce_rank1_k on the CPU: the row space is shared out over DW_BLOCKS workgroups (at least
    DS_MINROWS rows each); a workgroup multiplies the 0/1 mask by the three bf16 planes of rs * x (formed in fp32) and by the
    planes of rs (the db column), 16 rows per MFMA, small planes first, accumulating in fp32; the slabs are summed in fp32 in
    workgroup order and scaled by cv.  -> (dw, db, S, T), fp32 (S, T: the unscaled sums the head gradient is formed from).
    defect: None, "drop_l" (third plane zero), "shift_l" (third plane taken from the next column), "swap_l" (the two rows
    of a split3_pair word exchanged in the third plane)."""
    n, K = x.shape
    H = mask.shape[1]
    xt, rst = torch.from_numpy(x), torch.from_numpy(rs)
    v = torch.cat([rst[:, None] * xt, rst[:, None]], 1)            # [n, K + 1]: rs x, and the rs column (db)
    planes = list(split3(v))
    if defect == "drop_l":
        planes[2] = torch.zeros_like(planes[2])
    elif defect == "shift_l":
        planes[2] = torch.cat([planes[2][:, 1:K], torch.zeros(n, 1), planes[2][:, K:]], 1)
    elif defect == "swap_l":
        m4 = n // 4 * 4
        planes[2] = torch.cat([planes[2][:m4].reshape(-1, 2, 2, K + 1).flip(2).reshape(m4, K + 1), planes[2][m4:]])
    per = max(-(-n // DW_BLOCKS), DS_MINROWS)
    nwg = -(-n // per)
    steps = -(-per // 16)
    rows = nwg * steps * 16
    pad = lambda t: torch.cat([t, torch.zeros((nwg * per - n,) + tuple(t.shape[1:]))]).reshape(nwg, per, *t.shape[1:])
    pad2 = lambda t: torch.cat([t, torch.zeros((nwg, steps * 16 - per) + tuple(t.shape[2:]))], 1)
    A = pad2(pad(torch.from_numpy(mask.astype(np.float32))))                      # [nwg, steps * 16, H]
    B = [pad2(pad(p)) for p in planes]                                             # [nwg, steps * 16, K + 1]
    assert rows >= n
    accs = torch.zeros(nwg, H, K + 1)
    for s in range(steps):
        a = A[:, 16 * s:16 * s + 16].transpose(1, 2)
        for p in (2, 1, 0):
            accs = accs + torch.bmm(a, B[p][:, 16 * s:16 * s + 16])
    S = torch.zeros(H, K + 1)
    for z in range(nwg):
        S = S + accs[z]
    cvt = torch.from_numpy(cv)
    return cvt[:, None] * S[:, :K], cvt * S[:, K], S[:, :K], S[:, K]


def emulate_split_fwd(x, w, defect=None):
    """gemm_wsplit_f32_k's product x w^T on the CPU: both operands split into three bf16 planes, per 16-wide k step the six
    cross terms in two fp32 chains (hl, hh, lh, hm, mm, mh: the large terms in one, the small in the other), the chains added
    at the end.  defect: None, "drop_mm", "drop_hl_lh"."""
    xh, xm, xl = split3(torch.from_numpy(x))
    wh, wm, wl = split3(torch.from_numpy(w))
    n, K = x.shape
    acc0 = torch.zeros(n, w.shape[0]); acc1 = torch.zeros(n, w.shape[0])
    for k in range(0, K, 16):
        s = slice(k, k + 16)
        mm = lambda a, b: a[:, s] @ b[:, s].T
        if defect != "drop_hl_lh":
            acc1 = acc1 + mm(xl, wh)
        acc0 = acc0 + mm(xh, wh)
        if defect != "drop_hl_lh":
            acc1 = acc1 + mm(xh, wl)
        acc0 = acc0 + mm(xm, wh)
        if defect != "drop_mm":
            acc1 = acc1 + mm(xm, wm)
        acc0 = acc0 + mm(xh, wm)
    return acc0 + acc1


@pytest.fixture(autouse=True)
def _threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(min(16, prev))
    yield
    torch.set_num_threads(prev)


@pytest.mark.parametrize("n,K,H,kind", [(37500, 104, 256, "normal"), (5000, 100, 256, "mixed"), (2500, 64, 96, "zeros"),
                                        (37000, 132, 256, "mixed"), (3000, 144, 128, "normal")])
def test_criterion_accepts_the_faithful_split_dw_and_rejects_a_lost_third_plane(n, K, H, kind):
    """dW1, db1 and dW2 of the gate-word weight-gradient GEMM, emulated: the faithful split passes the criterion; dropping the third
    plane, shifting it by one column or exchanging the two rows of its packed pairs fails it — while every one of them stays
    inside the norm-wise bound max|got - ref| <= 2e-5 max(1, max|ref|) that the older tests apply."""
    p = acc.layer_problem(n, K, H, kind, seed=n + K)
    mask = acc.host_mask(p["x"], p["w"], p["b"])
    x = p["x"][:, :K]
    ref = acc.dw_reference([(mask, x, p["rs"])], p["w2"], p["w"], p["b"])
    dw, db, S, T = emulate_split_dw(mask, x, p["rs"], p["w2"])
    w1, b1 = torch.from_numpy(p["w"][:, :K]), torch.from_numpy(p["b"])
    dwh = torch.zeros(H)
    for k in range(K):          # the head gradient <S, w1> + b1 T of the emulated sums (the kernel forms it from S, T)
        dwh += S[:, k] * w1[:, k]
    dwh += b1 * T
    for got, name in ((dw, "dw"), (db, "db"), (dwh, "dwh")):
        acc.assert_fp32_accuracy(got, *ref[name], what=f"faithful {name}")
    for defect in ("drop_l", "shift_l", "swap_l"):
        dw = emulate_split_dw(mask, x, p["rs"], p["w2"], defect)[0]
        assert not acc.Accuracy(dw, *ref["dw"]).ok(), defect
        live = ref["dw"][1] > 0           # rejected by the ratios too, not only by a non-zero output where mag == 0
        a = acc.Accuracy(dw[live], *(t[live] for t in ref["dw"]))
        assert not a.ok(), f"{defect}: {a}"
        r = ref["dw"][0]
        if kind == "normal":        # (the mixed-magnitude sums are where a norm-wise bound is weakest of all)
            assert float((dw.double() - r).abs().max()) <= 2e-5 * max(1.0, float(r.abs().max())), defect


@pytest.mark.parametrize("n,K,H", acc.FWD_SHAPES[1:])
def test_criterion_accepts_the_faithful_split_forward_and_rejects_dropped_terms(n, K, H):
    """The six-term forward product: faithful passes; without the mm term, or without the hl + lh terms, it fails."""
    p = acc.layer_problem(n, K, H, "normal", seed=n + H)
    x, w = p["x"][:, :K], p["w"][:, :K]
    ref = acc.matmul_reference(x, w.T)
    acc.assert_fp32_accuracy(emulate_split_fwd(x, w), *ref, what="faithful forward")
    for defect in ("drop_mm", "drop_hl_lh"):
        a = acc.Accuracy(emulate_split_fwd(x, w, defect), *ref)
        assert not a.ok(), f"{defect}: {a}"


def test_criterion_requires_exact_zeros_and_rejects_nan():
    ref = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64)
    mag = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64)
    assert acc.elementwise(ref, ref, mag) == (0.0, 0.0)
    assert acc.elementwise(torch.tensor([1.0, 1e-30, 2.0]), ref, mag)[0] == float("inf")
    assert acc.elementwise(torch.tensor([float("nan"), 0.0, 2.0]), ref, mag)[0] == float("inf")
    # an exact baseline: the floor keeps the ratio finite, and a kernel error far above it still fails
    a = acc.Accuracy(torch.tensor([1.0 + 2.0 ** -20, 0.0, 2.0]), ref, mag, ref)
    assert a.base_max == 0.0 and not a.ok()
    assert acc.Accuracy(ref, ref, mag, ref).ok()


def test_split_holds_tiny_products_only_to_the_bf16_subnormal_step():
    """The lower edge of the split's range (include/grapes_hip.h): rows at 1e-28 are split exactly enough to pass the
    criterion; at 1e-35 the third (and for the smallest products the second) plane falls below bf16's smallest subnormal step
    2^-133, so each product is held only to 2^-134 — the criterion fails, the absolute bound holds.  The GPU test
    test_split_dw_domain_edges pins the kernel to the same two outcomes on the same data."""
    n, K, H = 3000, 104, 256
    p = acc.layer_problem(n, K, H, "normal", seed=77)
    mask = acc.host_mask(p["x"], p["w"], p["b"])
    rs = acc.domain_edge_row_scale(n)
    for scale, inside in ((1e-28, True), (1e-35, False)):
        x = (p["x"][:, :K] * scale).astype(np.float32)
        ref = acc.dw_reference([(mask, x, rs)], p["w2"])
        dw = emulate_split_dw(mask, x, rs, p["w2"])[0]
        assert acc.Accuracy(dw, *ref["dw"]).ok() == inside, scale
        assert acc.within_split_resolution(dw, ref["dw"], mask, p["w2"])
