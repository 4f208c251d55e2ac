"""TEST INFRASTRUCTURE — the element-wise accuracy criterion of the fp32-accuracy GEMMs, and the data they are judged on.

The matrix-pipe GEMMs split every fp32 operand exactly into three bf16 planes and sum the cross products in fp32
(grapes_amd/csrc/gemm_kernels.hip: split3 / split3_pair).  A norm-wise tolerance such as
``max|got - ref| <= 2e-5 max|ref|`` cannot see the lowest plane: it carries about 2^-16 of each product.  The criterion
here can.  Each output is judged against an fp64 reference relative to ITS OWN magnitude, the fp64 sum of |a||b| of the
terms it adds up:

    e = |got - ref| / mag          (where mag == 0 the output must be exactly 0: e = 0 if it is, inf if not)

and the max and rms of e must stay within RMS_FACTOR / MAX_FACTOR of the same two numbers for a host fp32 baseline: the same
product over the same fp32 operands, summed in fp32 in ONE fixed order (fp32_contract: blocks of BLOCK terms added one after
the other, the block sums then added in block order) — where a kernel forms a product before it splits it, as
gemm_dw_split_k forms rs * x, the baseline forms that product in fp32 first.  The order is written out here rather than left
to a BLAS: a BLAS sums a long contraction in an order of its own choosing, and the same fp32 matmul was measured 10x more
accurate (rms) on one host than on another, which made the criterion depend on the machine running the test.  So "fp32
accuracy" means: no worse than a plain blocked fp32 sum of the same products, by a small factor that leaves room for
another summation order.

The data generators below are shared by tests/test_accuracy_criterion_cpu.py (a CPU emulation of the split kernels,
faithful and with defects, which shows the criterion rejects a lost plane) and tests/test_split_dw_accuracy_gpu.py /
tests/test_tsplit_accuracy_gpu.py (the kernels themselves), so the two cannot drift apart.  The emulations of the tiled
gathered-operand GEMMs (emulate_tsplit_fwd / emulate_tsplit_dw) live here too: the GPU tests check an output that exceeds
the factors against them.  The plain fp32 dense GEMMs have their own section at the end (dense_problem, DENSE_CASES, the
sequential-chain baseline and the emulations of their summation orders), shared by tests/test_dense_gemm_accuracy_cpu.py and
tests/test_dense_gemm_accuracy_gpu.py.  Only tests import this module.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

RMS_FACTOR = 3.0
MAX_FACTOR = 6.0
# the baseline's error can be exactly 0 (a unit live in one row, an output of one term): below FLOOR the ratios are taken
# against FLOOR instead — 2^-30 of an output's magnitude is 1/64 ulp of it, far below any defect the criterion is for
FLOOR = 2.0 ** -30

# (n, K, H) of the weight-gradient GEMM gemm_dw_split_k: the sampler nets' first layer (K = 100 / 104 features +
# indicators, H = 256), the log-Z net's narrow form (K = 64, H = 96) and the 160-column form (K = 128 / 132 / 144;
# 144 is its widest: 8 (K / 4) + 32 staging tasks <= 320).
DW_SHAPES = [(37500, 104, 256), (5000, 100, 256), (2500, 64, 96), (37000, 132, 256), (5000, 128, 256), (3000, 144, 128)]
# (n, K, H) of the forward GEMM with the fused head (test_hip_parity.py: test_forward_gemm_with_fused_head_projection)
FWD_SHAPES = [(37501, 104, 256), (5000, 100, 256), (2100, 64, 96), (700, 104, 256)]
KINDS = ("normal", "mixed", "zeros")
DEAD_UNIT, ONE_ROW_UNIT = 0, 1          # units of every generated layer: gated off in every row / live in exactly one row


def elementwise(got, ref, mag) -> Tuple[float, float]:
    """(max, rms) of |got - ref| / mag over all outputs; an output with mag == 0 must be exactly 0 (else inf)."""
    got = torch.as_tensor(got).double().cpu().reshape(-1)
    ref = torch.as_tensor(ref).double().cpu().reshape(-1)
    mag = torch.as_tensor(mag).double().cpu().reshape(-1)
    if got.numel() == 0:
        return 0.0, 0.0
    zero = mag == 0
    e = (got - ref).abs() / torch.where(zero, torch.ones_like(mag), mag)
    e = torch.where(zero, torch.where(got == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))), e)
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    return float(e.max()), float((e ** 2).mean().sqrt())


class Accuracy:
    """Element-wise errors of one output tensor and of its host fp32 baseline."""

    def __init__(self, got, ref, mag, base):
        self.max, self.rms = elementwise(got, ref, mag)
        self.base_max, self.base_rms = elementwise(base, ref, mag)

    @property
    def rms_ratio(self) -> float:
        return self.rms / max(self.base_rms, FLOOR)

    @property
    def max_ratio(self) -> float:
        return self.max / max(self.base_max, FLOOR)

    def ok(self, rms_factor: float = RMS_FACTOR, max_factor: float = MAX_FACTOR) -> bool:
        return self.rms_ratio <= rms_factor and self.max_ratio <= max_factor

    def __repr__(self):
        return (f"max {self.max:.3e} (fp32 {self.base_max:.3e}, x{self.max_ratio:.2f}), "
                f"rms {self.rms:.3e} (fp32 {self.base_rms:.3e}, x{self.rms_ratio:.2f})")


def assert_fp32_accuracy(got, ref, mag, base, what: str = "") -> Accuracy:
    a = Accuracy(got, ref, mag, base)
    print(f"[accuracy] {what}: {a}")
    assert a.ok(), f"{what}: {a}"
    return a


# ------------------------------------------------------------------------------------------------------------- data
def layer_problem(n: int, K: int, H: int, kind: str, seed: int, n_pad: int = 0) -> Dict[str, np.ndarray]:
    """One row set of the layer  x -> ReLU(x w^T + b) -> 1-wide head w2  and the head's gradient rs, fp32:
    x [n, ceil4(K)] (zero pad columns), rs [n], w [H, ceil4(K)], b [H], w2 [H].  kind:
      normal  N(0,1) rows;
      mixed   row r of x at 10^a_r and rs_r at 10^(-a_r + c_r), a in [-20, 20], c in [-3, 3]: every output of the
              weight gradient sums terms of very different sizes (the products rs x stay finite);
      zeros   N(0,1) with exact zeros: whole rows of x, entries of rs, single entries, a whole column of x.
    Every kind has unit DEAD_UNIT gated off in every row (w row 0, b = -1) and unit ONE_ROW_UNIT live in exactly one row
    (x column 0 is zero except x[n // 2, 0] = 1, w row = e_0, b = -0.5: its pre-activation is +-0.5 exactly)."""
    rng = np.random.default_rng(seed)
    Kp = (K + 3) // 4 * 4
    x = rng.standard_normal((n, Kp))
    rs = rng.standard_normal(n)
    if kind == "mixed":
        a = rng.uniform(-20, 20, n)
        x *= 10.0 ** a[:, None]
        rs *= 10.0 ** (-a + rng.uniform(-3, 3, n))
    elif kind == "zeros" and n:
        x[rng.integers(0, n, max(1, n // 50))] = 0.0
        rs[rng.integers(0, n, max(1, n // 50))] = 0.0
        x[rng.integers(0, n, n), rng.integers(0, K, n)] = 0.0
        x[:, K // 2] = 0.0
    elif kind not in KINDS:
        raise ValueError(kind)
    x[:, K:] = 0.0
    x[:, 0] = 0.0
    if n:
        x[n // 2, 0] = 1.0
    w = rng.standard_normal((H, Kp)) * 0.2
    w[:, K:] = 0.0
    b = rng.standard_normal(H) * 0.1
    w[DEAD_UNIT] = 0.0; b[DEAD_UNIT] = -1.0
    w[ONE_ROW_UNIT] = 0.0; w[ONE_ROW_UNIT, 0] = 1.0; b[ONE_ROW_UNIT] = -0.5
    w2 = rng.standard_normal(H) * 0.3
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    if n_pad:       # rows beyond the live count: NaN (a kernel that reads them poisons its outputs)
        x = np.concatenate([x, np.full((n_pad, Kp), np.nan)])
        rs = np.concatenate([rs, np.full(n_pad, np.nan)])
    return {"x": f(x), "rs": f(rs), "w": f(w), "b": f(b), "w2": f(w2)}


def host_mask(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """[n, H] bool: the ReLU gate of the fp64 pre-activation (the CPU emulation's mask; the GPU tests take the device's)."""
    return (x.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)) > 0


# ------------------------------------------------------------------------------------------------------- references
BLOCK = 128     # terms per block of the baseline's fixed summation order (a workgroup's share of rows is of this order)


def _f32(a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


def fp32_contract(a, b) -> torch.Tensor:
    """aᵀ b for a [n, M], b [n, N] in fp32, in a fixed order that does not depend on the host: the n terms of each output in
    blocks of BLOCK, each block summed term by term (product rounded to fp32, then added in fp32), then the block sums added in
    block order.  Element-wise torch ops only, no BLAS."""
    a, b = _f32(a), _f32(b)
    n, M, N = a.shape[0], a.shape[1], b.shape[1]
    nb = max(1, -(-n // BLOCK))
    A = torch.cat([a, torch.zeros(nb * BLOCK - n, M)]).view(nb, BLOCK, M)
    B = torch.cat([b, torch.zeros(nb * BLOCK - n, N)]).view(nb, BLOCK, N)
    part = torch.zeros(nb, M, N)
    for j in range(min(BLOCK, n)):
        part += A[:, j, :, None] * B[:, j, None, :]
    out = torch.zeros(M, N)
    for z in range(nb):
        out += part[z]
    return out


def _t64(a):
    return torch.as_tensor(np.asarray(a)).double()


def dw_reference(segs: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]], cv, w1=None, b1=None,
                 prev: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """fp64 reference, fp64 magnitude and host fp32 baseline of the rank-1 gated weight gradient over row sets
    segs = [(mask [n, H] bool, x [n, K] fp32, rs [n] fp32), ...]:
        dw[m][k] = cv[m] S[m][k],  db[m] = cv[m] T[m],  S = sum_r mask rs x,  T = sum_r mask rs
    and with w1, b1 the gate-word form's head gradient  dwh[m] = <S[m], w1[m]> + b1[m] T[m]  (= sum_r rs relu(z) on the mask).
    The baseline forms rs * x in fp32 (as the kernel does before splitting) and sums with fp32_contract; its dwh adds the K
    products of <S, w1> term by term in fp32.
    prev: the buffers accumulated onto ({"dw", "db", "dwh"}).  -> {name: (ref, mag, base)}"""
    cv64, cv32 = _t64(cv), torch.as_tensor(np.asarray(cv, dtype=np.float32))
    H = cv64.numel()
    K = segs[0][1].shape[1]
    S, Sa, T, Ta = (torch.zeros(H, K, dtype=torch.float64), torch.zeros(H, K, dtype=torch.float64),
                    torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64))
    S32, T32 = torch.zeros(H, K), torch.zeros(H)
    for mask, x, rs in segs:
        if len(rs) == 0:
            continue
        m64 = torch.as_tensor(np.asarray(mask)).double()
        x64, rs64 = _t64(x), _t64(rs)
        v = rs64[:, None] * x64                                    # exact: a product of two fp32 values
        S += m64.T @ v; Sa += m64.T @ v.abs(); T += m64.T @ rs64; Ta += m64.T @ rs64.abs()
        x32, rs32 = _f32(x), _f32(rs)
        ST = fp32_contract(m64.float(), torch.cat([rs32[:, None] * x32, rs32[:, None]], 1))
        S32 += ST[:, :K]; T32 += ST[:, K]
    out = {"dw": [cv64[:, None] * S, cv64.abs()[:, None] * Sa, cv32[:, None] * S32],
           "db": [cv64 * T, cv64.abs() * Ta, cv32 * T32]}
    if w1 is not None:
        w64, b64 = _t64(w1)[:, :K], _t64(b1)
        w32, b32 = _f32(w1)[:, :K], _f32(b1)
        h32 = torch.zeros(H)
        for k in range(K):
            h32 += S32[:, k] * w32[:, k]
        h32 += b32 * T32
        out["dwh"] = [(S * w64).sum(1) + b64 * T, (Sa * w64.abs()).sum(1) + b64.abs() * Ta, h32]
    for k in out:
        if prev is not None and k in prev:
            p64, p32 = _t64(prev[k]), torch.as_tensor(np.asarray(prev[k], dtype=np.float32))
            out[k] = [out[k][0] + p64, out[k][1] + p64.abs(), out[k][2] + p32]
    return {k: tuple(v) for k, v in out.items()}


def head_reference(segs: Sequence[Tuple[np.ndarray, np.ndarray]], prev=None):
    """The activation form's head gradient  dwh[m] = sum_r rs[r] act[r][m]  over segs = [(act [n, H], rs [n]), ...]
    -> (ref, mag, base)."""
    ref = mag = base = None
    for act, rs in segs:
        a64, r64 = _t64(act), _t64(rs)
        parts = (r64 @ a64, r64.abs() @ a64.abs(), fp32_contract(_f32(rs)[:, None], act).view(-1))
        ref, mag, base = parts if ref is None else (ref + parts[0], mag + parts[1], base + parts[2])
    if prev is not None:
        p64 = _t64(prev)
        ref, mag, base = ref + p64, mag + p64.abs(), base + torch.as_tensor(np.asarray(prev, dtype=np.float32))
    return ref, mag, base


def matmul_reference(a, b) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """a [n, K] @ b [K, N]: (fp64 reference, fp64 sum |a||b|, host fp32 baseline)."""
    a64, b64 = _t64(a), _t64(b)
    return a64 @ b64, a64.abs() @ b64.abs(), fp32_contract(_f32(a).T.contiguous(), b)


# ------------------------------------------------------------------------------------------------------- domain edges
def domain_edge_row_scale(n: int) -> np.ndarray:
    """rs for the domain-edge cases: U(0.5, 1) (|rs| <= 1 keeps rs * x finite next to an x of 3.4e38; not all ones, whose
    integer sums an fp32 baseline would add exactly), rs[5] = 1."""
    rs = np.random.default_rng(5).uniform(0.5, 1.0, n).astype(np.float32)
    rs[5] = 1.0
    return rs


def within_split_resolution(dw, ref_dw, mask, cv) -> bool:
    """|dw - ref| <= |cv| (live rows) 2^-134 + 2^-20 mag per output: each product rs x held to half of bf16's smallest
    subnormal step, plus an fp32 sum's rounding — what the three-plane split guarantees for products below ~2^-109."""
    ref, mag = ref_dw[0], ref_dw[1]
    live = torch.from_numpy(np.asarray(mask).sum(0).astype(np.float64))
    bound = torch.from_numpy(np.asarray(cv, dtype=np.float64)).abs() * live * 2.0 ** -134
    err = (torch.as_tensor(dw).double() - ref).abs()
    return bool((err <= bound[:, None] + 2.0 ** -20 * mag).all())


# ------------------------------------------------------------------------------------- tiled gathered-operand GEMMs
# grapes_amd/csrc/gemm_tiled_split.hip: H = feat(ids) Wᵀ and dW = dHᵀ feat(ids), feat(ids[r]) = [X[ids[r], :F] | indicator bits | 0]
TS_BM, TS_BK = 128, 32                  # rows of a forward tile; K step (two k16 MFMA sub-steps)
TS_TAIL_GRID = 256                      # resident workgroups of the split-tail forward
TS_DW_WGS = 768                         # workgroups the weight gradient aims at


def split3(v) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 -> three fp32 tensors holding bf16 values, h + m + l = v (split3 / ts_split3_pair: round-to-nearest-even
    conversions, as v_cvt_pk_bf16_f32 rounds)."""
    v = torch.as_tensor(v, dtype=torch.float32)
    h = v.bfloat16().float()
    r1 = v - h
    m = r1.bfloat16().float()
    return h, m, (r1 - m).bfloat16().float()


def _cross_terms(a, b, defect):
    """The six cross products of one k16 sub-step in the kernels' order (ts_mfma_stage: lh, hl, mm, mh, hm, hh; a = the A
    image's planes, b = the B image's)."""
    (ah, am, al), (bh, bm, bl) = a, b
    terms = [(al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh)]
    if defect == "drop_mm":
        del terms[2]
    elif defect == "drop_hl_lh":
        del terms[:2]
    elif defect == "drop_lh":
        del terms[0]
    return terms


def emulate_tsplit_fwd(x, w, defect=None, k_pieces=None) -> torch.Tensor:
    """gemm_tsplit_fwd_k's x wᵀ on the CPU, x [n, K] (the gathered operand), w [N, K]: K in steps of 32, each two k16
    sub-steps, per sub-step the six cross terms in the kernel's order into ONE fp32 accumulator.  k_pieces: [(j0, j1), ...]
    ranges of K steps summed separately and added in piece order (the split-K form, grapes_linear_fwd_gathered_split_k, and
    the split tail's cut tiles); None = one piece.  defect: None, "drop_mm", "drop_hl_lh", "lost_l" (the l plane of the
    gathered operand zero)."""
    x, w = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(w, dtype=torch.float32)
    n, K = x.shape
    nk = -(-K // TS_BK)
    pad = nk * TS_BK - K
    xs = [torch.nn.functional.pad(p, (0, pad)) for p in split3(x)]
    ws = [torch.nn.functional.pad(p, (0, pad)) for p in split3(w)]
    if defect == "lost_l":
        xs[2] = torch.zeros_like(xs[2])
    out = None
    for j0, j1 in (k_pieces or [(0, nk)]):
        acc = torch.zeros(n, w.shape[0])
        for k in range(TS_BK * j0, TS_BK * j1, 16):
            s = slice(k, k + 16)
            for a, b in _cross_terms([p[:, s] for p in xs], [p[:, s] for p in ws], defect):
                acc = acc + a @ b.T
        out = acc if out is None else out + acc
    return out


def tsplit_fwd_pieces(n: int, kp: int):
    """The split-K form's K pieces at n rows (ts_fwd_slabs): [(j0, j1), ...]."""
    ntiles, nk = -(-n // TS_BM), -(-kp // TS_BK)
    want = max(1, 256 // max(ntiles, 1))
    if want > nk // 2:
        want = max(nk // 2, 1)
    want = min(want, 16)
    kper = -(-nk // want)
    return [(j, min(j + kper, nk)) for j in range(0, nk, kper)]


def tsplit_tail_cut(n: int, nprob: int, kp: int):
    """The split tail's cut tiles (gemm_tsplit_fwd_tail_k, ts_tail_of) at n rows and nprob nets:
    ({(tile, net): [(j0, j1), ...]} for every cut unit, S)."""
    ntiles, nk = -(-n // TS_BM), -(-kp // TS_BK)
    units, G = ntiles * nprob, TS_TAIL_GRID
    t_full = units // G * G
    R = units - t_full
    S = G // R if R > 0 else 1
    S = max(1, min(S, nk // 2, 8))
    kper = -(-nk // S)
    S = -(-nk // kper)
    if S <= 1:
        return {}, S
    pieces = [(j, min(j + kper, nk)) for j in range(0, nk, kper)]
    return {divmod(u, nprob): pieces for u in range(t_full, units)}, S


def tsplit_dw_slabs(cap: int, f_out: int, kp: int, wgs: int = TS_DW_WGS) -> int:
    """Slabs of grapes_linear_bwd_weight_gathered_split[_ld] at a row CAPACITY cap (ts_dw_slabs, the product's default form: the
    swapped tile where it needs no more tiles); the kernels share the LIVE rows' steps out over them."""
    swapped = 128 < f_out <= 256 and -(-kp // 128) <= -(-f_out // 128) * -(-kp // 256)
    tiles = -(-kp // 128) if swapped else -(-f_out // 128) * -(-kp // 256)
    ns = min(wgs // tiles, -(-(-(-cap // TS_BK)) // 4))
    return max(ns, 1)


def tsplit_multi_per(kps: Sequence[int], lives: Sequence[int]) -> int:
    """K steps per slab of grapes_linear_bwd_weight_gathered_split_multi (ts_dw_partition) at these live row counts."""
    ct = -(-max(kps) // 128)
    nslab = max(768 // ct, 4 + 4)
    steps = [-(-n // TS_BK) for n in lives]
    avail = nslab - len(lives)
    per = max(-(-sum(steps) // avail), 4)
    return per


def emulate_tsplit_dw(dh, feat, nslab=None, defect=None, per=None, lost_slab=None) -> torch.Tensor:
    """gemm_tsplit_dw_k / gemm_tsplit_dw_sw_k + ts_slab_sum_k on the CPU: dW = dhᵀ feat (dh [n, M], feat [n, K]).  The row
    space in 32-row steps is cut into slabs of `per` steps (per = ceil(steps / nslab), as the kernels derive it); each slab
    sums its 16-row sub-steps, the six cross terms in the kernels' order (dH.l x.h, dH.h x.l, m m, dH.m x.h, dH.h x.m, h h),
    into one fp32 accumulator; the slabs are added in index order.  defect: None, "drop_mm", "drop_hl_lh", "drop_lh",
    "lost_l" (the l plane of feat zero), "lost_l_slab" (that plane zero in slab lost_slab only)."""
    dh, feat = torch.as_tensor(dh, dtype=torch.float32), torch.as_tensor(feat, dtype=torch.float32)
    n, M = dh.shape
    K = feat.shape[1]
    steps = -(-n // TS_BK)
    if per is None:
        per = -(-steps // nslab)
    ns = max(1, -(-steps // per))
    rows = ns * per * TS_BK
    a = [torch.nn.functional.pad(p, (0, 0, 0, rows - n)).view(ns, per * TS_BK, M) for p in split3(dh)]
    b = [torch.nn.functional.pad(p, (0, 0, 0, rows - n)).view(ns, per * TS_BK, K) for p in split3(feat)]
    if defect == "lost_l":
        b[2] = torch.zeros_like(b[2])
    elif defect == "lost_l_slab":
        b[2] = b[2].clone()
        b[2][lost_slab] = 0.0
    accs = torch.zeros(ns, M, K)
    for t in range(0, per * TS_BK, 16):
        s = slice(t, t + 16)
        for pa, pb in _cross_terms([p[:, s] for p in a], [p[:, s] for p in b], defect):
            accs = accs + torch.bmm(pa.transpose(1, 2), pb)
    out = torch.zeros(M, K)
    for z in range(ns):
        out = out + accs[z]
    return out


NAN_ROW = -1        # the last row of every generated X: NaN, read only through the capacity rows' ids


def gathered_problem(N: int, F: int, num_ind: int, f_out: int, n: int, cap: int, kind: str, seed: int,
                     epoch: int = 77, rows_seed: Optional[int] = None) -> Dict[str, np.ndarray]:
    """One transform-first first layer over n gathered rows (capacity cap >= n):
      X [N, ceil4(F)] fp32 (zero pad columns, as pad_features leaves them; its last row NaN in [:F]);
      ids [cap] int32: live rows in [0, N - 1) (with repeats), capacity rows -> the NaN row;
      code [N] int32 indicator words (epoch << 8 | bits; every fourth node a stale epoch with all bits set, which reads 0);
      w [f_out, F + num_ind] N(0,1) / sqrt(K), a view of wide [f_out, F + num_ind + 5] whose extra columns are +inf (a
      weight read past its K poisons the output);
      dh [cap, f_out] N(0,1), capacity rows NaN.
    kind: normal; mixed (row g of X at 10^a_g, a in [-20, 20]: outputs of very different sizes in one tile — and dh row r
    at 10^(-a_ids[r] + c_r), c in [-3, 3], as layer_problem's rs); zeros (whole zero rows of X and of dh, single zero entries,
    a zero column of X).  X, code and w depend on (N, F, num_ind, f_out, kind, seed) only; ids and dh on rows_seed
    (default seed + 1) as well: problems that share X draw their rows with different rows_seed."""
    rng = np.random.default_rng(seed)
    K, ldx = F + num_ind, (F + 3) // 4 * 4
    X = np.zeros((N, ldx))
    X[:, :F] = rng.standard_normal((N, F))
    a = rng.uniform(-20, 20, N) if kind == "mixed" else np.zeros(N)
    X[:, :F] *= 10.0 ** a[:, None]
    if kind == "zeros":
        X[rng.integers(0, N - 1, max(1, N // 50))] = 0.0
        X[rng.integers(0, N - 1, N), rng.integers(0, F, N)] = 0.0
        X[:, F // 2] = 0.0
    elif kind not in KINDS:
        raise ValueError(kind)
    X[NAN_ROW, :F] = np.nan
    code = ((epoch << 8) | rng.integers(0, 1 << max(num_ind, 1), N)).astype(np.int64)
    code[::4] = ((epoch - 1) << 8) | 0xff
    wide = np.full((f_out, K + 5), np.inf)
    wide[:, :K] = rng.standard_normal((f_out, K)) / np.sqrt(K)
    rr = np.random.default_rng(seed + 1 if rows_seed is None else rows_seed)
    ids = np.full(cap, N - 1, np.int64)
    ids[:n] = rr.integers(0, N - 1, n)
    dh = rr.standard_normal((cap, f_out))
    if kind == "mixed":
        dh *= 10.0 ** (-a[ids] + rr.uniform(-3, 3, cap))[:, None]
    elif kind == "zeros":
        dh[rr.integers(0, cap, max(1, cap // 50))] = 0.0
        dh[rr.integers(0, cap, cap), rr.integers(0, f_out, cap)] = 0.0
    dh[n:] = np.nan
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    return {"X": f(X), "ids": ids.astype(np.int32), "code": code.astype(np.int32), "wide": f(wide), "w": f(wide[:, :K]),
            "dh": f(dh), "epoch": epoch, "F": F, "num_ind": num_ind, "n": n}


def gathered_feat(p: Dict[str, np.ndarray], rows=None, ind_mask: int = 0) -> np.ndarray:
    """feat(ids[r]) of gathered_problem p for the live rows (or `rows` of them), fp32 [len, F + num_ind]: X's columns, then the
    indicator bits of the node's word where its epoch is current, under ind_mask (0 = all bits)."""
    F, ni = p["F"], p["num_ind"]
    ids = p["ids"][:p["n"]] if rows is None else p["ids"][rows]
    out = np.zeros((len(ids), F + ni), np.float32)
    out[:, :F] = p["X"][ids, :F]
    if ni:
        cd = p["code"][ids].astype(np.int64) & 0xffffffff
        bits = np.where((cd >> 8) == p["epoch"], cd & 0xff, 0) & (ind_mask if ind_mask else 0xff)
        out[:, F:] = (bits[:, None] >> np.arange(ni)) & 1
    return out


def within_tiled_split_resolution(got, ref, other_abs) -> bool:
    """|got - ref| <= 2^-134 other_abs + 2^-20 mag per output of a tiled GEMM whose one operand is tiny: each of its entries
    held to half of bf16's smallest subnormal step, plus an fp32 sum's rounding.  other_abs: per output the sum of |.| of the
    other operand's terms (forward over tiny rows: sum_k |w[c][k]| broadcast over rows), broadcastable to got."""
    err = (torch.as_tensor(got).double() - ref[0]).abs()
    return bool((err <= 2.0 ** -134 * torch.as_tensor(other_abs).double() + 2.0 ** -20 * ref[1]).all())


# ------------------------------------------------------------------------------------------- sparse aggregation (GCN)
# grapes_amd/csrc/spmm_kernels.hip: out = Â h (+ b, ReLU), its transpose, the column sums and the rank-1 backward.  The same
# criterion as above, each output relative to the fp64 sum of |w||h| of ITS OWN terms, against a host fp32 baseline that adds a
# row's entries in CSR order.  A hard cap stands beside the ratio test (assert_aggregate_accuracy): the textbook bound of an
# (L + 1)-term fp32 sum, so that a poor baseline can never excuse a kernel.
AGG_KINDS = ("normal", "mixed", "zeros", "striped")
# every row-length boundary of the aggregation kernels, on both sides: 0; 1-4 (inside a head record); 5, 8, 9 (the record's second
# group); GRAPES_HUB_ROW = 16 (sequential up to it, eight chains above); GRAPES_LONG_ROW = 64 (chunk + combine above it on graphs
# of more than 2048 nodes); 127-129 (two chunks / a third begun); 200; 1000.  The hubs are named per problem.
AGG_ROW_LENGTHS = (0, 1, 2, 4, 5, 8, 9, 15, 16, 17, 24, 63, 64, 65, 127, 128, 129, 200, 1000)
AGG_FILL_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 24)     # what the rows that are not named cycle through
AGG_LOOP_ROWS = 64      # the baseline walks rows up to this length by position-in-row, longer ones by a sequential accumulate
U32 = 2.0 ** -24        # unit roundoff of fp32


def _seq_sum_f32(terms: np.ndarray) -> np.ndarray:
    """The sequential fp32 sum ((t_0 + t_1) + t_2) + ... of the rows of terms [L, f] (fp32): numpy's add.accumulate keeps the
    dtype and adds in order (r_i = r_{i-1} + t_i), which a reduce (pairwise) and torch.cumsum (a double accumulator) do not."""
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1], np.float32)
    return np.add.accumulate(terms, axis=0, dtype=np.float32)[-1]


def _spmm64(rows, cols, w, h64, n):
    a = torch.sparse_coo_tensor(torch.stack([rows, cols]), w, (n, h64.shape[0]), dtype=torch.float64)
    return torch.sparse.mm(a, h64)


def aggregate_sums(rowptr, csr, dinv, h, self_loop=True, prescaled=False, order=None):
    """The aggregation before bias and ReLU: (ref fp64, mag fp64, base fp32 numpy), see aggregate_reference; aggregate_finish
    adds a bias and the ReLU, so that one set of sums serves every bias / ReLU combination of a case."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    csr = np.asarray(csr, dtype=np.int64)[:rowptr[-1]]
    d32 = np.asarray(dinv, dtype=np.float32)
    h32 = np.ascontiguousarray(np.asarray(h, dtype=np.float32))
    f = h32.shape[1]
    lens = np.diff(rowptr)
    # ---- fp64 reference and magnitude (capacity rows of h, which no entry names, are zeroed: they are NaN)
    named = np.zeros(h32.shape[0], bool); named[csr] = True; named[:n] = True
    h64 = torch.from_numpy(np.where(named[:, None], h32, np.float32(0)).astype(np.float64))
    d64 = torch.from_numpy(d32.astype(np.float64))
    tr, tc = torch.from_numpy(np.repeat(np.arange(n), lens)), torch.from_numpy(csr)
    w64 = d64[tc] * d64[tr]
    ref = _spmm64(tr, tc, w64, h64, n)
    mag = _spmm64(tr, tc, w64, h64.abs(), n)
    if self_loop:
        ref = ref + (d64[:n] ** 2)[:, None] * h64[:n]
        mag = mag + (d64[:n] ** 2)[:, None] * h64[:n].abs()
    # ---- fp32 baseline: a row's terms in CSR order
    m = min(len(d32), h32.shape[0])
    src = (h32[:m] * d32[:m, None]).astype(np.float32) if prescaled else h32        # prescaled: hs = fl32(dinv h)

    def terms(rows, s):         # the fp32 products of entries s of `rows` (one entry per row, or one row's entries)
        return src[s] if prescaled else ((d32[s] * d32[rows])[:, None] * src[s]).astype(np.float32)

    acc = np.zeros((n, f), np.float32)
    if order is None:
        # rows of up to AGG_LOOP_ROWS entries, all together: step j adds entry j of every row that has one
        for j in range(min(AGG_LOOP_ROWS, int(lens.max()) if n else 0)):
            rows = np.nonzero((lens > j) & (lens <= AGG_LOOP_ROWS))[0]
            acc[rows] += terms(rows, csr[rowptr[rows] + j])
        long_rows = np.nonzero(lens > AGG_LOOP_ROWS)[0]
    else:
        long_rows = np.arange(n)
    for r in long_rows:         # longer rows one by one: the same chain through add.accumulate (or the order under test)
        t = np.ascontiguousarray(terms(r, csr[rowptr[r]:rowptr[r + 1]]), dtype=np.float32)
        acc[r] = _seq_sum_f32(t) if order is None else order(t)
    dc = d32[:n, None]
    if prescaled:
        base = dc * (acc + src[:n]) if self_loop else dc * acc
    else:
        base = acc + (dc * dc) * src[:n] if self_loop else acc
    return ref, mag, base.astype(np.float32)


def aggregate_finish(sums, bias=None, relu=False):
    """(ref, mag, base) of aggregate_sums' result with the bias added (mag gains |b|) and the ReLU applied."""
    ref, mag, base = sums
    if bias is not None:
        b32 = np.asarray(bias, dtype=np.float32)
        ref = ref + torch.from_numpy(b32.astype(np.float64))
        mag = mag + torch.from_numpy(np.abs(b32).astype(np.float64))
        base = base + b32
    if relu:
        ref = ref.clamp(min=0)
        base = np.maximum(base, np.float32(0))
    return ref, mag, torch.from_numpy(np.ascontiguousarray(base, dtype=np.float32))


def aggregate_reference(rowptr, csr, dinv, h, bias=None, relu=False, self_loop=True, prescaled=False, order=None):
    """out[c] = sum_j dinv[s_j] dinv[c] h[s_j] + dinv[c]^2 h[c] + b (then max(., 0)) over the rows c = 0 .. len(rowptr) - 2 of
    the CSR (rowptr, csr); the transpose (backward) is the same function over rowptr_s / csr_dst.  dinv is the fp32 array the
    graph build produced, taken as given and widened, so the aggregation alone is judged.  h may hold more rows than the CSR
    (capacity rows: never read by a correct kernel, and not read here).  -> (ref, mag, base):
      ref   fp64;  mag  fp64, the same sum over absolute values (+ |b|);
      base  fp32 in ONE fixed order, element-wise ops only: w = fl32(dinv[s] dinv[c]), the products fl32(w h[s]) added in CSR
            order, then the self-loop with fl32(dc dc), then the bias, then ReLU.  prescaled: the two roundings of that form,
            hs = fl32(dinv[s] h[s]), out = fl32(dc (sum + hs[c])) (+ b).
    order (tests of the criterion): a function (terms [L, f] fp32) -> [f] fp32 that replaces the sequential sum of a row's
    entries, for emulations of the kernels' other orders.
    What carries the test where: the baseline's MAX error is set by its longest row (a sequential sum of 20000 terms errs far more
    than the kernels' eight chains and chunks, which sit at 0.1-0.3 of it), so on graphs with a hub the max ratio bounds the hubs
    and little else; the short rows are held by the rms ratio, which every output enters, and by the hard cap
    (hard_cap_excess), which is per output and knows each row's own length."""
    return aggregate_finish(aggregate_sums(rowptr, csr, dinv, h, self_loop, prescaled, order), bias, relu)


def colsum_reference(src, gate=None, row_scale=None, prior=None):
    """out[c] = sum_r row_scale[r] [gate[r][c] > 0] src[r][c] (+ prior[c]) over the rows given (the bias gradient / masked
    column sums) -> (ref, mag, base); the baseline adds the rows in row order in fp32 (products rounded first)."""
    s32 = np.asarray(src, dtype=np.float32)
    if gate is not None:
        s32 = np.where(np.asarray(gate) > 0, s32, np.float32(0))
    s64 = s32.astype(np.float64)
    if row_scale is not None:
        r32 = np.asarray(row_scale, dtype=np.float32)
        s64 = r32.astype(np.float64)[:, None] * s64
        s32 = (r32[:, None] * s32).astype(np.float32)
    ref, mag, base = s64.sum(0), np.abs(s64).sum(0), _seq_sum_f32(np.ascontiguousarray(s32))
    if prior is not None:
        p32 = np.asarray(prior, dtype=np.float32)
        ref, mag, base = ref + p32.astype(np.float64), mag + np.abs(p32.astype(np.float64)), (p32 + base).astype(np.float32)
    return torch.from_numpy(ref), torch.from_numpy(mag), torch.from_numpy(base)


def rank1_reference(rowptr_s, csr_dst, dinv, act, dh2, w2, gate=None, prior_dw=None, prior_db=None):
    """grapes_gcn_aggregate_bwd_rank1[_bits] over the live rows 0 .. len(rowptr_s) - 2:
        dpre[r][m] = [gate[r][m] > 0] dh2[r] w2[m]   (gate = act unless the gate bits are given as a 0/1 array),
        dh = Âᵀ dpre,  dw_head = dh2ᵀ act,  dbias = colsum(dpre)
    -> {"dh" | "dw_head" | "dbias": (ref, mag, base)}.  The baseline forms fl32(dh2 w2) first, as the kernel does; the fp64
    reference takes that product exactly (one more rounding per term than the plain aggregation: the hard cap's L + 5)."""
    n = len(rowptr_s) - 1
    a32, d32, w32 = (np.asarray(v, dtype=np.float32) for v in (act, dh2, w2))
    g = (a32 if gate is None else np.asarray(gate))[:n] > 0
    dpre64 = np.where(g, d32[:n, None].astype(np.float64) * w32.astype(np.float64), 0.0)
    dpre32 = np.where(g, (d32[:n, None] * w32).astype(np.float32), np.float32(0))
    pad = np.zeros((a32.shape[0] - n, a32.shape[1]))
    exact = _agg64(rowptr_s, csr_dst, dinv, np.concatenate([dpre64, pad]))
    base = aggregate_reference(rowptr_s, csr_dst, dinv, np.concatenate([dpre32, pad.astype(np.float32)]))[2]
    out = {"dh": (exact[0], exact[1], base),
           "dw_head": colsum_reference(a32[:n], row_scale=d32[:n], prior=prior_dw)}
    db64 = dpre64.sum(0); dbm = np.abs(dpre64).sum(0); db32 = _seq_sum_f32(np.ascontiguousarray(dpre32))
    if prior_db is not None:
        p32 = np.asarray(prior_db, dtype=np.float32)
        db64, dbm, db32 = db64 + p32.astype(np.float64), dbm + np.abs(p32.astype(np.float64)), (p32 + db32).astype(np.float32)
    out["dbias"] = (torch.from_numpy(db64), torch.from_numpy(dbm), torch.from_numpy(db32))
    return out


def _agg64(rowptr, csr, dinv, h64np):
    """(ref, mag) of the aggregation over an fp64 operand (rank1_reference's exact products)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    csr = np.asarray(csr, dtype=np.int64)[:rowptr[-1]]
    d64 = torch.from_numpy(np.asarray(dinv, dtype=np.float32).astype(np.float64))
    h64 = torch.from_numpy(np.ascontiguousarray(h64np, dtype=np.float64))
    tr, tc = torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))), torch.from_numpy(csr)
    w64 = d64[tc] * d64[tr]
    loop = (d64[:n] ** 2)[:, None]
    return _spmm64(tr, tc, w64, h64, n) + loop * h64[:n], _spmm64(tr, tc, w64, h64.abs(), n) + loop * h64[:n].abs()


def aggregate_problem(kind: str, n: int, row_lengths: Sequence[int], f: int, seed: int, n_pad: int = 0) -> Dict[str, np.ndarray]:
    """A graph over n live nodes (capacity n + n_pad) and the operands of every aggregation entry point.
    Graph: the destination rows named by row_lengths (placed at seeded rows) have exactly that many entries, the others cycle
    through AGG_FILL_LENGTHS; a row's sources are drawn WITH repeats (duplicate edges: a 6000-entry hub fits a 1500-node graph)
    from the nodes other than itself, three popular sources among them (in about 1/2, 1/8 and 1/20 of the rows: sources with
    hundreds of out-edges, so the transpose has long rows of its own); every seventh row also has a self-loop in the edge list,
    which the build drops (the unit loop replaces it) and which therefore does not count.  The edge list is sorted by
    (source, destination): grouped by source, as the source-grouped builds require, sources ascending within a destination row.
      src, dst int32 [e];  lens int64 [n] expected entries per destination row;  n, cap
    Operands (fp32): h, dout, act [cap, f], dh2 [cap], bias, w2 [f]; act >= 0 with about half its entries 0 (a ReLU output).
      normal   N(0,1);
      mixed    row r of h, dout at 10^a_r, a in [-12, 12] (each its own a); act row r at 10^a_r and dh2_r at 10^(-a_r + c_r),
               c in [-3, 3], as layer_problem does;
      zeros    N(0,1) with whole zero rows, single zero entries and a zero column (h, dout, act), zero entries of dh2;
      striped  row s of h, dout, act is nonzero only in the columns c with c % G == s % G, G = min(f, 64): an output (r, c) sums
               only the entries of row r whose source falls in its stripe, so most outputs of rows up to a few hundred entries
               hold zero or one term — a lost term leaves an exact zero where a value belongs, a term read twice doubles it.
    Rows past the live count are NaN in every operand."""
    if kind not in AGG_KINDS:
        raise ValueError(kind)
    rng = np.random.default_rng(seed)
    cap = n + n_pad
    lens = np.array([AGG_FILL_LENGTHS[i % len(AGG_FILL_LENGTHS)] for i in range(n)], dtype=np.int64)
    named = rng.permutation(np.arange(3, n))[:len(row_lengths)]
    lens[named] = np.asarray(row_lengths, dtype=np.int64)
    e = int(lens.sum())
    dst = np.repeat(np.arange(n), lens)
    src = rng.integers(0, n - 1, e)
    src = src + (src >= dst)                                                   # never the row itself: draws are over n - 1 nodes
    first = np.concatenate([[True], dst[1:] != dst[:-1]]) if e else np.zeros(0, bool)
    u = rng.random(e)
    popular = np.where(u < 0.5, 0, np.where(u < 0.625, 1, 2))                  # (at most once per row: its first draw)
    src = np.where(first & (u < 0.675) & (popular != dst), popular, src)
    loops = np.arange(0, n, 7)
    src, dst = np.concatenate([src, loops]), np.concatenate([dst, loops])
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    G = min(f, 64)

    def rows(scale=None):
        x = rng.standard_normal((cap, f))
        if scale is not None:
            x *= 10.0 ** scale[:, None]
        if kind == "zeros":
            x[rng.integers(0, n, max(1, n // 50))] = 0.0
            x[rng.integers(0, n, n), rng.integers(0, f, n)] = 0.0
            x[:, f // 2] = 0.0
        elif kind == "striped":
            x *= (np.arange(f)[None, :] % G) == (np.arange(cap)[:, None] % G)
        x[n:] = np.nan
        return x

    mixed = kind == "mixed"
    h = rows(rng.uniform(-12, 12, cap) if mixed else None)
    dout = rows(rng.uniform(-12, 12, cap) if mixed else None)
    a = rng.uniform(-12, 12, cap) if mixed else None
    act = np.maximum(rows(a), 0.0)
    act[n:] = np.nan
    dh2 = rng.standard_normal(cap)
    if mixed:
        dh2 *= 10.0 ** (-a + rng.uniform(-3, 3, cap))
    elif kind == "zeros":
        dh2[rng.integers(0, n, max(1, n // 50))] = 0.0
    dh2[n:] = np.nan
    c = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    return {"src": src.astype(np.int32), "dst": dst.astype(np.int32), "lens": lens, "named": named, "n": n, "cap": cap,
            "h": c(h), "dout": c(dout), "act": c(act), "dh2": c(dh2),
            "bias": c(rng.standard_normal(f) * 0.1), "w2": c(rng.standard_normal(f) * 0.3)}


def host_csr(src, dst, n):
    """(rowptr_t, csr_src, rowptr_s, csr_dst, dinv fp32) of an edge list as the graph build leaves them: self-loops dropped,
    duplicates kept, a row's entries ascending; dinv = fl32(1 / sqrt(in-degree + 1)) from fp64.  For the CPU tests; the GPU tests
    read the device's arrays."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    o = np.lexsort((src, dst))
    rowptr_t = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    o2 = np.lexsort((dst, src))
    rowptr_s = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
    dinv = (1.0 / np.sqrt(np.diff(rowptr_t) + 1.0)).astype(np.float32)
    return rowptr_t, src[o], rowptr_s, dst[o2], dinv


def hard_cap_excess(got, ref, mag, lens, extra: int = 4) -> float:
    """max over the outputs of |got - ref| / ((L_r + extra) 2^-24 mag), L_r the entry count of the output's row (lens [n], or a
    scalar for column sums): <= 1 is the textbook bound of an (L + 1)-term fp32 sum with one rounding in each weight (extra = 4;
    the prescaled and rank-1 forms round once more per term: extra = 5).  An output with mag == 0 must be 0."""
    got, ref, mag = (torch.as_tensor(v).double().cpu() for v in (got, ref, mag))
    L = torch.as_tensor(np.asarray(lens, dtype=np.float64))
    if got.dim() == 2 and L.dim() == 1:
        L = L[:, None]
    bound = (L + extra) * U32 * mag
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if err.numel() == 0:
        return 0.0
    q = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(q.max())


def assert_aggregate_accuracy(got, ref, mag, base, lens, what: str = "", extra: int = 4) -> Accuracy:
    """The ratio criterion (assert_fp32_accuracy) and, beside it, the hard cap |got - ref| <= (L_r + extra) 2^-24 mag."""
    x = hard_cap_excess(got, ref, mag, lens, extra)
    print(f"[cap] {what}: worst |err| / ((L + {extra}) u mag) = {x:.3f}")
    a = assert_fp32_accuracy(got, ref, mag, base, what)
    assert x <= 1.0, f"{what}: an output exceeds the (L + {extra}) 2^-24 mag bound by x{x:.3f}"
    return a


# the graphs the CPU test of the criterion and the GPU test of the kernels share: (live nodes, capacity rows past them, hubs)
#   small   <= 2048 nodes: every row by one wavefront whatever its length (no work items);
#   large   > 2048 nodes: rows above GRAPES_LONG_ROW become chunk items; a 20000-entry hub;
#   rows9k  > 8192 rows: the backward's two-launch column sums instead of the one-launch ticket form.
AGG_GRAPHS = {"small": (1500, 37, (6000,)), "large": (2600, 41, (5000, 20000)), "rows9k": (9000, 23, (5000,))}


def aggregate_case(size: str, kind: str, f: int, seed: int = 0, pad: bool = True,
                   row_lengths: Sequence[int] = AGG_ROW_LENGTHS) -> Dict[str, np.ndarray]:
    n, n_pad, hubs = AGG_GRAPHS[size]
    return aggregate_problem(kind, n, tuple(row_lengths) + tuple(hubs), f, seed, n_pad=n_pad if pad else 0)


# --------------------------------------------------------------------------------- attention aggregation (GAT, GATv2)
# grapes_amd/csrc/gat_kernels.hip, gatv2_kernels.hip: out_i = sum_j alpha_ij H_j + b over a row's entries and the implied unit
# self-loop, alpha = softmax_j e_ij, and the analytic backward.  The same criterion as the plain aggregation — each output relative
# to the fp64 sum of |terms| of ITS OWN terms, against a host fp32 baseline in CSR order (self-loop first) — and beside it a hard
# cap per output, |got - ref| <= K 2^-24 mag with K = L_r + c0 + c1 S_r (attention_cap_excess; the constants are derived at
# gat_forward_sums and gat_backward_reference).  The graphs and [cap, f] operands are aggregate_problem's; the row lengths gain
# the attention kernels' own boundaries: 3; 30-33 and 62-65 (one batch of LPR = 32 / 64 lanes with the self-loop at position -1,
# one entry short of it, one and two past it); 95-97 and 127-129 (the second work item; three batches of 32); 191-193, 257, 321
# (chunk counts 3, 4 (+1 entry), 5, 6: gat_fwd_combine_k's four quarters with per = 1 and 2, an empty last quarter at nc = 5).
ATT_ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 24, 30, 31, 32, 33, 62, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193,
                   200, 257, 321, 1000)
ATT_KINDS = AGG_KINDS
ATT_REGIMES = ("narrow", "wide_asc", "wide_desc", "wide_rand", "ties")
# the row groups a result is also judged on one by one, so that a failure names the boundary: (name, shortest, longest)
ATT_GROUPS = (("L<=5", 0, 5), ("L30..33", 30, 33), ("L62..65", 62, 65), ("L95..129", 95, 129), ("L191..321", 191, 321),
              ("hubs", 1000, 1 << 30))
ATT_QUANTUM = 2.0 ** -7
GAT_SLOPE32 = np.float32(0.2)       # GAT_SLOPE of gat_kernels.hip: the kernels' constant IS this fp32 value, and so is the reference's
ATT_C0, ATT_C1 = 14, 2              # forward cap K = L + ATT_C0 + ATT_C1 S (gat_forward_sums)


def attention_case(size: str, kind: str, f: int, seed: int = 0, pad: bool = True, transpose: bool = False,
                   hub_cap: Optional[int] = None, compress: bool = True) -> Dict[str, np.ndarray]:
    """aggregate_case over ATT_ROW_LENGTHS (+ the hubs of AGG_GRAPHS[size], each cut to hub_cap entries if given).
    transpose: the same graph with src and dst swapped (re-sorted by (source, destination)), so that the named lengths are the
    rows of the by-source CSR, the one the backward walks.  lens / lens_s: entries per by-target / by-source row as the build
    leaves them (stored self-loops dropped).  kind `mixed`: the operand rows are spread over 10^[-4, 4] instead of
    10^[-12, 12] (h, dout -> sign |.|^(1/3), formed in fp64 and rounded to fp32 once): the attention backward multiplies three
    operand rows into one parameter gradient (ds H with ds ~ alpha G.H), which at 10^12 each leaves fp32's range, and a weight of
    e^-56 beside a row at 10^-12 its normal range; nothing else of the operands changes.  compress=False keeps 10^[-12, 12], which
    the forward alone can take (tests of the criterion)."""
    n, n_pad, hubs = AGG_GRAPHS[size]
    if hub_cap is not None:
        hubs = tuple(min(h, hub_cap) for h in hubs)
    p = aggregate_problem(kind, n, tuple(ATT_ROW_LENGTHS) + hubs, f, seed, n_pad=n_pad if pad else 0)
    if transpose:
        src, dst = p["dst"].astype(np.int64), p["src"].astype(np.int64)
        o = np.lexsort((dst, src))
        p["src"], p["dst"] = src[o].astype(np.int32), dst[o].astype(np.int32)
    keep = p["src"] != p["dst"]
    p["lens"] = np.bincount(p["dst"][keep], minlength=n).astype(np.int64)
    p["lens_s"] = np.bincount(p["src"][keep], minlength=n).astype(np.int64)
    if kind == "mixed" and compress:
        for k in ("h", "dout"):
            p[k] = np.ascontiguousarray(np.cbrt(p[k].astype(np.float64)), dtype=np.float32)
    return p


def attention_scores(n: int, cap: int, regime: str, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(s_src, s_dst) fp32 [cap], NaN past n.  s_src is an EVEN multiple of 2^-7 and s_dst an ODD one, both below 2^6: every
    raw = s_src[j] + s_dst[i] is exact in fp32 (at most 14 significant bits) and never 0, LeakyReLU's kink.  A row's entries
    ascend by source id, so the node order of s_src places a row's maximum:
      narrow     |raw| <= 2, random;
      wide_asc   s_src ascending in node id over [-40, 40] (the maximum in a row's LAST batch or chunk), s_dst random in [-8, 8]:
                 e spans 50 and more, most weights of a long row fall below 2^-24 of the largest;
      wide_desc  descending (the maximum at the first entry, or the self-loop);  wide_rand  a random permutation of the same;
      ties       every raw the same negative value."""
    rng = np.random.default_rng(7919 + seed)
    q = ATT_QUANTUM
    if regime == "narrow":
        s_src, s_dst = 2 * q * rng.integers(-64, 65, n), q * (2 * rng.integers(-64, 64, n) + 1)
    elif regime in ("wide_asc", "wide_desc", "wide_rand"):
        s_src = 2 * q * np.round(np.linspace(-40.0, 40.0, n) / (2 * q))
        if regime == "wide_desc":
            s_src = s_src[::-1]
        elif regime == "wide_rand":
            s_src = rng.permutation(s_src)
        s_dst = q * (2 * rng.integers(-512, 512, n) + 1)
    elif regime == "ties":
        s_src, s_dst = np.full(n, 32 * q), np.full(n, -81 * q)
    else:
        raise ValueError(regime)
    out = []
    for s in (s_src, s_dst):
        v = np.full(cap, np.nan, np.float32)
        v[:n] = s
        assert np.array_equal(v[:n].astype(np.float64), s)
        out.append(v)
    return out[0], out[1]


def _ext_csr(rowptr, csr, n):
    """The walk of the attention kernels: every row's implied self-loop FIRST, then its entries -> (ptr [n + 1], row [E + n],
    col [E + n]) int64."""
    rowptr = np.asarray(rowptr, dtype=np.int64)[:n + 1]
    csr = np.asarray(csr, dtype=np.int64)[:rowptr[-1]]
    ptr = rowptr + np.arange(n + 1)
    row = np.repeat(np.arange(n), np.diff(ptr))
    col = np.empty(ptr[-1], np.int64)
    stored = np.ones(len(col), bool)
    stored[ptr[:-1]] = False
    col[ptr[:-1]] = np.arange(n)
    col[stored] = csr
    return ptr, row, col


def _seq_rows(ptr, f: int, terms) -> np.ndarray:
    """[n, f] fp32: for every row of the walk `ptr` the sequential fp32 sum of terms(entry ids) ([k, f] fp32) in entry order — rows
    of up to AGG_LOOP_ROWS + 1 entries all together by position-in-row, longer ones through _seq_sum_f32 (the same chain)."""
    n = len(ptr) - 1
    lens = np.diff(ptr)
    acc = np.zeros((n, f), np.float32)
    short = lens <= AGG_LOOP_ROWS + 1
    for j in range(int(min(AGG_LOOP_ROWS + 1, lens.max())) if n else 0):
        rows = np.nonzero(short & (lens > j))[0]
        acc[rows] += np.asarray(terms(ptr[rows] + j), dtype=np.float32)
    for r in np.nonzero(~short)[0]:
        acc[r] = _seq_sum_f32(np.ascontiguousarray(terms(np.arange(ptr[r], ptr[r + 1])), dtype=np.float32))
    return acc


def _row_max(v, ptr):
    return np.maximum.reduceat(v, ptr[:-1])         # (every row of an extended walk has its self-loop: no empty segment)


class GatWeights:
    """The attention weights of one graph and one pair of score vectors, which do not depend on the width: by-target walk
    (ptr, row, col; L = stored entries per row), fp64 alpha per entry, and the fp32 two-pass softmax of the baseline:
      e32 = raw > 0 ? raw : fl32(0.2f raw)  (as gat_leaky forms it; raw itself is exact),  m32 = the row's fp32 maximum,
      p32 = fl32(exp(fl64(fl32(e32 - m32))))  (widened before exp: the same on every host),  sum32 = the p32 added sequentially
      in walk order, lse32 = fl32(log(fl64(sum32))).
    S [n] = max_j |e_ij| + max_j |e_ij - m_i| in fp64, the score term of the caps.  lse_ref = log sum_j exp(e64_ij - m32_i): what
    row_ms[i, 1] must be beside a maximum of m32_i."""

    def __init__(self, rowptr, csr, s_src, s_dst, n):
        f32, f64 = np.float32, np.float64
        self.n = n
        self.s_src, self.s_dst = np.asarray(s_src, dtype=f32), np.asarray(s_dst, dtype=f32)
        self.ptr, self.row, self.col = _ext_csr(rowptr, csr, n)
        ptr, row, col = self.ptr, self.row, self.col
        self.L = np.diff(ptr) - 1
        e32, e64, _, _ = self.scores(row, col)
        self.m32 = _row_max(e32, ptr)
        self.p32 = np.exp((e32 - self.m32[row]).astype(f32).astype(f64)).astype(f32)
        self.sum32 = _seq_rows(ptr, 1, lambda idx: self.p32[idx, None])[:, 0]
        self.lse32 = np.log(self.sum32.astype(f64)).astype(f32)
        self.m64 = _row_max(e64, ptr)
        p64 = np.exp(e64 - self.m64[row])
        self.den64 = np.add.reduceat(p64, ptr[:-1])
        self.alpha64 = p64 / self.den64[row]
        self.lse_ref = np.log(np.add.reduceat(np.exp(e64 - self.m32.astype(f64)[row]), ptr[:-1]))
        self.S = _row_max(np.abs(e64), ptr) + _row_max(np.abs(e64 - self.m64[row]), ptr)

    def scores(self, i, j):
        """(e32, e64, slope32, slope64) of the entries j -> i."""
        raw32 = self.s_src[j] + self.s_dst[i]
        raw64 = self.s_src[j].astype(np.float64) + self.s_dst[i].astype(np.float64)
        assert np.array_equal(raw32.astype(np.float64), raw64), "a score sum is not exact in fp32"
        pos = raw32 > 0
        e32 = np.where(pos, raw32, GAT_SLOPE32 * raw32).astype(np.float32)
        e64 = np.where(pos, raw64, float(GAT_SLOPE32) * raw64)
        return e32, e64, np.where(pos, np.float32(1), GAT_SLOPE32), np.where(pos, 1.0, float(GAT_SLOPE32))

    def K(self):
        """The forward cap's per-row factor L + ATT_C0 + ATT_C1 S."""
        return self.L + ATT_C0 + ATT_C1 * self.S


def _named_rows64(h32, n):
    """[cap, f] fp64 with the capacity rows (NaN: no entry names them) zeroed."""
    h64 = np.asarray(h32, dtype=np.float64).copy()
    h64[n:] = 0.0
    return torch.from_numpy(h64)


def _sp64(row, col, val, n, cap):
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])), torch.from_numpy(np.asarray(val, dtype=np.float64)),
                                   (n, cap), dtype=torch.float64)


def gat_forward_sums(w: GatWeights, h):
    """out before bias and ReLU: (ref fp64, mag fp64, base fp32 numpy) with ref = sum_j alpha_ij H_j, mag = sum_j alpha_ij |H_j|
    (aggregate_finish adds the bias and the ReLU).  The baseline adds the products fl32(p32 h) sequentially in walk order (self-loop
    first) and divides once by sum32.

    The cap K = L + ATT_C0 + ATT_C1 S, first-order roundings of out = (sum p h) / (sum p) in units of u = 2^-24 of mag:
      a weight:  e = fl32(0.2f raw) errs by u |e| (exact where raw > 0), d = fl32(e - m) by u |d|, expf is documented to 1 ulp = 2 u:
                 p = exp(e - m)(1 + t), |t| <= u (|e| + |d| + 2) <= u (S + 2).  A shift of every e of a row by the same amount — the
                 error of the maximum itself, the common factor exp(m_old - m_new) of a rescale or exp(m_c - M) of the combine, which
                 multiplies accumulator and sum alike — cancels in the quotient and costs nothing.
      the quotient carries that error once in the numerator and once in the denominator:           2 S + 4
      the accumulator: L + 1 fused multiply-adds in a chain (the product is not rounded):           L
      the denominator: a butterfly of log2(64) adds, one rounding joining the running sum:          6 + 1
      the reciprocal of the sum, its product with the accumulator, and the bias:                    2 + 1
    so c1 = 2 and c0 = 4 + 7 + 3 = 14.  Not in the form: the roundings a row makes once per BATCH after the first (acc *= sc, and
    the running sum's fused multiply-add): at most 2 ceil((L + 1) / 32) - 2, a sixteenth of L.  The L of the chain is itself a
    worst case that only the row's first entries suffer and that rounding errors of alternating sign never reach; tests/
    test_attention_accuracy_cpu.py shows a faithful emulation at a fifth of the cap on every row of the cases judged."""
    n = w.n
    h32 = np.ascontiguousarray(np.asarray(h, dtype=np.float32))
    f = h32.shape[1]
    h64 = _named_rows64(h32, n)
    A = _sp64(w.row, w.col, w.alpha64, n, h32.shape[0])
    ref, mag = torch.sparse.mm(A, h64), torch.sparse.mm(A, h64.abs())
    acc = _seq_rows(w.ptr, f, lambda idx: w.p32[idx, None] * h32[w.col[idx]])
    return ref, mag, (acc / w.sum32[:, None]).astype(np.float32)


def attention_cap_excess(got, ref, capw) -> float:
    """max over the outputs of |got - ref| / (2^-24 capw): capw is K mag for an output with one factor K, or the sum of its parts'
    K |part| for one that adds up results with factors of their own (dh, da_src).  An output with capw == 0 must be 0."""
    got, ref, capw = (torch.as_tensor(v).double().cpu() for v in (got, ref, capw))
    if got.numel() == 0:
        return 0.0
    bound = U32 * capw.expand_as(ref)
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    q = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(q.max())


def row_groups(lens) -> Dict[str, np.ndarray]:
    """{"all": every row, group name: the rows whose length falls in the group} over ATT_GROUPS (empty groups left out)."""
    lens = np.asarray(lens)
    out = {"all": np.arange(len(lens))}
    for name, lo, hi in ATT_GROUPS:
        rows = np.nonzero((lens >= lo) & (lens <= hi))[0]
        if len(rows):
            out[name] = rows
    return out


def assert_attention_accuracy(got, ref, mag, base, capw, lens=None, what: str = "") -> Dict[str, Tuple[Accuracy, float]]:
    """The ratio criterion and the cap |got - ref| <= 2^-24 capw on all outputs together and, where lens [rows] is given, on every
    row group of ATT_GROUPS by itself, one [accuracy] and one [cap] line each.  -> {group: (Accuracy, cap quotient)}; every group
    is printed before the first failure is raised.
    All rows together are judged by the project's criterion unchanged.  A GROUP may be one row of one column, a single draw of the
    baseline's error, which lies anywhere between 0 and its typical size (measured: 0.05 u on the one output of a 1262-entry row at
    f = 1, where the kernel's 0.3 u then stood at a ratio of 8).  So within a group the baseline's max and rms are not taken below
    the baseline's rms over ALL outputs of the tensor, its typical error per output; the factors stay RMS_FACTOR and MAX_FACTOR, and
    the cap, which knows each row's own length, is unchanged."""
    got, ref, mag, base = (torch.as_tensor(np.asarray(v) if isinstance(v, np.ndarray) else v).cpu() for v in (got, ref, mag, base))
    capw = torch.as_tensor(capw).double().expand_as(ref)
    res, bad = {}, []
    for name, rows in (row_groups(lens) if lens is not None else {"all": slice(None)}).items():
        a = Accuracy(got[rows], ref[rows], mag[rows], base[rows])
        if name == "all":
            typical = a.base_rms
        else:       # (see the docstring: a group's baseline is not taken below the baseline's typical error over the tensor)
            a.base_max, a.base_rms = max(a.base_max, typical), max(a.base_rms, typical)
        x = attention_cap_excess(got[rows], ref[rows], capw[rows])
        print(f"[accuracy] {what} {name}: {a}")
        print(f"[cap] {what} {name}: worst |err| / (K u mag) = {x:.3f}")
        res[name] = (a, x)
        if not (a.ok() and x <= 1.0):
            bad.append(f"{what} {name}: {a}; cap x{x:.3f}")
    assert not bad, "; ".join(bad)
    return res


def gat_row_ms_excess(w: GatWeights, row_ms) -> float:
    """row_ms [n, 2] = (maximum, log of the softmax sum) of the forward.  The maximum must be the fp32 maximum of the fp32 e BIT
    FOR BIT (asserted).  Returns the worst |row_ms[:, 1] - lse_ref| / bound with the absolute bound
        (L + ATT_C0 + ATT_C1 S + 2 lse_ref) 2^-24:
    the sum's relative error is that of the forward's denominator (weights S + 2, butterfly and running sum 7, under
    L + ATT_C0 + ATT_C1 S), which is the absolute error of its logarithm, and logf adds 1 ulp = 2 u of its result."""
    r = np.asarray(row_ms, dtype=np.float32)[:w.n]
    assert np.array_equal(r[:, 0].view(np.int32), w.m32.view(np.int32)), "row_ms maximum is not the fp32 maximum of the fp32 scores"
    bound = (w.K() + 2 * w.lse_ref) * U32
    err = np.abs(r[:, 1].astype(np.float64) - w.lse_ref)
    return float(np.max(np.where(np.isnan(err), np.inf, err) / bound))


_DOT_BLOCK = 4096


def _dots(a32, ia, b32, ib):
    """Per pair k the dot product a[ia[k]] . b[ib[k]] over the columns: (fp64, fp64 of |a||b|, fp32 with the products rounded and
    added in column order)."""
    m = len(ia)
    d64, dm, d32 = np.zeros(m), np.zeros(m), np.zeros(m, np.float32)
    for k in range(0, m, _DOT_BLOCK):
        x, y = a32[ia[k:k + _DOT_BLOCK]], b32[ib[k:k + _DOT_BLOCK]]
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        d64[k:k + _DOT_BLOCK] = (x64 * y64).sum(1)
        dm[k:k + _DOT_BLOCK] = np.abs(x64 * y64).sum(1)
        d32[k:k + _DOT_BLOCK] = np.add.accumulate(x * y, axis=1, dtype=np.float32)[:, -1]
    return d64, dm, d32


def gat_backward_reference(wt: GatWeights, rowptr_s, csr_dst, h, dout, out, a_src, a_dst, bias=None, relu=False):
    """ops.gat_aggregate_bwd at aggregation level (tests/gat_oracle.gat_conv_grads restated over the entry point's own inputs):
        G = dout (where out > 0 under ReLU; `out` is the DEVICE forward's fp32 output),  c_i = G_i . (out_i - b),
        g_ij = alpha_ij (G_i . H_j - c_i) slope_ij,   ds_dst[i] = sum_j g_ij,   ds_src[j] = sum_i g_ij,
        dh_j = sum_i alpha_ij G_i + ds_src[j] a_src + ds_dst[j] a_dst,   da_src = ds_srcᵀ H,  da_dst = ds_dstᵀ H,  dbias = colsum G
    over the by-target walk of wt and the by-source walk of (rowptr_s, csr_dst), self-loop first in both.  alpha is recomputed in
    fp64 from the scores: row_ms is not read, so a wrong row_ms shows in the gradients.
    -> {"dh" | "da_src" | "da_dst" | "dbias" | "ds_src" | "ds_dst": (ref, mag, base, capw)}.
    mag: the fp64 sum of |terms|, products taken apart — sum_f |G_if| |H_jf| + sum_f |G_if| |out_if - b_f| for (G_i . H_j - c_i), and
    for dh the magnitudes of ds_src and ds_dst times |a_src|, |a_dst|.
    base: the same formulas in fp32: alpha32 = fl32(exp(fl64(fl32(fl32(e32 - m32) - lse32)))) from the baseline forward's own
    (m32, lse32), dot products with rounded products added in column order, every row sum sequential in walk order, the
    parameter gradients in row order (colsum_reference's).
    capw (first-order roundings in u = 2^-24; B_i = ceil((L_t(i) + 1) / 32) batches, lse <= log(L + 1) <= 10 here):
      alpha as the backward forms it, expf((e - m) - lse) from the stored pair: e, d and d - lse round (S_i + S_i + 10), expf 2; the
        stored lse carries the forward denominator's error (S_i + 2 + 6 + B_i) and logf's 2 lse (20):  K_a(i) = 3 S_i + B_i + 40
      G_i . H_j and c_i: a chain of ceil(F / 32) fused multiply-adds per lane and a butterfly (D = ceil(F / 32) + 6), out - b,
        the difference and two products:                                                            K_g(i) = K_a(i) + D + 4
      ds_dst[i]: L_t(i) adds;  ds_src[j]: L_s(j) adds, each term with its own K_g(i)
      dh_j: sum_i (L_s(j) + 2 + K_a(i)) alpha |G_i| + (cap of ds_src[j] + 2 its mag) |a_src| + the same for ds_dst[j]
      da_src, da_dst: sum_r (cap of ds[r] + (n + 1) its mag) |H_r|;  dbias: n mag."""
    f32, f64 = np.float32, np.float64
    n = wt.n
    h32, d32, o32 = (np.ascontiguousarray(np.asarray(v, dtype=f32)) for v in (h, dout, out))
    cap, F = h32.shape
    as32, ad32 = np.asarray(a_src, dtype=f32).reshape(-1), np.asarray(a_dst, dtype=f32).reshape(-1)
    b32 = np.zeros(F, f32) if bias is None else np.asarray(bias, dtype=f32)
    G32 = np.zeros((cap, F), f32)
    G32[:n] = np.where(o32[:n] > 0, d32[:n], f32(0)) if relu else d32[:n]
    H32 = h32.copy()
    H32[n:] = 0
    ob32 = np.zeros((cap, F), f32)
    ob32[:n] = o32[:n] - b32
    ob64 = np.zeros((cap, F))
    ob64[:n] = o32[:n].astype(f64) - b32.astype(f64)
    G64, H64 = G32.astype(f64), H32.astype(f64)
    c64, magc = (G64 * ob64).sum(1), np.abs(G64 * ob64).sum(1)
    c32 = np.add.accumulate(G32 * ob32, axis=1, dtype=f32)[:, -1]
    ptr_s, row_s, col_s = _ext_csr(rowptr_s, csr_dst, n)
    Lt, Ls = wt.L, np.diff(ptr_s) - 1
    Ka = 3 * wt.S + np.ceil((Lt + 1) / 32.0) + 40
    Kg = Ka + np.ceil(F / 32.0) + 6 + 4

    def edges(i, j):
        e32, e64, sl32, sl64 = wt.scores(i, j)
        a64 = np.exp(e64 - wt.m64[i]) / wt.den64[i]
        a32 = np.exp(((e32 - wt.m32[i]).astype(f32) - wt.lse32[i]).astype(f32).astype(f64)).astype(f32)
        dot64, dotm, dot32 = _dots(G32, i, H32, j)
        g64 = a64 * (dot64 - c64[i]) * sl64
        tm = a64 * sl64 * (dotm + magc[i])
        g32 = ((a32 * (dot32 - c32[i])).astype(f32) * sl32).astype(f32)
        return a64, a32, g64, tm, g32

    _, _, g64, tm, g32 = edges(wt.row, wt.col)
    dsd64, dsdm = np.add.reduceat(g64, wt.ptr[:-1]), np.add.reduceat(tm, wt.ptr[:-1])
    dsd32 = _seq_rows(wt.ptr, 1, lambda idx: g32[idx, None])[:, 0]
    dsdc = (Lt + Kg) * dsdm
    a64, a32, g64, tm, g32 = edges(col_s, row_s)
    dss64, dssm = np.add.reduceat(g64, ptr_s[:-1]), np.add.reduceat(tm, ptr_s[:-1])
    dss32 = _seq_rows(ptr_s, 1, lambda idx: g32[idx, None])[:, 0]
    dssc = np.add.reduceat(tm * (Ls[row_s] + Kg[col_s]), ptr_s[:-1])

    t = torch.from_numpy
    Gt, Ht = t(G64), t(H64[:n])
    as64, ad64 = t(as32.astype(f64)), t(ad32.astype(f64))
    A = _sp64(row_s, col_s, a64, n, cap)
    Ac = _sp64(row_s, col_s, a64 * (Ls[row_s] + 2 + Ka[col_s]), n, cap)
    col = lambda v: t(np.asarray(v, dtype=f64))[:, None]
    dh_ref = torch.sparse.mm(A, Gt) + col(dss64) * as64 + col(dsd64) * ad64
    dh_mag = torch.sparse.mm(A, Gt.abs()) + col(dssm) * as64.abs() + col(dsdm) * ad64.abs()
    dh_cap = torch.sparse.mm(Ac, Gt.abs()) + col(dssc + 2 * dssm) * as64.abs() + col(dsdc + 2 * dsdm) * ad64.abs()
    acc = _seq_rows(ptr_s, F, lambda idx: a32[idx, None] * G32[col_s[idx]])
    dh_base = ((acc + dss32[:, None] * as32).astype(f32) + dsd32[:, None] * ad32).astype(f32)
    res = {"dh": (dh_ref, dh_mag, t(dh_base), dh_cap),
           "ds_src": (t(dss64), t(dssm), t(dss32), t(dssc)), "ds_dst": (t(dsd64), t(dsdm), t(dsd32), t(dsdc))}
    for name, s64, sm, sc, s32 in (("da_src", dss64, dssm, dssc, dss32), ("da_dst", dsd64, dsdm, dsdc, dsd32)):
        res[name] = (t(s64) @ Ht, t(sm) @ Ht.abs(), t(_seq_sum_f32(np.ascontiguousarray(s32[:, None] * H32[:n]))),
                     t(sc + (n + 1) * sm) @ Ht.abs())
    db = colsum_reference(G32[:n])
    res["dbias"] = (db[0], db[1], db[2], float(n) * db[1])
    return res
# ----------------------------------------------------------------------------------------------------------- GATv2
GATV2_KINDS = ("normal", "zeros", "striped")
# K = L + GATV2_C0 + GATV2_C1 S of the GATv2 forward (Gatv2Weights)
GATV2_SCORE_ROUNDINGS = 15
GATV2_C0, GATV2_C1 = ATT_C0, 2 * GATV2_SCORE_ROUNDINGS
_V2_BLOCK = 2048


def gatv2_inputs(p: Dict[str, np.ndarray], heads: int, c: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """The GATv2 operands over an attention_case p of width heads * c: x_l = p["h"] rounded to an EVEN multiple of 2^-7 (zeros and
    stripes stay exact zeros), x_r = N(0,1) rounded to an ODD multiple, so that every z = x_l[j] + x_r[i] is exact in fp32 and never
    on LeakyReLU's kink; att ~ N(0,1) 0.3 [heads * c]; dout = p["dout"]; bias [heads * c] (concat; the head mean takes its first c).
    Kinds normal, zeros and striped only: there is no `mixed` kind here, because GATv2's score att . LeakyReLU(x_l + x_r) depends
    on x_l itself — rows of x_l at 10^[-4, 4] would put every score beyond exp's range."""
    q = ATT_QUANTUM
    n, cap, f = p["n"], p["cap"], heads * c
    assert p["h"].shape[1] == f
    rng = np.random.default_rng(31337 + seed)
    x_l = np.full((cap, f), np.nan, np.float32)
    x_r = np.full((cap, f), np.nan, np.float32)
    x_l[:n] = 2 * q * np.round(p["h"][:n].astype(np.float64) / (2 * q))
    x_r[:n] = q * (2 * np.round(rng.standard_normal((n, f)) / (2 * q)) + 1)
    att = (rng.standard_normal(f) * 0.3).astype(np.float32)
    return {"x_l": x_l, "x_r": x_r, "att": att, "dout": p["dout"], "bias": p["bias"]}


class Gatv2Weights:
    """Per head the attention weights of gatv2_aggregate_fwd over the by-target walk (self-loop first), [entries, heads]:
      e = sum_c att[h, c] LeakyReLU(z),  z = x_l[j] + x_r[i] (exact),  T = sum_c |att| |LeakyReLU z|
    in fp64 (alpha64, m64, den64, lse64) and for the baseline in fp32: products fl32(att fl32(LeakyReLU z)) added in column order,
    then the two-pass softmax of GatWeights (m32, p32, sum32, lse32).
    S [n, heads] = max_j |e| + max_j |e - m| + max_j T.  The forward cap is K = L + GATV2_C0 + GATV2_C1 S: as in gat_forward_sums,
    but a weight's exponent now carries the score's own rounding — the slope product, at most 4 fused multiply-adds per slab, up
    to 4 slabs and a butterfly of 6 (head_sum): 15 roundings relative to T — besides that of e - m: |t| <= u (15 T + |d| + 2) <=
    u (15 S + 2), once in the numerator and once in the denominator: GATV2_C1 = 30, GATV2_C0 = ATT_C0."""

    def __init__(self, rowptr, csr, x_l, x_r, att, heads, slope, n):
        f32, f64 = np.float32, np.float64
        self.n, self.H = n, heads
        self.x_l, self.x_r = (np.ascontiguousarray(np.asarray(v, dtype=f32)) for v in (x_l, x_r))
        self.att = np.asarray(att, dtype=f32).reshape(-1)
        self.F = self.att.size
        self.C = self.F // heads
        self.slope32 = f32(slope)
        self.ptr, self.row, self.col = _ext_csr(rowptr, csr, n)
        ptr, row = self.ptr, self.row
        self.L = np.diff(ptr) - 1
        e32, e64, T = self.scores(row, self.col)
        self.m32 = _row_max(e32, ptr)
        self.p32 = np.exp((e32 - self.m32[row]).astype(f32).astype(f64)).astype(f32)
        self.sum32 = _seq_rows(ptr, heads, lambda idx: self.p32[idx])
        self.lse32 = np.log(self.sum32.astype(f64)).astype(f32)
        self.m64 = _row_max(e64, ptr)
        p64 = np.exp(e64 - self.m64[row])
        self.den64 = np.add.reduceat(p64, ptr[:-1])
        self.alpha64 = p64 / self.den64[row]
        self.lse64 = np.log(self.den64)
        self.S = _row_max(np.abs(e64), ptr) + _row_max(np.abs(e64 - self.m64[row]), ptr) + _row_max(T, ptr)

    def leaky(self, i, j):
        """(z32, LeakyReLU z in fp32 as gv2_leaky forms it, in fp64, dLeaky/dz fp32) of the entries j -> i, [k, F]."""
        z = self.x_l[j] + self.x_r[i]
        pos = z > 0
        return z, np.where(pos, z, self.slope32 * z).astype(np.float32), np.where(pos, z.astype(np.float64), float(self.slope32) * z.astype(np.float64)), \
            np.where(pos, np.float32(1), self.slope32)

    def scores(self, i, j):
        """(e32, e64, T) [k, heads] of the entries j -> i."""
        k, H, C = len(i), self.H, self.C
        e32, e64, T = np.zeros((k, H), np.float32), np.zeros((k, H)), np.zeros((k, H))
        a64 = self.att.astype(np.float64)
        for b in range(0, k, _V2_BLOCK):
            s = slice(b, b + _V2_BLOCK)
            z, l32, l64, _ = self.leaky(i[s], j[s])
            assert np.array_equal(z.astype(np.float64), self.x_l[j[s]].astype(np.float64) + self.x_r[i[s]]), "z is not exact in fp32"
            e64[s] = (a64 * l64).reshape(-1, H, C).sum(2)
            T[s] = np.abs(a64 * l64).reshape(-1, H, C).sum(2)
            e32[s] = np.add.accumulate((self.att * l32).reshape(-1, H, C), axis=2, dtype=np.float32)[:, :, -1]
        return e32, e64, T

    def K(self):
        return self.L[:, None] + GATV2_C0 + GATV2_C1 * self.S            # [n, heads]


def _per_col(v, C):
    """[k, heads] -> [k, heads * C]: every head's value over its C columns."""
    return np.repeat(v, C, axis=1)


def gatv2_forward_reference(w: Gatv2Weights, bias=None, relu=False, concat=True):
    """ops.gatv2_aggregate_fwd -> {"out": (ref, mag, base, capw), "agg": the per-head aggregate before bias likewise}:
    agg_i[h] = sum_j alpha_ij[h] x_l[j, h];  out = agg + b (ReLU), or mean_h agg[h] + b (ReLU) with the heads added in head order and
    one division by H in the baseline (cap: the heads' own caps / H + (H + 2) mag)."""
    n, H, C, F = w.n, w.H, w.C, w.F
    cap_rows = w.x_l.shape[0]
    xl64 = _named_rows64(w.x_l, n)
    ref, mag = torch.zeros(n, F, dtype=torch.float64), torch.zeros(n, F, dtype=torch.float64)
    for h in range(H):
        A = _sp64(w.row, w.col, w.alpha64[:, h], n, cap_rows)
        cols = slice(h * C, (h + 1) * C)
        ref[:, cols], mag[:, cols] = torch.sparse.mm(A, xl64[:, cols].contiguous()), torch.sparse.mm(A, xl64[:, cols].abs().contiguous())
    acc = _seq_rows(w.ptr, F, lambda idx: _per_col(w.p32[idx], C) * w.x_l[w.col[idx]])
    base = (acc / _per_col(w.sum32, C)).astype(np.float32)
    K = torch.from_numpy(_per_col(w.K(), C))
    agg = (ref, mag, torch.from_numpy(base), K * mag)
    b32 = None if bias is None else np.asarray(bias, dtype=np.float32)[:F if concat else C]
    if concat:
        r, m, b = aggregate_finish((ref, mag, base), b32, relu)
        return {"agg": agg, "out": (r, m, b, K * m)}
    r, m = ref.view(n, H, C).sum(1) / H, mag.view(n, H, C).sum(1) / H
    capw = (K * mag).view(n, H, C).sum(1) / H + (H + 2) * m
    b = np.add.accumulate(base.reshape(n, H, C), axis=1, dtype=np.float32)[:, -1] / np.float32(H)
    r, m2, b = aggregate_finish((r, m, b.astype(np.float32)), b32, relu)
    return {"agg": agg, "out": (r, m2, b, capw + (m2 - m))}


def gatv2_row_ms_excess(w: Gatv2Weights, row_ms) -> float:
    """row_ms [n, heads, 2] = (maximum, log sum).  The kernel's score is not the baseline's bit for bit (another order of the C
    products), so the PAIR is judged: row_ms[.., 0] + row_ms[.., 1] against m64 + lse64, the logarithm of sum_j exp(e_ij), within
    (K + 2 lse64) 2^-24 + 15 u max T (the maximum's own rounding, under GATV2_C1 S) -> worst error / bound; and the maximum alone
    within 15 u max T <= 15 u S of m64."""
    r = np.asarray(row_ms, dtype=np.float64).reshape(-1, w.H, 2)[:w.n]
    bound = (w.K() + 2 * w.lse64 + GATV2_SCORE_ROUNDINGS * w.S) * U32
    err = np.abs(r[:, :, 0] + r[:, :, 1] - (w.m64 + w.lse64))
    bm = GATV2_SCORE_ROUNDINGS * w.S * U32
    errm = np.abs(r[:, :, 0] - w.m64)
    errm = np.where(bm > 0, errm / np.where(bm > 0, bm, 1.0), np.where(errm == 0, 0.0, np.inf))     # (S = 0: every score exactly 0)
    q = np.maximum(err / bound, errm)
    return float(np.max(np.where(np.isnan(q), np.inf, q)))


def gatv2_backward_reference(w: Gatv2Weights, rowptr_s, csr_dst, dout, out, agg_dev, bias=None, relu=False, concat=True):
    """ops.gatv2_aggregate_bwd (tests/gatv2_oracle.gatv2_conv_grads restated over the entry point's own inputs):
        G[i, h] = dout (where out > 0 under ReLU; / H for the head mean),  c[i, h] = G[i, h] . A[i, h],  A = out - b (concat) or the
        forward's saved per-head aggregate,  de_ij[h] = alpha_ij[h] (G[i, h] . x_l[j, h] - c[i, h]),  dz_ij = de att (z > 0 ? 1 : slope),
        dx_r[i] = sum_j dz_ij,  dx_l[j] = sum_i alpha_ij G_i + dz_ij,  datt = sum_ij de_ij LeakyReLU(z_ij),  dbias = colsum of the gated dout
    -> {"dx_l" | "dx_r" | "datt" | "dbias": (ref, mag, base, capw)}; `out` and `agg_dev` are the DEVICE forward's; alpha is recomputed
    in fp64 from x_l, x_r, att (row_ms is not read).  mag: sums of |terms| with the products taken apart, as gat_backward_reference.
    base: the same formulas in fp32 — alpha32 = fl32(exp(fl64(fl32(fl32(e32 - m32) - lse32)))), dot products in column order, row
    sums in walk order, datt over all entries in by-target walk order, dbias in row order (head mean: every head's column sum of
    fl32(g fl32(1 / H)), the heads added in head order, as gatv2_bwd_rows_k and gatv2_bwd_params_final_k form it).
    capw, in u = 2^-24 (B_i = ceil((L_t(i) + 1) / 32), lse <= 10):
      alpha from the stored pair: K_a = 3 * 15 S + B_i + 40 (gat_backward_reference's K_a with the score's 15 roundings in S);
      de: + the two C-term dot products (at most 15 roundings each, as the score's), the difference, the product, G / H:  K_e = K_a + 20
      dz = de att slope': + 2;  dx_r[i]: L_t(i) adds;  dx_l[j]: 2 L_s(j) adds (two terms per entry);  datt: E + n adds and
      LeakyReLU's product;  dbias: n mag."""
    f32, f64 = np.float32, np.float64
    n, H, C, F = w.n, w.H, w.C, w.F
    cap_rows = w.x_l.shape[0]
    W = F if concat else C
    d32, o32 = np.asarray(dout, dtype=f32)[:n, :W], np.asarray(out, dtype=f32)[:n]
    g = np.where(o32 > 0, d32, f32(0)) if relu else d32
    G32 = np.zeros((cap_rows, F), f32)
    G32[:n] = g if concat else np.tile((g * (f32(1) / f32(H))).astype(f32), (1, H))
    G64 = np.zeros((cap_rows, F))
    G64[:n] = g.astype(f64) if concat else np.tile(g.astype(f64) / H, (1, H))
    A32 = np.zeros((cap_rows, F), f32)
    if concat:
        b32 = np.zeros(F, f32) if bias is None else np.asarray(bias, dtype=f32)[:F]
        A32[:n] = o32 - b32
        A64 = np.zeros((cap_rows, F))
        A64[:n] = o32.astype(f64) - b32.astype(f64)
    else:
        A32[:n] = np.asarray(agg_dev, dtype=f32)[:n]
        A64 = A32.astype(f64)
    hs = lambda v: v.reshape(-1, H, C)
    c64, magc = hs(G64 * A64).sum(2), hs(np.abs(G64 * A64)).sum(2)
    c32 = np.add.accumulate(hs(G32 * A32), axis=2, dtype=f32)[:, :, -1]
    ptr_s, row_s, col_s = _ext_csr(rowptr_s, csr_dst, n)
    Lt, Ls = w.L, np.diff(ptr_s) - 1
    Ka = 3 * GATV2_SCORE_ROUNDINGS * w.S + np.ceil((Lt + 1) / 32.0)[:, None] + 40
    Ke = Ka + 20
    a64t, a32t = w.att.astype(f64), w.att
    xl32 = w.x_l.copy(); xl32[n:] = 0
    t = torch.from_numpy

    def walk(i, j, ptr, out_rows, Lrow, with_alpha_g, want_datt):
        """One walk over the entries j -> i: the row sums over `out_rows` of dz (+ alpha G) as (ref, mag, capw) fp64 [n, F], the
        per-entry fp32 scalars (alpha32, de32) for the baseline, and datt's (ref, mag, capw, base)."""
        k = len(i)
        ref, mag, cw = (torch.zeros(n, F, dtype=torch.float64) for _ in range(3))
        al32, de32 = np.zeros((k, H), f32), np.zeros((k, H), f32)
        da = [np.zeros(F), np.zeros(F), np.zeros(F), np.zeros(F, f32)]
        rows_t = t(out_rows)
        e32, e64, _ = w.scores(i, j)
        for b in range(0, k, _V2_BLOCK):
            s = slice(b, b + _V2_BLOCK)
            ii, jj = i[s], j[s]
            a64 = np.exp(e64[s] - w.m64[ii]) / w.den64[ii]
            a32 = np.exp(((e32[s] - w.m32[ii]).astype(f32) - w.lse32[ii]).astype(f32).astype(f64)).astype(f32)
            gx = G64[ii] * xl32[jj].astype(f64)
            dot64, dotm = hs(gx).sum(2), hs(np.abs(gx)).sum(2)
            dot32 = np.add.accumulate(hs(G32[ii] * xl32[jj]), axis=2, dtype=f32)[:, :, -1]
            de64 = a64 * (dot64 - c64[ii])
            tm = a64 * (dotm + magc[ii])
            d32_ = (a32 * (dot32 - c32[ii])).astype(f32)
            al32[s], de32[s] = a32, d32_
            z, l32, l64, sl32 = w.leaky(ii, jj)
            sl64 = sl32.astype(f64)
            dz = _per_col(de64, C) * a64t * sl64
            dzm = _per_col(tm, C) * np.abs(a64t) * sl64
            dzc = _per_col(tm * (Ke[ii] + 2 + Lrow[out_rows[s]][:, None] * (2 if with_alpha_g else 1)), C) * np.abs(a64t) * sl64
            if with_alpha_g:
                ag = _per_col(a64, C) * np.abs(G64[ii])
                dz = dz + _per_col(a64, C) * G64[ii]
                dzm = dzm + ag
                dzc = dzc + _per_col(Ka[ii] + 1 + 2 * Lrow[out_rows[s]][:, None], C) * ag
            ref.index_add_(0, rows_t[s], t(dz)); mag.index_add_(0, rows_t[s], t(dzm)); cw.index_add_(0, rows_t[s], t(dzc))
            if want_datt:
                da[0] += (_per_col(de64, C) * l64).sum(0)
                da[1] += (_per_col(tm, C) * np.abs(l64)).sum(0)
                da[2] += (_per_col(tm * (Ke[ii] + 2 + k), C) * np.abs(l64)).sum(0)
                terms = np.concatenate([da[3][None], _per_col(d32_, C) * l32])
                da[3] = _seq_sum_f32(np.ascontiguousarray(terms, dtype=f32))
        return (ref, mag, cw), al32, de32, da

    def dz32(i, j, de):
        _, _, _, sl32 = w.leaky(i, j)
        return ((_per_col(de, C) * a32t).astype(f32) * sl32).astype(f32)

    (r_ref, r_mag, r_cw), _, de_t, da = walk(w.row, w.col, w.ptr, w.row, Lt, False, True)
    r_base = _seq_rows(w.ptr, F, lambda idx: dz32(w.row[idx], w.col[idx], de_t[idx]))
    (l_ref, l_mag, l_cw), al_s, de_s, _ = walk(col_s, row_s, ptr_s, row_s, Ls, True, False)
    l_base = _seq_rows(ptr_s, F, lambda idx: (dz32(col_s[idx], row_s[idx], de_s[idx]) + _per_col(al_s[idx], C) * G32[col_s[idx]]).astype(f32))
    res = {"dx_r": (r_ref, r_mag, t(r_base), r_cw), "dx_l": (l_ref, l_mag, t(l_base), l_cw),
           "datt": (t(da[0]), t(da[1]), t(da[3]), t(da[2]))}
    db = colsum_reference(g)
    if not concat:      # the head mean hands every head fl32(g fl32(1 / H)) and adds the heads' column sums in head order
        part = _seq_sum_f32(np.ascontiguousarray((g * (f32(1) / f32(H))).astype(f32)))
        db = (db[0], db[1], t(np.add.accumulate(np.tile(part, (H, 1)), axis=0, dtype=f32)[-1].copy()))
    res["dbias"] = (db[0], db[1], db[2], float(n + H + 2) * db[1])
    return res


# --------------------------------------------------------------------------------------------- plain fp32 dense GEMMs
# grapes_amd/csrc/gemm_kernels.hip: grapes_linear_fwd / _fwd_row_scaled / _bias_act_fwd / _bwd_input / _bwd_weight and the
# few-row slab path (grapes_linear_bwd_weight_slabs[_and_input] + grapes_slab_reduce_sets).  Same criterion as above: each
# output relative to the fp64 sum of |a||b| of ITS OWN terms, the ratio test against a fixed-order fp32 baseline, and beside it
# the hard cap |got - ref| <= (L + extra) 2^-24 mag (hard_cap_excess with a scalar L: the contraction length).
#   baseline of the forward forms and the input gradient: ONE sequential fp32 chain in k order (product rounded, then added) —
#     the order of the tiled kernel's single accumulator.  fp32_contract's 128-blocks are 4-6x more accurate than that chain at
#     K = 1433, so under them a correct tiled kernel would miss RMS_FACTOR;
#   baseline of the weight gradient (the contraction runs over the rows): fp32_contract, as for every dW test here.
GB_TILE, GB_K = 128, 16                 # gemm_mfma_f32_k: tile edge, K step
SK_KMAX, SK_MAX_ROWS = 256, 4096        # gemm_skinny_f32_k takes host row counts <= 4096 and 1 <= K <= 256
DWS_ROWS = 128                          # rows per slab of gemm_dw_small_k
DW_BLOCKS_TARGET = 512                  # dw_nslab: slabs x output tiles


def skinny_ok(rows: int, K: int) -> bool:
    return rows <= SK_MAX_ROWS and 1 <= K <= SK_KMAX


def dw_nslab(f_out: int, f_in: int) -> int:
    return max(1, DW_BLOCKS_TARGET // (-(-f_out // GB_TILE) * -(-f_in // GB_TILE)))


def dw_small_ok(rows: int, f_out: int, f_in: int) -> bool:
    return rows <= SK_MAX_ROWS and -(-rows // DWS_ROWS) <= dw_nslab(f_out, f_in)


def auto_kchunk(K: int, nslab: int) -> int:
    kc = -(-K // nslab)
    kc = (kc + 1) & ~1
    return max(kc, 16)


def wsplit_ok(K: int, N: int) -> bool:
    """Shapes of the bf16x3 forward (aligned operands taken for granted): grapes_linear_bias_act_fwd takes it at >= 2048 rows."""
    return K % 4 == 0 and 4 <= K <= 192 and N % 32 == 0 and 32 <= N <= 256


def dense_route(entry: str, rows: int, f_in: int, f_out: int) -> str:
    """The kernel an entry point hands a HOST row count `rows` (the capacity: dispatch never sees the device-side count) to."""
    if entry in ("fwd", "fwd_row_scaled", "bias_act"):
        if entry == "fwd" and f_out == 1:
            return "gemv"
        if entry == "bias_act" and rows >= 2048 and wsplit_ok(f_in, f_out):
            return "wsplit"
        return "skinny" if skinny_ok(rows, f_in) else "tiled"
    if entry == "bwd_input":
        if f_out == 1:
            return "outer"
        return "skinny" if skinny_ok(rows, f_out) else "tiled"
    if entry == "bwd_weight":
        if f_out == 1:
            return "colsum"
        return "dw_small" if dw_small_ok(rows, f_out, f_in) else "split_k"
    raise ValueError(entry)


def dense_vec(entry: str, f_in: int, f_out: int, aligned: bool = True) -> bool:
    """launch_gemm's `vec` for the tiled kernels of an entry point: both leading dimensions % 4 == 0 and 16-byte bases."""
    lda, ldb = {"bwd_input": (f_out, f_in), "bwd_weight": (f_out, f_in)}.get(entry, (f_in, f_in))
    return aligned and lda % 4 == 0 and ldb % 4 == 0


class DenseCase:
    """One shape of the dense accuracy tests: (rows live on the device, f_in, f_out), `pad` capacity rows past them (the host
    count is rows + pad), the kernel the host count must reach, the kinds it runs on and an operand to misalign."""

    def __init__(self, entry, kernel, rows, f_in, f_out, pad=3, kinds=KINDS, unaligned=None, vec=None, note=""):
        self.entry, self.kernel, self.rows, self.f_in, self.f_out = entry, kernel, rows, f_in, f_out
        self.pad, self.kinds, self.unaligned, self.vec, self.note = pad, tuple(kinds), unaligned, vec, note

    @property
    def cap(self) -> int:
        return self.rows + self.pad

    @property
    def id(self) -> str:
        s = f"{self.kernel}-{self.rows}x{self.f_in}x{self.f_out}"
        if self.pad != 3:
            s += f"+{self.pad}"
        return s + (f"-off_{self.unaligned}" if self.unaligned else "")

    def check_route(self):
        """The shape is on the intended side of every dispatch boundary."""
        got = dense_route(self.entry, self.cap, self.f_in, self.f_out)
        assert got == self.kernel, f"{self.id}: host count {self.cap} reaches {got}, not {self.kernel}"
        if self.vec is not None:
            assert dense_vec(self.entry, self.f_in, self.f_out, self.unaligned is None) == self.vec, self.id
        if self.kernel == "tiled" and self.note.startswith("mt"):
            mt = -(-self.cap // GB_TILE)
            assert (mt >= 8) == (self.note == "mt>=8"), f"{self.id}: mt = {mt}"


def _dc(entry, kernel, shapes, **kw):
    return [DenseCase(entry, kernel, *s, **kw) for s in shapes]


DENSE_CASES: Dict[str, list] = {
    # ---- grapes_linear_fwd
    "fwd": (
        # gemv_rows_k: the float4 loop's trip count (260: a second trip), the scalar loop, the grid cap's stride loop
        _dc("fwd", "gemv", [(1029, 1, 1), (1029, 3, 1), (1029, 8, 1), (1029, 103, 1), (1029, 256, 1), (1029, 260, 1),
                            (1, 103, 1), (4, 103, 1), (5, 103, 1)])
        + _dc("fwd", "gemv", [(1029, 256, 1)], unaligned="x")
        + _dc("fwd", "gemv", [(32773, 8, 1)])
        # gemm_skinny_f32_k<false>: K around the quarter split, rows around a 32-row tile, f_out around a 64-column tile
        + _dc("fwd", "skinny", [(33, 1, 2), (31, 3, 63), (32, 4, 64), (33, 5, 65), (1, 13, 130), (33, 13, 7), (31, 47, 65),
                                (130, 47, 2), (33, 255, 63), (32, 256, 64), (1, 256, 65), (259, 255, 130)])
        + _dc("fwd", "skinny", [(4096, 256, 64), (4096, 47, 65)], pad=0)
        + _dc("fwd", "skinny", [(33, 48, 65)], unaligned="x") + _dc("fwd", "skinny", [(33, 48, 66)], unaligned="w")
        # gemm_mfma_f32_k<false, false>
        + _dc("fwd", "tiled", [(130, 260, 130)], vec=True, note="mt<8")           # 17 K-steps, mt = 2
        + _dc("fwd", "tiled", [(129, 1433, 7)], vec=False, note="mt<8")            # scalar loads, 90 K-steps
        + _dc("fwd", "tiled", [(1030, 272, 136)], vec=True, note="mt>=8")          # mt = 9: the XCD-aware map, idle padded blocks
        + _dc("fwd", "tiled", [(4100, 16, 130), (4100, 20, 64), (4100, 48, 40)], vec=True, note="mt>=8")  # 1, 2, 3 K-steps
        + _dc("fwd", "tiled", [(100, 20, 64)], pad=4100, vec=True, note="mt>=8")   # capacity 4200, 100 live: most blocks return
    ),
    # ---- grapes_linear_fwd_row_scaled
    "fwd_row_scaled": (
        _dc("fwd_row_scaled", "skinny", [(33, 47, 65)]) + _dc("fwd_row_scaled", "skinny", [(4096, 256, 64)], pad=0)
        + _dc("fwd_row_scaled", "tiled", [(4100, 20, 64)], vec=True) + _dc("fwd_row_scaled", "tiled", [(130, 260, 130)], vec=True)
    ),
    # ---- grapes_linear_bias_act_fwd (each with bias on/off x ReLU on/off)
    "bias_act": (
        _dc("bias_act", "skinny", [(33, 47, 65)]) + _dc("bias_act", "skinny", [(2047, 104, 256)], pad=0)
        + _dc("bias_act", "tiled", [(4100, 20, 72)], vec=True) + _dc("bias_act", "tiled", [(130, 260, 130)], vec=True)
    ),
    # ---- grapes_linear_bwd_input
    "bwd_input": (
        _dc("bwd_input", "outer", [(5, 7, 1)]) + _dc("bwd_input", "outer", [(8200, 257, 1)])
        # gemm_skinny_f32_k<true>: K = f_out; f_in % 4 decides the k-major B tile's vector / scalar loads
        + _dc("bwd_input", "skinny", [(33, 3, 2), (31, 64, 5), (33, 65, 47), (130, 130, 256), (1, 64, 47), (259, 64, 256),
                                      (32, 3, 256), (33, 130, 5)])
        + _dc("bwd_input", "tiled", [(4100, 130, 20)], vec=False)
        + _dc("bwd_input", "tiled", [(130, 100, 260)], vec=True) + _dc("bwd_input", "tiled", [(129, 103, 262)], vec=False)
    ),
    # ---- grapes_linear_bwd_weight (each fresh and accumulated)
    "bwd_weight": (
        _dc("bwd_weight", "colsum", [(1, 103, 1), (129, 1, 1), (129, 256, 1), (9000, 103, 1), (9000, 256, 1), (1, 1, 1)])
        # gemm_dw_small_k + slab_reduce_k: 1 .. 32 slabs, ragged last slab, tiles around 32 x 64
        + _dc("bwd_weight", "dw_small", [(1, 13, 7), (127, 63, 31), (128, 64, 32), (129, 65, 33), (1022, 256, 256), (1022, 64, 32),
                                         (129, 256, 256), (127, 13, 7), (128, 65, 33)])
        + _dc("bwd_weight", "dw_small", [(4096, 13, 7), (4096, 256, 256)], pad=0)
        # gemm_mfma_f32_k<true, true> in split-K form + slab_reduce_k
        + _dc("bwd_weight", "split_k", [(4100, 20, 8)], vec=True)        # chunk floor 16: 257 live slabs of 512
        + _dc("bwd_weight", "split_k", [(8200, 20, 8)], vec=True)        # chunk 18: a second K-step of 2 rows
        + _dc("bwd_weight", "split_k", [(4097, 260, 130)], vec=False)    # 6 tiles -> 85 slabs
        + _dc("bwd_weight", "split_k", [(4100, 103, 7)], vec=False)      # scalar loads
        + _dc("bwd_weight", "split_k", [(100, 20, 8)], pad=4100, vec=True)         # capacity 4200, 100 live
    ),
}
# the deferred slab path: layers (f_in, f_out, form) over one row count; form: plain dW, gated dW + dbias, dW + dx (pair launch)
SLAB_ROWS = (129, 1022)
SLAB_LAYERS = ((65, 33, "dw"), (64, 32, "gated"), (13, 7, "pair"))
SLAB_MANY = (129, 13, 7, 9)     # (rows, f_in, f_out, layers): more than 8 sets force DeferredSlabs' internal flush


def dense_problem(n: int, K: int, N: int, kind: str, seed: int, n_pad: int = 0) -> Dict[str, np.ndarray]:
    """The operands of every dense entry point over n live rows (capacity n + n_pad), fp32:
      forward           x [cap, K], w [N, K], bias [N], row_scale [cap] (signs mixed, magnitudes 10^[-6, 6]);
      input gradient    dh_in [cap, N], w_in [N, K]                       (dx = dh_in w_in, contraction over N);
      weight gradient   dh [cap, N], x_dw [cap, K], gate [cap, N] (an input: kept where > 0), prior_dw [N, K], prior_db [N].
    kind:
      normal  N(0,1); the three roles share x = x_dw, w = w_in, dh = dh_in.
      mixed   the contraction index carries the magnitude, products stay within 10^[-3, 3]:
              forward: column k of x at 10^a_k and column k of w at 10^(-a_k + c_k); input gradient: column j of dh_in at 10^a_j,
              row j of w_in at 10^(-a_j + c_j); weight gradient: row r of x_dw at 10^a_r, row r of dh at 10^(-a_r + c_r);
              a in [-20, 20], c in [-3, 3], each role its own draw (one array cannot carry two roles' scales: 10^40 overflows).
      zeros   N(0,1) with exact zeros: whole rows of x / dh (n >= 3), a column of x and of dh (K, N >= 3), single entries, one
              row and one column of w (N, K >= 3), entries of row_scale and gate.  Outputs whose terms all vanish must be 0.
    Rows past n are NaN in x, x_dw, dh, dh_in, row_scale and gate."""
    if kind not in KINDS:
        raise ValueError(kind)
    rng = np.random.default_rng(seed)
    cap = n + n_pad
    g = lambda *s: rng.standard_normal(s)
    x, w, dh = g(cap, K), g(N, K) / np.sqrt(K), g(cap, N)
    x_dw, w_in, dh_in = x, w, dh
    if kind == "mixed":
        a = rng.uniform(-20, 20, K)
        x = x * 10.0 ** a
        w = w * 10.0 ** (-a + rng.uniform(-3, 3, K))
        a = rng.uniform(-20, 20, N)
        dh_in = g(cap, N) * 10.0 ** a
        w_in = (g(N, K) / np.sqrt(K)) * (10.0 ** (-a + rng.uniform(-3, 3, N)))[:, None]
        a = rng.uniform(-20, 20, cap)
        x_dw = g(cap, K) * (10.0 ** a)[:, None]
        dh = dh * (10.0 ** (-a + rng.uniform(-3, 3, cap)))[:, None]
    row_scale = rng.choice([-1.0, 1.0], cap) * 10.0 ** rng.uniform(-6, 6, cap)
    gate = g(cap, N)
    if kind == "zeros":
        if n >= 3:
            x[rng.integers(0, n, max(1, n // 50))] = 0.0
            dh[rng.integers(0, n, max(1, n // 50))] = 0.0
            row_scale[rng.integers(0, n, max(1, n // 50))] = 0.0
        x[rng.integers(0, n, n), rng.integers(0, K, n)] = 0.0
        dh[rng.integers(0, n, n), rng.integers(0, N, n)] = 0.0
        gate[rng.integers(0, n, n), rng.integers(0, N, n)] = 0.0
        if K >= 3:
            x[:, K // 2] = 0.0
            w[:, K - 1] = 0.0
        if N >= 3:
            dh[:, N // 2] = 0.0
            w[N - 1] = 0.0
    for v in (x, x_dw, dh, dh_in, gate):
        v[n:] = np.nan
    row_scale[n:] = np.nan
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    return {"x": f(x), "w": f(w), "bias": f(g(N) * 0.5), "row_scale": f(row_scale), "dh_in": f(dh_in), "w_in": f(w_in),
            "dh": f(dh), "x_dw": f(x_dw), "gate": f(gate), "prior_dw": f(g(N, K)), "prior_db": f(g(N)), "n": n, "cap": cap}


def _seq_chain(a: torch.Tensor, bt: torch.Tensor, k0: int, k1: int, fma: bool = False) -> torch.Tensor:
    """sum_{k0 <= k < k1} a[:, k] (x) bt[:, k] as ONE fp32 chain in k order, element-wise ops only.  fma: each step one fused
    multiply-add (the product exact in fp64, one rounding per step; the double rounding moves tie cases only)."""
    acc = torch.zeros(a.shape[0], bt.shape[0])
    if fma:
        a, bt = a.double(), bt.double()
        for k in range(k0, k1):
            acc = (acc.double() + a[:, k, None] * bt[None, :, k]).float()
        return acc
    for k in range(k0, k1):
        acc += a[:, k, None] * bt[None, :, k]
    return acc


def dense_epilogue(out: torch.Tensor, bias=None, relu=False, row_scale=None, bias_twice=False, scale_shift=False):
    """+ bias, ReLU, x row_scale in the kernels' order, in out's precision (fp32 emulation / baseline, or fp64 reference)."""
    if bias is not None:
        b = torch.as_tensor(np.asarray(bias, dtype=np.float32)).to(out.dtype)
        out = out + b
        if bias_twice:
            out = out + b
    if relu:
        out = out.clamp(min=0)
    if row_scale is not None:
        s = torch.as_tensor(np.asarray(row_scale, dtype=np.float32)).to(out.dtype)
        out = out * (torch.roll(s, 1) if scale_shift else s)[:, None]
    return out


def dense_fwd_reference(a, bt, bias=None, relu=False, row_scale=None):
    """out = rowscale ⊙ act(a btᵀ + bias) for a [n, K], bt [N, K] (the forward forms; the input gradient with a = dh,
    bt = wᵀ) -> (ref, mag, base): mag = |a||bt|ᵀ + |bias|, times |row_scale| (the pre-activation's: ReLU is 1-Lipschitz);
    base = the sequential fp32 chain in k order, then the same epilogue in fp32."""
    a64, b64 = _t64(a), _t64(bt)
    ref = dense_epilogue(a64 @ b64.T, bias, relu, row_scale)
    mag = dense_epilogue(a64.abs() @ b64.abs().T, None if bias is None else np.abs(bias), False,
                         None if row_scale is None else np.abs(row_scale))
    base = dense_epilogue(_seq_chain(_f32(a), _f32(bt), 0, a64.shape[1]), bias, relu, row_scale)
    return ref, mag, base


def dense_dw_reference(dh, x, gate=None, prior_dw=None, prior_db=None):
    """dW = (dh ⊙ [gate > 0])ᵀ x and db = its column sums over the rows given (+ priors) -> {"dw" | "db": (ref, mag, base)};
    base = fp32_contract (+ prior in fp32, the buffer first: o + t)."""
    d32 = np.asarray(dh, dtype=np.float32)
    if gate is not None:
        d32 = np.where(np.asarray(gate) > 0, d32, np.float32(0))
    d64, x64 = _t64(d32), _t64(x)
    ones = np.ones((d32.shape[0], 1), np.float32)
    out = {"dw": [d64.T @ x64, d64.abs().T @ x64.abs(), fp32_contract(d32, x)],
           "db": [d64.sum(0), d64.abs().sum(0), fp32_contract(d32, ones).view(-1)]}
    for k, p in (("dw", prior_dw), ("db", prior_db)):
        if p is not None:
            p64, p32 = _t64(p), _f32(p)
            out[k] = [out[k][0] + p64, out[k][1] + p64.abs(), p32 + out[k][2]]
    return {k: tuple(v) for k, v in out.items()}


def dense_accuracy(got, ref, mag, base, L: int, extra: int = 4) -> Tuple[Accuracy, float]:
    """(the ratio criterion's numbers, worst |got - ref| / ((L + extra) 2^-24 mag)) of one output tensor: the two pass conditions
    of the dense GEMMs (dense_ok).  L is the contraction length (K, or the live row count of a weight gradient): the gamma_L bound
    of an L-term fp32 dot product in any order, with room for bias, row scale, accumulation and the store."""
    return Accuracy(got, ref, mag, base), hard_cap_excess(got, ref, mag, float(L), extra)


def dense_ok(a: Accuracy, cap: float) -> bool:
    return a.ok() and cap <= 1.0


def normwise_ok(got, ref, tol: float = 2e-5) -> bool:
    """The bound of test_hip_parity.py's dense tests: max|got - ref| <= tol max(1, max|ref|)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return bool((got - ref).abs().max() <= tol * max(1.0, float(ref.abs().max())))


# ---- the kernels' summation orders, plain torch fp32.  defect= seeds one fault (tests/test_dense_gemm_accuracy_cpu.py)
def emulate_tiled(a, bt, bias=None, relu=False, row_scale=None, defect=None, fma=False) -> torch.Tensor:
    """gemm_mfma_f32_k: one accumulator per output, K streamed in order -> one chain over k; bias, ReLU, row scale after it.
    defect: "drop_partial_kstep" (the K % 16 terms of the last, partial K-step lost), "bias_twice", "scale_shift"."""
    a, bt = _f32(a), _f32(bt)
    K = a.shape[1]
    k1 = K - K % GB_K if defect == "drop_partial_kstep" else K
    return dense_epilogue(_seq_chain(a, bt, 0, k1, fma), bias, relu, row_scale, defect == "bias_twice", defect == "scale_shift")


def emulate_gemv(a, w, vec: bool) -> torch.Tensor:
    """gemv_rows_k: a wavefront per row; lane l chains fused multiply-adds over its elements (vec: the float4s at 4 l + 256 t,
    else the floats at l + 64 t), then the xor butterfly 32, 16, .. 1, of which lane 0's value is stored.  -> [n, 1]"""
    a, w = _f32(a), _f32(w).view(-1)
    n, F = a.shape
    step = 256 if vec else 64
    Fp = -(-F // step) * step
    p = torch.nn.functional.pad(a.double() * w.double(), (0, Fp - F))         # exact products
    p = p.view(n, Fp // step, 64, 4) if vec else p.view(n, Fp // step, 64, 1)
    acc = torch.zeros(n, 64)
    for t in range(p.shape[1]):
        for j in range(p.shape[3]):
            acc = (acc.double() + p[:, t, :, j]).float()
    lanes = torch.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ d]
    return acc[:, :1].clone()


def skinny_quarters(K: int):
    """[(k0, k1)] x 4: the k ranges of gemm_skinny_body's four wavefront groups (quads of 4 k, ceil(KQ / 4) quads each)."""
    KQ = -(-K // 4)
    per = -(-KQ // 4)
    return [(min(4 * q * per, K), min(4 * min((q + 1) * per, KQ), K)) for q in range(4)]


def _skinny_sum(a, bt, defect=None, fma=False) -> torch.Tensor:
    qs = skinny_quarters(a.shape[1])
    if defect == "drop_quad":           # the last quad of the last non-empty quarter never reaches the accumulator
        j = max(i for i, (k0, k1) in enumerate(qs) if k1 > k0)
        k0, k1 = qs[j]
        qs[j] = (k0, max(k0, k1 - ((k1 - k0 - 1) % 4 + 1)))
    p = [_seq_chain(a, bt, k0, k1, fma) for k0, k1 in qs]
    return ((p[0] + p[1]) + p[2]) + p[3]


def emulate_skinny(a, bt, bias=None, relu=False, row_scale=None, defect=None, fma=False) -> torch.Tensor:
    """gemm_skinny_f32_k: four k ranges (skinny_quarters), each one chain, combined ((q0 + q1) + q2) + q3, then bias and ReLU;
    the row scale is scale_rows_few_k's pass over the stored product.  defect: "drop_quad", "bias_twice", "scale_shift"."""
    out = _skinny_sum(_f32(a), _f32(bt), defect, fma)
    return dense_epilogue(out, bias, relu, row_scale, defect == "bias_twice", defect == "scale_shift")


def emulate_slab_reduce(slabs: torch.Tensor, prior=None, defect=None) -> torch.Tensor:
    """slab_reduce_k / slab_reduce_sets_k over slabs [ns, ...]: four contiguous quarters of ceil(ns / 4) slabs, each added in slab
    order from 0, combined (p0 + p1) + (p2 + p3), then prior + t.  defect: "drop_last_slab" (the last slab of the first
    quarter), "slab_twice" (slab 0 added again), "overwrite" (the prior lost)."""
    ns = slabs.shape[0]
    per = -(-ns // 4)
    p = []
    for g in range(4):
        z0, z1 = min(g * per, ns), min(g * per + per, ns)
        if defect == "drop_last_slab" and g == 0:
            z1 -= 1
        acc = torch.zeros(slabs.shape[1:])
        for z in range(z0, z1):
            acc = acc + slabs[z]
        if defect == "slab_twice" and g == 0:
            acc = acc + slabs[0]
        p.append(acc)
    t = (p[0] + p[1]) + (p[2] + p[3])
    if prior is None or defect == "overwrite":
        return t
    return _f32(prior) + t


def _live(dh, x, gate, n, defect):
    """The live rows' operands (the gate applied); "read_capacity": the first capacity row taken as live."""
    m = n + 1 if defect == "read_capacity" else n
    d = _f32(np.asarray(dh)[:m])
    if gate is not None:
        d = torch.where(_f32(np.asarray(gate)[:m]) > 0, d, torch.zeros(()))
    return d, _f32(np.asarray(x)[:m]), m


def emulate_dw_small(dh, x, n: int, gate=None, prior=None, defect=None, fma=False, want="dw") -> torch.Tensor:
    """gemm_dw_small_k + the slab reduction: 128-row slabs, each summed over its rows in the skinny order (four quarters of 32
    rows; rows past the live count are zeros), the slabs then by emulate_slab_reduce.  want = "db": the column sums that ride
    along (an MFMA against ones: the same order).  dh, x: the capacity arrays (their first n rows are read)."""
    d, xs, m = _live(dh, x, gate, n, defect)
    if want == "db":
        xs = torch.ones(m, 1)
    ns = -(-m // DWS_ROWS)
    pad = ns * DWS_ROWS - m
    A = torch.nn.functional.pad(d, (0, 0, 0, pad)).view(ns, DWS_ROWS, -1)
    B = torch.nn.functional.pad(xs, (0, 0, 0, pad)).view(ns, DWS_ROWS, -1)
    q = []
    for k0 in range(0, DWS_ROWS, DWS_ROWS // 4):
        acc = torch.zeros(ns, A.shape[2], B.shape[2])
        for k in range(k0, k0 + DWS_ROWS // 4):
            t = A[:, k, :, None].double() * B[:, k, None, :].double() if fma else A[:, k, :, None] * B[:, k, None, :]
            acc = (acc.double() + t).float() if fma else acc + t
        q.append(acc)
    slabs = ((q[0] + q[1]) + q[2]) + q[3]
    out = emulate_slab_reduce(slabs, prior, defect)
    return out.view(-1) if want == "db" else out


def emulate_split_k(dh, x, n: int, prior=None, defect=None, fma=False) -> torch.Tensor:
    """grapes_linear_bwd_weight's tiled split-K form: nslab = max(1, 512 // tiles) slabs requested, the chunk from the live
    count (auto_kchunk), every live slab one chain over its rows, then the slab reduction.  defect "drop_partial_kstep": each
    chunk loses the rows of its last, partial 16-row step."""
    d, xs, m = _live(dh, x, None, n, defect)
    N, K = d.shape[1], xs.shape[1]
    kc = auto_kchunk(m, dw_nslab(N, K))
    ns = -(-m // kc)
    pad = ns * kc - m
    A = torch.nn.functional.pad(d, (0, 0, 0, pad)).view(ns, kc, N)
    B = torch.nn.functional.pad(xs, (0, 0, 0, pad)).view(ns, kc, K)
    steps = kc - kc % GB_K if defect == "drop_partial_kstep" else kc
    acc = torch.zeros(ns, N, K)
    for k in range(steps):
        t = A[:, k, :, None].double() * B[:, k, None, :].double() if fma else A[:, k, :, None] * B[:, k, None, :]
        acc = (acc.double() + t).float() if fma else acc + t
    return emulate_slab_reduce(acc, prior, defect)


def dense_case_refs(case: DenseCase, p, bias=False, relu=False, accumulate=False):
    """{output: (ref, mag, base, L, extra)} of one DenseCase on dense_problem p: L the contraction length of the hard cap."""
    n, e = p["n"], case.entry
    if e in ("fwd", "fwd_row_scaled", "bias_act"):
        scaled = e == "fwd_row_scaled"
        r = dense_fwd_reference(p["x"][:n], p["w"], p["bias"] if bias else None, relu, p["row_scale"][:n] if scaled else None)
        return {"out": r + (case.f_in, 5 if scaled else 4)}
    if e == "bwd_input":
        return {"dx": dense_fwd_reference(p["dh_in"][:n], np.ascontiguousarray(p["w_in"].T)) + (case.f_out, 4)}
    r = dense_dw_reference(p["dh"][:n], p["x_dw"][:n], None, p["prior_dw"] if accumulate else None)
    return {"dw": r["dw"] + (n, 4)}


def dense_case_emulation(case: DenseCase, p, bias=False, relu=False, accumulate=False, defect=None, fma=False):
    """{output: fp32 tensor} in the summation order of the kernel the case reaches, or None where this module has none (the
    weighted column sum behind f_out == 1: tests/test_spmm_accuracy_cpu.py emulates the column sums' blocking)."""
    n, e, k = p["n"], case.entry, case.kernel
    if e in ("fwd", "fwd_row_scaled", "bias_act"):
        a, bt = p["x"][:n], p["w"]
        if k == "gemv":
            return {"out": emulate_gemv(a, bt, case.f_in % 4 == 0 and case.unaligned is None)}
        f = emulate_skinny if k == "skinny" else emulate_tiled
        return {"out": f(a, bt, p["bias"] if bias else None, relu, p["row_scale"][:n] if e == "fwd_row_scaled" else None, defect, fma)}
    if e == "bwd_input":
        a, bt = p["dh_in"][:n], np.ascontiguousarray(p["w_in"].T)
        if k == "outer":
            return {"dx": _f32(a) * _f32(bt).view(1, -1)}
        return {"dx": (emulate_skinny if k == "skinny" else emulate_tiled)(a, bt, defect=defect, fma=fma)}
    if k == "colsum":
        return None
    prior = p["prior_dw"] if accumulate else None
    if k == "dw_small":
        return {"dw": emulate_dw_small(p["dh"], p["x_dw"], n, None, prior, defect, fma)}
    return {"dw": emulate_split_k(p["dh"], p["x_dw"], n, prior, defect, fma)}
