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
the factors against them.  Only tests import this module.
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


def aggregate_case(size: str, kind: str, f: int, seed: int = 0, pad: bool = True) -> Dict[str, np.ndarray]:
    n, n_pad, hubs = AGG_GRAPHS[size]
    return aggregate_problem(kind, n, tuple(AGG_ROW_LENGTHS) + tuple(hubs), f, seed, n_pad=n_pad if pad else 0)
