"""Element-wise accuracy of the tiled bf16x3 gathered-operand GEMMs (grapes_amd/csrc/gemm_tiled_split.hip) against fp64:
H = feat(ids) Wᵀ on its three forward paths (the plain kernel, the few-row split-K form, the split tail for one and two nets)
and dW = dHᵀ feat(ids) on its kernels (the swapped 128 x 256 tile at f_out = 256, gemm_tsplit_dw_k<8> at f_out <= 128, the
several-problem launch), with the A/B forms of the diagnostic build in child processes.  Each output's error is taken
relative to its own sum |a||b| and its max and rms must stay within the factors of oracle/accuracy.py of a fixed-order fp32 sum
on the same operands.  The reference operand is the device's own materialisation (ops.gather_rows: indicator bits included,
stale epochs read as 0).  tests/test_accuracy_criterion_cpu.py shows the criterion rejects a dropped term or a lost plane of
this arithmetic, which the older bounds (test_widths_gpu.py, test_hip_parity.py) let through.

The data (oracle/accuracy.py: gathered_problem): normal, mixed (rows of X at 10^a, a in [-20, 20]; dh rows at the inverse
scale) and zeros (zero rows, a zero column, zero dh rows); the capacity rows past the live count read a NaN row of X and have
NaN dh rows; W's storage past its K columns is +inf.  Forward rows are independent: every live row is checked for finiteness,
the criterion runs on a seeded subset that always holds the last (partial) tile and every tile the split tail cuts.  dW outputs
are independent: the criterion runs on a seeded subset of columns that always holds the indicator columns and the last one.

Measured on the MI355X, worst max / rms ratio to the fp32 baseline over the cases of each path: plain forward 2.88 / 1.81
(the producer / consumer form included), split-K forward 1.75 / 1.24, split tail 3.17 / 1.73 (the log-Z net of the two-net
launch), dW 1.06 / 1.05 (the A/B forms 0.85 / 1.76), several problems 1.17 / 1.14.  No output exceeds the factors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import accuracy as acc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_X = 20000                     # rows of every generated X (the gathered ids repeat)
KINDS = ("normal", "mixed", "zeros")


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes):
    t = torch.empty(int(nbytes) + 64, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + (-t.data_ptr()) % 16


class _Layer:
    """gathered_problem p on the device, and the device's materialised operand feat [n, F + num_ind] (fp32, host)."""

    def __init__(self, ops, p, cap):
        F, ni, n = p["F"], p["num_ind"], p["n"]
        self.p, self.F, self.ni, self.n, self.cap = p, F, ni, n, cap
        self.kp = (F + ni + 3) // 4 * 4
        self.X = _dev(p["X"])
        self.ids = _dev(p["ids"])
        self.code = _dev(p["code"])
        self.d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        self.wide = _dev(p["wide"])
        self.w = self.wide[:, :F + ni]                 # a view: the image must not read the +inf columns past K
        self.img = ops.weight_split_image(self.w)
        self.dh = _dev(p["dh"])
        feat = ops.gather_rows(_dev(p["X"][:, :F]), self.ids[:n].contiguous(), self.code if ni else None, p["epoch"], ni).cpu()
        assert torch.equal(feat, torch.from_numpy(acc.gathered_feat(p)))
        self.feat = feat.numpy()

    def code_ptr(self):
        return self.code.data_ptr() if self.ni else None


def _fwd_rows(n, seed, must=()):
    """the rows the forward criterion runs on: ~2k seeded ones, the last tile's, and `must`"""
    rng = np.random.default_rng(seed)
    last = np.arange((n - 1) // acc.TS_BM * acc.TS_BM, n)
    return np.unique(np.concatenate([rng.integers(0, n, min(n, 2048)), last, np.asarray(must, dtype=np.int64)]))


def _check_fwd(h, L, w_np, rows, what, pieces_of):
    """h [cap, f_out] on the device: every live row finite; the criterion on `rows`.  On failure the CPU emulation of the same
    path on the same rows is measured too (pieces_of(row) -> its K pieces): a ratio it reproduces is the summation order."""
    h = h.cpu()
    assert bool(torch.isfinite(h[:L.n]).all()), f"{what}: non-finite outputs"
    feat = L.feat[rows]
    ref = acc.matmul_reference(feat, w_np.T)
    a = acc.Accuracy(h[rows], *ref)
    print(f"[accuracy] {what}: {a}")
    if not a.ok():
        groups = {}
        for i, r in enumerate(rows):
            groups.setdefault(tuple(pieces_of(r) or ()), []).append(i)
        emu = torch.zeros(len(rows), w_np.shape[0])
        for pc, idx in groups.items():
            emu[idx] = acc.emulate_tsplit_fwd(feat[idx], w_np, k_pieces=list(pc) or None)
        pytest.fail(f"{what}: {a}; CPU emulation of the path on the same rows: {acc.Accuracy(emu, *ref)}")
    return a


# ------------------------------------------------------------------------------------------------ forward, plain kernel
@pytest.mark.parametrize("kind", KINDS)
def test_plain_tiled_forward_is_elementwise_as_accurate_as_fp32(kind):
    """grapes_linear_fwd_gathered_split (gemm_tsplit_fwd_k<false>, n >= 8192): Reddit's 602 + 3 -> 256 (K = 605 in 19 K steps of
    32) at 77,015 live rows — a partial last tile of 87 rows — and 41 capacity rows."""
    ops = _ops()
    n, F, ni, fo = 77015, 602, 3, 256
    L = _Layer(ops, acc.gathered_problem(N_X, F, ni, fo, n, n + 41, kind, seed=11), n + 41)
    h = torch.full((L.cap, fo), 7.0, device="cuda")
    assert ops.lib().grapes_linear_fwd_gathered_split(L.X.data_ptr(), F, L.X.shape[1], L.ids.data_ptr(), L.code_ptr(), L.p["epoch"],
                                                      None, ni, L.img.data_ptr(), h.data_ptr(), L.cap, L.d_n.data_ptr(), fo,
                                                      _stream()) == 0
    assert float(h[n:].sub(7.0).abs().max()) == 0.0                        # rows past the live count are not written
    _check_fwd(h, L, L.p["w"], _fwd_rows(n, 1), f"plain fwd {kind}", lambda r: None)


# ------------------------------------------------------------------------------------------------ forward, split-K
@pytest.mark.parametrize("n,F,ni,fo", [(2708, 1433, 3, 256), (129, 1433, 3, 256), (1000, 602, 3, 132)])
@pytest.mark.parametrize("kind", KINDS)
def test_split_k_tiled_forward_is_elementwise_as_accurate_as_fp32(n, F, ni, fo, kind):
    """grapes_linear_fwd_gathered_split_k (128 <= n < 8192: K pieces into slabs + ts_fwd_slab_sum_k in slab order): Cora's
    2,708 rows x 1436, the smallest row count that takes it (129: a one-row second tile) and f_out = 132 (a partial column
    tile).  Every live row is checked."""
    ops = _ops()
    L = _Layer(ops, acc.gathered_problem(N_X, F, ni, fo, n, n + 29, kind, seed=n + F), n + 29)
    pieces = acc.tsplit_fwd_pieces(L.cap, L.kp)
    assert len(pieces) > 1
    h = torch.full((L.cap, fo), 7.0, device="cuda")
    ws, wsp = _ws(ops.lib().grapes_linear_fwd_gathered_split_k_workspace_bytes(L.cap, L.kp, fo))
    assert ops.lib().grapes_linear_fwd_gathered_split_k(L.X.data_ptr(), F, L.X.shape[1], L.ids.data_ptr(), L.code_ptr(), L.p["epoch"],
                                                        None, ni, L.img.data_ptr(), h.data_ptr(), L.cap, L.d_n.data_ptr(), fo, wsp,
                                                        _stream()) == 0
    _check_fwd(h, L, L.p["w"], np.arange(n), f"split-K fwd n={n} K={F + ni} fo={fo} {kind}", lambda r: pieces)


# ------------------------------------------------------------------------------------------------ forward, split tail
@pytest.mark.parametrize("n,nets", [(9000, 1), (38500, 1), (16600, 2)])
@pytest.mark.parametrize("kind", KINDS)
def test_split_tail_forward_is_elementwise_as_accurate_as_fp32(n, nets, kind):
    """grapes_linear_fwd_gathered_split_tail with one net (Reddit's sampler net, 602 + 3 columns) and two (with the log-Z net,
    602 columns, over the same rows): 9,000 rows = 71 units all cut into 3 pieces, 38,500 rows = a round of 256 and 45 units
    cut into 5, two nets x 16,600 rows = 2 rounds and 4 units cut into 8 (the last of them the partial tile).  The criterion
    covers every row of a cut tile."""
    ops = _ops()
    F, fo = 602, 256
    cap = n + 300
    La = _Layer(ops, acc.gathered_problem(N_X, F, 3, fo, n, cap, kind, seed=n), cap)
    layers = [La]
    if nets == 2:
        # the log-Z net: the same X and rows (X and ids do not depend on num_ind), its own [256, 602] weight
        layers.append(_Layer(ops, acc.gathered_problem(N_X, F, 0, fo, n, cap, kind, seed=n), cap))
        assert np.array_equal(layers[1].p["ids"], La.p["ids"]) and not np.array_equal(layers[1].p["w"][:, :F], La.p["w"][:, :F])
    cut, S = acc.tsplit_tail_cut(n, nets, 608)
    assert S > 1 and len({t for t, _ in cut}) > 0
    outs = ops.linear_fwd_gathered_tail(La.X, F, La.ids, [L.img for L in layers], fo, [La.code] + [None] * (nets - 1),
                                        [3] + [0] * (nets - 1), epoch=La.p["epoch"], d_n=La.d_n)
    for q, (L, h) in enumerate(zip(layers, outs)):
        tiles = sorted(t for t, pq in cut if pq == q)
        must = np.concatenate([np.arange(t * acc.TS_BM, min((t + 1) * acc.TS_BM, n)) for t in tiles]) if tiles else []
        pieces = {t: cut[(t, q)] for t in tiles}
        _check_fwd(h, L, L.p["w"], _fwd_rows(n, q + 3, must), f"tail fwd n={n} nets={nets} net {q} ({len(tiles)} cut tiles, S={S}) {kind}",
                   lambda r: pieces.get(r // acc.TS_BM))


# ------------------------------------------------------------------------------------------------ dW
def _dw_cols(K, kp, ni, seed):
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([rng.integers(0, K, 96), [0, K - 1], np.arange(K - ni, K)]))


def _dw_reference(L, cols, ind_mask, prev=None):
    """(ref, mag, base) of dW[:, cols] = dhᵀ feat over the live rows (feat under ind_mask), plus prev[:, cols] if accumulating"""
    feat = acc.gathered_feat(L.p, ind_mask=ind_mask) if ind_mask else L.feat
    dh = L.p["dh"][:L.n]
    ref, mag, base = acc.matmul_reference(dh.T, np.ascontiguousarray(feat[:, cols]))
    if prev is not None:
        p = prev[:, cols]
        ref, mag, base = ref + torch.from_numpy(p).double(), mag + torch.from_numpy(np.abs(p)).double(), base + torch.from_numpy(p)
    return ref, mag, base, feat


def _check_dw(dw, L, cols, ind_mask, what, prev=None, nslab=None):
    dw = dw.cpu()
    K = L.F + L.ni
    assert bool(torch.isfinite(dw[:, :K]).all()), f"{what}: non-finite outputs"
    ref, mag, base, feat = _dw_reference(L, cols, ind_mask, prev)
    a = acc.Accuracy(dw[:, cols], ref, mag, base)
    print(f"[accuracy] {what}: {a}")
    if not a.ok():
        ns = nslab or acc.tsplit_dw_slabs(L.cap, L.p["dh"].shape[1], L.kp)
        emu = acc.emulate_tsplit_dw(L.p["dh"][:L.n], np.ascontiguousarray(feat[:, cols]), ns)
        if prev is not None:
            emu = emu + torch.from_numpy(prev[:, cols])
        pytest.fail(f"{what}: {a}; CPU emulation ({ns} slabs) on the same data: {acc.Accuracy(emu, ref, mag, base)}")
    return a


@pytest.mark.parametrize("n,F,ni,fo", [(2708, 1433, 3, 256), (20000, 602, 3, 256), (16000, 602, 3, 128), (300, 602, 3, 64)])
@pytest.mark.parametrize("kind", KINDS)
def test_tiled_dw_is_elementwise_as_accurate_as_fp32(n, F, ni, fo, kind):
    """grapes_linear_bwd_weight_gathered_split and _split_ld: f_out = 256 takes the swapped tile (gemm_tsplit_dw_sw_k: Cora's
    1436 columns, Reddit's 605), f_out <= 128 gemm_tsplit_dw_k<8, false> (16k rows x 605 -> 128; 300 rows in 3 slabs -> 64).
    Padded layout overwriting a buffer of 7.0 (its pad columns must come out 0), accumulating onto a non-zero buffer, the
    parameter's own [f_out, F + num_ind] layout both ways; the indicator mask drops bit 1 (ind_mask = 5)."""
    ops = _ops()
    cap = n + 37
    L = _Layer(ops, acc.gathered_problem(N_X, F, ni, fo, n, cap, kind, seed=n + F + fo), cap)
    K, mask = F + ni, 5
    cols = _dw_cols(K, L.kp, ni, n)
    prev = np.random.default_rng(n + 1).standard_normal((fo, L.kp)).astype(np.float32)
    for layout in ("padded", "own"):
        width = L.kp if layout == "padded" else K
        if layout == "own" and width == L.kp:
            continue
        for accumulate in (False, True):
            pv = np.ascontiguousarray(prev[:, :width])
            dw = _dev(pv) if accumulate else torch.full((fo, width), 7.0, device="cuda")
            ops.linear_bwd_weight_gathered(L.dh, L.X, F, L.ids, dw, L.code if ni else None, L.p["epoch"], ni, d_n=L.d_n,
                                           accumulate=accumulate, ind_mask=mask, split=True)
            _check_dw(dw, L, cols, mask, f"dW n={n} K={K} fo={fo} {kind} {layout} acc={accumulate}", pv if accumulate else None)
            if width > K and not accumulate:
                assert float(dw[:, K:].abs().max()) == 0.0          # the padded layout's pad columns


def test_several_problem_dw_is_elementwise_as_accurate_as_fp32():
    """grapes_linear_bwd_weight_gathered_split_multi: three problems over one X — the sampler net at two hops into ONE gradient
    (indicator masks 3 and 7; the second hop with no live row) and the log-Z net (no indicators) into its own — for each data
    kind, the gradients in the parameter's layout, the shared one accumulating onto a non-zero buffer."""
    ops = _ops()
    F, ni, fo = 602, 3, 256
    for kind in KINDS:
        lives, caps = (7013, 0, 21877), (9000, 9000, 22000)
        Ls = []
        for q, (n, cap) in enumerate(zip(lives, caps)):
            p = acc.gathered_problem(N_X, F, ni if q < 2 else 0, fo, n, cap, kind, seed=31, rows_seed=100 + q)
            Ls.append(_Layer(ops, p, cap))
        prev = np.random.default_rng(3).standard_normal((fo, F + ni)).astype(np.float32)
        dw_gf, dw_z = _dev(prev), torch.full((fo, F), 5.0, device="cuda")
        probs = [dict(dh=L.dh, ids=L.ids, dw=(dw_gf if q < 2 else dw_z), ind_code=(L.code if q < 2 else None),
                      num_ind=(ni if q < 2 else 0), d_n=L.d_n, accumulate=(q == 0), ind_mask=(3, 7, 0)[q], split=True)
                 for q, L in enumerate(Ls)]
        assert ops.linear_bwd_weight_gathered_multi_ok(F, probs)
        ops.linear_bwd_weight_gathered_multi(Ls[0].X, F, probs, epoch=Ls[0].p["epoch"])
        cols = _dw_cols(F + ni, 608, ni, 7)
        ref, mag, base, _ = _dw_reference(Ls[0], cols, 3, prev)            # problem 1 has no live row
        a = acc.assert_fp32_accuracy(dw_gf.cpu()[:, cols], ref, mag, base, what=f"multi gf {kind}")
        colz = _dw_cols(F, 604, 0, 8)
        a = acc.assert_fp32_accuracy(dw_z.cpu()[:, colz], *_dw_reference(Ls[2], colz, 0)[:3], what=f"multi z {kind}")


# ------------------------------------------------------------------------------------------------ A/B forms (child processes)
def _run_child_with_env(env, fn, *args):
    """the library reads its A/B switches once per process: run the case in a child process with the switch set"""
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_tsplit_accuracy_gpu as T; T.{fn}(*{args!r}); print('child ok')")
    e = dict(os.environ); e.update(env)
    e["GRAPES_DIAG"] = "1"          # the A/B switches exist in the diagnostic build only (grapes_amd/_lib.py)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def _ab_dw_case(n, F, ni, fo, kind, wgs):
    ops = _ops()
    L = _Layer(ops, acc.gathered_problem(N_X, F, ni, fo, n, n + 37, kind, seed=n + 3), n + 37)
    K = F + ni
    dw = torch.full((fo, L.kp), 7.0, device="cuda")
    ops.linear_bwd_weight_gathered(L.dh, L.X, F, L.ids, dw, L.code, L.p["epoch"], ni, d_n=L.d_n, ind_mask=5, split=True)
    _check_dw(dw, L, _dw_cols(K, L.kp, ni, n), 5, f"A/B dW n={n} fo={fo} {kind}", nslab=acc.tsplit_dw_slabs(L.cap, fo, L.kp, wgs))


def _ab_fwd_pc_case(kind):
    test_plain_tiled_forward_is_elementwise_as_accurate_as_fp32(kind)


@pytest.mark.parametrize("env,fn,args", [
    ({"GRAPES_TSPLIT_FWD_PC": "1"}, "_ab_fwd_pc_case", ("mixed",)),                              # gemm_tsplit_fwd_pc_k
    ({"GRAPES_TSPLIT_DW_CW": "4"}, "_ab_dw_case", (20000, 602, 3, 128, "mixed", 768)),          # gemm_tsplit_dw_k<4>
    ({"GRAPES_TSPLIT_DW_SWAP": "0"}, "_ab_dw_case", (20000, 602, 3, 256, "normal", 768)),       # gemm_tsplit_dw_k<8> at f_out 256
    ({"GRAPES_TSPLIT_DW_WGS": "40"}, "_ab_dw_case", (20000, 602, 3, 256, "mixed", 40))],        # 8 slabs of 79 K steps
    ids=["fwd-pc", "dw-cw4", "dw-noswap", "dw-wgs40"])
def test_tiled_ab_forms_are_elementwise_as_accurate_as_fp32(env, fn, args):
    """The A/B forms of the diagnostic build, one case each: the producer / consumer forward kernel, the four-consumer dW
    kernel, the unswapped dW tile at f_out = 256, and few long slabs."""
    _ops()
    _run_child_with_env(env, fn, *args)


# ------------------------------------------------------------------------------------------------ range edges
def test_tiled_split_range_edges():
    """The two edges of the tiled GEMMs' range (include/grapes_hip.h, beside grapes_linear_fwd_gathered_split), on both sides.
    Large: an entry of 3.39e38 still splits (its bf16 is finite) and the outputs meet the criterion; at 3.40e38 the h plane
    rounds to inf, m to -inf and l to NaN — the forward row of every gathered row holding it is NaN in every column, and the
    dW column of that feature is NaN for every unit (0 x NaN is NaN), with the other rows / columns unaffected.  Small: X at
    1e-28 meets the criterion; at 1e-35 an entry is held only to bf16's smallest subnormal step (2^-134 per entry, not 2^-24
    relative) — the criterion fails, within_tiled_split_resolution holds, as in the CPU emulation
    (test_accuracy_criterion_cpu.py: test_tiled_split_holds_tiny_operands_only_to_the_bf16_subnormal_step)."""
    ops = _ops()
    n, F, fo = 700, 602, 256
    base = acc.gathered_problem(N_X, F, 0, fo, n, n + 29, "normal", seed=5)
    wabs = torch.from_numpy(np.abs(base["w"]).astype(np.float64).sum(1))[None, :]
    g0, c0 = int(base["ids"][3]), 11

    def run(X):
        p = dict(base, X=X)
        L = _Layer(ops, p, n + 29)
        h = torch.full((L.cap, fo), 7.0, device="cuda")
        ws, wsp = _ws(ops.lib().grapes_linear_fwd_gathered_split_k_workspace_bytes(L.cap, L.kp, fo))
        assert ops.lib().grapes_linear_fwd_gathered_split_k(L.X.data_ptr(), F, L.X.shape[1], L.ids.data_ptr(), None, p["epoch"], None,
                                                            0, L.img.data_ptr(), h.data_ptr(), L.cap, L.d_n.data_ptr(), fo, wsp,
                                                            _stream()) == 0
        dh = _dev(np.where(np.arange(L.cap)[:, None] < n, np.random.default_rng(2).uniform(-0.9, 0.9, (L.cap, fo)), np.nan).astype(np.float32))
        dw = torch.full((fo, L.kp), 7.0, device="cuda")
        ops.linear_bwd_weight_gathered(dh, L.X, F, L.ids, dw, None, p["epoch"], 0, d_n=L.d_n, split=True)
        return L, h[:n].cpu(), dw[:, :F].cpu(), dh[:n].cpu().numpy()

    for big, finite in ((3.39e38, True), (3.40e38, False)):
        X = base["X"].copy(); X[:, :F] *= 1e-3; X[g0, c0] = big
        L, h, dw, dh = run(X)
        bad = base["ids"][:n] == g0
        fref = acc.matmul_reference(L.feat, base["w"].T)
        wref = acc.matmul_reference(dh.T, L.feat)
        assert bool(torch.isfinite(fref[0]).all()) and bool(torch.isfinite(wref[0]).all())
        if finite:
            acc.assert_fp32_accuracy(h, *fref, what=f"fwd {big}")
            acc.assert_fp32_accuracy(dw, *wref, what=f"dW {big}")
        else:
            assert bool(torch.isnan(h[bad]).all())
            acc.assert_fp32_accuracy(h[~bad], *(t[~bad] for t in fref), what=f"fwd {big} other rows")
            assert bool(torch.isnan(dw[:, c0]).all())
            others = [c for c in range(F) if c != c0]
            acc.assert_fp32_accuracy(dw[:, others], *(t[:, others] for t in wref), what=f"dW {big} other columns")
    for scale, inside in ((1e-28, True), (1e-35, False)):
        X = base["X"].copy(); X[:N_X - 1, :F] = (X[:N_X - 1, :F] * scale).astype(np.float32)
        L, h, dw, dh = run(X)
        fref = acc.matmul_reference(L.feat, base["w"].T)
        a = acc.Accuracy(h, *fref)
        print(f"[range edge {scale}] fwd: {a}")
        assert a.ok() == inside, a
        assert acc.within_tiled_split_resolution(h, fref, wabs)
        wref = acc.matmul_reference(dh.T, L.feat)
        a = acc.Accuracy(dw, *wref)
        print(f"[range edge {scale}] dW: {a}")
        assert a.ok() == inside, a
        assert acc.within_tiled_split_resolution(dw, wref, torch.from_numpy(np.abs(dh).astype(np.float64).sum(0))[:, None])
