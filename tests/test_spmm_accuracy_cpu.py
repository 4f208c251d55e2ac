"""The element-wise criterion of oracle/accuracy.py on the sparse aggregation  out = Â h (+ b, ReLU)  of
grapes_amd/csrc/spmm_kernels.hip, shown on the CPU: faithful fp32 emulations of the kernels' summation orders stay inside
the project's factors (RMS_FACTOR = 3, MAX_FACTOR = 6 against the sequential fp32 baseline of aggregate_reference) and under
the hard cap (L + 4) 2^-24 mag, and seeded defects are rejected — on the very problems tests/test_spmm_accuracy_gpu.py runs
the kernels on (accuracy.aggregate_case: rows of 0 .. 200, 1000 entries and hubs of 5000 and 20000, f = 64, 2600 nodes, so
that rows above 64 entries are chunked).

Orders that pass: the sequential order with fused multiply-adds (row_accumulate), the eight-chain hub order
(row_accumulate_hub), 64-entry chunks of four 16-entry quarters whose partials are added in four contiguous quarters of the
chunks, each in chunk order (gcn_aggregate_chunks_k + gcn_aggregate_combine_k), the prescaled form judged against the PLAIN form's reference and baseline, bias before the
self-loop, and the column sums in CS_BLOCKS x CS_ROWS blocking.

Defects, and the kinds that reject each (asserted below, DEFECTS): a defect that drops, doubles or misweights a whole term is
caught on every kind here because this graph has rows of 65-200 entries where one term is not negligible; `striped` is the
kind on which a lost term leaves an exact zero where a value belongs (the ratio is infinite); `mixed` does not see a lost
self-loop (the row's own scale is one of many, and the term is below the rounding of its neighbours).  dinv wrong by 3e-6
is caught by its rms on every kind.  The >= 0 gate is visible only where the gate operand holds exact zeros under nonzero
gradients: `zeros` (and every kind whose activations are a ReLU's output; the test uses an N(0,1) gate so that only `zeros`
has them)."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc

F = 64
HUB_ROW, LONG_ROW, SMALL_GRAPH = 16, 64, 2048       # GRAPES_HUB_ROW, GRAPES_LONG_ROW (spmm_kernels.hip), _SMALL_GRAPH (ops.py)
CS_BLOCKS, CS_ROWS = 512, 32
f32 = np.float32


def _seq(t):
    return acc._seq_sum_f32(np.ascontiguousarray(t, dtype=f32))


def _eight_chains(t):
    parts = [_seq(t[g::8]) for g in range(8)]
    out = parts[0]
    for g in range(1, 8):
        out = (out + parts[g]).astype(f32)
    return out


def _chunks(t, defect=None):
    """gcn_aggregate_chunks_k + gcn_aggregate_combine_k: every 64-entry chunk as four sequential 16-entry quarters added
    ((q0 + q1) + q2) + q3; the nc chunk partials in four contiguous quarters of ceil(nc / 4) chunks, each added in chunk order,
    the four sums again ((g0 + g1) + g2) + g3."""
    parts = []
    for c0 in range(0, len(t), LONG_ROW):
        ch = t[c0:c0 + LONG_ROW]
        if defect == "chunk_last_lost" and len(ch) == LONG_ROW:
            ch = ch[:-1]
        q = [_seq(ch[k:k + 16]) for k in range(0, LONG_ROW, 16)]
        part = (((q[0] + q[1]).astype(f32) + q[2]).astype(f32) + q[3]).astype(f32)
        if defect == "chunk_first_twice":
            part = (part + ch[0]).astype(f32)
        parts.append(part)
    nc = len(parts)
    per = (nc + 3) >> 2
    zero = np.zeros(t.shape[1], f32)
    g = [_seq(np.stack([zero] + parts[k * per:min(k * per + per, nc)])) for k in range(4)]
    return (((g[0] + g[1]).astype(f32) + g[2]).astype(f32) + g[3]).astype(f32)


def _fma_seq(w, hs):
    """acc = fma(w_j, h_j, acc) in order: the product exact in fp64 (two fp32 factors), one rounding to fp32 per step (the double
    rounding through fp64 moves a result by at most 2^-29 of an ulp's tie cases: immaterial here)."""
    a = np.zeros(hs.shape[1], f32)
    w64 = w.astype(np.float64)
    for j in range(len(w)):
        a = (a.astype(np.float64) + w64[j] * hs[j].astype(np.float64)).astype(f32)
    return a


def emulate(rowptr, csr, dinv, h, bias, relu, n_nodes, form="kernel", defect=None):
    """The forward aggregation in fp32 on the CPU.  form: "kernel" (per row length the order the kernels take: sequential up to
    HUB_ROW, eight chains above, chunks above LONG_ROW when the graph has more than SMALL_GRAPH nodes), "fma" (sequential with
    fused multiply-adds), "chains" / "chunks" (that order for every row), "bias_first"."""
    n = len(rowptr) - 1
    d = np.asarray(dinv, dtype=f32).copy()
    if defect == "dinv_3e-6":
        d = (d.astype(np.float64) * (1 + 3e-6)).astype(f32)
    h = np.asarray(h, dtype=f32)
    out = np.zeros((n, h.shape[1]), f32)
    for r in range(n):
        s = csr[rowptr[r]:rowptr[r + 1]]
        L = len(s)
        if defect == "head_only4" and 5 <= L <= 8:
            s = s[:4]
        w = (d[r] * d[r] if defect == "dinv_c" else d[s] * d[r]) * np.ones(len(s), f32)
        if defect == "w_bf16":
            w = torch.from_numpy(w).bfloat16().float().numpy()
        t = (w[:, None] * h[s]).astype(f32)
        chunked = L > LONG_ROW and n_nodes > SMALL_GRAPH
        if form == "fma":
            a = _fma_seq(w, h[s]) if L <= 256 else _seq(t)
        elif form == "chains" or (form in ("kernel", "bias_first") and L > HUB_ROW and not chunked):
            a = _eight_chains(t)
        elif form == "chunks" or (form in ("kernel", "bias_first") and chunked):
            a = _chunks(t, defect)
        else:
            a = _seq(t)
        loop = ((d[r] * d[r]) * h[r]).astype(f32)
        if defect == "loop_lost_gt64" and L > LONG_ROW:
            loop = np.zeros_like(loop)
        if form == "bias_first" and bias is not None:
            a = ((a + bias).astype(f32) + loop).astype(f32)
        else:
            a = (a + loop).astype(f32)
            if bias is not None:
                a = (a + bias).astype(f32)
        out[r] = np.maximum(a, f32(0)) if relu else a
    return out


def emulate_colsum(src, gate=None, ge=False):
    """colsum_partial_k + colsum_final_k: block b owns the 32-row chunks b, b + 512, ...; rows in order inside a block; the 512
    partials in four ranges of 128, added in block order, the ranges as (p0 + p1) + (p2 + p3)."""
    src = np.asarray(src, dtype=f32)
    if gate is not None:
        src = np.where((gate >= 0) if ge else (gate > 0), src, f32(0))
    n, f = src.shape
    part = np.zeros((CS_BLOCKS, f), f32)
    for b in range(min(CS_BLOCKS, -(-n // CS_ROWS))):
        rows = np.concatenate([np.arange(r0, min(r0 + CS_ROWS, n)) for r0 in range(b * CS_ROWS, n, CS_BLOCKS * CS_ROWS)])
        part[b] = _seq(src[rows])
    rng4 = [_seq(part[g * 128:(g + 1) * 128]) for g in range(4)]
    return ((rng4[0] + rng4[1]).astype(f32) + (rng4[2] + rng4[3]).astype(f32)).astype(f32)


_CASES = {}


def _case(kind):
    if kind not in _CASES:
        p = acc.aggregate_case("large", kind, F, seed=11)
        n = p["n"]
        rt, cs, rs, cd, dinv = acc.host_csr(p["src"], p["dst"], n)
        assert np.array_equal(np.diff(rt), p["lens"])
        assert np.diff(rs).max() > LONG_ROW                      # the transpose has long rows of its own
        ref = acc.aggregate_reference(rt, cs, dinv, p["h"], p["bias"], True)
        _CASES[kind] = (p, rt, cs, dinv, ref)
    return _CASES[kind]


def _judge(kind, out):
    p, rt, cs, dinv, ref = _case(kind)
    a = acc.Accuracy(out, *ref)
    cap = acc.hard_cap_excess(out, ref[0], ref[1], p["lens"])
    return a, cap


def test_sequential_accumulate_is_the_position_in_row_walk_bit_for_bit():
    """aggregate_reference walks rows of up to AGG_LOOP_ROWS entries by position-in-row and sums longer ones with numpy's
    add.accumulate: both are the same sequential fp32 chain."""
    p, rt, cs, dinv, ref = _case("normal")
    lens = p["lens"]
    rows = np.nonzero((lens > 0) & (lens <= acc.AGG_LOOP_ROWS))[0][::7]
    for r in rows:
        s = cs[rt[r]:rt[r + 1]]
        t = ((dinv[s] * dinv[r])[:, None] * p["h"][s]).astype(f32)
        a = np.zeros(F, f32)
        for j in range(len(s)):
            a = (a + t[j]).astype(f32)
        assert np.array_equal(a, _seq(t))
        want = np.maximum(((a + (dinv[r] * dinv[r]) * p["h"][r]).astype(f32) + p["bias"]).astype(f32), f32(0))
        assert np.array_equal(want, ref[2][r].numpy()), r


@pytest.mark.parametrize("kind", acc.AGG_KINDS)
@pytest.mark.parametrize("form", ["kernel", "fma", "chains", "chunks", "bias_first"])
def test_faithful_orders_are_accepted(kind, form):
    p, rt, cs, dinv, ref = _case(kind)
    out = emulate(rt, cs, dinv, p["h"], p["bias"], True, p["n"], form)
    a, cap = _judge(kind, out)
    print(f"[faithful] {form} {kind}: {a}; cap x{cap:.3f}")
    assert a.ok(), (form, kind, a)
    assert cap <= 1.0, (form, kind, cap)


@pytest.mark.parametrize("kind", acc.AGG_KINDS)
def test_prescaled_form_is_accepted_against_the_plain_reference(kind):
    """out = fl32(dc (sum fl32(dinv[s] h[s]) + hs[c])): one more rounding per term than the plain form (cap L + 5), still inside
    the factors of the PLAIN baseline; and the prescaled baseline is what it says (the rows' own dinv applied first)."""
    p, rt, cs, dinv, ref = _case(kind)
    pre = acc.aggregate_reference(rt, cs, dinv, p["h"], p["bias"], True, prescaled=True)
    assert torch.equal(pre[0], ref[0]) and torch.equal(pre[1], ref[1])
    a = acc.Accuracy(pre[2], *ref)
    cap = acc.hard_cap_excess(pre[2], ref[0], ref[1], p["lens"], extra=5)
    print(f"[faithful] prescaled {kind}: {a}; cap x{cap:.3f}")
    assert a.ok() and cap <= 1.0, (kind, a, cap)
    chains = acc.aggregate_reference(rt, cs, dinv, p["h"], p["bias"], True, prescaled=True, order=_eight_chains)
    assert acc.Accuracy(chains[2], *pre).ok()


# defect -> the kinds that must reject it
DEFECTS = {
    # self-loop lost on rows longer than 64: not on `mixed`, where a row of 65+ entries at ten random scales is dominated by its
    # largest neighbour and its own term falls below the rounding of the sum (max ratio 3.9, rms 1.7: inside the factors)
    "loop_lost_gt64": ("normal", "zeros", "striped"),
    "chunk_last_lost": acc.AGG_KINDS,       # last entry of a 64-entry chunk lost
    "chunk_first_twice": acc.AGG_KINDS,     # first entry of a chunk added twice
    "dinv_c": acc.AGG_KINDS,                # dinv[c] used where dinv[s] belongs
    "w_bf16": acc.AGG_KINDS,                # edge weight rounded to bf16
    "dinv_3e-6": acc.AGG_KINDS,             # dinv wrong by 3e-6 relative (a fast rsqrt)
    "head_only4": acc.AGG_KINDS,            # rows beyond 4 entries of a head record ignored
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defects_are_rejected(defect):
    seen = {}
    for kind in acc.AGG_KINDS:
        p, rt, cs, dinv, ref = _case(kind)
        out = emulate(rt, cs, dinv, p["h"], p["bias"], True, p["n"], "kernel", defect)
        a, cap = _judge(kind, out)
        seen[kind] = (not a.ok(), cap > 1.0)
        print(f"[defect] {defect} {kind}: {a}; cap x{cap:.3g}")
    for kind in DEFECTS[defect]:
        assert seen[kind][0], (defect, kind, "the ratio criterion accepted it")
    assert any(c for _, c in seen.values()), (defect, "the hard cap accepted it on every kind")


def test_a_lost_self_loop_stands_out_most_on_striped_data():
    """On a graph whose only rows above 64 entries are one of 70 and a hub of 5000: the lost loop of the 70-entry row is one of
    71 terms on normal data but one of about two in its own stripe's column on striped data, where the error is then of the
    size of the output itself."""
    res = {}
    for kind in ("normal", "striped"):
        p = acc.aggregate_problem(kind, 2600, (70, 5000), F, 5)
        rt, cs, rs, cd, dinv = acc.host_csr(p["src"], p["dst"], p["n"])
        ref = acc.aggregate_reference(rt, cs, dinv, p["h"], None, False)
        out = emulate(rt, cs, dinv, p["h"], None, False, p["n"], "kernel", "loop_lost_gt64")
        res[kind] = acc.Accuracy(out, *ref)
        print(f"[hub loop] {kind}: {res[kind]}")
    assert not res["striped"].ok() and res["striped"].max > 1e-2 and res["striped"].max > 2 * res["normal"].max


@pytest.mark.parametrize("kind", acc.AGG_KINDS)
def test_column_sums_blocking_accepted_and_wrong_gate_rejected(kind):
    """colsum in CS_BLOCKS x CS_ROWS blocking against the row-order baseline; the gate taken as >= 0 instead of > 0 passes
    every exact zero of the gate operand: rejected on `zeros` (whole zero rows, a zero column under nonzero gradients)."""
    p, rt, cs, dinv, ref = _case(kind)
    n = p["n"]
    rng = np.random.default_rng(3)
    gate = np.where(p["h"][:n] == 0, f32(0), rng.standard_normal((n, F)).astype(f32))      # zero exactly where h is (zeros / striped)
    src = p["dout"][:n]
    r = acc.colsum_reference(src, gate=gate)
    good = acc.Accuracy(emulate_colsum(src, gate), *r)
    bad = acc.Accuracy(emulate_colsum(src, gate, ge=True), *r)
    print(f"[colsum] {kind}: blocked {good}; gate >= 0 {bad}")
    assert good.ok() and acc.hard_cap_excess(emulate_colsum(src, gate), r[0], r[1], float(n)) <= 1.0
    if kind == "zeros":
        assert not bad.ok()


def test_rank1_reference_is_the_three_step_computation():
    """rank1_reference against its definition written out densely in fp64 on a small problem."""
    p = acc.aggregate_problem("zeros", 300, (0, 5, 17, 65, 130), 20, 2, n_pad=3)
    n = p["n"]
    rt, cs, rs, cd, dinv = acc.host_csr(p["src"], p["dst"], n)
    r = acc.rank1_reference(rs, cd, dinv, p["act"], p["dh2"], p["w2"], prior_dw=p["bias"], prior_db=p["bias"])
    A = np.zeros((n, n))
    d = dinv.astype(np.float64)
    np.add.at(A, (p["dst"][p["src"] != p["dst"]], p["src"][p["src"] != p["dst"]]), 1.0)
    A = d[:, None] * (A + np.eye(n)) * d[None, :]
    act, dh2, w2 = (p[k].astype(np.float64) for k in ("act", "dh2", "w2"))
    dpre = np.where(act[:n] > 0, dh2[:n, None] * w2[None, :], 0.0)
    assert np.allclose(r["dh"][0].numpy(), A.T @ dpre, rtol=1e-12, atol=0)
    assert np.allclose(r["dw_head"][0].numpy(), dh2[:n] @ act[:n] + p["bias"], rtol=1e-12)
    assert np.allclose(r["dbias"][0].numpy(), dpre.sum(0) + p["bias"], rtol=1e-12)
    for k, L in (("dh", np.diff(rs)), ("dw_head", float(n)), ("dbias", float(n))):
        assert acc.Accuracy(r[k][2], *r[k]).ok() and acc.hard_cap_excess(r[k][2], r[k][0], r[k][1], L, 5) <= 1.0, k
