"""Element-wise accuracy of the GCN aggregation kernels (grapes_amd/csrc/spmm_kernels.hip, and the 64-bit form in spmm_large.hip)
against fp64: every public aggregation entry point of grapes_amd.ops, on graphs built by ops.PreparedGraph, each output judged
relative to the fp64 sum of |w||h| of ITS OWN terms.  Two conditions per output tensor (oracle/accuracy.py:
assert_aggregate_accuracy): max and rms of that error within MAX_FACTOR = 6 / RMS_FACTOR = 3 of a host fp32 baseline that adds
a row's entries in CSR order, and the hard cap |got - ref| <= (L_r + 4) 2^-24 mag (L_r + 5 for the prescaled and rank-1 forms,
which round once more per term).  tests/test_spmm_accuracy_cpu.py shows on the same problems that the kernels' summation
orders pass and that a lost, doubled or misweighted term does not.

Data (accuracy.aggregate_case): rows of 0, 1, 2, 4, 5, 8, 9, 15, 16, 17, 24, 63, 64, 65, 127, 128, 129, 200, 1000 entries and
hubs of 5000-20000, duplicate edges, self-loops in the edge list, sources with hundreds of out-edges; kinds normal, mixed
(rows at 10^[-12, 12]), zeros, striped (an output sums only the entries of its own stripe: a lost term leaves an exact zero).
Capacity rows past the device-side count are NaN, the CSR past its live extent names a NaN row, outputs given by the caller
are prefilled with a sentinel that must survive.  The references take the DEVICE's rowptr / csr / dinv (the entry order of a
row is the build's), so the aggregation alone is judged; the build's dinv has its own test.

Cases (the kernel each is meant to reach; what is asserted from Python that the path was taken):
  forward small   f = 1, 7, 16                        gcn_aggregate_narrow_k
                  f = 17, 47, 100 (unaligned view)    gcn_aggregate_k<1, 0>                 (h.data_ptr() % 16 != 0)
                  f = 20 .. 512                       gcn_aggregate_k<4, 0>                 (n <= 2048: no items)
  forward large   f = 17, 47, 100u                    gcn_aggregate_k<1> + chunks_k<1> + combine_k      (n_items_t > 0)
                  f = 20, 32 / 64 / 100, 128          gcn_aggregate_lpr_k<8 / 16 / 32> + chunks_lpr_k + combine_k
                  f = 256, 260, 512                   gcn_aggregate_k<4> + chunks_k<4> + combine_k (two passes above 256)
  record form     f = 20, 64, 100, 256                gcn_aggregate_rec_k<0>                (ops._rec_form)
  head (+ bits)   f = 64, 100, 256                    gcn_aggregate_k<4, 3>, gcn_aggregate_rec_k<3>
  prescaled       f = 32 .. 256, small and from_csr   gcn_aggregate_k<4, 1>, lpr_k<.., true>, chunks_k<4, 1>, scale_rows_k
  narrow pair     f = 1                               gcn_aggregate_narrow_multi_k
  gather          6+5, 100+4, 128+3, 602+3            gcn_aggregate_gather_k<32 / 64>, gcn_aggregate_gather_head5_k<32 / 64>
  backward small  f = 1, 16 / 47 / 64, 256 / 512      1537 rows <= 8192: the one-launch ticket forms (gcn_aggregate_bwd_small_k<1 / 4> up to
                                                      f = 256, colsum_ticket_k + the aggregation at 512); f <= 16: the narrow kernels
  backward rows9k the same widths, 9023 rows          colsum_partial[_narrow]_k + colsum_final_k, aggregation with items
  rank-1          f = 64, 100, 256                    colsum_rank1_partial_k + colsum_final2_k + gcn_aggregate_k<4, 2> (+ chunks /
                                                      combine on the large graph); gate bits: gcn_aggregate_r1bits_k, chunks_k<4, 4>;
                                                      _multi: the *_multi_k kernels
  large graph     f = 100, 128                        spmm_large.hip (64-bit offsets), chunk = 1024 < the hubs
The kernels that ran in a `rocprofv3 --kernel-trace --stats` run of this module, against the __global__ kernels of
spmm_kernels.hip, are listed in DESIGN.md ("Kernel coverage of the aggregation accuracy test").

Measured on the MI355X, worst max / rms ratio to the fp32 baseline and worst fraction of the hard cap over the cases of each
entry point: forward 1.18 / 0.99, cap 0.63; record form 0.84 / 0.98, 0.58; fused head (out, head_out) 1.22 / 0.99, 0.53;
prescaled 0.89 / 0.99, 0.51; narrow pair 1.13 / 0.92, 0.42; gather 0.10 / 0.86, 0.50 (the hub rows set the baseline's max: a
sequential 6000-term sum against eight chains of fused multiply-adds); backward (dh, dbias) 1.25 / 1.13, 0.62; rank-1 (dh,
dw_head, dbias) 1.01 / 1.00, 0.48; 64-bit form 0.66 / 0.97, 0.56; dinv 1.063 ulp.  No output exceeds a factor or the cap, and
no kernel defect was found.  The module takes 23 s there (tests/test_tsplit_accuracy_gpu.py on the same machine: 30 s)."""
import numpy as np
import pytest
import torch

from oracle import accuracy as acc

pytestmark = pytest.mark.gpu

KINDS = acc.AGG_KINDS
SENTINEL = -12345.5
EPOCH = 77


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unaligned(a):
    """a [rows, f] on the device at an address that is 4 mod 16 (the VEC = 1 kernels)."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    off = next(o for o in range(1, 5) if (buf.data_ptr() + 4 * o) % 16 == 4)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


class _Graph:
    """One built graph and its arrays read back: rt / cs (by target), rs / cd (by source), dinv; live rows n of cap."""

    def __init__(self, prep, n, cap, p):
        self.prep, self.n, self.cap = prep, n, cap
        lens = p["lens"]
        torch.cuda.synchronize()
        self.rt = prep.rowptr_t[:n + 1].cpu().numpy().astype(np.int64)
        self.rs = prep.rowptr_s[:n + 1].cpu().numpy().astype(np.int64)
        self.cs = prep.csr_src.cpu().numpy()[:self.rt[-1]]
        self.cd = prep.csr_dst.cpu().numpy()[:self.rs[-1]]
        self.dinv = prep.dinv.cpu().numpy()
        self.lens, self.lens_s = np.diff(self.rt), np.diff(self.rs)
        assert self.rt[0] == 0 and self.rs[0] == 0 and self.rt[-1] == self.rs[-1]
        assert np.array_equal(self.lens, lens), "the build's rows do not have the prescribed entry counts"
        assert self.cs.max() < n and self.cd.max() < n and self.cs.min() >= 0
        assert self.lens_s.max() > 64
        # ... and the prescribed entries: each row's device entries, sorted, are the edge list's (self-loops dropped, duplicates
        # kept), by target and by source — the references follow the device's ORDER inside a row, not its content
        h_rt, h_cs, h_rs, h_cd, _ = acc.host_csr(p["src"], p["dst"], n)
        for rp, col, h_rp, h_col in ((self.rt, self.cs, h_rt, h_cs), (self.rs, self.cd, h_rs, h_cd)):
            assert np.array_equal(rp, h_rp)
            rows = np.repeat(np.arange(n), np.diff(rp))
            assert np.array_equal(col[np.lexsort((col, rows))], h_col), "the build's rows do not hold the prescribed entries"
        if cap > n:     # the CSR past its live extent names a NaN row
            prep.csr_src[int(self.rt[-1]):] = cap - 1
            prep.csr_dst[int(self.rs[-1]):] = cap - 1


_GRAPHS = {}


def _graph(ops, size, build):
    """build: generic | grouped (source-grouped, one wavefront per row) | records (grouped + head records over local ids) |
    from_csr.  The graph of a size does not depend on kind or width (aggregate_problem draws it first)."""
    key = (size, build)
    if key in _GRAPHS:
        return _GRAPHS[key]
    pad = build != "from_csr"
    p = acc.aggregate_case(size, "normal", 4, pad=pad)
    n, cap = p["n"], p["cap"]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    src, dst = _dev(p["src"]), _dev(p["dst"])
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda") if pad else None
    if build == "generic":
        prep = ops.PreparedGraph(src, dst, cap, d_n=d_n, status=st)
    elif build == "grouped":
        prep = ops.PreparedGraph(src, dst, cap, d_n=d_n, status=st, src_grouped=True, items_fwd=False)
    elif build == "records":
        iota = torch.arange(cap, dtype=torch.int32, device="cuda")
        prep = ops.PreparedGraph(src, dst, cap, d_n=d_n, status=st, src_grouped=True, items_fwd=False, head_ids=iota, head_local=True)
        assert prep.row_head is not None and prep.head_local
    else:
        rt, cs, rs, cd, _ = acc.host_csr(p["src"], p["dst"], n)
        prep = ops.PreparedGraph.from_csr(_dev(rt.astype(np.int32)), _dev(cs.astype(np.int32)), n,
                                          _dev(rs.astype(np.int32)), _dev(cd.astype(np.int32)))
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    g = _Graph(prep, n, cap, p)
    if n > 2048 and build in ("generic", "from_csr"):
        assert int(prep.n_items_t.item()) > 0 and int(prep.n_items_s.item()) > 0        # rows above 64 entries became chunk items
    _GRAPHS[key] = g
    return g


def _judge(got, g, ref, what, lens=None, extra=4):
    """got [cap or n, f] on the device: live rows under both conditions."""
    got = got[:g.n].cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite outputs in live rows"
    return acc.assert_aggregate_accuracy(got, ref[0], ref[1], ref[2], g.lens if lens is None else lens, what, extra)


def _sentinel(cap, f, unaligned=False):
    return _unaligned(np.full((cap, f), SENTINEL, np.float32)) if unaligned else torch.full((cap, f), SENTINEL, device="cuda")


def _untouched(out, g, what):
    if g.cap > g.n:
        assert bool((out[g.n:] == SENTINEL).all()), f"{what}: rows past the live count were written"


# ----------------------------------------------------------------------------------------------------------- the build
def test_dinv_is_within_one_and_a_half_ulp_of_fp64():
    """prep.dinv against fp64 1 / sqrt(deg + 1) for degrees 0, 1, 2, 3, 63, 64, 4095, 19999 (and every other row).  Every build
    computes 1.0f / sqrtf(deg + 1), two IEEE operations that the compiler rounds correctly by default (no fast-math flag in the
    Makefile).  Their documented bound is not 1 ulp but 1.5: the square root is within 2^-24 relative; the quotient inherits that
    relative error, which is up to 1 ulp of a quotient at the top of its binade (an ulp there is 2^-24 relative), and adds
    half an ulp of its own rounding.  So the bound asserted is 1.5 ulp, the documented one of this instruction pair.  Measured on
    the MI355X: worst 1.063 ulp (degree 17) — a single 1-ulp rsqrt would not be met, the pair's bound is."""
    ops = _ops()
    want = (0, 1, 2, 3, 63, 64, 4095, 19999)
    p = acc.aggregate_problem("normal", 2600, want, 4, 9, n_pad=5)
    n, cap = p["n"], p["cap"]
    src, dst = _dev(p["src"]), _dev(p["dst"])
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    rt, cs, rs, cd, _ = acc.host_csr(p["src"], p["dst"], n)
    iota = torch.arange(cap, dtype=torch.int32, device="cuda")
    builds = {
        "generic": ops.PreparedGraph(src, dst, cap, d_n=d_n).dinv,
        "grouped": ops.PreparedGraph(src, dst, cap, d_n=d_n, src_grouped=True, items_fwd=False).dinv,
        "records": ops.PreparedGraph(src, dst, cap, d_n=d_n, src_grouped=True, items_fwd=False, head_ids=iota, head_local=True).dinv,
        "from_csr": ops.PreparedGraph.from_csr(_dev(rt.astype(np.int32)), _dev(cs.astype(np.int32)), n).dinv,
        "large": ops.LargeGraphPlan(_dev(rt), _dev(cs.astype(np.int32)), n, False).dinv,
    }
    deg = p["lens"]
    assert set(want) <= set(deg.tolist())
    exact = 1.0 / np.sqrt(deg.astype(np.float64) + 1.0)
    ulp = np.spacing(exact.astype(np.float32)).astype(np.float64)
    for name, d in builds.items():
        d = d[:n].cpu().numpy().astype(np.float64)
        err = np.abs(d - exact) / ulp
        print(f"[dinv] {name}: worst {err.max():.3f} ulp (degree {int(deg[err.argmax()])})")
        assert err.max() <= 1.5, (name, err.max())


# ------------------------------------------------------------------------------------------------------------- forward
# (width, unaligned view) of gcn_aggregate_fwd
FWD_WIDTHS = [(1, False), (7, False), (16, False), (17, False), (47, False), (100, True), (20, False), (32, False), (64, False),
              (100, False), (128, False), (256, False), (260, False), (512, False)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", ["small", "large"])
def test_forward_aggregation(size, kind):
    """ops.gcn_aggregate_fwd on the generic build with a device-side row count and NaN capacity rows: small graph (every row by
    one wavefront: sequential up to 16 entries, eight chains above) and large graph (rows above 64 entries as chunk items), every
    width with and without bias, with and without ReLU (one set of reference sums per width serves the four)."""
    ops = _ops()
    g = _graph(ops, size, "generic")
    assert g.prep.items_fwd and (g.prep.n > 2048) == (size == "large")
    for f, un in FWD_WIDTHS:
        p = acc.aggregate_case(size, kind, f)
        h = _unaligned(p["h"]) if un else _dev(p["h"])
        bias = _dev(p["bias"])
        sums = acc.aggregate_sums(g.rt, g.cs, g.dinv, p["h"])
        for with_bias, relu in ((True, True), (False, False), (True, False), (False, True)):
            what = f"fwd {size} {kind} f={f}{'u' if un else ''} bias={int(with_bias)} relu={int(relu)}"
            out = _sentinel(g.cap, f, un)
            ops.gcn_aggregate_fwd(h, g.prep, bias if with_bias else None, relu, out=out)
            ref = acc.aggregate_finish(sums, p["bias"] if with_bias else None, relu)
            _judge(out, g, ref, what)
            _untouched(out, g, what)


@pytest.mark.parametrize("kind", KINDS)
def test_record_driven_forward_and_fused_head(kind):
    """The record form (head records over local ids: rows of 0 .. 4 entries inside the record, 5, 16, 17, 200, ... by the walk)
    and the CSR-walking gcn_aggregate_fwd_head, with the head product and the gate bits: `out` under the aggregation's
    conditions; head_out against sum_m out[r][m] w2[m] formed in fp64 FROM THE DEVICE'S out (the head judged on its own: an
    f-term fp32 sum, cap (f + 4) 2^-24 mag); gate bit e of row r == (out[r][e] > 0) of the device's out, bits past f zero."""
    ops = _ops()
    rec, grp = _graph(ops, "small", "records"), _graph(ops, "small", "grouped")
    for ln in (0, 1, 2, 4, 5, 16, 17, 200):
        assert (rec.lens == ln).any()
    for f in (20, 64, 100, 256):
        p = acc.aggregate_case("small", kind, f)
        h, bias, w2 = _dev(p["h"]), _dev(p["bias"]), _dev(p["w2"])
        assert ops._rec_form(rec.prep, rec.cap, f) and not ops._rec_form(grp.prep, grp.cap, f)
        for relu in (True, False):
            ref = acc.aggregate_reference(rec.rt, rec.cs, rec.dinv, p["h"], p["bias"], relu)
            out = _sentinel(rec.cap, f)
            ops.gcn_aggregate_fwd(h, rec.prep, bias, relu, out=out)
            _judge(out, rec, ref, f"rec {kind} f={f} relu={int(relu)}")
            _untouched(out, rec, "rec")
        if f == 20:
            continue
        ref = acc.aggregate_reference(rec.rt, rec.cs, rec.dinv, p["h"], p["bias"], True)
        for name, g in (("rec", rec), ("walk", grp)):
            if name == "walk" and not np.array_equal(g.cs, rec.cs):      # (a row's entry order is each build's own)
                ref = acc.aggregate_reference(g.rt, g.cs, g.dinv, p["h"], p["bias"], True)
            r = ops.gcn_aggregate_fwd_head(h, g.prep, bias, True, w2, want_bits=True)
            assert r is not None and r[2] is not None
            out, hw, bits = r
            n = g.n
            what = f"head/{name} {kind} f={f}"
            _judge(out, g, ref, what + " out")
            o64 = out[:n].cpu().double()
            w64 = torch.from_numpy(p["w2"].astype(np.float64))
            terms = (out[:n].cpu().numpy() * p["w2"]).astype(np.float32)
            base = torch.from_numpy(np.add.accumulate(terms, axis=1, dtype=np.float32)[:, -1].copy())
            acc.assert_aggregate_accuracy(hw[:n, 0].cpu(), o64 @ w64, o64.abs() @ w64.abs(), base, float(f), what + " head_out")
            got = ((bits[:n].view(n, 8, 1) >> torch.arange(32, device="cuda", dtype=torch.int32).view(1, 1, 32)) & 1).reshape(n, 256)
            assert torch.equal(got[:, :f].bool(), out[:n] > 0), what + " gate bits"
            assert int(got[:, f:].sum()) == 0, what + " bits past f"


@pytest.mark.parametrize("kind", KINDS)
def test_prescaled_forward(kind):
    """scale_rows (exactly fl32(dinv h)) + gcn_aggregate_fwd_prescaled: small generic build (device-side count) and the
    full-graph from_csr build (long rows as items), each with and without bias, with and without ReLU.  One more rounding per term: cap L + 5."""
    ops = _ops()
    for size, build in (("small", "generic"), ("large", "from_csr")):
        g = _graph(ops, size, build)
        for f in (32, 48, 64, 100, 128, 256):
            p = acc.aggregate_case(size, kind, f, pad=build != "from_csr")
            h = _dev(p["h"])
            hs = ops.scale_rows(h, g.prep.dinv)
            want = (g.dinv[:g.n, None] * p["h"][:g.n]).astype(np.float32)
            assert np.array_equal(hs[:g.n].cpu().numpy(), want), f"scale_rows {kind} f={f}"
            sums = acc.aggregate_sums(g.rt, g.cs, g.dinv, p["h"], prescaled=True)
            for with_bias, relu in ((True, True), (False, False), (True, False), (False, True)):
                out = _sentinel(g.cap, f)
                ops.gcn_aggregate_fwd_prescaled(hs, g.prep, _dev(p["bias"]) if with_bias else None, relu, out=out)
                ref = acc.aggregate_finish(sums, p["bias"] if with_bias else None, relu)
                what = f"prescaled {size} {kind} f={f} bias={int(with_bias)} relu={int(relu)}"
                _judge(out, g, ref, what, extra=5)
                _untouched(out, g, what)


@pytest.mark.parametrize("kind", KINDS)
def test_narrow_pair(kind):
    """gcn_aggregate_narrow_pair: two [n, 1] vectors over one graph in one launch, one with a bias."""
    ops = _ops()
    for size in ("small", "large"):
        g = _graph(ops, size, "generic")
        p = acc.aggregate_case(size, kind, 1)
        a, b = ops.gcn_aggregate_narrow_pair(_dev(p["h"]), _dev(p["dout"]), g.prep, _dev(p["bias"]), None)
        _judge(a, g, acc.aggregate_reference(g.rt, g.cs, g.dinv, p["h"], p["bias"], False), f"narrow pair a {size} {kind}")
        _judge(b, g, acc.aggregate_reference(g.rt, g.cs, g.dinv, p["dout"], None, False), f"narrow pair b {size} {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_fused_gather_aggregation(kind):
    """gcn_aggregate_gather: Â [X[ids] | indicator bits | 0] without the gathered matrix, by the CSR walk (plain build) and by
    the head records (build with head_ids = ids): 32- and 64-lane forms; ids with repeats, capacity ids -> a NaN row of X;
    every fourth node's indicator word carries a stale epoch with all bits set, which reads 0.  The pad columns have mag 0 and
    must be exactly 0."""
    ops = _ops()
    plain = _graph(ops, "small", "grouped")
    n, cap = plain.n, plain.cap
    rng = np.random.default_rng(17)
    ids_np = np.full(cap, cap - 1, np.int32)
    ids_np[:n] = rng.integers(0, n, n)
    ids = _dev(ids_np)
    key = ("small", "heads")
    if key not in _GRAPHS:
        p0 = acc.aggregate_case("small", "normal", 4)
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        prep = ops.PreparedGraph(_dev(p0["src"]), _dev(p0["dst"]), cap, d_n=d_n, status=st, src_grouped=True, head_ids=ids)
        assert int(st.item()) == 0 and prep.row_head is not None
        _GRAPHS[key] = (_Graph(prep, n, cap, p0), ids)
    heads, ids = _GRAPHS[key]
    ids_np = ids.cpu().numpy()
    for F, ni in ((6, 5), (100, 4), (128, 3), (602, 3)):
        p = acc.aggregate_case("small", kind, F)
        ldx, kp = (F + 3) // 4 * 4, (F + ni + 3) // 4 * 4
        Xp = np.zeros((cap, ldx), np.float32)
        Xp[:, :F] = p["h"]                                          # (rows n .. cap - 1 NaN: the capacity ids read the last)
        code = ((EPOCH << 8) | rng.integers(0, 1 << ni, cap)).astype(np.int64)
        code[::4] = ((EPOCH - 1) << 8) | 0xff
        feat = np.zeros((cap, kp), np.float32)
        feat[:, :F] = p["h"][ids_np]
        bits = np.where((code >> 8) == EPOCH, code & 0xff, 0)[ids_np]
        feat[:, F:F + ni] = (bits[:, None] >> np.arange(ni)) & 1
        feat[n:] = np.nan
        X, cd = _dev(Xp), _dev(code.astype(np.int32))
        ref = acc.aggregate_reference(plain.rt, plain.cs, plain.dinv, feat, None, False)
        for name, g in (("plain", plain), ("heads", heads)):
            if name == "heads" and not np.array_equal(g.cs, plain.cs):    # (a row's entry order is each build's own)
                ref = acc.aggregate_reference(g.rt, g.cs, g.dinv, feat, None, False)
            out = _sentinel(cap, kp)
            ops.gcn_aggregate_gather(X, ids, g.prep, cd, EPOCH, ni, out=out, F=F)
            what = f"gather/{name} {kind} {F}+{ni}"
            _judge(out, g, ref, what)
            _untouched(out, g, what)


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", ["small", "rows9k"])
def test_backward_aggregation(size, kind):
    """ops.gcn_aggregate_bwd: dh = Âᵀ (dout ⊙ [relu_out > 0]) over the by-source CSR and dbias = its column sums, judged
    separately; 1537 rows (the one-launch ticket form) and 9023 (> 8192: column-sum pass + aggregation, long rows as items);
    relu_out given / not, crossed with dbias fresh / accumulated onto a prior value (its magnitude gains |prior|), at every width."""
    ops = _ops()
    g = _graph(ops, size, "generic")
    assert (g.cap > 8192) == (size == "rows9k")
    n = g.n
    for f in (1, 16, 47, 64, 256, 512):
        p = acc.aggregate_case(size, kind, f)
        dout, act = _dev(p["dout"]), _dev(p["act"])
        for gated in (True, False):
            dpre = np.where(p["act"] > 0, p["dout"], np.float32(0)) if gated else p["dout"]
            dpre = np.where(np.isnan(p["dout"]), np.float32(np.nan), dpre)
            ref = acc.aggregate_reference(g.rs, g.cd, g.dinv, dpre, None, False)
            for accumulate in (False, True):
                what = f"bwd {size} {kind} f={f} gate={int(gated)} acc={int(accumulate)}"
                prior = p["bias"] * 3 if accumulate else None
                db = _dev(prior) if accumulate else None
                dh, db = ops.gcn_aggregate_bwd(dout, g.prep, relu_out=act if gated else None, dbias=db, accumulate_bias=accumulate)
                _judge(dh, g, ref, what + " dh", lens=g.lens_s)
                cref = acc.colsum_reference(p["dout"][:n], gate=p["act"][:n] if gated else None, prior=prior)
                acc.assert_aggregate_accuracy(db.cpu(), *cref, float(n), what + " dbias")


def _pack_bits(act, f):
    """[rows, 8] int32: element e of a row = bit e % 32 of word e // 32, set where act > 0 (NaN rows: 0)."""
    rows = act.shape[0]
    b = np.zeros((rows, 256), np.uint64)
    b[:, :f] = np.nan_to_num(act, nan=0.0) > 0
    words = (b.reshape(rows, 8, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return words.view(np.int32)


@pytest.mark.parametrize("kind", KINDS)
def test_rank1_backward(kind):
    """gcn_aggregate_bwd_rank1 from the activation rows, from their gate bits, and two problems in one _multi call: dh, dw_head
    and dbias each; fresh and accumulated.  Small graph (no items) and large (long by-source rows as chunk items)."""
    ops = _ops()
    gs = {size: _graph(ops, size, "generic") for size in ("small", "large")}
    for f in (64, 100, 256):
        probs = {}
        for size, g in gs.items():
            n = g.n
            p = acc.aggregate_case(size, kind, f)
            act, dh2, w2 = _dev(p["act"]), _dev(p["dh2"]), _dev(p["w2"])
            bits = _dev(_pack_bits(p["act"], f))
            prior_w, prior_b = p["bias"] * 2, p["bias"] * -3
            fresh = acc.rank1_reference(g.rs, g.cd, g.dinv, p["act"], p["dh2"], p["w2"])
            accum = acc.rank1_reference(g.rs, g.cd, g.dinv, p["act"], p["dh2"], p["w2"], prior_dw=prior_w, prior_db=prior_b)
            probs[size] = dict(act=act, dh2=dh2, w2=w2, bits=bits, fresh=fresh, accum=accum, prior_w=prior_w, prior_b=prior_b)
            for form, gb in (("act", None), ("bits", bits)):
                for accumulate, ref in ((False, fresh), (True, accum)):
                    dw = _dev(prior_w) if accumulate else torch.full((f,), SENTINEL, device="cuda")
                    db = _dev(prior_b) if accumulate else torch.full((f,), SENTINEL, device="cuda")
                    dh = ops.gcn_aggregate_bwd_rank1(act, dh2, w2, g.prep, dw_head=dw, dbias=db, accumulate=accumulate, gate_bits=gb)
                    what = f"rank1/{form} {size} {kind} f={f} acc={int(accumulate)}"
                    _judge(dh, g, ref["dh"], what + " dh", lens=g.lens_s, extra=5)
                    acc.assert_aggregate_accuracy(dw.cpu(), *ref["dw_head"], float(n), what + " dw_head", 5)
                    acc.assert_aggregate_accuracy(db.cpu(), *ref["dbias"], float(n), what + " dbias", 5)
        # two problems, one call: the small one accumulates onto its priors, the large one writes fresh
        a, b = probs["small"], probs["large"]
        dwa, dba = _dev(a["prior_w"]), _dev(a["prior_b"])
        dwb, dbb = torch.full((f,), SENTINEL, device="cuda"), torch.full((f,), SENTINEL, device="cuda")
        dhs = ops.gcn_aggregate_bwd_rank1_multi([
            dict(act=a["act"], dh2=a["dh2"], w2=a["w2"], prep=gs["small"].prep, gate_bits=a["bits"], dw_head=dwa, dbias=dba, accumulate=True),
            dict(act=b["act"], dh2=b["dh2"], w2=b["w2"], prep=gs["large"].prep, gate_bits=b["bits"], dw_head=dwb, dbias=dbb)])
        for size, dh, dw, db, ref in (("small", dhs[0], dwa, dba, a["accum"]), ("large", dhs[1], dwb, dbb, b["fresh"])):
            g = gs[size]
            what = f"rank1/multi {size} {kind} f={f}"
            _judge(dh, g, ref["dh"], what + " dh", lens=g.lens_s, extra=5)
            acc.assert_aggregate_accuracy(dw.cpu(), *ref["dw_head"], float(g.n), what + " dw_head", 5)
            acc.assert_aggregate_accuracy(db.cpu(), *ref["dbias"], float(g.n), what + " dbias", 5)


# --------------------------------------------------------------------------------------------- 64-bit full-graph form
@pytest.mark.parametrize("kind", KINDS)
def test_large_graph_aggregation(kind):
    """gcn_large_aggregate forced on a small graph (64-bit row offsets, chunk = 1024 < the hubs of 5000 and 20000): the by-target
    CSR of the directed graph (not symmetric: the plan holds the transpose) and a symmetrised graph's own arrays (symmetric);
    prescaled and not.  Self-loop entries stay in the CSR: the kernels skip them.  Both CSRs are formed on the host, not with
    ops.csr_transpose: that build collapses duplicate (row, col) pairs to one entry by contract (csrc/ingest_kernels.hip), and
    the duplicate edges of these rows — how a 20000-entry hub fits 2600 nodes — are part of what is tested."""
    ops = _ops()
    p0 = acc.aggregate_case("large", "normal", 4, pad=False)
    n = p0["n"]
    src, dst = p0["src"].astype(np.int64), p0["dst"].astype(np.int64)
    for symmetric in (False, True):
        if symmetric:
            s2, d2 = np.concatenate([src, dst]), np.concatenate([dst, src])
        else:
            s2, d2 = src, dst
        o = np.lexsort((s2, d2))                                    # by target, sources ascending (self-loops kept)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(d2, minlength=n))]).astype(np.int64)
        col = s2[o].astype(np.int32)
        rp, cl = _dev(rowptr), _dev(col)
        plan = ops.LargeGraphPlan(rp, cl, n, symmetric, chunk=1024)
        assert plan.item_cap > 0
        keep = col != np.repeat(np.arange(n), np.diff(rowptr))
        rt = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(n), np.diff(rowptr))[keep], minlength=n))])
        cs = col[keep]
        dinv = plan.dinv.cpu().numpy()
        lens = np.diff(rt)
        assert lens.max() > 1024
        for f in (100, 128):
            p = acc.aggregate_case("large", kind, f, pad=False)
            h, bias = _dev(p["h"]), _dev(p["bias"])
            for prescaled in (False, True):
                hin = ops.scale_rows(h, plan.dinv) if prescaled else h
                out = ops.gcn_large_aggregate(hin, plan, prescaled, r0=0, m=n, bias=bias, relu=True)
                ref = acc.aggregate_reference(rt, cs, dinv, p["h"], p["bias"], True, prescaled=prescaled)
                what = f"large sym={int(symmetric)} {kind} f={f} pre={int(prescaled)}"
                got = out.cpu()
                assert bool(torch.isfinite(got).all()), what
                acc.assert_aggregate_accuracy(got, ref[0], ref[1], ref[2], lens, what, 5 if prescaled else 4)
