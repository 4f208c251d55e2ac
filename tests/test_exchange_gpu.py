"""csrc/exchange_kernels.hip on ONE MI355X with P simulated ranks: every rank's shard lives on the same GPU, the
all-gather / all-to-all are done by hand (concatenate / transpose the slots), and the kernels either side of them
must reproduce, for every case of tests/exchange_oracle.CASES, (a) the independent reference's messages word for word —
headers, columns, untouched words and status words included — and (b) the oracle's get_neighborhoods (utils.py:74-82) /
X[ids] plus indicator columns bit for bit.  tests/test_exchange_cpu.py holds the CPU double of the gloo tests
(tests/dist_worker.OracleLocalOps) to the same reference, so the test families pin one layout.  Integer work and bit
copies: every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exchange_oracle as XO  # noqa: E402


def _ids(cases):
    return [c.id for c in cases]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _dev(a, off=0):
    """numpy array -> cuda tensor of its shape that starts `off` elements into its allocation: 0 = 16-byte aligned (what the
    vector paths need), 1 = one float in (what takes them away)"""
    a = np.ascontiguousarray(a)
    flat = torch.empty(a.size + 4, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    t = flat[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and (a.size == 0 or t.data_ptr() % 16 == 4 * off)
    return t


def _word(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def _bits(t):
    return XO.bits(t.detach().cpu().numpy())


@pytest.mark.parametrize("case", XO.ROWS_CASES, ids=_ids(XO.ROWS_CASES))
def test_adjacency_rows(case):
    """serve_offsets_k / serve_expand_k at every owner, recv_offsets_k / recv_expand_k at every requester"""
    _cuda()
    from grapes_amd import ops
    part = case.part
    ref, P, cap, stride, e_cap = part.ref, part.P, part.cap, part.stride, part.e_cap
    req, b32 = _dev(part.req.reshape(-1)), _dev(np.asarray(part.bounds, np.int32))
    for o in range(P):
        rp, cl, lo, hi = part.shard(o)
        reply, status = _dev(np.full(P * stride, XO.FILL, np.int32)), _word(0)
        ops.exchange_serve_rows(_dev(rp), _dev(cl), req, P, cap, lo, hi, reply, stride, part.e_slot, status=status)
        got = reply.cpu().numpy().reshape(P, stride)
        for p in range(P):
            assert np.array_equal(got[p], ref["replies"][o][p]), f"owner {o}: the slot of peer {p} differs from the reference"
        assert int(status) == ref["serve_status"][o], f"owner {o}"
    for r in range(P):
        # (the replies ARE the reference's, word for word: the requester reads the reference's, transposed by hand)
        back = _dev(ref["backs"][r].reshape(-1))
        nodes, m = part.req[r, :cap], part.counts[r]
        status = _word(0)
        src, dst, d_e, eoff = ops.exchange_recv_rows(back, stride, _dev(nodes), b32, P, e_cap, d_m=_word(int(part.req[r, cap])),
                                                     status=status)
        rsrc, rdst, re, reoff, rstatus = ref["recv"][r]
        true = XO.true_edges(part.indptr, part.indices, nodes, m)
        e = true.shape[1]
        k = min(e, e_cap)
        assert src.numel() == dst.numel() == e_cap
        assert int(d_e) == e == re and int(eoff[m]) == e                              # the TRUE total, overflow or not
        assert int(status) == rstatus == (XO.EDGE_OVERFLOW if e > e_cap else 0)
        assert np.array_equal(eoff[:m + 1].cpu().numpy(), reoff[:m + 1])
        assert np.array_equal(src[:k].cpu().numpy(), rsrc[:k]) and np.array_equal(dst[:k].cpu().numpy(), rdst[:k])
        assert np.array_equal(src[:k].cpu().numpy().astype(np.int64), true[0, :k])    # the exact prefix of the true edge list
        assert np.array_equal(dst[:k].cpu().numpy().astype(np.int64), true[1, :k])
    # d_m = None: the whole list (only where no padding follows the count), and a requester whose capacity is below its total
    # (the owners did not overflow): status, the true total, the exact prefix, and nothing past its buffers
    r = next((r for r in range(P) if part.counts[r] == cap), None)
    if r is not None and not any(ref["serve_status"]):
        nodes = part.req[r, :cap]
        true = XO.true_edges(part.indptr, part.indices, nodes, cap)
        e = true.shape[1]
        back = _dev(ref["backs"][r].reshape(-1))
        status = _word(0)
        src, dst, d_e, eoff = ops.exchange_recv_rows(back, stride, _dev(nodes), b32, P, e_cap, d_m=None, status=status)
        assert int(d_e) == e and int(status) == ref["recv"][r][4]
        assert np.array_equal(dst[:min(e, e_cap)].cpu().numpy().astype(np.int64), true[1, :e_cap])
        small = 1000 if "legacy" in case.id else e // 2
        if small >= 1:
            status = _word(0)
            src, dst, d_e, eoff = ops.exchange_recv_rows(back, stride, _dev(nodes), b32, P, small, d_m=None, status=status)
            assert int(status) == XO.EDGE_OVERFLOW and src.numel() == small and int(d_e) == e and int(eoff[cap]) == e
            assert np.array_equal(src.cpu().numpy().astype(np.int64), true[0, :small])
            assert np.array_equal(dst.cpu().numpy().astype(np.int64), true[1, :small])


def test_recv_rows_refuses_a_stride_below_its_capacity():
    """a requester's e_cap must not exceed the owners' e_slot; reply_stride < 2 cap + e_cap is all the call can see of it, and
    it is refused on the host: nothing is launched"""
    _cuda()
    from grapes_amd import _lib, ops
    P, cap, e_slot = 2, 8, 16
    stride = 2 * cap + e_slot
    back = torch.zeros(P * stride, dtype=torch.int32, device="cuda")
    nodes = torch.arange(cap, dtype=torch.int32, device="cuda")
    b32 = torch.tensor([0, 4, 8], dtype=torch.int32, device="cuda")
    status = _word(0)
    with pytest.raises(_lib.GrapesHipError, match="invalid argument"):
        ops.exchange_recv_rows(back, stride, nodes, b32, P, e_slot + 1, status=status)
    src, dst, d_e, _ = ops.exchange_recv_rows(back, stride, nodes, b32, P, e_slot, status=status)     # the largest it takes
    assert int(d_e) == 0 and int(status) == 0


@pytest.mark.parametrize("case", XO.FEAT_CASES, ids=_ids(XO.FEAT_CASES))
def test_halo_rows(case):
    """serve_rows_k<VEC> at every owner, halo_assemble_k<VLOAD, VSTORE> at every requester — on the path the case is named for"""
    _cuda()
    from grapes_amd import ops
    part = case.part
    ref, P, F, capf, n_slot, k, mis = part.ref, part.P, part.F, part.capf, part.n_slot, part.num_ind, part.misalign
    assert f"serve<{XO.serve_path(F, mis)}>" in case.id and f"assemble<{XO.assemble_path(F, k, mis)}>" in case.id
    req, b32, code = _dev(part.req.reshape(-1)), _dev(np.asarray(part.bounds, np.int32)), _dev(part.code)
    for o in range(P):
        lo, hi = part.bounds[o], part.bounds[o + 1]
        reply, status = _dev(np.full(P * n_slot * F, XO.FILL_F, np.float32), off=int(mis == "reply")), _word(0)
        ops.exchange_serve_features(_dev(part.X[lo:hi], off=int(mis == "X_local")), req, P, capf, lo, hi, reply, n_slot, status=status)
        assert np.array_equal(_bits(reply).reshape(P, n_slot, F), XO.bits(ref["replies"][o])), f"owner {o}"
        assert int(status) == ref["serve_status"][o], f"owner {o}"
    d_epoch = None if part.d_epoch is None else _dev(np.array([part.d_epoch], np.uint32).view(np.int32))
    for r in range(P):
        ids, n = part.req[r, :capf], part.counts[r]
        back = _dev(ref["backs"][r].reshape(-1), off=int(mis == "back"))
        out = _dev(np.full((capf, F + k), XO.FILL_F, np.float32), off=int(mis == "out"))
        got = ops.exchange_assemble_features(back, F, n_slot, _dev(ids), b32, P, d_n=_word(int(part.req[r, capf])),
                                             ind_code=code if k else None, epoch=part.epoch, d_epoch=d_epoch, num_ind=k, out=out)
        assert got is out and out.shape == (capf, F + k)
        assert np.array_equal(_bits(out), XO.bits(ref["outs"][r])), f"requester {r}"   # rows past the count keep their NaN fill
        ex = part.exact_rows(r)
        assert np.array_equal(_bits(out[:n])[ex], XO.bits(XO.true_rows(part.X, ids, n, part.code, part.epoch_live, k))[ex])
        assert np.array_equal(_bits(out[:n]), XO.bits(XO.true_rows_clamped(part, r)))
    if "legacy" in case.id:
        # d_n = None takes the whole list; a halo slot that is too small raises NODE_OVERFLOW (and nothing else)
        out = ops.exchange_assemble_features(_dev(ref["backs"][0].reshape(-1)), F, n_slot, _dev(part.req[0, :capf]), b32, P,
                                             ind_code=code if k else None, epoch=part.epoch, num_ind=k)
        assert part.counts[0] == capf and np.array_equal(_bits(out), XO.bits(ref["outs"][0]))
        status = _word(0)
        tiny = torch.zeros(P * 8 * F, dtype=torch.float32, device="cuda")
        ops.exchange_serve_features(_dev(part.X[:part.bounds[1]]), req, P, capf, 0, part.bounds[1], tiny, 8, status=status)
        assert int(status) == XO.NODE_OVERFLOW


@pytest.mark.parametrize("case", XO.FEAT_CASES, ids=_ids(XO.FEAT_CASES))
def test_positions_and_noted_rows(case):
    """halo_positions_k with code_pos on every halo case; exchange_note_rows_k in both forms over a kept buffer"""
    _cuda()
    import ctypes as C
    from grapes_amd import _lib, ops
    part = case.part
    ref, P, capf, n_slot = part.ref, part.P, part.capf, part.n_slot
    b32, code = _dev(np.asarray(part.bounds, np.int32)), _dev(part.code)
    for r in range(P):
        ids, n = part.req[r, :capf], part.counts[r]
        rpos, rcpos, shared = ref["positions"][r]
        pos, cpos = _dev(np.full(capf, XO.FILL, np.int32)), _dev(np.full(P * n_slot, XO.FILL, np.int32))
        got = ops.exchange_halo_positions(_dev(ids), b32, P, n_slot, d_n=_word(int(part.req[r, capf])), ind_code=code, pos=pos,
                                          code_pos=cpos)
        assert got[0] is pos and got[1] is cpos
        keep = np.ones(P * n_slot, bool)
        keep[sorted(shared)] = False                # clamped rows of an overflowing run share a word: its value is unspecified
        assert np.array_equal(pos.cpu().numpy(), rpos), f"requester {r}"               # rows past the count: 0
        assert np.array_equal(cpos.cpu().numpy()[keep], rcpos[keep]), f"requester {r}"  # untouched words keep their fill
        own = ~np.isin(rpos[:n], sorted(shared))
        assert np.array_equal(cpos.cpu().numpy()[rpos[:n][own]], part.code[ids[:n][own]])
        pos2 = _dev(np.full(capf, XO.FILL, np.int32))                                   # without indicator words
        assert ops.exchange_halo_positions(_dev(ids), b32, P, n_slot, d_n=_word(int(part.req[r, capf])), pos=pos2)[1] is None
        assert np.array_equal(pos2.cpu().numpy(), rpos)
    # the n == 0 early return leaves pos alone; ind_code without code_pos and code_pos without ind_code are refused
    L = _lib.load()
    ids0 = _dev(part.req[0, :capf])
    pos = _dev(np.full(capf, XO.FILL, np.int32))
    args = lambda n, code_, cpos_: (C.c_void_p(ids0.data_ptr()), n, None, C.c_void_p(b32.data_ptr()), P, n_slot, code_,
                                    C.c_void_p(pos.data_ptr()), cpos_, None)
    cpos = _dev(np.full(P * n_slot, XO.FILL, np.int32))
    assert L.grapes_exchange_halo_positions(*args(0, None, None)) == 0
    assert L.grapes_exchange_halo_positions(*args(capf, C.c_void_p(code.data_ptr()), None)) != 0
    assert L.grapes_exchange_halo_positions(*args(capf, None, C.c_void_p(cpos.data_ptr()))) != 0
    torch.cuda.synchronize()
    assert bool((pos == XO.FILL).all()) and bool((cpos == XO.FILL).all())
    if case not in XO.NOTE_CASES:
        return
    # ---- noted rows: loc word for word, then rows_from_kept's gather over a buffer laid out as dist._kept_buffer lays it out
    s = XO.note_scenario(part)
    loc, pos = _dev(s["loc0"]), _dev(s["pos"])
    ops.exchange_note_rows(loc, _dev(s["ids_a"]), pos, s["base"], d_n=_word(s["count_a"]), node_map=_dev(s["node_map"]),
                           batch=_dev(s["batch"]), d_n_batch=_word(s["n_batch"]))
    assert np.array_equal(loc.cpu().numpy(), s["loc_a"])
    ops.exchange_note_rows(loc, _dev(s["ids_b"]), pos, s["base"], d_n=_word(s["count_b"]), idx_a=_dev(s["idx_a"]), idx_b=_dev(s["idx_b"]))
    assert np.array_equal(loc.cpu().numpy(), s["loc_b"])
    want = _dev(s["want"].astype(np.int32))
    rows = _dev(s["kept"])[loc[want.long()].long()]
    assert np.array_equal(_bits(rows), XO.bits(part.X[s["want"]]))


@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("lanes", [32, 64])
def test_in_place_gather_over_exchanged_rows(P, lanes):
    """The in-place form the header promises: grapes_gcn_aggregate_gather_fwd(X = back, ids = pos, ind_code = code_pos) with head
    records built on head_ids = pos equals, bit for bit, the gather over the full padded matrix with head_ids = ids and ind_code
    (same rows, same summation order).  The graph is test_gather_pair_gpu._Problem's — rows of 0, 1-4 and 5-16 entries and a hub
    row — over ASCENDING ids, with a device row count below the capacity."""
    _cuda()
    from grapes_amd import ops
    from grapes_amd.dist import partition_bounds
    import test_gather_pair_gpu as G
    F, n_cap, n_live = G.WIDTHS[lanes], G.N_ROWS, G.N_ROWS - 19
    rng = np.random.default_rng(100 * P + lanes)
    lens = rng.choice([0, 1, 2, 3, 4, 5, 9, 16], n_live, p=[.1, .25, .2, .15, .1, .08, .07, .05])
    lens[:4] = [0, 4, 5, 16]
    lens[int(rng.integers(4, n_live))] = 40
    ids_np = np.sort(rng.permutation(G.N_X)[:n_cap]).astype(np.int32)
    ids_np[n_live:] = 0                                                        # padding past the device count
    code_np = ((G.EPOCH << 8) | rng.integers(0, 1 << G.NUM_IND, G.N_X)).astype(np.int32)
    code_np[::5] = ((G.EPOCH - 1) << 8) | 0x7                                  # stale words
    X = G._t(rng.standard_normal((G.N_X, F)).astype(np.float32))
    Xp = ops.pad_features(X)[0]                                                # [N_X, ldx]: what every rank's shard is cut from
    ldx = Xp.shape[1]
    src, dst = G._edges(rng, n_live, lens)
    ids, code, d_n = G._t(ids_np), G._t(code_np), _word(n_live)
    prep = ops.PreparedGraph(src, dst, n_cap, d_n=d_n, head_ids=ids)
    got = (prep.rowptr_t[1:n_live + 1] - prep.rowptr_t[:n_live]).cpu().numpy()
    assert prep.row_head is not None and np.array_equal(got, lens) and got.max() == 40
    want = torch.full((n_cap, (F + G.NUM_IND + 3) // 4 * 4), float("nan"), device="cuda")
    ops.gcn_aggregate_gather(Xp, ids, prep, code, G.EPOCH, G.NUM_IND, out=want, F=F)
    # the exchange: one requester's list, served by P owners out of their shards of the padded matrix
    b = partition_bounds(G.N_X, P)
    b32 = G._t(np.asarray(b, np.int32))
    runs = np.diff(np.searchsorted(ids_np[:n_live], b))
    n_slot = int(runs.max()) + 3
    req = torch.cat([ids, d_n])
    status = _word(0)
    back = torch.full((P, n_slot * ldx), float("nan"), device="cuda")
    for o in range(P):
        reply = torch.full((n_slot * ldx,), float("nan"), device="cuda")
        ops.exchange_serve_features(Xp[b[o]:b[o + 1]].contiguous(), req, 1, n_cap, b[o], b[o + 1], reply, n_slot, status=status)
        back[o] = reply                                                        # the all-to-all, by hand
    back = back.reshape(-1)
    pos, code_pos = ops.exchange_halo_positions(ids, b32, P, n_slot, d_n=d_n, ind_code=code)
    assert int(status) == 0 and bool((pos[n_live:] == 0).all())
    prep_pos = ops.PreparedGraph(src, dst, n_cap, d_n=d_n, head_ids=pos)
    out = torch.full_like(want, float("nan"))
    ops.gcn_aggregate_gather(back.view(-1, ldx), pos, prep_pos, code_pos, G.EPOCH, G.NUM_IND, out=out, F=F)
    assert not bool(torch.isnan(want[:n_live]).any())
    assert torch.equal(out[:n_live], want[:n_live])
    assert np.array_equal(_bits(out[n_live:]), _bits(want[n_live:]))           # rows past the device count: both leave them alone


def test_pack_query_message():
    """[cap ids | live count] in one launch: ids copied, padding untouched, count clamped to the list length."""
    from grapes_amd import ops
    ids = torch.arange(100, 700, dtype=torch.int32, device="cuda")
    for cap, d_n, want in ((600, None, 600), (900, torch.tensor([123], dtype=torch.int32, device="cuda"), 123),
                           (900, torch.tensor([5000], dtype=torch.int32, device="cuda"), 600)):
        q = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
        ops.exchange_pack_query(ids, d_n, cap, q)
        assert torch.equal(q[:600], ids) and int(q[cap]) == want and bool((q[600:cap] == -7).all())
