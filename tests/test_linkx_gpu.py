"""LINKX on the MI355X (grapes_amd/csrc/bag_kernels.hip, modules/linkx.py, linkx.py) against the host oracle of tests/linkx_oracle.py.

The batch tables are integers and bit-exact.  The forward and the row-sparse backward are held element-wise to the derived bound
gamma_d sum |terms| against fp64 (d = the row's or segment's length plus the bias; tests/test_pprgo_gpu.py's bound).  The fused
row-sparse Adam is held to the fp32-baseline criterion of the LABOR importance test: its largest element-wise error against fp64
may be at most 4 times that of torch.optim.SparseAdam run in fp32 on the CPU from the same inputs — a different but equally
valid fp32 summation order — on the same tensor; both errors are printed.  The trainer is judged at tests/test_sage_gpu.py's
tolerances (1e-5 activations and losses, 1e-4 gradients and parameters) by its measure."""
import re

import numpy as np
import pytest
import torch

from tests import linkx_oracle as LO

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4
MARK = -7
GUARD = 16
F32, F64 = np.float32, np.float64
WIDTHS = [1, 3, 4, 63, 64, 65, 256, 1024]


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def rel_err(a, ref):
    a, ref = np.asarray(a, dtype=F64), np.asarray(ref, dtype=F64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


# ---------------------------------------------------------------------------------------------------- the batch tables
def _batch(ops, ip, ix, rows, u_cap=None, e_cap=None, scratch=None):
    """One grapes_bag_batch with guard values behind the capacities -> (oracle, the five host arrays, status, scratch)."""
    N = len(ip) - 1
    ob = LO.batch(ip, ix, rows)
    uc, ec = max(ob.n_u, 1) if u_cap is None else u_cap, max(ob.e, 1) if e_cap is None else e_cap
    m = len(rows)
    if scratch is None:
        scratch = (torch.zeros((N + 63) // 64, dtype=torch.int64, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"))
    full = lambda n: torch.full((n + GUARD,), MARK, dtype=torch.int32, device="cuda")
    out = (full(m + 1), full(uc), full(uc + 1), full(ec), full(4))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.bag_batch(_dev(ip), _dev(ix), N, _dev(np.asarray(rows, dtype=np.int32)), scratch, uc, ec, status=status, out=out)
    host = [_np(t) for t in out]
    for h, n in zip(host, (m + 1, uc, uc + 1, ec, 4)):
        assert (h[n:] == MARK).all(), "a write behind a capacity"
    assert int(scratch[0].abs().sum()) == 0 and int(scratch[1].abs().sum()) == 0, "the scratch maps are not returned zero"
    return ob, host, int(status.item()), scratch


def _same(ob, host):
    bptr, uniq, tptr, trow, counts = host
    assert counts[:4].tolist() == [ob.n_u, ob.e, ob.seg_max, ob.row_max]
    assert np.array_equal(bptr[:len(ob.bptr)], ob.bptr)
    assert np.array_equal(uniq[:ob.n_u], ob.uniq) and np.array_equal(tptr[:ob.n_u + 1], ob.tptr) and np.array_equal(trow[:ob.e], ob.trow)


def _hand_graph():
    """1 200 nodes; rows 0 .. 5 hold 0 / 1 / 63 / 64 / 65 / 1 000 entries (the hub row), the others 0 .. 6; with duplicates and loops."""
    rng = np.random.default_rng(5)
    N = 1200
    rows_of = [rng.integers(0, N, d).tolist() for d in [0, 1, 63, 64, 65, 1000] + rng.integers(0, 7, N - 6).tolist()]
    rows_of[2][5] = rows_of[2][4]; rows_of[5][10] = 5; rows_of[5][500] = rows_of[5][499]; rows_of[7] = [7, 0, N - 1, 7]
    return LO.csr(rows_of, N)


def test_batch_hand_graph_row_lengths_and_the_hub_row():
    ops = _ops()
    ip, ix = _hand_graph()
    rows = [5, 0, 1, 2, 3, 4, 7, 100, 5, 1199, 0]                       # the hub twice, empty rows, ids 0 and N - 1
    ob, host, status, scratch = _batch(ops, ip, ix, rows)
    assert status == 0 and ob.row_max == 1000 and ob.uniq[0] == 0 and ob.uniq[-1] == 1199
    _same(ob, host)
    ob2, host2, status2, _ = _batch(ops, ip, ix, rows, scratch=scratch)  # the scratch again, as it was returned
    assert status2 == 0 and all(np.array_equal(a, b) for a, b in zip(host, host2))


@pytest.mark.parametrize("m", [1, 7, 64, 65, 300, 4096])
def test_batch_one_column_stored_by_all_rows(m):
    """Column 0 is in every row: its segment has m entries — inside a wavefront's registers, in LDS, and on both sides of the long-segment
    limit; row i also stores i + 1 and, every third row, column 0 a second time (adjacent copies)."""
    ops = _ops()
    rows_of = [[i + 1, 0] + ([0] if i % 3 == 0 and m <= 2048 else []) for i in range(m)] + [[]]
    ip, ix = LO.csr(rows_of, m + 1)
    rows = np.random.default_rng(m).permutation(m)
    ob, host, status, _ = _batch(ops, ip, ix, rows)
    assert status == 0 and ob.seg_max >= m
    _same(ob, host)


def test_batch_duplicates_loops_repeated_and_bad_rows():
    ops = _ops()
    ip, ix = LO.random_graph(500, 9, 11, dup=0.3)
    rng = np.random.default_rng(12)
    rows = rng.integers(0, 500, 200).tolist()
    rows[5] = rows[4]; rows[0], rows[-1] = 0, 499
    ob, host, status, _ = _batch(ops, ip, ix, rows)
    assert status == 0
    _same(ob, host)
    bad = rows[:20] + [-1, 500, 2 ** 30] + rows[20:40]
    ob, host, status, _ = _batch(ops, ip, ix, bad)
    assert status == 4                                                   # GRAPES_STATUS_BAD_INDEX; the rows are empty rows
    _same(ob, host)


def test_batch_capacities_one_below_the_need():
    ops = _ops()
    ip, ix = LO.random_graph(500, 9, 13)
    rows = np.random.default_rng(14).integers(0, 500, 100)
    ob, host, status, _ = _batch(ops, ip, ix, rows, u_cap=LO.batch(ip, ix, rows).n_u - 1)
    assert status & 2 and host[4][:2].tolist() == [ob.n_u, ob.e] and np.array_equal(host[0][:101], ob.bptr)
    assert np.array_equal(host[1][:ob.n_u - 1], ob.uniq[:-1])
    ob, host, status, _ = _batch(ops, ip, ix, rows, e_cap=ob.e - 1)
    assert status & 1 and host[4][:2].tolist() == [ob.n_u, ob.e] and np.array_equal(host[0][:101], ob.bptr)
    assert np.array_equal(host[1][:ob.n_u], ob.uniq)
    ob, host, status, _ = _batch(ops, ip, ix, rows)                      # and the retry with the totals it reported
    assert status == 0
    _same(ob, host)


def test_batcher_retries_and_names_the_tables():
    _ops()
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.linkx import BagBatcher
    ip, ix = _hand_graph()
    bb = BagBatcher(DeviceGraph.from_csr(ip, ix))
    bb._u_cap, bb._e_cap = 4, 8                                          # far too small: two tries
    rows = [5, 0, 1, 2, 3, 4, 7, 100, 5]
    b = bb.batch(torch.tensor(rows))
    b.check()
    ob = LO.batch(ip, ix, rows)
    assert (b.num_unique, b.num_entries, b.seg_max, b.row_max) == (ob.n_u, ob.e, ob.seg_max, ob.row_max)
    assert np.array_equal(_np(b.uniq), ob.uniq) and np.array_equal(_np(b.tptr), ob.tptr) and np.array_equal(_np(b.trow), ob.trow)
    assert np.array_equal(_np(b.bptr), ob.bptr) and np.array_equal(_np(b.rows), rows) and int(bb.graph.bits.abs().sum()) == 0
    bb.batch(torch.tensor([3, 1200]))
    with pytest.raises(GrapesHipError, match="LINKX batcher: index out of range"):
        bb.check()
    bb.check()


# ---------------------------------------------------------------------------------------------------- forward and backward
_G = {}


def _gather_graph():
    """300 nodes.  Rows 0 .. 5: 0 / 1 / 63 / 64 / 65 / 200 entries; column 7 is stored by 64 rows, column 8 by 65, column 9 by 200 (a
    segment on each side of the long-row limit of 64); duplicates and a loop."""
    if "g" not in _G:
        rng = np.random.default_rng(21)
        N = 300
        rows_of = [rng.integers(10, N, d).tolist() for d in [0, 1, 63, 64, 65, 200] + rng.integers(0, 5, N - 6).tolist()]
        for i in range(6, N):
            rows_of[i] += [c for c, k in ((7, 64), (8, 65), (9, 200)) if i < 6 + k]
        rows_of[20] += [20, 20]
        ip, ix = LO.csr(rows_of, N)
        rows = np.concatenate([np.arange(0, 6), np.arange(6, 230), [5, 3]])
        _G["g"] = (ip, ix, rows, LO.batch(ip, ix, rows))
    return _G["g"]


def _block(rng, n, H, nan=False):
    """An [n, H] column block of a wider matrix (a non-contiguous leading dimension, 16-byte aligned rows) and the wide one."""
    wide = torch.full((n, H + 8), float("nan"), device="cuda") if nan else _dev(rng.standard_normal((n, H + 8)).astype(F32))
    return wide[:, 4:4 + H], wide


@pytest.mark.parametrize("H", WIDTHS)
def test_forward_and_backward_against_fp64(H):
    ops = _ops()
    ip, ix, rows, ob = _gather_graph()
    N, m = len(ip) - 1, len(rows)
    rng = np.random.default_rng(300 + H)
    W, _ = _block(rng, N, H)
    bias = _dev(rng.standard_normal(H).astype(F32))
    drows, dip, dix = _dev(rows.astype(np.int32)), _dev(ip), _dev(ix)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = []
    for _ in range(2):
        out, wide = _block(rng, m, H, nan=True)
        ops.bag_fwd(dip, dix, N, drows, W, bias, status=status, out=out)
        assert torch.isnan(wide[:, :4]).all() and torch.isnan(wide[:, 4 + H:]).all() and torch.isfinite(out).all()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and int(status.item()) == 0
    assert torch.equal(outs[0][0], bias)
    ref, mag = LO.fwd(ip, ix, rows, _np(W), _np(bias))
    deg = np.diff(ob.bptr)
    bound = LO.gamma(deg + 1)[:, None] * mag
    whole = ops.bag_fwd(dip, dix, N, drows, W, bias, item_cap=0)         # every row by one group: another order, the same bound
    assert (np.abs(_np(whole).astype(F64) - ref) <= bound).all()
    err = np.abs(_np(outs[0]).astype(F64) - ref)
    print(f"[linkx] H {H}: forward max err / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
    assert (err <= bound).all(), float((err - bound).max())
    nob = ops.bag_fwd(dip, dix, N, drows, W, None)                       # no bias: an empty row gives 0
    assert (nob[0] == 0).all()
    G, _ = _block(rng, m, H)
    vals = []
    for _ in range(2):
        v, wide = _block(rng, ob.n_u, H, nan=True)
        ops.bag_bwd(G, _dev(ob.tptr), _dev(ob.trow), ob.n_u, ob.e, status=status, out=v)
        assert torch.isnan(wide[:, :4]).all() and torch.isnan(wide[:, 4 + H:]).all() and torch.isfinite(v).all()
        vals.append(v)
    assert torch.equal(vals[0], vals[1]) and int(status.item()) == 0
    rref, rmag = LO.grad_rows(ob, _np(G))
    seg = np.diff(ob.tptr)
    assert {64, 65}.issubset(set(seg.tolist())) and seg.max() >= 200 and {0, 1, 63, 64, 65}.issubset(set(deg.tolist())) and deg.max() >= 200
    rbound = LO.gamma(seg + 1)[:, None] * rmag
    rerr = np.abs(_np(vals[0]).astype(F64) - rref)
    print(f"[linkx] H {H}: backward max err / bound {float((rerr[rbound > 0] / rbound[rbound > 0]).max()):.3f}")
    assert (rerr <= rbound).all(), float((rerr - rbound).max())
    one = ops.bag_bwd(G, _dev(ob.tptr), _dev(ob.trow), ob.n_u, ob.e, item_cap=0)        # every segment by one group: the same sums
    assert (np.abs(_np(one).astype(F64) - rref) <= rbound).all()


# ---------------------------------------------------------------------------------------------------- the fused row-sparse Adam
def _adam_graph():
    """2 000 nodes, about 6 entries a row, and column 11 in every row: a batch of 300 rows gives it a 300-long segment."""
    if "a" not in _G:
        ip, ix = LO.random_graph(2000, 6, 31, dup=0.2, empty=(3, 40))
        rows_of = [ix[ip[i]:ip[i + 1]].tolist() + [11] for i in range(2000)]
        _G["a"] = LO.csr(rows_of, 2000)
    return _G["a"]


def _max_err(a, ref):
    return float(np.abs(np.asarray(a, dtype=F64) - ref).max())


@pytest.mark.parametrize("H", [1, 64, 65, 256])
def test_fused_adam_against_fp64_by_the_fp32_baseline(H):
    """Three consecutive steps from identical fp32 inputs; per tensor the kernel's largest error against fp64 may be at most 4 times
    that of torch.optim.SparseAdam in fp32 on the CPU (which sums a column's entries in its own order).  With a plain fixed-order
    segment sum this was missed at H = 1 (exp_avg 1.216e-06 against 2.623e-07, exp_avg_sq 8.843e-07 against 6.940e-08: the tensor's
    largest error is the single element that sums the 300-entry segment, and the CPU's sum there is correctly rounded), which is why
    the kernel's sum is compensated."""
    ops = _ops()
    ip, ix = _adam_graph()
    N, m, lr, b1, b2, eps = 2000, 300, 1e-2, 0.9, 0.999, 1e-8
    rng = np.random.default_rng(400 + H)
    W0 = rng.standard_normal((N, H)).astype(F32)
    W, ea, eas = _dev(W0.copy()), torch.zeros(N, H, device="cuda"), torch.zeros(N, H, device="cuda")
    p64, m64, v64 = W0.astype(F64), np.zeros((N, H)), np.zeros((N, H))
    tp = torch.tensor(W0.copy(), requires_grad=True)
    ref_opt = torch.optim.SparseAdam([tp], lr=lr, betas=(b1, b2), eps=eps)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    touched = np.zeros(N, dtype=bool)
    for t in (1, 2, 3):
        rows = rng.permutation(N)[:m] if t != 2 else np.concatenate([rows[:150], rng.permutation(N)[:150]])   # the sets overlap partly
        ob = LO.batch(ip, ix, rows)
        assert ob.seg_max >= m and ob.n_u < N
        touched[ob.uniq] = True
        G = rng.standard_normal((m, H)).astype(F32)
        before = [t_.clone() for t_ in (W, ea, eas)]
        ops.bag_bwd_adam(_dev(G), _dev(ob.tptr), _dev(ob.trow), _dev(ob.uniq), ob.n_u, ob.e, W, ea, eas, lr, b1, b2, eps, t, status=status)
        rest = _dev(np.setdiff1d(np.arange(N), ob.uniq))
        assert all(torch.equal(a[rest], b[rest]) for a, b in zip(before, (W, ea, eas))), "a row outside uniq changed"
        g64, _ = LO.grad_rows(ob, G)
        LO.adam_rows(p64, m64, v64, ob.uniq, g64, lr, b1, b2, eps, t)
        cols = np.concatenate([ix[ip[r]:ip[r + 1]] for r in rows]).astype(np.int64)     # the reference: one sparse entry per stored entry,
        brow = np.repeat(np.arange(m), np.diff(ob.bptr))                               # summed by torch in fp32 on the CPU
        tp.grad = torch.sparse_coo_tensor(torch.tensor(cols)[None], torch.tensor(G[brow]), (N, H))
        ref_opt.step()
    assert int(status.item()) == 0 and not touched.all()
    st = ref_opt.state[tp]
    for name, got, ref32, ref64 in (("weight", W, tp.detach(), p64), ("exp_avg", ea, st["exp_avg"], m64), ("exp_avg_sq", eas, st["exp_avg_sq"], v64)):
        e_k, e_r = _max_err(_np(got), ref64), _max_err(ref32.numpy(), ref64)
        print(f"[linkx] fused Adam H {H} {name}: kernel err {e_k:.3e}, fp32 SparseAdam on the CPU err {e_r:.3e}")
        assert e_k <= 4 * e_r, (name, e_k, e_r)
    assert np.array_equal(_np(W)[~touched], W0[~touched]) and (_np(ea)[~touched] == 0).all() and (_np(eas)[~touched] == 0).all()


def test_sparse_and_fused_modes_land_on_the_same_step():
    """AdjacencyBag(grad="sparse") + torch.optim.SparseAdam on the device against AdjacencyBag(grad="fused") + BagAdam: one step from
    the same table and the same d out; the fused step's error against fp64 is held to 4 times the sparse one's."""
    _ops()
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.linkx import AdjacencyBag, BagAdam, BagBatcher
    ip, ix = _adam_graph()
    N, H, m, lr = 2000, 64, 300, 1e-2
    rng = np.random.default_rng(77)
    rows = rng.permutation(N)[:m]
    bb = BagBatcher(DeviceGraph.from_csr(ip, ix))
    batch = bb.batch(torch.tensor(rows))
    bb.check()
    torch.manual_seed(5)
    fused = AdjacencyBag(N, H, grad="fused").cuda()
    sparse = AdjacencyBag(N, H, grad="sparse").cuda()
    sparse.load_state_dict(fused.state_dict())
    W0, b0 = _np(fused.weight).copy(), _np(fused.bias).copy()
    co = _dev(rng.standard_normal((m, H)).astype(F32))
    fo, so = BagAdam(fused, lr=lr), torch.optim.SparseAdam([sparse.weight], lr=lr)
    of, os_ = fused(batch), sparse(batch)
    assert torch.equal(of, os_)
    ref, mag = LO.fwd(ip, ix, rows, W0, b0)
    assert (np.abs(_np(of).astype(F64) - ref) <= LO.gamma(np.diff(_np(batch.bptr)) + 1)[:, None] * mag).all()
    (of * co).sum().backward()
    (os_ * co).sum().backward()
    assert fused.weight.grad is None and sparse.weight.grad.is_sparse and torch.equal(fused.bias.grad, sparse.bias.grad)
    assert np.array_equal(_np(sparse.weight.grad.coalesce().indices())[0], _np(batch.uniq))
    fo.step(); so.step()
    with pytest.raises(RuntimeError, match="pending"):
        fo.step()
    ob = LO.batch(ip, ix, rows)
    p64, m64, v64 = W0.astype(F64), np.zeros((N, H)), np.zeros((N, H))
    LO.adam_rows(p64, m64, v64, ob.uniq, LO.grad_rows(ob, _np(co))[0], lr, 0.9, 0.999, 1e-8, 1)
    e_f, e_s = _max_err(_np(fused.weight), p64), _max_err(_np(sparse.weight), p64)
    print(f"[linkx] one step: fused err {e_f:.3e}, device SparseAdam err {e_s:.3e}")
    assert e_f <= 4 * e_s
    rest = np.setdiff1d(np.arange(N), ob.uniq)
    assert np.array_equal(_np(fused.weight)[rest], W0[rest])


# ---------------------------------------------------------------------------------------------------- the trainer
def _trainer(grad, seed=4321):
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.linkx import LinkxTrainer
    from grapes_amd.modules.linkx import LINKX
    torch.manual_seed(seed)
    n, F, H, C = 300, 12, 32, 4
    ip, ix = LO.random_graph(n, 7, 61, dup=0.2)
    rng = np.random.default_rng(62)
    x32 = rng.standard_normal((n, F)).astype(F32)
    labels = rng.integers(0, C, n)
    model = LINKX(n, F, H, C, num_node_layers=2, num_final_layers=2, grad=grad).cuda()
    tr = LinkxTrainer(DeviceGraph.from_csr(ip, ix), _dev(x32), _dev(labels), model, torch.optim.SGD(model.dense_parameters(), lr=0.05),
                      bag_lr=1e-2, eval_batch=128)
    return tr, model, ip, ix, x32, labels, rng


@pytest.mark.parametrize("grad", ["fused", "sparse"])
def test_three_trainer_steps_against_the_fp64_oracle(grad):
    """Three steps, SGD on the dense parameters and the row-sparse Adam on the table, against the same three steps in fp64 (dense
    A[rows], autograd, torch.optim.SparseAdam in fp64): every loss at ACT_TOL, and after the third step the table at GRAD_TOL on
    the elements whose first Adam step is fixed in sign (tests/test_sage_gpu.py's argument: Adam's first step is lr g / (|g| + eps),
    so where |g| is within the gradient tolerance of 0 a valid gradient may step the other way)."""
    _ops()
    tr, model, ip, ix, x32, labels, rng = _trainer(grad)
    n, B = 300, 48
    sd = {k: torch.tensor(_np(v).astype(F64), requires_grad=True) for k, v in model.state_dict().items()}
    W0 = _np(model.edge_lin.weight).copy()
    dense = torch.optim.SGD([v for k, v in sd.items() if k != "edge_lin.weight"], lr=0.05)
    table = torch.optim.SparseAdam([sd["edge_lin.weight"]], lr=1e-2)
    x64 = torch.tensor(x32.astype(F64))
    touched, unsure = np.zeros(n, dtype=bool), np.zeros(W0.shape, dtype=bool)
    for step in range(3):
        rows = rng.permutation(n)[:B]
        loss, b = tr.step(_dev(rows))
        ob = LO.batch(ip, ix, rows)
        assert np.array_equal(_np(b.uniq), ob.uniq) and np.array_equal(_np(b.trow), ob.trow)
        dense.zero_grad(); table.zero_grad()
        A = torch.tensor(LO.count_matrix(ip, ix, rows))
        edge = LO._BagFn.apply(sd["edge_lin.weight"], sd["edge_lin.bias"], A, ob)
        rest = {k: v for k, v in sd.items()}
        out = edge + (edge @ rest["cat_lin1.weight"].T + rest["cat_lin1.bias"])
        xx = torch.relu(x64[rows] @ rest["node_mlp.lins.0.weight"].T + rest["node_mlp.lins.0.bias"]) @ rest["node_mlp.lins.1.weight"].T \
            + rest["node_mlp.lins.1.bias"]
        out = torch.relu(out + xx + (xx @ rest["cat_lin2.weight"].T + rest["cat_lin2.bias"]))
        logits = torch.relu(out @ rest["final_mlp.lins.0.weight"].T + rest["final_mlp.lins.0.bias"]) @ rest["final_mlp.lins.1.weight"].T \
            + rest["final_mlp.lins.1.bias"]
        l64 = torch.nn.functional.cross_entropy(logits, torch.tensor(labels[rows]))
        l64.backward()
        g = sd["edge_lin.weight"].grad.coalesce()
        gv = np.zeros(W0.shape)
        gv[g.indices().numpy()[0]] = g.values().numpy()
        unsure |= (np.abs(gv) <= 2 * GRAD_TOL * max(1.0, float(np.abs(gv).max()))) & (gv != 0)
        touched[ob.uniq] = True
        dense.step(); table.step()
        print(f"[linkx] {grad} step {step}: loss {float(loss):.6f}, fp64 {float(l64):.6f}")
        assert abs(float(loss) - float(l64)) <= ACT_TOL * max(1.0, abs(float(l64)))
    got, want = _np(model.edge_lin.weight), sd["edge_lin.weight"].detach().numpy()
    sure = ~unsure
    err = rel_err(got[sure], want[sure])
    print(f"[linkx] {grad}: table err {err:.2e} on {int(sure.sum())}/{sure.size} sure elements")
    assert err <= GRAD_TOL and np.abs(got - W0).max() > 0
    assert np.array_equal(got[~touched], W0[~touched]) and not touched.all()
    for k in ("cat_lin1.weight", "final_mlp.lins.1.bias", "edge_lin.bias"):
        assert rel_err(_np(model.state_dict()[k]), sd[k].detach().numpy()) <= GRAD_TOL


def test_evaluate_is_the_oracles_full_forward():
    _ops()
    tr, model, ip, ix, x32, labels, rng = _trainer("fused", seed=99)
    n = 300
    sd = {k: torch.tensor(_np(v).astype(F64)) for k, v in model.state_dict().items()}
    want = LO.linkx_forward(sd, torch.tensor(LO.count_matrix(ip, ix, np.arange(n))), torch.tensor(x32.astype(F64))).numpy()
    model.eval()
    with torch.no_grad():
        got = _np(tr.logits_all())
    model.train()
    assert got.shape == want.shape and rel_err(got, want) <= ACT_TOL
    masks = (_dev(np.arange(n) < 100), _dev(np.arange(n) >= 200))
    val, test = tr.evaluate(masks)
    pred = got.argmax(1)
    assert val == pytest.approx(float((pred[:100] == labels[:100]).mean())) and test == pytest.approx(float((pred[200:] == labels[200:]).mean()))
    assert model.training
    with pytest.raises(ValueError, match="inject"):
        tr.step(_dev(np.arange(4)), inject=object())


@pytest.mark.parametrize("grad", ["fused", "sparse"])
def test_cli_two_epochs(grad, capsys):
    _ops()
    from grapes_amd import linkx
    v = linkx.main(["--dataset", "cora", "--max_epoch", "2", "--hidden_dim", "32", "--seed", "1", "--bag_grad", grad, "--bag_lr", "0.01"])
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"Loss: ([0-9.]+)", out)]
    assert out.count("Epoch: ") == 2 and "Acc: " in out and np.isfinite(v) and 0.0 <= v <= 1.0 and len(losses) == 2
    assert all(np.isfinite(losses))
