"""GraphSAINT's normalisation on the MI355X (modules/saint.py estimate_norm, saint.py, csrc/saint_kernels.hip) against
tests/saint_norm_oracle.py: the coverage counts bit for bit, the norms, the subgraph with entry ids, the estimate end to end, the
weighted loss, the normalised step of both trainers and the driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

from oracle.accuracy import assert_fp32_accuracy, fp32_contract
from tests import saint_norm_oracle as NO
from tests import saint_oracle as O
from tests import saint_samplers_oracle as S
from tests.test_graphsaint_cpu import COL, ROWPTR
from tests.test_graphsaint_gpu import _dev_graph, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graphsaint_cli_rw_seed5.txt")
F32 = np.float32
KINDS = ("rw", "node", "edge")


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _random_graph():
    """Directed, N = 300, about 1500 stored entries: duplicates (each its own entry), stored loops, the hub row 7 with 200 entries
    (more than three wavefront strides) and isolated nodes (every 23rd)."""
    rng = np.random.default_rng(20261018)
    n = 300
    iso = np.arange(0, n, 23)
    rest = np.setdiff1d(np.arange(n), iso)
    s, d = rng.choice(rest, 1150), rng.choice(rest, 1150)
    keep = s != 7
    s, d = s[keep], d[keep]
    loops = rest[5::9]
    dup = rng.integers(0, len(s), 70)
    s = np.concatenate([s, loops, s[dup], s[dup[:10]], np.full(200, 7)])
    d = np.concatenate([d, loops, d[dup], d[dup[:10]], rng.choice(rest, 200, replace=False)])
    order = np.lexsort((d, s))
    s, d = s[order], d[order]
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, s + 1, 1)
    indptr = np.cumsum(indptr)
    deg = np.diff(indptr)
    assert deg[7] == 200 and 1400 <= len(d) <= 1600 and not deg[iso].any()
    assert ((s[1:] == s[:-1]) & (d[1:] == d[:-1])).sum() >= 60 and (s == d).sum() >= len(loops)
    return indptr, d.astype(np.int64)


GRAPHS = {"six": lambda: (ROWPTR.astype(np.int64), COL.astype(np.int64)), "random": _random_graph}


def _sampler(kind, g, B, L=2, **kw):
    from grapes_amd.modules.saint import make_sampler
    return make_sampler(kind, g, B, L, **kw)


def _inject(kind, indptr, indices, B, L, rng):
    """(the arrays to inject into draw(), the oracle's node set) of one batch."""
    n = len(indptr) - 1
    if kind == "rw":
        roots = rng.integers(0, n, B).astype(np.int32)
        u = rng.random((B, L), dtype=np.float32)
        return (torch.from_numpy(roots).cuda(), torch.from_numpy(u.reshape(-1)).cuda()), O.node_set(O.walk(indptr, indices, roots, u, L))
    total = len(indices) if kind == "node" else int(S.entry_weights(indptr, indices).sum())
    t = rng.integers(0, total, B).astype(np.int64)
    ids = S.node_draw(indptr, t)[1] if kind == "node" else S.edge_draw(indptr, indices, t)[1]
    return (torch.from_numpy(t).cuda(),), S.node_set(ids)


def _count_five_batches(name, kind):
    """Five injected batches of sampler `kind` on graph `name`: the device counts and the oracle's, both as numpy."""
    from grapes_amd import ops
    indptr, indices = GRAPHS[name]()
    g = _dev_graph(indptr, indices)
    B, L = (3, 2) if name == "six" else ((40, 2) if kind == "rw" else (64, 2))
    ld = _sampler(kind, g, B, L, seed=1)
    rng = np.random.default_rng(len(name) + len(kind))
    sets, counts = [], None
    for i in range(5):
        inj, ns = _inject(kind, indptr, indices, B, L, rng)
        if name == "random" and kind == "rw" and i == 0:
            inj[0][0] = 7                                               # the hub row is in the first set
            ns = None
        d = ld.draw(*inj)
        got = d["node_idx"][: int(d["count"].item())].cpu().numpy().astype(np.int64)
        if ns is None:
            roots = inj[0].cpu().numpy()
            ns = O.node_set(O.walk(indptr, indices, roots, inj[1].cpu().numpy().reshape(B, L), L))
        assert np.array_equal(got, ns)
        sets.append(ns)
        counts = ops.saint_coverage_count(g.rowptr, g.col, g.num_nodes, d["node_idx"], d["count"], g.node_map, out=counts)
    ld.check()
    nc, ec, total = (t.cpu().numpy() for t in counts)
    return indptr, indices, g, sets, (nc, ec, int(total[0])), NO.coverage_counts(indptr, indices, sets)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["six", "random"])
def test_coverage_counts_equal_the_oracle(name, kind):
    _cuda()
    indptr, indices, g, sets, (nc, ec, total), (rnc, rec, rtotal) = _count_five_batches(name, kind)
    assert nc.dtype == np.int32 and ec.dtype == np.int32
    assert np.array_equal(nc, rnc) and np.array_equal(ec[: len(indices)], rec) and total == rtotal
    assert rec.max() >= 1 and rnc.max() >= 1
    if name == "random" and kind == "rw":
        assert rnc[7] >= 1


def _ulps(got, ref):
    """max |got - ref| / |ref| over the entries (0 where both are 0)."""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    return float((np.abs(got - ref) / np.where(ref == 0, 1.0, np.abs(ref))).max())


def _check_norms(indptr, nc, ec, num_samples, special):
    """edge_norm / node_norm of the device against the oracle: the constants 0.1 and 1e4 exact, every integer-derived value within
    rel 5e-7 (4 ulp, the bound of a non-IEEE fp32 divide).  The build divides correctly rounded (hipcc's default), so the
    difference measured is 0; it is printed."""
    from grapes_amd import ops
    n, nnz = len(indptr) - 1, len(ec)
    en, nn = ops.saint_norms(torch.from_numpy(indptr).cuda(), n, torch.from_numpy(nc.astype(np.int32)).cuda(),
                             torch.from_numpy(ec.astype(np.int32)).cuda(), num_samples)
    en, nn = en.cpu().numpy(), nn.cpu().numpy()
    ren, rnn = NO.norms(indptr, nc, ec, num_samples)
    assert en.dtype == np.float32 and nn.dtype == np.float32 and en.shape == (nnz,) and nn.shape == (n,)
    row = NO.entry_rows(indptr)
    zero_e, zero_n = ec == 0, nc[row] == 0
    nan, inf = zero_e & zero_n, zero_e & ~zero_n
    big = ~zero_e & (nc[row].astype(np.float64) / np.maximum(ec, 1) > 1e4)
    assert np.all(en[nan] == F32(0.1)) and np.all(en[inf] == F32(1e4)) and np.all(en[big] == F32(1e4))
    assert np.all(en >= 0) and np.all(en <= F32(1e4)) and not np.isnan(en).any()
    rest = ~(nan | inf | big)
    e_err, n_err = _ulps(en[rest], ren[rest]), _ulps(nn, rnn)
    print(f"norms: max rel err edge {e_err:.3e}, node {n_err:.3e} (bound 5e-7; 0 = correctly rounded divide)")
    assert e_err <= 5e-7 and n_err <= 5e-7
    assert np.array_equal(en[~rest], ren[~rest])
    if special:
        assert nan.any() and inf.any() and big.any() and (nc == 0).any()
    return en, nn


@pytest.mark.parametrize("name", ["six", "random"])
def test_norms_from_the_counted_batches(name):
    _cuda()
    indptr, indices, g, sets, (nc, ec, total), _ = _count_five_batches(name, "rw")
    _check_norms(indptr, nc, ec[: len(indices)], 5, special=False)


def test_norms_from_a_count_table_with_every_special_case():
    """Rows of 0, 1, 63, 64, 65 and 200 entries; counts that give 0 / 0, x / 0, a quotient above 1e4, 0 / x, a never-sampled node
    and counts above 2^24 (fp32 rounds them)."""
    _cuda()
    lens = np.array([0, 1, 63, 64, 65, 200, 3, 0, 5])
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.default_rng(4)
    nc = np.array([3, 0, 17, 2 ** 24 + 3, 40000, 9, 0, 0, 123457], np.int64)
    ec = rng.integers(1, 30, int(lens.sum())).astype(np.int64)
    ec[rng.random(len(ec)) < 0.2] = 0
    ec[0] = 0                                                # row 1 (node count 0): 0 / 0
    ec[1 + 63 + 5] = 1                                       # row 3: (2^24 + 3) / 1 > 1e4
    ec[1 + 63 + 64 + 7] = 3                                  # row 4: 40000 / 3 > 1e4
    ec[1 + 63 + 64 + 8] = 2 ** 24 + 1
    _check_norms(indptr, nc, ec, 2 ** 24 + 5, special=True)


def test_subgraph_ids():
    _cuda()
    from grapes_amd import ops
    indptr, indices = _random_graph()
    g = _dev_graph(indptr, indices)
    ld = _sampler("rw", g, 40, 2, seed=1)
    rng = np.random.default_rng(2)
    inj, ns = _inject("rw", indptr, indices, 40, 2, rng)
    inj[0][0] = 7
    d = ld.draw(*inj)
    n = int(d["count"].item())
    ns = d["node_idx"][:n].cpu().numpy().astype(np.int64)
    table = torch.from_numpy(rng.random(len(indices), dtype=np.float32)).cuda()
    e_cap = ld.e_cap
    a = ops.saint_subgraph(g.rowptr, g.col, d["node_idx"], d["count"], g.node_map, e_cap, status=ld.status)
    b = ops.saint_subgraph(g.rowptr, g.col, d["node_idx"], d["count"], g.node_map, e_cap, edge_norm=table, status=ld.status)
    ld.check()
    e = int(a[2].item())
    assert e > 40 and int(b[2].item()) == e and torch.equal(a[3], b[3])
    assert torch.equal(a[0][:e], b[0][:e]) and torch.equal(a[1][:e], b[1][:e])
    eid = b[4][:e].cpu().numpy()
    assert b[4].dtype == torch.int64 and b[5].dtype == torch.float32
    src, dst = b[0][:e].cpu().numpy(), b[1][:e].cpu().numpy()
    assert np.array_equal(indices[eid], ns[dst]) and np.array_equal(NO.entry_rows(indptr)[eid], ns[src])
    assert len(np.unique(eid)) == e                                       # duplicate entries keep their own ids
    assert torch.equal(b[5][:e], table[b[4][:e]])
    c = ops.saint_subgraph(g.rowptr, g.col, d["node_idx"], d["count"], g.node_map, e_cap, ids=True, status=ld.status)   # no table
    assert c[5] is None and torch.equal(c[4][:e], b[4][:e])
    # e_cap below the edge count: the overflow bit, and nothing at or past e_cap (a guard region behind every buffer)
    small, guard = e - 37, 64
    i32 = dict(dtype=torch.int32, device="cuda")
    bufs = (torch.full((small + guard,), -7, **i32), torch.full((small + guard,), -7, **i32), torch.zeros(1, **i32),
            torch.zeros(ld.n_cap + 1, **i32), torch.full((small + guard,), -7, dtype=torch.int64, device="cuda"),
            torch.full((small + guard,), -7.0, dtype=torch.float32, device="cuda"))
    status = torch.zeros(1, **i32)
    ops.saint_subgraph(g.rowptr, g.col, d["node_idx"], d["count"], g.node_map, small, edge_norm=table, status=status, out=bufs)
    assert int(status.item()) & 1 and int(bufs[2].item()) == small
    for k in (0, 1, 4, 5):
        assert torch.all(bufs[k][small:] == -7), k
    assert torch.equal(bufs[0][:small], b[0][:small]) and torch.equal(bufs[4][:small], b[4][:small])
    assert torch.equal(bufs[5][:small], b[5][:small])


def test_subgraph_of_a_node_set_past_one_scan_tile():
    """4 500 of 5 000 nodes (more than one tile of 4 096 of a row-list prefix, below SAINT_MAX_IDS) in a buffer of 4 600, over a sparse
    directed graph with one 300-entry row: edges, local row pointers and — ids=True — entry ids against the oracle; then e_cap one
    below the count."""
    _cuda()
    from grapes_amd import ops
    rng = np.random.default_rng(41)
    n, n_set, n_cap = 5000, 4500, 4600
    s = np.concatenate([rng.integers(0, n, 4 * n), np.full(300, 17)])
    d = np.concatenate([rng.integers(0, n, 4 * n), rng.choice(n, 300, replace=False)])
    order = np.lexsort((d, s))
    s, d = s[order], d[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n))]).astype(np.int64)
    ns = np.sort(np.concatenate([[17], rng.permutation(np.setdiff1d(np.arange(n), [17]))[:n_set - 1]]))
    node_idx = np.concatenate([ns, np.zeros(n_cap - n_set, np.int64)]).astype(np.int32)
    node_map = rng.integers(0, n_cap, n).astype(np.int32)                # stale everywhere but at the set's nodes
    node_map[ns] = np.arange(n_set)
    i32 = dict(dtype=torch.int32, device="cuda")
    rowptr, col = torch.from_numpy(indptr).cuda(), torch.from_numpy(d.astype(np.int32)).cuda()
    d_idx, d_map, count = torch.from_numpy(node_idx).cuda(), torch.from_numpy(node_map).cuda(), torch.tensor([n_set], **i32)
    rs, rd = O.induced_subgraph(indptr, d, ns)
    e = len(rs)
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(rs, minlength=n_cap))])
    assert e > 4096 and want_ptr[4096] < e
    status = torch.zeros(1, **i32)
    a = ops.saint_subgraph(rowptr, col, d_idx, count, d_map, e, status=status)           # the capacity exact
    c = ops.saint_subgraph(rowptr, col, d_idx, count, d_map, e, ids=True, status=status)
    assert int(status.item()) == 0 and int(a[2].item()) == e and int(c[2].item()) == e
    for got in (a, c):
        assert np.array_equal(got[0].cpu().numpy(), rs) and np.array_equal(got[1].cpu().numpy(), rd)
        assert np.array_equal(got[3].cpu().numpy(), want_ptr)
    eid = c[4].cpu().numpy()
    assert c[5] is None and np.array_equal(d[eid], ns[rd]) and np.array_equal(NO.entry_rows(indptr)[eid], ns[rs])
    assert (np.diff(eid) > 0).all()
    small, guard = e - 1, 64
    bufs = (torch.full((small + guard,), -7, **i32), torch.full((small + guard,), -7, **i32), torch.zeros(1, **i32),
            torch.zeros(n_cap + 1, **i32), torch.full((small + guard,), -7, dtype=torch.int64, device="cuda"), None)
    ops.saint_subgraph(rowptr, col, d_idx, count, d_map, small, ids=True, status=status, out=bufs)
    assert int(status.item()) & 1 and int(bufs[2].item()) == small
    for k in (0, 1, 4):
        assert torch.all(bufs[k][small:] == -7), k
    assert torch.equal(bufs[0][:small], c[0][:small]) and torch.equal(bufs[4][:small], c[4][:small])
    assert np.array_equal(bufs[3].cpu().numpy(), want_ptr)               # the row pointers are not clamped


@pytest.mark.parametrize("kind", KINDS)
def test_estimate_norm_end_to_end(kind):
    _cuda()
    indptr, indices = _random_graph()
    n, nnz = len(indptr) - 1, len(indices)
    B, L, steps, cov = (20, 2, 3, 5) if kind == "rw" else (48, 2, 3, 5)
    a = _sampler(kind, _dev_graph(indptr, indices), B, L, num_steps=steps, seed=33)
    b = _sampler(kind, _dev_graph(indptr, indices), B, L, num_steps=steps, seed=33)
    assert a.estimate_norm(cov) is a
    assert a.sample_coverage == cov and a.num_samples % steps == 0 and a.num_samples >= steps
    nc, ec, total = np.zeros(n, np.int64), np.zeros(nnz, np.int64), 0
    row = NO.entry_rows(indptr)
    before_last = 0
    for i in range(a.num_samples):
        if i == a.num_samples - steps:
            before_last = total
        bb = b.batch()
        assert not hasattr(bb, "edge_norm")                           # without the call batches are what they were
        ns, ei = bb.node_idx.cpu().numpy(), bb.edge_index.cpu().numpy()
        nc[ns] += 1
        total += len(ns)
        # the batch's edges are the member entries in CSR order, so the i-th edge of local row r is the i-th member entry of its row
        member = np.zeros(n, bool); member[ns] = True
        ids = np.nonzero(member[row] & member[indices])[0]
        assert len(ids) == ei.shape[1] and np.array_equal(ns[ei[0]], row[ids]) and np.array_equal(ns[ei[1]], indices[ids])
        ec[ids] += 1
    assert np.array_equal(a.node_count.cpu().numpy(), nc) and np.array_equal(a.edge_count.cpu().numpy()[:nnz], ec)
    assert a.total_sampled_nodes == total and total >= n * cov and before_last < n * cov
    assert int(a.philox_offset.item()) == int(b.philox_offset.item()) > 0
    per = (B * (L + 1) + 3) // 4 if kind == "rw" else S.offset_advance(B)
    assert int(a.philox_offset.item()) == a.num_samples * per
    ren, rnn = NO.norms(indptr, nc, ec, a.num_samples)
    assert _ulps(a.edge_norm.cpu().numpy()[:nnz], ren) <= 5e-7 and _ulps(a.node_norm.cpu().numpy(), rnn) <= 5e-7
    bb = a.batch()                                                    # afterwards a batch carries its norms
    assert bb.edge_id.dtype == torch.int64 and bb.edge_id.shape == (bb.edge_index.shape[1],)
    assert torch.equal(bb.edge_norm, a.edge_norm[bb.edge_id]) and torch.equal(bb.node_norm, a.node_norm[bb.node_idx])
    assert bb.node_norm.shape == (bb.num_nodes,)


# ------------------------------------------------------------------------------------------------------ the weighted loss
def _loss_case(C, multi, seed, T0=False, shifted=False):
    rng = np.random.default_rng(seed)
    N, n_cap, n = 500, 96, 83
    node_idx = np.sort(rng.choice(N, n, replace=False)).astype(np.int32)
    pad = np.concatenate([node_idx, np.zeros(n_cap - n, np.int32)])
    z = (2 * rng.standard_normal((n_cap, C))).astype(np.float32)
    if shifted:     # a common offset of -1000 or +1000 per row: softmax and row loss do not depend on it
        z = (z + np.random.default_rng(seed + 1).choice([-1000.0, 1000.0], n_cap)[:, None]).astype(np.float32)
    y = (rng.random((N, C)) < 0.3).astype(np.float32) if multi else rng.integers(0, C, N)
    mask = np.zeros(N, bool) if T0 else rng.random(N) < 0.5
    ws = [(rng.random(N) * 3 + 0.01).astype(np.float32) for _ in range(8)]
    return N, n_cap, n, pad, z, y, mask, ws


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("C", [7, 70])
def test_weighted_loss_against_fp64(C, multi):
    """Loss and g against the fp64 oracle under oracle/accuracy.py's criterion, its factors unchanged.  The baseline is the
    loss's formulas evaluated in numpy fp32, shift first (NO.weighted_loss(dtype=float32)), the magnitude of an output the sum of the
    absolute values of the terms it adds up.  The loss is one number per launch, so eight weight tables are judged together."""
    _weighted_loss_against_fp64(C, multi, False)


@pytest.mark.parametrize("C", [7, 70])
def test_weighted_loss_against_fp64_on_shifted_logits(C):
    """The CE case of the test above with a common offset of +-1000 added to every row, and saint_masked_loss_k (no weights) on the
    same logits.  A row written lse = max + log(se), p = exp(z - lse) rounds lse at the size of the offset and carries 2^-24 * 1000
    into every p (grapes_rowlist_loss in that order: about 100 times the baseline's rms error of g); the kernels form
    (z - max) - log(se), as the baseline does."""
    _weighted_loss_against_fp64(C, False, True)
    from grapes_amd import ops
    N, n_cap, n, pad, z, y, mask, _ = _loss_case(C, False, 10 * C, shifted=True)
    train = np.concatenate([mask[pad[:n]], np.zeros(n_cap - n, bool)])
    w = np.full(n_cap, F32(1) / F32(train.sum()), np.float32)
    lm, gm = ops.saint_masked_loss(torch.from_numpy(z).cuda(), C, torch.from_numpy(pad).cuda(),
                                   torch.tensor([n], dtype=torch.int32, device="cuda"), torch.from_numpy(mask).cuda(),
                                   torch.from_numpy(y).cuda())
    yl = np.concatenate([y[pad[:n]], y[pad[n:]]])
    rl, rg, ml, mg = NO.weighted_loss(z, yl, w, train)
    _, bg, _, _ = NO.weighted_loss(z, yl, w, train, dtype=np.float32)
    assert_fp32_accuracy(gm.cpu().numpy(), rg, mg, bg, f"masked loss g C={C} shifted")
    assert abs(float(lm.item()) - rl) <= 4 * 2.0 ** -24 * ml, (float(lm.item()), rl)          # one number: 4 ulp of its magnitude


def _weighted_loss_against_fp64(C, multi, shifted):
    _cuda()
    from grapes_amd import ops
    N, n_cap, n, pad, z, y, mask, ws = _loss_case(C, multi, 10 * C + multi, shifted=shifted)
    zd, yd, md = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(mask).cuda()
    idx, cnt = torch.from_numpy(pad).cuda(), torch.tensor([n], dtype=torch.int32, device="cuda")
    train = np.concatenate([mask[pad[:n]], np.zeros(n_cap - n, bool)])
    assert train.sum() > 16
    yl = np.concatenate([y[pad[:n]], y[pad[n:]]])
    got_l, ref_l, mag_l, base_l = [], [], [], []
    for k, w in enumerate(ws):
        d_train, status = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        loss, g = ops.saint_masked_loss(zd, C, idx, cnt, md, yd, node_norm=torch.from_numpy(w).cuda(), d_train=d_train, status=status)
        wl = w[pad]
        rl, rg, ml, mg = NO.weighted_loss(z, yl, wl, train)
        bl, bg, _, _ = NO.weighted_loss(z, yl, wl, train, dtype=np.float32)
        assert int(d_train.item()) == int(train.sum()) and int(status.item()) == 0
        got_l.append(float(loss.item())); ref_l.append(rl); mag_l.append(ml); base_l.append(float(bl))
        if k == 0:
            assert g.shape == (n_cap, C) and not g.cpu().numpy()[~train].any()
            assert_fp32_accuracy(g.cpu().numpy(), rg, mg, bg, f"weighted loss g C={C} multi={multi}" + " shifted" * shifted)
    assert_fp32_accuracy(np.array(got_l), np.array(ref_l), np.array(mag_l), np.array(base_l),
                         f"weighted loss C={C} multi={multi}" + " shifted" * shifted)


@pytest.mark.parametrize("multi", [False, True])
def test_weighted_loss_with_uniform_weights_is_the_masked_loss(multi):
    """w = 1 / T everywhere: ops.saint_masked_loss's loss and g.  Both g are judged against the fp64 oracle at the criterion of
    the test above.  Each loss is ONE number (a ratio to a baseline's error is chance there), so it is held to 4 * 2^-24 of its
    magnitude (the sum of w (|lse| + |z_y|), or of the absolute BCE terms): every row loss carries the rounding of expf, logf / log1pf
    and two or three fp32 additions, each at most 2^-24 of a term of that magnitude; the rows are summed in double and the result is
    rounded to fp32 once."""
    _cuda()
    from grapes_amd import ops
    C = 70
    N, n_cap, n, pad, z, y, mask, _ = _loss_case(C, multi, 5)
    zd, yd, md = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(mask).cuda()
    idx, cnt = torch.from_numpy(pad).cuda(), torch.tensor([n], dtype=torch.int32, device="cuda")
    train = np.concatenate([mask[pad[:n]], np.zeros(n_cap - n, bool)])
    T = int(train.sum())
    w = np.full(N, F32(1) / F32(T), np.float32)
    lw, gw = ops.saint_masked_loss(zd, C, idx, cnt, md, yd, node_norm=torch.from_numpy(w).cuda())
    lm, gm = ops.saint_masked_loss(zd, C, idx, cnt, md, yd)
    yl = np.concatenate([y[pad[:n]], y[pad[n:]]])
    rl, rg, ml, mg = NO.weighted_loss(z, yl, w[pad], train)
    bl, bg, _, _ = NO.weighted_loss(z, yl, w[pad], train, dtype=np.float32)
    for name, l, g in (("weighted", lw, gw), ("masked", lm, gm)):
        assert_fp32_accuracy(g.cpu().numpy(), rg, mg, bg, f"{name} g, w = 1/T, multi={multi}")
        assert abs(float(l.item()) - rl) <= 4 * 2.0 ** -24 * ml, (name, float(l.item()), rl)      # one number: 4 ulp of its magnitude


@pytest.mark.parametrize("multi", [False, True])
def test_weighted_loss_without_a_training_row_is_zero(multi):
    _cuda()
    from grapes_amd import ops
    N, n_cap, n, pad, z, y, mask, ws = _loss_case(7, multi, 6, T0=True)
    loss, g = ops.saint_masked_loss(torch.from_numpy(z).cuda(), 7, torch.from_numpy(pad).cuda(),
                                    torch.tensor([n], dtype=torch.int32, device="cuda"), torch.from_numpy(mask).cuda(),
                                    torch.from_numpy(y).cuda(), node_norm=torch.from_numpy(ws[0]).cuda())
    assert float(loss.item()) == 0.0 and not g.any()


def test_weighted_loss_flags_a_label_out_of_range():
    _cuda()
    from grapes_amd import ops
    N, n_cap, n, pad, z, y, mask, ws = _loss_case(7, False, 8)
    mask[pad[3]] = True
    y = y.copy(); y[pad[3]] = 7
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss, g = ops.saint_masked_loss(torch.from_numpy(z).cuda(), 7, torch.from_numpy(pad).cuda(),
                                    torch.tensor([n], dtype=torch.int32, device="cuda"), torch.from_numpy(mask).cuda(),
                                    torch.from_numpy(y).cuda(), node_norm=torch.from_numpy(ws[0]).cuda(), status=status)
    assert int(status.item()) & 4 and not g[3].any() and np.isfinite(float(loss.item()))


def test_c_entry_points_refuse_half_given_pairs():
    """Refused on the host before any launch: a table without edge_norm_b (grapes_saint_subgraph), both label pointers
    (grapes_saint_masked_loss)."""
    _cuda()
    from grapes_amd import _lib
    L = _lib.load()
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    i64, f32, u8 = i32.long(), i32.float(), i32.to(torch.uint8)
    p = lambda t: t.data_ptr()
    EINVAL = -1
    assert L.grapes_saint_subgraph(p(i64), p(i32), p(i32), p(i32), p(i32), 4, 4, p(i32), p(i32), p(i32), p(i32), p(i64), p(f32), None,
                                   p(i32), p(i32), None) == EINVAL
    assert L.grapes_saint_masked_loss(p(f32), 2, 2, p(i32), p(i32), 4, p(u8), None, p(i64), p(f32), p(f32), 2, p(f32), p(i32), p(i32),
                                      None) == EINVAL
    torch.cuda.synchronize()
    assert not i32.any() and not f32.any()                                # nothing was launched


# ------------------------------------------------------------------------------------------------------------ trainers
def _mm32(a, b):
    return fp32_contract(np.ascontiguousarray(np.asarray(a).T), b).numpy()


@pytest.mark.parametrize("kind", ["rw", "edge"])
def test_one_eager_normalised_step_against_fp64(kind):
    """The parameter gradients of one normalised eager step against tests/saint_norm_oracle.normalised_step in fp64 (dense weighted
    normalised adjacency, two layers, the weighted loss) under oracle/accuracy.py's criterion, factors unchanged.  Baseline: the
    same restatement in fp32 with every contraction in the fixed order of fp32_contract.  Magnitude of a gradient entry: the sum
    of the absolute terms of the contraction that forms it (dW = dHᵀ X: |dH|ᵀ |X|; db: the column sums of |dZ|), from the fp64 pass."""
    _cuda()
    from grapes_amd.saint import make_trainer
    indptr, indices, g, x, y, tm, model = _setup(n=600, seed=4)
    tr = make_trainer("eager", g, x, y, tm, model, 0.01, batch_size=48, walk_length=2, seed=12, sampler=kind, num_steps=2,
                      sample_coverage=3, use_normalization=True)
    assert tr.normalised and tr.loader.sample_coverage == 3
    c1, c2 = model.gcn_layers
    params = [c1.lin.weight, c1.bias, c2.lin.weight, c2.bias]
    w0 = [p.detach().cpu().numpy().copy() for p in params]
    loss, b = tr.step()
    tr.check()
    ns, ei = b.node_idx.cpu().numpy(), b.edge_index.cpu().numpy()
    en, nn = b.edge_norm.cpu().numpy(), b.node_norm.cpu().numpy()
    assert np.array_equal(en, tr.loader.edge_norm.cpu().numpy()[b.edge_id.cpu().numpy()])
    train = tm.cpu().numpy()[ns]
    assert train.sum() > 4
    P = NO.wgcn_dense(ei[0], ei[1], en, len(ns))
    xr, yr = x.cpu().numpy()[ns], y.cpu().numpy()[ns]
    rl, rgrads, mags = NO.normalised_step(xr, P, w0, yr, nn, train)
    bl, bgrads, _ = NO.normalised_step(xr, P, w0, yr, nn, train, mm=_mm32, dtype=np.float32)
    assert abs(float(loss) - rl) <= 1e-5 * max(1.0, abs(rl)), (float(loss), rl)
    for p, r, m, bs, name in zip(params, rgrads, mags, bgrads, ("W1", "b1", "W2", "b2")):
        assert_fp32_accuracy(p.grad.cpu().numpy(), r, m, bs, f"normalised step {kind} d{name}")


@pytest.mark.parametrize("kind", ["rw", "edge"])
def test_captured_normalised_steps_match_eager(kind):
    """Three normalised steps of both engines from one seed: the same batches, losses and weights within the 2e-3 of
    test_captured_trainer_matches_eager (torch Adam against FusedAdam)."""
    _cuda()
    from grapes_amd.saint import make_trainer
    runs = {}
    for engine in ("eager", "graph"):
        indptr, indices, g, x, y, tm, model = _setup(n=3000, seed=2)
        tr = make_trainer(engine, g, x, y, tm, model, 0.01, batch_size=128, walk_length=2, seed=77, sampler=kind, num_steps=2,
                          sample_coverage=1, use_normalization=True)
        sets, losses = [], []
        for _ in range(3):
            if engine == "eager":
                loss, b = tr.step()
                losses.append(float(loss))
                sets.append((b.node_idx.cpu().numpy(), b.edge_index.cpu().numpy(), b.edge_norm.cpu().numpy()))
            else:
                tr.step()
                losses.append(float(tr.lossbuf.item()))
                n, e = int(tr.draw_out[2].item()), int(tr.sub_out[2].item())
                sets.append((tr.draw_out[1][:n].long().cpu().numpy(),
                             torch.stack([tr.sub_out[0][:e], tr.sub_out[1][:e]]).long().cpu().numpy(), tr.sub_out[5][:e].cpu().numpy()))
        tr.check()
        runs[engine] = (sets, losses, [p.detach().cpu().numpy() for p in model.parameters()], tr.loader.num_samples)
    (es, el, ew, en), (gs, gl, gw, gn) = runs["eager"], runs["graph"]
    assert en == gn
    for a, b in zip(es, gs):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.all(np.isfinite(el)) and float(np.abs(np.array(el) - np.array(gl)).max()) <= 2e-3, (el, gl)
    for a, b in zip(ew, gw):
        assert float(np.abs(a - b).max()) <= 2e-3


@pytest.mark.parametrize("engine", ["eager", "graph"])
def test_default_trainer_never_enters_the_normalised_path(engine, monkeypatch):
    """A trainer built with the defaults launches what it launched before: none of the normalisation's entry points is called over
    three steps, the subgraph and the loss are — each time without a table, without ids and without node_norm — and the Philox
    offset is three draws' worth.  (The driver's output with the defaults is
    pinned to the parent's by tests/test_saint_samplers_gpu.py::test_cli_rw_output_is_the_parents and by test_cli below.)"""
    _cuda()
    from grapes_amd import ops
    from grapes_amd.saint import make_trainer
    calls = {"subgraph": 0, "loss": 0}

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} was called by a default trainer")
        return f
    for name in ("saint_coverage_count", "saint_norms", "WeightedStructure"):
        monkeypatch.setattr(ops, name, refuse(name))
    old_sub, old_loss = ops.saint_subgraph, ops.saint_masked_loss

    def plain_sub(*a, **k):                                   # (rowptr, col, node_idx, count, node_map, e_cap) and keywords only
        assert len(a) <= 6 and k.get("edge_norm") is None and not k.get("ids", False), (len(a), sorted(k))
        calls["subgraph"] += 1
        return old_sub(*a, **k)

    def plain_loss(*a, **k):                                  # (z, C, node_idx, count, train_mask, labels) and keywords only
        assert len(a) <= 6 and k.get("node_norm") is None, (len(a), sorted(k))
        calls["loss"] += 1
        return old_loss(*a, **k)
    monkeypatch.setattr(ops, "saint_subgraph", plain_sub)
    monkeypatch.setattr(ops, "saint_masked_loss", plain_loss)
    indptr, indices, g, x, y, tm, model = _setup(n=3000, seed=2)
    tr = make_trainer(engine, g, x, y, tm, model, 0.01, batch_size=128, walk_length=2, seed=77)
    assert tr.normalised is False and tr.loader.edge_norm is None and len(tr.sub_out if engine == "graph" else (0,) * 4) == 4
    losses = []
    for _ in range(3):
        out = tr.step()
        losses.append(float(out[0]) if engine == "eager" else float(tr.lossbuf.item()))
    tr.check()
    assert np.all(np.isfinite(losses))
    assert int(tr.loader.philox_offset.item()) == 3 * ((128 * 3 + 3) // 4)
    # eager: one call per step; captured: the warm-up pass and the capture (replays call nothing)
    assert calls["subgraph"] == calls["loss"] == (3 if engine == "eager" else 2)


def test_trainers_refuse_normalisation_without_coverage():
    _cuda()
    from grapes_amd.saint import make_trainer
    indptr, indices, g, x, y, tm, model = _setup(n=600, seed=4)
    for engine in ("eager", "graph"):
        with pytest.raises(ValueError):
            make_trainer(engine, g, x, y, tm, model, 0.01, batch_size=32, use_normalization=True)
        with pytest.raises(ValueError):
            make_trainer(engine, g, x, y, tm, model, 0.01, batch_size=32, sample_coverage=2)


# -------------------------------------------------------------------------------------------------------------- driver
def _cli(*flags):
    r = subprocess.run([sys.executable, "-m", "grapes_amd.graphsaint", "--dataset", "cora", "--max_epoch", "2", "--seed", "5", *flags],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("engine", ["graph", "eager"])
def test_cli_normalised_two_epochs(engine):
    _cuda()
    out = _cli("--use_normalization", "--sample_coverage", "5", "--engine", engine)
    losses = [float(m) for m in re.findall(r"^Epoch: \d+, Loss: (\S+),", out, flags=re.M)]
    print(engine, losses)
    assert len(losses) == 2 and np.all(np.isfinite(losses)), out
    assert sum(l.startswith("Acc: ") for l in out.splitlines()) == 1, out


def test_cli_without_the_flags_prints_the_parents_lines():
    """Two epochs of the default driver, seed 5: the first two lines of the three-epoch run recorded from the parent of the sampler
    change (tests/golden), and the Acc line of the second epoch's validation value."""
    _cuda()
    want = open(GOLDEN).read().splitlines()[:2]
    got = _cli().splitlines()
    assert got[:2] == want, got
    val = float(re.search(r"Val: (\S+),", want[1]).group(1))
    m = re.fullmatch(r"Acc: (\S+) ± 0\.00", got[2])
    assert m and abs(float(m.group(1)) - 100 * val) <= 0.0051, got
