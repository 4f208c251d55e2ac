"""The gather step the row aggregations share (gather_batch, grapes_amd/csrc/row_gather.h) on the MI355X, where a shared loop can
go wrong: a batch tail that is no multiple of the rows in flight (U = 1, 2, 4 or, in the history walks, up to 16), and the 32- and
64-lane batch boundary.

One symmetric graph of 400 nodes without loops or duplicates: the ladder rows 0 .. 15 have exactly LADDER[r] entries, drawn from the
pool nodes 16 .. 335 (a pool node's entries are the ladder rows that drew it and a few of the outside nodes 336 .. 399).  It goes
through sage_aggregate_fwd, cluster_aggregate_fwd, gat_aggregate_fwd (whose walk adds the self-loop: LADDER[r] + 1 entries),
vrgcn_aggregate_fwd / _bwd (every node listed, every entry kept: the kept walk, the full walk and, the graph being symmetric, the
backward's by-source rows all have the ladder's lengths) and gas_aggregate_fwd / _bwd (a batch of the ladder and its pool, the
outside nodes as halo: the ladder's lengths in both passes; and a batch of the ladder, every other pool node and the outside, where
the ladder rows mix in-batch and halo sources), at one width per instantiated shape <VEC, LPR, NS> (CASES of
tests/test_row_sum_gpu.py), against the fp64 oracles under tests/ at the sibling tests' tolerances: 1e-5 for activations, 1e-4 for
gradients, in max |a - ref| / max(1, max |ref|)."""
import numpy as np
import pytest
import torch

from tests import cluster_oracle as CO
from tests import gas_oracle as GO
from tests import gat_oracle as AO
from tests import sage_oracle as SO
from tests import vrgcn_oracle as VO
from tests.gat_oracle import rel_err

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4
F32, F64 = np.float32, np.float64
LADDER = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 129]
N, POOL_END = 400, 336                                                   # ladder 0 .. 15, pool 16 .. 335, outside 336 .. 399
WIDTHS = [30, 47, 100, 200, 201, 320]                                    # <1,32,1> <1,64,1> <4,32,1> <4,64,1> <1,64,4> <4,64,4>
_G = {}


def _graph():
    """dict(ip, ix: the symmetric CSR, rows sorted; ei: its entries as (source, target) [2, e])."""
    if not _G:
        rng = np.random.default_rng(2024)
        nb = [set() for _ in range(N)]
        for r, d in enumerate(LADDER):
            for v in rng.choice(np.arange(len(LADDER), POOL_END), d, replace=False):
                nb[r].add(int(v)); nb[int(v)].add(r)
        for o in range(POOL_END, N):
            for v in rng.choice(np.arange(len(LADDER), POOL_END), 3, replace=False):
                nb[o].add(int(v)); nb[int(v)].add(o)
        ip, ix = SO.csr_from_rows([sorted(s) for s in nb])
        ip, ix = np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int64)
        dst = np.repeat(np.arange(N), np.diff(ip))
        _G.update(ip=ip, ix=ix, ei=np.stack([ix, dst]))
    return _G


def test_the_graph_has_the_ladder():
    """On the CPU, before any launch: the ladder's degrees, symmetry, no loop, no duplicate, at most 400 nodes."""
    G = _graph()
    ip, ix, ei = G["ip"], G["ix"], G["ei"]
    assert len(ip) - 1 == N <= 400
    assert np.diff(ip)[:len(LADDER)].tolist() == LADDER
    assert np.bincount(ei[1], minlength=N)[:len(LADDER)].tolist() == LADDER          # by target
    assert np.bincount(ei[0], minlength=N)[:len(LADDER)].tolist() == LADDER          # by source
    key = ei[0] * N + ei[1]
    assert len(np.unique(key)) == len(key) and (ei[0] != ei[1]).all()
    assert set(key.tolist()) == set((ei[1] * N + ei[0]).tolist())
    assert (ix[ip[0]:ip[len(LADDER)]] >= len(LADDER)).all() and (ix[ip[0]:ip[len(LADDER)]] < POOL_END).all()


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from grapes_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _judge(got, want, tol, what):
    err = rel_err(_np(got), np.asarray(want))
    print(f"[gather_batch] {what}: rel err {err:.3e} (tolerance {tol:g})")
    assert err <= tol, what


def _prepared(ops):
    if "prep" not in _G:
        ei = _graph()["ei"]
        src, dst = _dev(ei[0].astype(np.int32)), _dev(ei[1].astype(np.int32))
        _G["prep"] = ops.gcn2_attach_loops(ops.PreparedGraph(src, dst, N), src, dst)
    return _G["prep"]


@pytest.mark.parametrize("f", WIDTHS)
def test_plain_sums_and_attention(f):
    ops = _ops()
    test_the_graph_has_the_ladder()
    ei, prep = _graph()["ei"], _prepared(ops)
    rng = np.random.default_rng(300 + f)
    x = rng.standard_normal((N, f)).astype(F32)
    a_s, a_d, b = (0.2 * rng.standard_normal(f).astype(F32) for _ in range(3))
    xd, x64 = _dev(x), torch.from_numpy(x.astype(F64))
    for long_rows in (True, False):
        for aggr in ("sum", "mean"):
            _judge(ops.sage_aggregate_fwd(xd, prep, aggr, long_rows=long_rows), SO.aggregate64(x64, ei, N, aggr).numpy(), ACT_TOL,
                   f"f={f} long_rows={long_rows} sage {aggr}")
        _judge(ops.cluster_aggregate_fwd(xd, prep, 0.5, long_rows=long_rows), CO.propagate64(x64, ei, N, 0.5).numpy(), ACT_TOL,
               f"f={f} long_rows={long_rows} cluster")
    s_src, s_dst = ops.gat_scores(xd, _dev(a_s), _dev(a_d))
    out, _ = ops.gat_aggregate_fwd(xd, s_src, s_dst, prep, _dev(b))
    want = AO.gat_conv(x64, torch.eye(f, dtype=torch.float64), *(torch.from_numpy(t.astype(F64)) for t in (a_s, a_d, b)), ei)
    _judge(out, want.numpy(), ACT_TOL, f"f={f} gat")
    assert prep.status is None or int(prep.status.item()) == 0


@pytest.mark.parametrize("f", WIDTHS)
def test_vrgcn_every_node_listed_every_entry_kept(f):
    ops = _ops()
    test_the_graph_has_the_ladder()
    G = _graph()
    ip, ix, ei = G["ip"], G["ix"], G["ei"]
    rng = np.random.default_rng(400 + f)
    H, Hbar, dA = (rng.standard_normal((N, f)).astype(F32) for _ in range(3))
    rows = np.arange(N)
    kept = [ix[ip[u]:ip[u + 1]] for u in rows]
    ids = _dev(rows.astype(np.int32))
    prep = ops.PreparedGraph(_dev(ei[0].astype(np.int32)), _dev(ei[1].astype(np.int32)), N)
    dinv = _dev(VO.dinv(ip).astype(F32))
    A64, dH64 = VO.aggregate(ip, ix, rows, kept, H, Hbar), VO.aggregate_grad(ip, rows, kept, dA, N)
    for item_cap in (None, 0):                                           # the rows of 65 and 129 entries in chunks, and whole
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        A, coef = ops.vrgcn_aggregate_fwd(_dev(H), ids, _dev(Hbar), dinv, _dev(ip), _dev(ix.astype(np.int32)), ids, ids, prep,
                                          item_cap=item_cap, status=st)
        _judge(A, A64, ACT_TOL, f"f={f} item_cap={item_cap} vrgcn fwd")
        _judge(ops.vrgcn_aggregate_bwd(_dev(dA), coef, ids, ids, dinv, prep, status=st), dH64, GRAD_TOL,
               f"f={f} item_cap={item_cap} vrgcn bwd")
        assert int(st.item()) == 0


@pytest.mark.parametrize("f", WIDTHS)
def test_gas_ladder_in_batch_and_mixed(f):
    ops = _ops()
    test_the_graph_has_the_ladder()
    G = _graph()
    ip, ix = G["ip"], G["ix"]
    rng = np.random.default_rng(500 + f)
    hbar = rng.standard_normal((N, f)).astype(F32)
    dv = GO.dinv(ip)
    dinv = _dev(dv.numpy().astype(F32))
    whole = np.concatenate([np.arange(len(LADDER)), rng.permutation(np.arange(len(LADDER), POOL_END))])
    mixed = np.concatenate([np.arange(len(LADDER)), np.arange(len(LADDER), POOL_END, 2), np.arange(POOL_END, N)])
    for name, node_idx in (("ladder and pool", whole), ("mixed", mixed)):
        n = len(node_idx)
        rowptr_h, code, counts = GO.resolve(ip, ix, node_idx)
        assert np.diff(rowptr_h)[:len(LADDER)].tolist() == LADDER and counts[1] > 0
        src, dst = GO.induced_edges(rowptr_h, code)
        if name == "ladder and pool":                                    # the backward's by-source rows have the ladder's lengths too
            assert (code[:rowptr_h[len(LADDER)]] >= 0).all()
            assert np.bincount(src, minlength=n)[:len(LADDER)].tolist() == LADDER
        else:
            head = code[:rowptr_h[len(LADDER)]]
            assert (head >= 0).any() and (head < 0).any()
        h, da = (rng.standard_normal((n, f)).astype(F32) for _ in range(2))
        ids = _dev(node_idx.astype(np.int32))
        prep = ops.PreparedGraph(_dev(src.astype(np.int32)), _dev(dst.astype(np.int32)), n)
        want = GO.aggregate(torch.from_numpy(h), torch.from_numpy(hbar), dv, node_idx, rowptr_h, code).numpy()
        for item_cap in (None, 0):
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            out = ops.gas_aggregate_fwd(_dev(h), _dev(hbar), dinv, ids, _dev(rowptr_h), _dev(code), item_cap=item_cap, status=st)
            _judge(out, want, ACT_TOL, f"f={f} {name} item_cap={item_cap} gas fwd")
            assert int(st.item()) == 0
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        _judge(ops.gas_aggregate_bwd(_dev(da), ids, dinv, prep, status=st),
               GO.aggregate_bwd(torch.from_numpy(da), dv, node_idx, src, dst).numpy(), GRAD_TOL, f"f={f} {name} gas bwd")
        assert int(st.item()) == 0
