"""The plain-sum gather GCN2Conv and SAGEConv share (grapes_amd/csrc/row_sum.h) on the MI355X, through the four entry points that
launch it — grapes_gcn2_propagate_fwd / _bwd and grapes_rootsum_aggregate_fwd / _bwd — against the fp64 oracles of tests/gcn2_oracle.py
and tests/sage_oracle.py at the project's tolerances (activations 1e-5, gradients 1e-4 in max|a − ref| / max(1, max|ref|)).

One graph of 300 allocated rows, 260 of them live (d_n): node 5 is a hub as target AND as source (more than 3 GRAPES_LONG_ROW
entries in its row of either CSR), with stored loops, duplicate edges and isolated rows.  One width per instantiated shape
<VEC, LPR, NS> of the kernels, each once with the long-row item lists (rows, chunks and combine kernels) and once without (every
row through the rows kernel).  Rows past d_n keep the mark the buffers were filled with."""
import numpy as np
import pytest
import torch

from tests import gcn2_oracle as O
from tests import sage_oracle as SO

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-5, 1e-4
LONG_ROW = 64                          # GRAPES_LONG_ROW
N_ALLOC, N_LIVE, HUB = 300, 260, 5
ALPHA = 0.3
FMARK = 12345.0
F64 = np.float64
# (width, operands' offset from a 16-byte boundary in floats): <4,32,1> <4,64,1> <4,64,4> <1,32,1> <1,64,1> <1,64,4> <1,64,16>, and
# the scalar shape of an aligned width
CASES = [(100, 0), (200, 0), (320, 0), (30, 0), (47, 0), (201, 0), (330, 0), (100, 1)]
_SHARED = {}


def _graph():
    """(edge list [2, e] among the live rows, its PreparedGraph over the allocated rows with the loop counts, d_n)."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if "graph" not in _SHARED:
        from grapes_amd import ops
        rng = np.random.default_rng(91)
        base = O.random_graph(N_LIVE, seed=92, mean_deg=4, hub=HUB, hub_deg=200, n_dup=15, n_loops=12, n_isolated=8)
        out_edges = np.stack([np.full(200, HUB), rng.integers(0, N_LIVE - 8, 200)])       # the hub as source
        ei = np.concatenate([base, out_edges, np.array([[HUB, HUB], [HUB, HUB]]).T.reshape(2, -1)], axis=1).astype(np.int64)
        off = ei[0] != ei[1]
        indeg, outdeg = np.bincount(ei[1][off], minlength=N_LIVE), np.bincount(ei[0][off], minlength=N_LIVE)
        assert indeg[HUB] > 3 * LONG_ROW and outdeg[HUB] > 3 * LONG_ROW
        assert np.delete(indeg, HUB).max() <= LONG_ROW and np.delete(outdeg, HUB).max() <= LONG_ROW
        _, cnt = np.unique(ei[0] * N_LIVE + ei[1], return_counts=True)
        assert (cnt > 1).any() and (~off).sum() >= 14 and ((indeg == 0) & (outdeg == 0)).sum() >= 8
        d_n = torch.tensor([N_LIVE], dtype=torch.int32, device="cuda")
        src, dst = (torch.from_numpy(ei[k]).int().cuda().contiguous() for k in (0, 1))
        prep = ops.gcn2_attach_loops(ops.PreparedGraph(src, dst, N_ALLOC, d_n=d_n), src, dst)
        assert int(prep.n_items_t.item()) >= 4 and int(prep.n_items_s.item()) >= 4
        _SHARED["graph"] = (ei, prep, d_n)
    return _SHARED["graph"]


def _place(a, off):
    """The fp32 array on the device, its first element `off` floats past a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 4, device="cuda")
    t = buf[off:off + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * off
    return t


def _marked(f, off):
    return _place(np.full((N_ALLOC, f), FMARK, np.float32), off)


def _check(got, want, tol, what):
    got = got.cpu().numpy()
    err = SO.rel_err(got[:N_LIVE], want)
    print(f"{what}: rel err {err:.3e} (tolerance {tol:g})")
    assert err <= tol, what
    assert (got[N_LIVE:] == FMARK).all(), what + ": rows past d_n"


@pytest.mark.parametrize("f,off", CASES)
def test_shared_gather_through_the_four_entry_points(f, off):
    ei, prep, d_n = _graph()
    from grapes_amd import ops
    L, P_ = ops.lib(), ops._p
    m = N_LIVE
    rng = np.random.default_rng(1000 + 2 * f + off)
    x, x0, g, add = (rng.standard_normal((N_ALLOC, f)).astype(np.float32) for _ in range(4))
    bias = rng.standard_normal(f).astype(np.float32)
    xd, x0d, gd, addd, biasd = (_place(a, off) for a in (x, x0, g, add, bias))
    # the references, once per width
    x64, g64 = torch.as_tensor(x[:m].astype(F64)), torch.as_tensor(g[:m].astype(F64))
    P = O.propagate(x64, ei).numpy()
    s_, d_ = O.edges(ei)
    At_g = torch.zeros(m, f, dtype=O.F64).index_add(0, s_, g64[d_]).numpy()
    want_p, want_s = (1 - ALPHA) * P, (1 - ALPHA) * P + ALPHA * x0[:m].astype(F64)
    want_dx, want_dx0 = (1 - ALPHA) * At_g, ALPHA * g[:m].astype(F64)
    sage_ok = f <= 256 or (f % 4 == 0 and off == 0)
    ws = ops._ws(max(L.grapes_gcn2_propagate_workspace_bytes(N_ALLOC, prep.item_cap, f),
                     L.grapes_rootsum_aggregate_workspace_bytes(N_ALLOC, prep.item_cap, f)), "cuda")
    for long_rows in (True, False):
        tag = f"f={f} off={off} long_rows={long_rows}"
        it_t, nt, it_s, ns, cap = (P_(prep.items_t), P_(prep.n_items_t), P_(prep.items_s), P_(prep.n_items_s), prep.item_cap) \
            if long_rows else (None, None, None, None, 0)
        so, po, dx, dx0 = (_marked(f, off) for _ in range(4))
        assert L.grapes_gcn2_propagate_fwd(P_(xd), P_(x0d), P_(prep.loops), P_(prep.rowptr_t), P_(prep.csr_src), ALPHA, P_(so), P_(po),
                                           N_ALLOC, P_(d_n), f, it_t, nt, cap, P_(ws), P_(prep.status), ops._stream()) == 0
        assert L.grapes_gcn2_propagate_bwd(P_(gd), None, 0, None, P_(prep.loops), P_(prep.rowptr_s), P_(prep.csr_dst), ALPHA, P_(dx),
                                           P_(dx0), 0, N_ALLOC, P_(d_n), f, it_s, ns, cap, P_(ws), P_(prep.status), ops._stream()) == 0
        _check(so, want_s, ACT_TOL, tag + " gcn2 fwd S"); _check(po, want_p, ACT_TOL, tag + " gcn2 fwd P'")
        _check(dx, want_dx, GRAD_TOL, tag + " gcn2 bwd dx"); _check(dx0, want_dx0, GRAD_TOL, tag + " gcn2 bwd dx0")
        if not sage_ok:                                                  # the wide scalar shape is GCN2's alone
            out = _marked(f, off)
            with pytest.raises(ValueError, match="not built"):
                ops.sage_aggregate_fwd(xd, prep, "mean", out=out, long_rows=long_rows)
            assert L.grapes_rootsum_aggregate_fwd(P_(xd), f, None, 0, None, P_(prep.loops), P_(prep.rowptr_t), P_(prep.csr_src), 0.0, 0,
                                                  ops.ROOTSUM_SCALE_MEAN, 0, P_(out), f, None, 0, N_ALLOC, P_(d_n), f, it_t, nt, cap,
                                                  P_(ws), P_(prep.status), ops._stream()) < 0
            assert L.grapes_rootsum_aggregate_bwd(P_(gd), f, None, 0, P_(prep.loops), P_(prep.rowptr_t), P_(prep.rowptr_s),
                                                  P_(prep.csr_dst), 0.0, 0, ops.ROOTSUM_SCALE_NONE, None, 0, P_(out), f, None, 0, None,
                                                  N_ALLOC, P_(d_n), f, it_s, ns, cap, P_(ws), P_(prep.status), ops._stream()) < 0
            assert bool((out == FMARK).all())
            continue
        for aggr in ("mean", "sum"):
            out, copy, dsrc, dadd = (_marked(f, off) for _ in range(4))
            ops.sage_aggregate_fwd(xd, prep, aggr, add=addd, bias=biasd, relu=True, out=out, copy_out=copy, long_rows=long_rows)
            agg = SO.aggregate64(x64, ei, m, aggr).numpy()
            _check(out, (agg + add[:m] + bias).clip(min=0), ACT_TOL, f"{tag} sage fwd {aggr}")
            assert torch.equal(copy[:m], xd[:m]) and bool((copy[m:] == FMARK).all())
            _, _, dbias = ops.sage_aggregate_bwd(gd, prep, aggr, relu_out=out, add=addd, dsrc=dsrc, dadd=dadd, want_bias=True,
                                                 long_rows=long_rows)
            gate = g[:m].astype(F64) * (out[:m].cpu().numpy() > 0)       # (the device's own gates)
            _check(dsrc, SO.mean_sum_backward_closed_form(gate, ei, m, aggr) + add[:m], GRAD_TOL, f"{tag} sage bwd {aggr} dsrc")
            _check(dadd, gate, ACT_TOL, f"{tag} sage bwd {aggr} dadd")
            assert SO.rel_err(dbias.cpu().numpy(), gate.sum(0)) <= GRAD_TOL
            # without add, bias and ReLU: the backward gathers dout itself (sum) or its scaled copy (mean)
            out, dsrc = _marked(f, off), _marked(f, off)
            ops.sage_aggregate_fwd(xd, prep, aggr, out=out, long_rows=long_rows)
            _check(out, agg, ACT_TOL, f"{tag} sage fwd {aggr} plain")
            ops.sage_aggregate_bwd(gd, prep, aggr, dsrc=dsrc, long_rows=long_rows)
            _check(dsrc, SO.mean_sum_backward_closed_form(g[:m], ei, m, aggr), GRAD_TOL, f"{tag} sage bwd {aggr} plain dsrc")
    assert prep.status is None or int(prep.status.item()) == 0
