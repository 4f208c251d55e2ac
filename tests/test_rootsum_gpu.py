"""The folded aggregation (grapes_rootsum_aggregate_fwd / _bwd) on the MI355X with arguments neither SAGEConv nor ClusterGCNConv
passes — stored loops AND the self term (self_weight = 0.5) AND the mean-plus-one scale — against a numpy fp64 reference of the
formula grapes_hip.h states:
    out[i] = relu(s_i (sum_{j -> i} src[j] + (loops[i] + 0.5) src[i]) + add[i] + bias),  s_i = 1 / (1 + deg_i),
    deg_i = the row's stored entries, its loops among them.
tests/test_row_sum_gpu.py's graph (a hub as target and as source, stored loops, duplicates, isolated rows, 260 live rows of 300),
widths 30 (scalar columns) and 100 (float4 columns), with and without the long-row items, at the project's tolerances:
activations 1e-5, gradients 1e-4 in max|a - ref| / max(1, max|ref|)."""
import numpy as np
import pytest

from tests import sage_oracle as SO
from tests.test_row_sum_gpu import ACT_TOL, GRAD_TOL, N_ALLOC, N_LIVE, _check, _graph, _marked, _place

pytestmark = pytest.mark.gpu

SELF_WEIGHT = 0.5
F64 = np.float64


@pytest.mark.parametrize("f", [30, 100])
def test_loops_self_term_and_mean_plus_one_together_against_fp64(f):
    ei, prep, _ = _graph()
    from grapes_amd import ops
    m = N_LIVE
    rng = np.random.default_rng(500 + f)
    x, g, add, add_b = (rng.standard_normal((N_ALLOC, f)).astype(np.float32) for _ in range(4))
    bias = rng.standard_normal(f).astype(np.float32)
    xd, gd, addd, addbd, biasd = (_place(a, 0) for a in (x, g, add, add_b, bias))
    # the reference, once per width: A[i, j] = the stored edges j -> i, loops among them
    A = np.zeros((m, m), F64)
    np.add.at(A, (ei[1], ei[0]), 1.0)
    s = 1.0 / (1.0 + A.sum(1))
    M = s[:, None] * (A + SELF_WEIGHT * np.eye(m))                       # out = act(M src + add + bias)
    want_out = (M @ x[:m].astype(F64) + add[:m] + bias).clip(min=0)
    args = ("sage", ops.ROOTSUM_SCALE_MEAN_PLUS_ONE, SELF_WEIGHT, True, prep.loops)
    for long_rows in (True, False):
        tag = f"f={f} long_rows={long_rows}"
        out, dsrc, dadd = (_marked(f, 0) for _ in range(3))
        ops._rootsum_fwd(*args, xd, prep, addd, biasd, True, out, None, long_rows)
        _check(out, want_out, ACT_TOL, tag + " fwd")
        _, _, dbias = ops._rootsum_bwd(*args, gd, prep, out, addbd, True, True, True, dsrc, dadd, long_rows)
        gate = g[:m].astype(F64) * (out[:m].cpu().numpy() > 0)           # (the device's own gates)
        _check(dsrc, M.T @ gate + add_b[:m], GRAD_TOL, tag + " bwd dsrc")
        _check(dadd, gate, ACT_TOL, tag + " bwd dadd")
        err = SO.rel_err(dbias.cpu().numpy(), gate.sum(0))
        print(f"{tag} bwd dbias: rel err {err:.3e} (tolerance {GRAD_TOL:g})")
        assert err <= GRAD_TOL
    assert prep.status is None or int(prep.status.item()) == 0
