"""Bits of the SAGEConv / ClusterGCNConv aggregation on the MI355X: every output of ops.sage_aggregate_fwd / _bwd and
ops.cluster_aggregate_fwd / _bwd on tests/test_row_sum_gpu.py's graph has the SHA-256 recorded in tests/golden/rootsum_bits.json —
recorded once, before the two aggregations were folded into one code path, by

    python -m tests.test_rootsum_bits_gpu --record [PATH]

Only the four public functions are called, so this file runs unchanged on either side of that change.  Each of the 8 widths, with
and without the long-row items.  SAGE: mean and sum; forward with add, bias, ReLU and copy_out, and bare; backward with relu_out,
add, dsrc, dadd and dbias, and dsrc alone (for sum: no row-local pass).  Cluster-GCN (the same edges, loops not attached):
diag_lambda 0, 0.5 and -1, the same four calls.  The hash is over the bytes of the live rows."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_row_sum_gpu import CASES, N_ALLOC, N_LIVE, _graph, _marked, _place

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rootsum_bits.json")
LAMBDAS = (0.0, 0.5, -1.0)
_SHARED = {}


def _sha(t, rows=True):
    a = (t[:N_LIVE] if rows else t).contiguous().cpu().numpy()
    return hashlib.sha256(a.tobytes()).hexdigest()


def _cluster_prep():
    """The graph's edges prepared without the loop counts: ClusterGCNConv's loop-free CSRs."""
    if "prep" not in _SHARED:
        from grapes_amd import ops
        ei, _, d_n = _graph()
        src, dst = (torch.from_numpy(ei[k]).int().cuda().contiguous() for k in (0, 1))
        _SHARED["prep"] = ops.PreparedGraph(src, dst, N_ALLOC, d_n=d_n)
    return _SHARED["prep"]


def _four_calls(tag, fwd, bwd, xd, gd, addd, biasd, f, off, long_rows, got):
    out, copy, dsrc, dadd = (_marked(f, off) for _ in range(4))
    fwd(add=addd, bias=biasd, relu=True, out=out, copy_out=copy, long_rows=long_rows)
    _, _, dbias = bwd(relu_out=out, add=addd, dsrc=dsrc, dadd=dadd, want_bias=True, long_rows=long_rows)
    for name, t in (("out", out), ("copy", copy), ("dsrc", dsrc), ("dadd", dadd)):
        got[f"{tag} full {name}"] = _sha(t)
    got[f"{tag} full dbias"] = _sha(dbias, rows=False)
    out, dsrc = _marked(f, off), _marked(f, off)
    fwd(out=out, long_rows=long_rows)
    bwd(dsrc=dsrc, long_rows=long_rows)
    got[f"{tag} bare out"], got[f"{tag} bare dsrc"] = _sha(out), _sha(dsrc)


def _hashes(f, off):
    """{name: sha256} of every output at one width, both item forms."""
    from grapes_amd import ops
    _, prep, _ = _graph()
    cprep = _cluster_prep()
    rng = np.random.default_rng(7000 + 2 * f + off)
    x, g, add = (rng.standard_normal((N_ALLOC, f)).astype(np.float32) for _ in range(3))
    bias = rng.standard_normal(f).astype(np.float32)
    xd, gd, addd, biasd = (_place(a, off) for a in (x, g, add, bias))
    got = {}
    for long_rows in (True, False):
        for aggr in ("mean", "sum"):
            _four_calls(f"f={f} off={off} long_rows={long_rows} sage {aggr}",
                        lambda **kw: ops.sage_aggregate_fwd(xd, prep, aggr, **kw),
                        lambda **kw: ops.sage_aggregate_bwd(gd, prep, aggr, **kw), xd, gd, addd, biasd, f, off, long_rows, got)
        for lam in LAMBDAS:
            _four_calls(f"f={f} off={off} long_rows={long_rows} cluster lambda={lam}",
                        lambda **kw: ops.cluster_aggregate_fwd(xd, cprep, lam, **kw),
                        lambda **kw: ops.cluster_aggregate_bwd(gd, cprep, lam, **kw), xd, gd, addd, biasd, f, off, long_rows, got)
    torch.cuda.synchronize()
    for p in (prep, cprep):
        assert p.status is None or int(p.status.item()) == 0
    return got


def _built(f, off):
    """test_row_sum_gpu's sage_ok: the widths the aggregation takes (that test asserts the refusal of the others)."""
    return f <= 256 or (f % 4 == 0 and off == 0)


@pytest.mark.parametrize("f,off", [c for c in CASES if _built(*c)])
def test_every_output_keeps_its_recorded_bits(f, off):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = _hashes(f, off)
    prefix = f"f={f} off={off} "
    assert sorted(got) == sorted(k for k in want if k.startswith(prefix))
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(got)} outputs changed bits: {bad[:6]}"


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: python -m tests.test_rootsum_bits_gpu --record [PATH]")
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    rec = {}
    for f_, off_ in CASES:
        if _built(f_, off_):
            rec.update(_hashes(f_, off_))
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(rec)} hashes to {path}")
