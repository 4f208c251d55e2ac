"""VR-GCN without a GPU: the host oracle (tests/vrgcn_oracle.py) against a dense closed form and fp64 torch.autograd, the
estimator's unbiasedness over every kept subset, its two identities, the driver's flags, the refusal of host tensors, and the new
entry points in the header, the ctypes table and the library."""
import ctypes
import itertools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import ladies_oracle as LO
from tests import vrgcn_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


def _graph(n=40, max_deg=7, seed=3, loops=4):
    ip, ix = LO.random_symmetric(n, max_deg, seed, loops=loops)
    return VO.loop_free(ip, ix)


def _kept_random(ip, ix, rows, k, rng):
    out = []
    for u in rows:
        cols = ix[ip[u]:ip[u + 1]]
        out.append(cols if (k == -1 or len(cols) <= k) else cols[np.sort(rng.choice(len(cols), k, replace=False))])
    return out


def _dense_forms(ip, ix, n, rows, kept):
    """(S [m, n], Q [m, n], self [m, n]) with A = self H + S (H - Hbar) + Q Hbar."""
    di = VO.dinv(ip)
    m = len(rows)
    S, Q, E = np.zeros((m, n)), np.zeros((m, n)), np.zeros((m, n))
    for r, u in enumerate(rows):
        d = ip[u + 1] - ip[u]
        E[r, u] = di[u] ** 2
        for v in kept[r]:
            S[r, v] += (d / len(kept[r])) * di[u] * di[v]
        for v in ix[ip[u]:ip[u + 1]]:
            Q[r, v] += di[u] * di[v]
    return S, Q, E


def test_loop_free_keeps_p():
    ip0, ix0 = LO.random_symmetric(30, 6, 9, loops=5)
    ip, ix = VO.loop_free(ip0, ix0)
    assert ip[-1] == ip0[-1] - 5 and not any(u in ix[ip[u]:ip[u + 1]] for u in range(30))
    # gcn_norm's P of the graph as stored: stored loops dropped, one unit loop per node
    V = np.eye(30)
    for i in range(30):
        for j in ix0[ip0[i]:ip0[i + 1]]:
            if i != j:
                V[i, j] += 1.0
    d = V.sum(1)
    assert np.abs(VO.dense_p(ip, ix, 30) - V / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]).max() <= 1e-15


def test_oracle_against_the_dense_closed_form_and_autograd():
    ip, ix = _graph()
    n, f = len(ip) - 1, 5
    rng = np.random.default_rng(1)
    rows = rng.permutation(n)[:17]
    kept = _kept_random(ip, ix, rows, 2, rng)
    H, Hbar, G = rng.standard_normal((n, f)), rng.standard_normal((n, f)), rng.standard_normal((17, f))
    A = VO.aggregate(ip, ix, rows, kept, H, Hbar)
    S, Q, E = _dense_forms(ip, ix, n, rows, kept)
    assert np.abs(A - (E @ H + S @ (H - Hbar) + Q @ Hbar)).max() <= 1e-12
    dH = VO.aggregate_grad(ip, rows, kept, G, n)
    assert np.abs(dH - (E + S).T @ G).max() <= 1e-12
    Ht, Hb = torch.tensor(H, requires_grad=True), torch.tensor(Hbar, requires_grad=True)
    At = torch.tensor(E) @ Ht + torch.tensor(S) @ (Ht - Hb.detach()) + torch.tensor(Q) @ Hb.detach()
    (At * torch.tensor(G)).sum().backward()
    assert np.abs(dH - Ht.grad.numpy()).max() <= 1e-12 and Hb.grad is None


def test_unbiased_over_every_kept_subset():
    """The mean of A[u] over ALL C(d_u, k) kept subsets is (P H)[u]: this pins the d_u / k_u factor."""
    e = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (2, 3), (3, 6), (4, 6), (5, 6), (1, 6)]
    s, d = [a for a, b in e] + [b for a, b in e], [b for a, b in e] + [a for a, b in e]
    ip, ix = LO.csr_from_edges(s, d, 8)                                  # node 7 is isolated: d = 0
    rng = np.random.default_rng(2)
    H, Hbar = rng.standard_normal((8, 3)), rng.standard_normal((8, 3))
    PH = VO.dense_p(ip, ix, 8) @ H
    for k in (1, 2, 3):
        for u in range(8):
            cols = ix[ip[u]:ip[u + 1]]
            subsets = list(itertools.combinations(cols.tolist(), min(k, len(cols))))
            mean = np.mean([VO.aggregate(ip, ix, [u], [np.array(sub, dtype=np.int64)], H, Hbar)[0] for sub in subsets], axis=0)
            assert np.abs(mean - PH[u]).max() <= 1e-12, (k, u)
    assert np.abs(VO.aggregate(ip, ix, [7], [np.zeros(0, np.int64)], H, Hbar)[0] - H[7]).max() == 0.0     # d = 0: dinv = 1, the self term


def test_identities_in_fp64():
    ip, ix = _graph(seed=5)
    n, f = len(ip) - 1, 4
    rng = np.random.default_rng(6)
    H, Hbar = rng.standard_normal((n, f)), rng.standard_normal((n, f))
    rows = rng.permutation(n)[:20]
    P = VO.dense_p(ip, ix, n)
    every = _kept_random(ip, ix, rows, -1, rng)
    assert np.abs(VO.aggregate(ip, ix, rows, every, H, Hbar) - (P @ H)[rows]).max() <= 1e-12          # fanout -1, any history
    for k in (1, 2, 5):
        kept = _kept_random(ip, ix, rows, k, rng)
        assert np.abs(VO.aggregate(ip, ix, rows, kept, H, H) - (P @ H)[rows]).max() <= 1e-12         # history = H, anything kept


def test_step_against_autograd_and_history_carry():
    """Three steps of the 3-layer oracle: loss and every gradient against fp64 torch.autograd over dense operators with the
    histories detached; each step's histories are the previous step's activations."""
    from tests import sage_oracle as SO
    ip0, ix0 = LO.random_symmetric(60, 6, 11, loops=3)
    n, F, widths, C = 60, 6, [5, 4], 3
    rng = np.random.default_rng(12)
    x, y = rng.standard_normal((n, F)), rng.integers(0, C, n)
    dims = [F] + widths + [C]
    Ws = [rng.standard_normal((dims[i + 1], dims[i])) * 0.5 for i in range(3)]
    bs = [rng.standard_normal(dims[i + 1]) * 0.1 for i in range(3)]
    tr = VO.Trainer64(ip0, ix0, x, widths)
    ip, ix = tr.indptr, tr.indices
    for stepno in range(3):
        targets = rng.permutation(n)[:9]
        layers = VO.batch_layers(SO.sample(ip, ix, targets, [2, 2, 2], seed=40 + stepno))
        hb = [h.copy() for h in tr.hbar]
        out = tr.step(Ws, bs, layers, y[targets])
        if stepno:
            assert all(np.abs(h).max() > 0 for h in hb)                  # a non-zero history from the second step on
        Wt = [torch.tensor(w, requires_grad=True) for w in Ws]
        bt = [torch.tensor(v, requires_grad=True) for v in bs]
        rows = [layers[2 - i].prev for i in range(3)]
        h = torch.relu(torch.tensor(tr.px[rows[0]]) @ Wt[0].T + bt[0])
        for i in (1, 2):
            S, Q, E = _dense_forms(ip, ix, n, rows[i], layers[2 - i].kept)
            Hg = torch.zeros((n, h.shape[1]), dtype=torch.float64).index_add(0, torch.as_tensor(rows[i - 1]), h)
            Hb = torch.tensor(hb[i - 1])
            z = (torch.tensor(E) @ Hg + torch.tensor(S) @ (Hg - Hb) + torch.tensor(Q) @ Hb) @ Wt[i].T + bt[i]
            h = torch.relu(z) if i < 2 else z
        loss = torch.nn.functional.cross_entropy(h, torch.as_tensor(y[targets]))
        loss.backward()
        assert abs(out.loss - float(loss.detach())) <= 1e-12
        for i in range(3):
            assert np.abs(out.dW[i] - Wt[i].grad.numpy()).max() <= 1e-12 and np.abs(out.db[i] - bt[i].grad.numpy()).max() <= 1e-12
        for l, (r, hl) in enumerate(out.acts):                           # exactly the computed rows changed
            changed = np.zeros(n, bool); changed[r] = True
            assert np.array_equal(tr.hbar[l][changed], hl) and np.array_equal(tr.hbar[l][~changed], hb[l][~changed])
    z2, g2 = VO.loss_and_grad(rng.standard_normal((4, 3)), (rng.random((4, 3)) > 0.5).astype(np.float32))
    assert np.isfinite(z2) and g2.shape == (4, 3)


# ------------------------------------------------------------------------------------------------------------ the driver
_DEFAULTS = dict(dataset="cora", batch_size=512, hidden_dim=256, num_layers=2, lr=1e-3, max_epoch=100, eval_frequency=1,
                 dropout=0.0, runs=1, seed=None, fanouts=[2, 2])


def test_parse_args():
    from grapes_amd import vrgcn
    assert vars(vrgcn.parse_args(["--dataset", "cora"])) == _DEFAULTS
    b = vrgcn.parse_args(["--dataset", "reddit", "--batch_size", "64", "--hidden_dim", "32", "--num_layers", "3", "--lr", "0.01",
                          "--max_epoch", "7", "--eval_frequency", "2", "--dropout", "0", "--runs", "3", "--seed", "5", "--fanouts",
                          "3,-1,64"])
    assert vars(b) == dict(dataset="reddit", batch_size=64, hidden_dim=32, num_layers=3, lr=0.01, max_epoch=7, eval_frequency=2,
                           dropout=0.0, runs=3, seed=5, fanouts=[3, -1, 64])
    assert vrgcn.parse_args(["--dataset", "cora", "--fanouts", "4"]).num_layers == 1
    with pytest.raises(SystemExit, match="--dataset is required"):
        vrgcn.parse_args([])
    with pytest.raises(ValueError, match="--dropout other than 0"):
        vrgcn.parse_args(["--dataset", "cora", "--dropout", "0.5"])
    with pytest.raises(ValueError, match="--fanouts holds one entry per layer: 2 given for --num_layers 3"):
        vrgcn.parse_args(["--dataset", "cora", "--fanouts", "2,2", "--num_layers", "3"])
    for fan in ("0", "65", "-2", ""):
        with pytest.raises(ValueError, match="fanout"):
            vrgcn.parse_args(["--dataset", "cora", "--fanouts", fan])
    with pytest.raises(SystemExit):
        vrgcn.parse_args(["--dataset", "cora", "--fanouts", "2,x"])
    with pytest.raises(ValueError, match="--batch_size is 1 .. 4096"):
        vrgcn.parse_args(["--dataset", "cora", "--batch_size", "5000"])
    with pytest.raises(SystemExit):                                      # no flag of another driver
        vrgcn.parse_args(["--dataset", "cora", "--aggr", "mean"])


def test_no_cpu_path():
    from grapes_amd import _lib, ops
    from grapes_amd.modules.gcn import GCN
    from grapes_amd.modules.vrgcn import VRGCNLayerFn
    from grapes_amd.vrgcn import VrgcnTrainer
    h, hbar = torch.zeros(3, 4), torch.zeros(5, 4)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    rowptr, col = torch.zeros(6, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        ops.vrgcn_aggregate_fwd(h, i32(0, 1, 2), hbar, torch.ones(5), rowptr, col, i32(0), i32(0), None)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        ops.vrgcn_aggregate_bwd(torch.zeros(1, 4), torch.zeros(1), i32(0, -1, -1), i32(0, 1, 2), torch.ones(5), None)
    lay = SimpleNamespace(node_idx=i32(0, 1, 2), dinv=torch.ones(5), rowptr=rowptr, col=col, rows_g=i32(0), rows_l=i32(0), prep=None,
                          pos=i32(0, -1, -1), item_cap=0, status=None)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        VRGCNLayerFn.apply(h, hbar, lay)
    with pytest.raises(_lib.GrapesHipError, match="no CPU path"):
        VrgcnTrainer(None, torch.zeros(5, 4), torch.zeros(5, dtype=torch.long), GCN(4, [8, 2]), None)


# ------------------------------------------------------------------------------------------------------------ the C surface
_NEW = {"grapes_vrgcn_long_row": 0, "grapes_vrgcn_aggregate_workspace_bytes": 3, "grapes_vrgcn_aggregate_fwd": 23,
        "grapes_vrgcn_aggregate_bwd": 16}


def test_header_ctypes_and_exports_agree():
    import __graft_entry__ as ge
    from grapes_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grapes_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in _NEW.items():
        m = re.search(r"\b(?:int|int32_t|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        args = m.group(1).strip()
        assert (0 if args in ("", "void") else len(args.split(","))) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs and hasattr(lib, name), name
    assert "#define GRAPES_ABI_VERSION 304" in src
    bound = _lib.load()
    long_row = bound.grapes_vrgcn_long_row()                             # host helpers: callable without a GPU
    assert long_row == ops.VRGCN_LONG_ROW and long_row % 64 == 0 and long_row >= 64
    assert int(re.search(r"#define GRAPES_LONG_ROW (\d+)", src).group(1)) == 64
    assert bound.grapes_vrgcn_aggregate_workspace_bytes(10, 3, 8) >= 11 * 4 + 3 * 8 * 4
    assert os.path.exists(os.path.join(ROOT, "grapes_amd", "csrc", "vrgcn_kernels.hip"))
    assert "vrgcn_kernels.o" in open(os.path.join(ROOT, "grapes_amd", "csrc", "Makefile")).read()
