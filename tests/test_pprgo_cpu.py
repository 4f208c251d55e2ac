"""PPRGo without a GPU: tests/pprgo_oracle.py against dense restatements; the C surface (the header declares the entry points, the
version stays 304, the signature table); the host-side argument checks; the trainer's refusals; the command line's namespace; and
the theorem that ties the training form to the power-iteration inference, in fp64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import pprgo_oracle as GO
from tests import shadow_oracle as SO
from tests import shadow_ppr_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"grapes_pprgo_topk": 17, "grapes_pprgo_batch_workspace_bytes": 2, "grapes_pprgo_batch": 19,
                "grapes_pprgo_aggregate_fwd_workspace_bytes": 3, "grapes_pprgo_aggregate_fwd": 12,
                "grapes_pprgo_aggregate_bwd_workspace_bytes": 3, "grapes_pprgo_aggregate_bwd": 14}
ONE = 1 << 30


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    from grapes_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.DIAG_LIB_PATH):
        ge.build()
    return _lib


# ---------------------------------------------------------------------------------------------------- the C surface
def test_header_table_and_both_libraries_carry_the_entry_points(built_lib):
    text = open(os.path.join(ROOT, "include", "grapes_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    prod, diag = ctypes.CDLL(built_lib.LIB_PATH), ctypes.CDLL(built_lib.DIAG_LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in grapes_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert name in built_lib.SIGNATURES and len(built_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(prod, name) and hasattr(diag, name), f"{name} is not exported"
    assert "#define GRAPES_ABI_VERSION 304" in text and built_lib.load().grapes_abi_version() == 304
    history = text[:text.index("#define GRAPES_ABI_VERSION")]
    assert "grapes_pprgo_topk" in history and "grapes_pprgo_batch" in history and "grapes_pprgo_aggregate_fwd" in history


def test_argument_checks_are_host_calls(built_lib):
    from grapes_amd import ops
    lib = built_lib.load()
    one = ctypes.c_void_p(16)                                            # a non-NULL aligned address that is never read

    def topk(m=4, k=10, alpha_q=16384, thr=65536, max_rounds=32, N=10):
        return lib.grapes_pprgo_topk(one, one, N, one, m, None, k, alpha_q, thr, max_rounds, one, one, one, None, None, None, None)
    assert topk(k=0) == -1 and topk(k=1024) == -1 and topk(m=0) == -1 and topk(m=4097) == -1 and topk(N=0) == -1
    assert topk(alpha_q=0) == -1 and topk(alpha_q=65536) == -1 and topk(thr=0) == -1 and topk(thr=ONE + 1) == -1
    assert topk(max_rounds=0) == -1 and topk(max_rounds=1025) == -1

    def batch(m=4, K=11, N=10, n_cap=8, e_cap=8, ws=one):
        return lib.grapes_pprgo_batch(one, one, m, K, N, one, one, n_cap, e_cap, one, one, one, one, one, one, None, ws, None, None)
    assert batch(m=0) == -1 and batch(m=4097) == -1 and batch(K=1) == -1 and batch(K=1025) == -1 and batch(N=0) == -1
    assert batch(n_cap=0) == -1 and batch(e_cap=0) == -1 and batch(ws=None) == -1 and batch(ws=ctypes.c_void_p(18)) == -2
    wb = lib.grapes_pprgo_batch_workspace_bytes
    assert wb(0, 10) == 0 and wb(10, 0) == 0 and wb(100, 1000) >= (3 * 100 + 4) * 4 and wb(100, 1000) < wb(1000, 1000)

    fw, bw = lib.grapes_pprgo_aggregate_fwd_workspace_bytes, lib.grapes_pprgo_aggregate_bwd_workspace_bytes
    long_row = lib.grapes_vrgcn_long_row()
    assert long_row == 64 == ops.VRGCN_LONG_ROW
    assert fw(8, long_row, 16) < 8 * 16 * 4 and fw(8, long_row + 1, 16) >= 8 * 1 * 16 * 4 and fw(8, 1024, 16) >= 8 * 15 * 16 * 4
    assert fw(0, 5, 4) == 0 and fw(4, 1, 4) == 0 and fw(4, 1025, 4) == 0 and fw(4097, 5, 4) == 0 and fw(4, 5, 0) == 0
    assert bw(0, 0, 4) == 0 and bw(5, -1, 4) == 0 and bw(5, (1 << 22) + 1, 4) == 0 and bw(5, 3, 16) >= 6 * 4 + 3 * 16 * 4

    def fwd(n=5, m=4, K=11, f=8, out=ctypes.c_void_p(32), ws=one):
        return lib.grapes_pprgo_aggregate_fwd(one, n, one, one, one, m, K, f, out, ws, None, None)
    assert fwd(n=0) == -1 and fwd(m=0) == -1 and fwd(K=1) == -1 and fwd(f=0) == -1 and fwd(f=1028) == -1 and fwd(f=257) == -1
    assert fwd(K=65, ws=None) == -1 and fwd(K=65, ws=ctypes.c_void_p(24)) == -2 and fwd(out=one) == -1      # (out may not be z)
    assert fwd(f=260, out=ctypes.c_void_p(20)) == -2                      # a float4 width over rows that are not 16-byte aligned

    def bwd(m=4, K=11, n=5, e=9, f=8, item_cap=0, ws=None):
        return lib.grapes_pprgo_aggregate_bwd(one, m, one, K, one, one, n, e, f, ctypes.c_void_p(32), item_cap, ws, None, None)
    assert bwd(n=0) == -1 and bwd(e=-1) == -1 and bwd(m=4097) == -1 and bwd(K=1) == -1 and bwd(f=0) == -1
    assert bwd(item_cap=-1) == -1 and bwd(item_cap=3) == -1 and bwd(item_cap=3, ws=ctypes.c_void_p(24)) == -2

    assert ops.PPRGO_MAX_ROOTS == 4096 and ops.PPRGO_MAX_SLOTS == 1024 and ops.pprgo_item_cap(4096 * 1024) == 4096 * 16 and ops.pprgo_item_cap(999, 64) == 0 and ops.pprgo_item_cap(999, 65) == 15
    rowptr, col = torch.tensor([0, 2, 3, 3]), torch.tensor([1, 2, 0], dtype=torch.int32)
    with pytest.raises(built_lib.GrapesHipError):                        # no CPU path
        ops.pprgo_topk(rowptr, col, 3, torch.tensor([0, 1], dtype=torch.int32), 2, 16384, 65536, 4)
    z, w = torch.zeros(3, 4), torch.zeros(2, 3)
    loc, cnt = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: ops.pprgo_aggregate_fwd(z, w, loc, cnt), lambda: ops.pprgo_aggregate_bwd(z[:2], w, cnt, cnt, 3, 0),
                 lambda: ops.pprgo_batch(loc, cnt, 3, (torch.zeros(1, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)))):
        with pytest.raises(built_lib.GrapesHipError):
            call()


# ---------------------------------------------------------------------------------------------------- the oracle
def _graphs():
    out = [SO.random_graph(n, d, 60 + i) for i, (n, d) in enumerate([(1, 0), (7, 2), (60, 5)])]
    out.append(SO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0], [], [4, 4]]))
    return out


def test_slot_tables_against_a_full_sort():
    aq, thr = PO.fixed(0.25, 2 ** -14)
    for ip, ix in _graphs():
        n = len(ip) - 1
        roots = [0, n - 1, n // 2, 0, n + 3, -1]
        for k in (1, 3, 64):
            K = k + 1
            t = GO.topk(ip, ix, roots, k, aq, thr, 32, live=5)
            assert t.bad_index and t.nbr.shape == t.score.shape == (6, K)
            assert (t.nbr[4:] == -1).all() and (t.score[4:] == 0).all() and t.cnt[4:].tolist() == [0, 0]      # a bad root, a root past *d_m
            assert np.array_equal(t.nbr[0], t.nbr[3]) and np.array_equal(t.score[0], t.score[3])             # a repeated root
            for b in range(4):
                res = PO.push(ip, ix, roots[b], aq, thr, 32)
                ids = np.array(sorted(v for v in res.score if v != roots[b] and res.score[v] > 0), dtype=np.int64)
                sc = np.array([res.score[int(v)] for v in ids], dtype=np.int64)
                full = ids[np.lexsort((ids, -sc))][:k] if len(ids) else ids
                c = int(t.cnt[b])
                assert c == 1 + len(full) and t.nbr[b, 0] == roots[b] and t.score[b, 0] == res.score[roots[b]]
                assert t.nbr[b, 1:c].tolist() == full.tolist() and t.score[b, 1:c].tolist() == [res.score[int(v)] for v in full]
                assert (t.nbr[b, c:] == roots[b]).all() and (t.score[b, c:] == 0).all()
                assert (t.rounds[b], t.stop[b]) == (res.rounds, res.stop)
                assert sorted(t.nbr[b, :c].tolist()) == sorted(PO.members(res, k))


def test_batch_structure_against_a_dense_restatement():
    rng = np.random.default_rng(5)
    for m, K, N in ((1, 2, 1), (5, 4, 9), (40, 7, 30), (3, 70, 200)):
        cnt = rng.integers(0, K + 1, m)
        cnt[0] = K
        nbr = np.stack([rng.permutation(max(N, K))[:K] % N for _ in range(m)]) if N >= K else np.zeros((m, K), dtype=np.int64)
        b = GO.batch(nbr, cnt, N)
        M = np.zeros((m * K, N), dtype=np.int64)                          # slot s lists node v
        for i in range(m):
            for t in range(cnt[i]):
                M[i * K + t, nbr[i, t]] = 1
        used = np.nonzero(M.sum(0))[0]
        assert b.node_idx.tolist() == used.tolist() and b.n == len(used) and b.e == int(cnt.sum()) == M.sum() and not b.bad_index
        assert b.tptr.tolist() == np.concatenate([[0], np.cumsum(M[:, used].sum(0))]).tolist()
        for u, v in enumerate(used):
            seg = b.tslot[b.tptr[u]:b.tptr[u + 1]]
            assert seg.tolist() == np.nonzero(M[:, v])[0].tolist()        # ascending slot indices
        for i in range(m):
            for t in range(K):
                want = -1 if cnt[i] == 0 else int(np.searchsorted(used, nbr[i, t if t < cnt[i] else 0]))
                assert b.loc[i, t] == want
    bad = GO.batch(np.array([[0, 9, 1]]), np.array([3]), 5)
    assert bad.bad_index and bad.loc.tolist() == [[0, -1, 1]] and bad.tslot.tolist() == [0, 2] and bad.n == 2


def test_gathers_against_dense_matrices():
    rng = np.random.default_rng(6)
    m, K, n, F = 6, 5, 9, 3
    cnt = np.array([5, 0, 1, 3, 5, 2])
    nbr = np.stack([rng.permutation(n)[:K] for _ in range(m)])
    b = GO.batch(nbr, cnt, n)
    w = rng.standard_normal((m, K))
    z, g = rng.standard_normal((b.n, F)), rng.standard_normal((m, F))
    W = np.zeros((m, b.n))                                               # the weighted incidence matrix
    for i in range(m):
        for t in range(cnt[i]):
            W[i, b.loc[i, t]] += w[i, t]
    out, mag = GO.aggregate_fwd(z, w, b.loc, cnt)
    dz, dmag = GO.aggregate_bwd(g, w, b.tptr, b.tslot, K)
    assert np.allclose(out, W @ z, rtol=0, atol=1e-12) and np.allclose(dz, W.T @ g, rtol=0, atol=1e-12)
    assert (mag >= np.abs(out) - 1e-12).all() and (dmag >= np.abs(dz) - 1e-12).all() and (out[1] == 0).all()
    assert abs((out * g).sum() - (z * dz).sum()) < 1e-10                 # <W z, g> = <z, W^T g>
    assert GO.gamma(3) == 3 * 2.0 ** -24 / (1 - 3 * 2.0 ** -24)


def test_weights_and_power_iteration_restated():
    ip, ix = SO.csr([[1, 2], [0], [0, 3, 3], [2, 2], []])
    d = GO.degrees(ip)
    assert d.tolist() == [2, 1, 3, 2, 1]
    nbr, score, cnt = np.array([[2, 0, 3], [4, 4, 4]]), np.array([[ONE >> 1, ONE >> 2, 3], [ONE, 0, 0]]), np.array([3, 1])
    row = GO.weights(ip, [2, 4], nbr, score, cnt, "row")
    assert row.tolist() == [[0.5, 0.25, 3 / ONE], [1.0, 0.0, 0.0]]
    sym, col = GO.weights(ip, [2, 4], nbr, score, cnt, "sym"), GO.weights(ip, [2, 4], nbr, score, cnt, "col")
    assert np.allclose(sym[0], row[0] * np.sqrt(3 / np.array([3, 2, 2]))) and np.allclose(col[0], row[0] * 3 / np.array([3, 2, 2]))
    assert sym[1].tolist() == col[1].tolist() == [1.0, 0.0, 0.0]
    A = GO.dense_adjacency(ip, ix)
    assert A[2].tolist() == [1, 0, 0, 2, 0] and np.allclose(GO.transition(A, "row").sum(1), [1, 1, 1, 1, 0])
    assert np.allclose(GO.transition(A, "col"), A / np.maximum(A.sum(1), 1)[None, :]) and np.allclose(GO.transition(A + A.T, "sym"), GO.transition(A + A.T, "sym").T)
    Z = np.arange(10.0).reshape(5, 2)
    S = GO.transition(A, "row")
    assert np.allclose(GO.power_iteration(S, Z, 0.3, 2), 0.7 * S @ (0.7 * S @ Z + 0.3 * Z) + 0.3 * Z) and np.array_equal(GO.power_iteration(S, Z, 0.3, 0), Z)


# ---------------------------------------------------------------------------------------------------- training form against inference
@pytest.mark.parametrize("alpha", [0.25, 0.5])
def test_the_training_form_is_the_power_iteration_up_to_the_missing_mass(alpha):
    """score_v <= pi_v elementwise, so for "row": |sum_t w_t Z_t - (power iteration, n rounds)_b| <= (1 - sum_t w_t + 2 (1 - alpha)^n)
    ||Z||_inf: the first term is the PPR mass the slots do not hold, the second the iteration's tail (alpha sum_{k >= n} (1 - alpha)^k
    plus its last term (1 - alpha)^n).  "sym" and "col" follow through the diagonal similarity S_sym = D^1/2 S_row D^-1/2, S_col = D
    S_row D^-1: with Z' = D^-1/2 Z (D^-1 Z) both sides are sqrt(d_b) (d_b) times the "row" statement for Z'."""
    ip, ix = PO.planted_graph(600, 6, 0)
    n, k, nprop = 600, 599, 200
    aq, thr = PO.fixed(alpha, 2.0 ** -30)
    assert thr == 1 and aq == alpha * 2 ** 16
    roots = [0, 17, 599]
    t = GO.topk(ip, ix, roots, k, aq, thr, 1024)
    assert (t.stop == 0).all() and (t.cnt == 600).all()
    A = GO.dense_adjacency(ip, ix)
    d = GO.degrees(ip)
    Z = np.random.default_rng(7).standard_normal((n, 5))
    row = GO.weights(ip, roots, t.nbr, t.score, t.cnt, "row")
    missing = 1.0 - row.sum(1)
    assert (missing >= 0).all() and (missing <= 1e-4).all()              # not vacuous: the slots hold the mass
    for b, root in enumerate(roots):
        pi = PO.exact_ppr(ip, ix, root, alpha)
        assert (pi[t.nbr[b]] - row[b] >= 0).all()
    tail = 2.0 * (1.0 - alpha) ** nprop
    for norm, scale in (("row", np.ones(n)), ("sym", np.sqrt(d)), ("col", d)):
        w = GO.weights(ip, roots, t.nbr, t.score, t.cnt, norm)
        train = np.stack([(w[b][:, None] * Z[t.nbr[b]]).sum(0) for b in range(len(roots))])
        infer = GO.power_iteration(GO.transition(A, norm), Z, alpha, nprop)[roots]
        zp = np.abs(Z / scale[:, None]).max()
        bound = scale[roots] * (missing + tail) * zp
        err = np.abs(train - infer).max(1)
        assert (err <= bound + 1e-12).all(), (norm, err, bound)
        assert (bound < 1e-3).all()


# ---------------------------------------------------------------------------------------------------- the sampler, the trainer, the driver
class _Col:
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def _fake_graph(nnz=3):
    from grapes_amd.graph import DeviceGraph
    g = object.__new__(DeviceGraph)
    g.rowptr, g.col, g.num_nodes, g.device = torch.tensor([0, 2, 3, 3]), _Col(nnz), 3, torch.device("cpu")
    g.bits, g.node_map = torch.zeros(1, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    return g


def test_sampler_and_trainer_refusals(monkeypatch):
    from grapes_amd import ops
    from grapes_amd.modules.pprgo import PPRGo, PPRGoSampler
    from grapes_amd.pprgo import PPRGoTrainer
    for kw, msg in ((dict(k=0), "k = 0 is not built"), (dict(k=1024), "k = 1024 is not built"), (dict(alpha=0.0), "alpha = 0.0 must lie"),
                    (dict(alpha=1.0), "alpha = 1.0 must lie"), (dict(eps=0.0), "eps = 0.0"), (dict(eps=float("nan")), "eps = nan"),
                    (dict(max_rounds=0), "max_rounds = 0 is outside"), (dict(normalization="max"), "normalization='max' is not built")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            PPRGoSampler(None, **kw)
    model = PPRGo(8, [16, 4])
    assert list(model.state_dict()) == ["lins.0.weight", "lins.1.weight"] and model.out_channels == 4
    assert model.mlp(torch.zeros(3, 8)).shape == (3, 4)
    with pytest.raises(ValueError, match="multiples of 4 up to 1024"):
        PPRGo(8, [16, 258])
    x = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="node features with a gradient are not built"):
        PPRGoTrainer(None, x.clone().requires_grad_(), None, model, None)
    with pytest.raises(TypeError, match="the model is a modules.pprgo.PPRGo, not Linear"):
        PPRGoTrainer(None, x, None, torch.nn.Linear(8, 4), None)
    with pytest.raises(ValueError, match="inference='exact' is not built"):
        PPRGoTrainer(None, x, None, model, None, inference="exact")
    with pytest.raises(ValueError, match="batch_size is 1 .. 4096"):
        PPRGoTrainer(None, x, None, model, None, batch_size=5000)
    with pytest.raises(ValueError, match="2\\^31 or more entries is not built"):
        PPRGoTrainer(_fake_graph(2 ** 31), x, None, model, None)
    monkeypatch.setattr(ops, "csr_symmetric_check", lambda rowptr, col, n: 1)
    with pytest.raises(ValueError, match="an asymmetric graph is not built"):
        PPRGoTrainer(_fake_graph(), x, None, model, None)
    monkeypatch.setattr(ops, "csr_symmetric_check", lambda rowptr, col, n: 0)
    tr = PPRGoTrainer(_fake_graph(), x, None, model, None)
    assert tr.sampler.deg.tolist() == [2.0, 1.0, 1.0] and tr.sampler.K == 33 and (tr.inference, tr.nprop) == ("power", 2)
    with pytest.raises(ValueError, match="nothing to inject"):
        tr._sample(torch.tensor([0]), object())
    with pytest.raises(ValueError, match="inference='exact' is not built"):
        tr.evaluate((), inference="exact")
    with pytest.raises(ValueError, match="normalization='max' is not built"):
        PPRGo.propagate(x, None, 0.5, 2, "max")


_DEFAULT = {'dataset': 'cora', 'batch_size': 512, 'hidden_dim': 256, 'num_layers': 2, 'lr': 0.001, 'max_epoch': 100, 'eval_frequency': 1,
            'dropout': 0.0, 'runs': 1, 'seed': None, 'ppr_k': 32, 'ppr_alpha': 0.5, 'ppr_eps': 1e-4, 'ppr_rounds': 32,
            'normalization': 'row', 'inference': 'power', 'nprop_inference': 2, 'precompute': True}


def test_parsed_namespace():
    from grapes_amd import pprgo
    got = vars(pprgo.parse_args(["--dataset", "cora"]))
    assert got == _DEFAULT and all(type(got[k]) is type(_DEFAULT[k]) for k in _DEFAULT)
    line = ("--dataset cora --ppr_k 32 --ppr_alpha 0.5 --ppr_eps 1e-4 --ppr_rounds 32 --normalization row --inference power "
            "--nprop_inference 2 --precompute true")
    assert line in pprgo.__doc__ and vars(pprgo.parse_args(line.split())) == _DEFAULT
    got = vars(pprgo.parse_args("--dataset cora --ppr_k 200 --normalization sym --inference ppr --nprop_inference 0 --precompute false".split()))
    assert got == dict(_DEFAULT, ppr_k=200, normalization="sym", inference="ppr", nprop_inference=0, precompute=False)


@pytest.mark.parametrize("argv,exc,message", [
    (["--normalization", "max"], SystemExit, None),
    (["--inference", "exact"], SystemExit, None),
    (["--precompute", "maybe"], SystemExit, None),
    (["--ppr_k", "1024"], ValueError, "k = 1024 is not built"),
    (["--ppr_alpha", "1.0"], ValueError, "--ppr_alpha lies inside (0, 1) and --ppr_eps inside (0, 1]"),
    (["--ppr_eps", "0"], ValueError, "--ppr_alpha lies inside (0, 1) and --ppr_eps inside (0, 1]"),
    (["--ppr_rounds", "2000"], ValueError, "max_rounds = 2000 is outside 1 .. 1024"),
    (["--nprop_inference", "-1"], ValueError, "--nprop_inference is at least 0"),
    (["--batch_size", "5000"], ValueError, "--batch_size is 1 .. 4096"),
    (["--num_layers", "0"], ValueError, "are at least 1"),
])
def test_command_line_refusals(argv, exc, message):
    from grapes_amd import pprgo
    with pytest.raises(exc) as e:
        pprgo.parse_args(["--dataset", "cora"] + argv)
    assert message is None or message in str(e.value)
