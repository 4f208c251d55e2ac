"""ShaDow-GNN's PPR scope without a GPU: the entry points and their host-side argument checks; tests/shadow_ppr_oracle.py against a
dense restatement in int64 matrices, its mass after every round, its member order against a full sort, its estimate against exact
PPR in fp64 at the push's own bound; the sampler's and the trainer's refusals and the command line's namespace."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import shadow_oracle as SO
from tests import shadow_ppr_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"grapes_shadow_ppr_sample": 27, "grapes_shadow_ppr_sample_workspace_bytes": 2}
ONE, T = 1 << 30, 4096


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    from grapes_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.DIAG_LIB_PATH):
        ge.build()
    return _lib


def test_header_table_and_both_libraries_carry_the_entry_points(built_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grapes_hip.h")).read(), flags=re.S)
    prod, diag = ctypes.CDLL(built_lib.LIB_PATH), ctypes.CDLL(built_lib.DIAG_LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in grapes_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert name in built_lib.SIGNATURES and len(built_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(prod, name) and hasattr(diag, name), f"{name} is not exported"
    assert built_lib.load().grapes_abi_version() == 304                  # additive: the version stays


def test_workspace_and_argument_checks_are_host_calls(built_lib):
    from grapes_amd import ops
    lib = built_lib.load()
    wb = lib.grapes_shadow_ppr_sample_workspace_bytes
    assert wb(4, 10) >= (3 * 4 * 11 + 3 * 4 + 1) * 4 and wb(4, 10) < wb(400, 10) < wb(400, 1023)
    assert wb(4, 1024) == 0 and wb(4, 0) == 0 and wb(0, 5) == 0 and wb(4097, 5) == 0 and wb(4096, 1023) > 0
    one = ctypes.c_void_p(16)                                            # a non-NULL aligned address that is never read

    def call(m=4, k=10, alpha_q=16384, thr=65536, max_rounds=32, n_cap=8, e_cap=8, ws=one):
        return lib.grapes_shadow_ppr_sample(one, one, 10, one, m, None, k, alpha_q, thr, max_rounds, n_cap, e_cap, one, one, one, one,
                                            one, one, None, None, None, None, one, one, ws, None, None)
    assert call(k=0) == -1 and call(k=1024) == -1 and call(m=0) == -1 and call(m=4097) == -1
    assert call(alpha_q=0) == -1 and call(alpha_q=65536) == -1 and call(thr=0) == -1 and call(thr=ONE + 1) == -1
    assert call(max_rounds=0) == -1 and call(max_rounds=1025) == -1 and call(n_cap=0) == -1 and call(e_cap=0) == -1
    assert call(ws=ctypes.c_void_p(18)) == -2
    assert ops.SHADOW_PPR_TOUCHED == T == PO.T and ops.SHADOW_PPR_ONE == ONE == PO.ONE
    assert ops.shadow_ppr_args(1023, 65535, ONE, 1024) == 1024 and ops.shadow_ppr_args(1, 1, 1, 1) == 2
    for bad in ((0, 1, 1, 1), (1024, 1, 1, 1), (5, 0, 1, 1), (5, 65536, 1, 1), (5, 1, 0, 1), (5, 1, ONE + 1, 1), (5, 1, 1, 0), (5, 1, 1, 1025)):
        with pytest.raises(ValueError, match="shadow_ppr_sample: "):
            ops.shadow_ppr_args(*bad)
    rowptr, col = torch.tensor([0, 2, 3, 3]), torch.tensor([1, 2, 0], dtype=torch.int32)
    with pytest.raises(built_lib.GrapesHipError):                        # no CPU path
        ops.shadow_ppr_sample(rowptr, col, 3, torch.tensor([0, 1], dtype=torch.int32), 2, 16384, 65536, 4, e_cap=16)


# ---------------------------------------------------------------------------------------------------- the dense restatement
def _dense(ip, ix, root, alpha_q, thr, max_rounds):
    """The rule with int64 matrices: A[v, u] = the multiplicity of u in row v; a round is one integer matrix step."""
    n = len(ip) - 1
    A = np.zeros((n, n), dtype=np.int64)
    for v in range(n):
        for u in ix[ip[v]:ip[v + 1]]:
            A[v, int(u)] += 1
    deg = A.sum(1)
    r, p, S = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    r[root], S[root] = ONE, True
    rounds = 0
    while True:
        F = S & (r > 0) & (r >= thr * deg)
        if not F.any():
            stop = 0
            break
        if rounds == max_rounds:
            stop = 1
            break
        if S.sum() + deg[F].sum() > T:
            stop = 2
            break
        spread = F & (deg > 0)
        keep = np.where(spread, (r * alpha_q) >> 16, 0)
        p = p + np.where(F & (deg == 0), r, keep)
        share = np.where(spread, (r - keep) // np.maximum(deg, 1), 0)
        r = np.where(F, 0, r) + A.T @ share
        S = S | ((A.T @ spread.astype(np.int64)) > 0)
        rounds += 1
    return p, r, S, p + ((r * alpha_q) >> 16), rounds, stop


def _small_graphs():
    out = []
    for seed, (n, d) in enumerate([(1, 0), (2, 1), (7, 2), (30, 3), (60, 5), (60, 12)]):
        out.append(SO.random_graph(n, d, 40 + seed))                     # loops, duplicates and empty rows occur
    out.append(SO.random_graph(60, 6, 50, hub=3, hub_degree=5000))       # a row that alone exceeds T: stop 2
    out.append(SO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0], [], [4, 4]]))
    return out


@pytest.mark.parametrize("alpha,eps,max_rounds", [(0.25, 2 ** -10, 32), (0.25, 2 ** -14, 32), (0.5, 2 ** -16, 32), (0.15, 2 ** -20, 3),
                                                  (0.9999, 2 ** -30, 1024), (2 ** -16, 1.0, 5)])
def test_oracle_against_the_dense_restatement(alpha, eps, max_rounds):
    aq, thr = PO.fixed(alpha, eps)
    stops = set()
    for ip, ix in _small_graphs():
        n = len(ip) - 1
        for root in sorted({0, n // 2, n - 1, min(3, n - 1)}):
            res = PO.push(ip, ix, root, aq, thr, max_rounds)
            p, r, S, score, rounds, stop = _dense(ip, ix, root, aq, thr, max_rounds)
            assert (res.rounds, res.stop) == (rounds, stop) and sorted(res.r) == np.nonzero(S)[0].tolist() == sorted(res.p)
            for v in res.r:
                assert (res.p[v], res.r[v], res.score[v]) == (int(p[v]), int(r[v]), int(score[v]))
            assert r[~S].sum() == 0 and p[~S].sum() == 0
            stops.add(stop)
    assert 0 in stops and (max_rounds > 3 or 1 in stops)


def test_the_hub_row_alone_stops_with_code_2_at_round_0():
    ip, ix = SO.random_graph(60, 6, 50, hub=3, hub_degree=5000)
    res = PO.push(ip, ix, 3, *PO.fixed(0.25, 2 ** -14), 32)
    assert (res.rounds, res.stop, list(res.r)) == (0, 2, [3]) and PO.members(res, 10) == [3]
    assert res.score[3] == (ONE * 16384) >> 16


# ---------------------------------------------------------------------------------------------------- the hub graph of the rule's table
_G = {}


def _hub_graph():
    if "hub" not in _G:
        _G["hub"] = SO.random_graph(3000, 8, 1, hub=7, hub_degree=2500)
    return _G["hub"]


def _hub_roots():
    ip, ix = _hub_graph()
    return [0, 7, int(ix[ip[7]]), 100, 1234, 2999]


@pytest.mark.parametrize("alpha,eps", [(0.25, 2 ** -10), (0.25, 2 ** -12), (0.25, 2 ** -14), (0.5, 2 ** -16), (0.15, 2 ** -20)])
def test_mass_never_exceeds_one_and_the_table_is_never_overfull(alpha, eps):
    ip, ix = _hub_graph()
    aq, thr = PO.fixed(alpha, eps)
    for root in _hub_roots():
        seen = []

        def after(r, p):
            assert sum(r.values()) + sum(p.values()) <= ONE and len(r) <= T and r.keys() == p.keys()
            seen.append(len(r))
        res = PO.push(ip, ix, root, aq, thr, 32, after_round=after)
        assert len(seen) == res.rounds and seen == sorted(seen)
        assert max(res.score.values()) <= ONE and sum(res.score.values()) <= ONE


def test_the_rules_table():
    """What was recorded of this graph when the rule was written — touched nodes (rounded there to tens), rounds and stop codes."""
    ip, ix = _hub_graph()
    roots = _hub_roots()
    run = lambda a, e, mr=32: [PO.push(ip, ix, r, *PO.fixed(a, e), mr) for r in roots]
    res = run(0.25, 2 ** -10)
    assert (res[1].rounds, res[1].stop, len(res[1].r)) == (0, 0, 1)      # the hub root never pushes: 2^30 < thr * 2500
    assert all(230 <= len(x.r) <= 340 and 3 <= x.rounds <= 4 and x.stop == 0 for i, x in enumerate(res) if i != 1)
    res = run(0.25, 2 ** -12)
    assert all(620 <= len(x.r) <= 1690 and 2 <= x.rounds <= 5 and x.stop == 0 for x in res)
    res = run(0.25, 2 ** -14)
    assert res[1].stop == 2 and all(2170 <= len(x.r) <= 2370 and 6 <= x.rounds <= 7 and x.stop == 0 for i, x in enumerate(res) if i != 1)
    assert all(x.stop == 1 and x.rounds == 2 for i, x in enumerate(run(0.25, 2 ** -14, 2)) if i != 1)
    for a, e in ((0.5, 2 ** -16), (0.15, 2 ** -20)):
        res = run(a, e)
        assert sum(x.stop == 2 for x in res) >= 4 and all(1 <= x.rounds <= 6 for x in res)


def test_member_order_against_a_full_sort():
    ip, ix = _hub_graph()
    for alpha, eps in ((0.25, 2 ** -10), (0.25, 2 ** -14), (0.5, 2 ** -16)):
        for root in _hub_roots():
            res = PO.push(ip, ix, root, *PO.fixed(alpha, eps), 32)
            ids = np.array(sorted(res.score), dtype=np.int64)
            sc = np.array([res.score[int(v)] for v in ids], dtype=np.int64)
            keep = (ids != root) & (sc > 0)
            ids, sc = ids[keep], sc[keep]
            full = ids[np.lexsort((ids, -sc))]                            # score descending, then id ascending
            if len(sc) > 1:                                               # ties are everywhere: the id order decides
                assert len(np.unique(sc)) < len(sc)
            for k in (1, 32, 200, 1023):
                mem = PO.members(res, k)
                assert mem[0] == root and mem[1:] == full[:k].tolist() and len(mem) == 1 + min(k, len(full))


def test_the_batch_of_the_oracle():
    ip, ix = SO.csr([[1, 1, 0, 2], [0, 0, 1], [2, 0, 2, 1, 1], [0], [], [4, 4]])
    ob = PO.sample(ip, ix, [0, 4, 9, 5, 0], 2, *PO.fixed(0.25, 2 ** -14), 32)
    assert ob.bad_index and ob.root_n_id[2] == -1 and ob.ptr[2] == ob.ptr[3] and ob.rounds[2] == ob.stop[2] == 0
    assert ob.n_id[ob.ptr[1]:ob.ptr[2]].tolist() == [4] and ob.score[ob.ptr[1]] == ONE        # an isolated root: all mass to p
    assert ob.n_id[ob.ptr[3]:ob.ptr[4]].tolist() == [4, 5]                                    # 5 reaches the empty row of 4
    a, b = slice(ob.ptr[0], ob.ptr[1]), slice(ob.ptr[4], ob.ptr[5])
    assert np.array_equal(ob.n_id[a], ob.n_id[b]) and np.array_equal(ob.score[a], ob.score[b]) and len(ob.n_id[a]) == 3
    assert ob.n == len(ob.n_id) == len(ob.score) == len(ob.batch) and ob.e == ob.edge_index.shape[1] == len(ob.e_id)
    assert (np.diff(ob.ptr) <= 3).all() and ob.n_id[ob.root_n_id[0]] == 0


# ---------------------------------------------------------------------------------------------------- against exact PPR
@pytest.mark.parametrize("alpha,eps", [(0.25, 2 ** -10), (0.25, 2 ** -14), (0.5, 2 ** -12)])
def test_estimate_against_exact_ppr_in_fp64(alpha, eps):
    """On a symmetric graph a push that stops because no node is left to push (code 0) leaves r_u < eps deg(u) everywhere, and
    pi_root(v) - p_v = sum_u r_u pi_u(v) with pi_u(v) = pi_v(u) deg(v) / deg(u): so 0 <= pi_v - p_v <= eps deg(v).  Fixed point
    drops remainders: the mass lost = 2^30 - sum p - sum r can only lower p, by at most itself.  Derived, not tuned; alpha and eps
    are exact in fixed point here.  T is never reached: 600 + 5 * 600 <= 4096."""
    ip, ix = PO.planted_graph()
    n = len(ip) - 1
    deg = np.diff(ip)
    aq, thr = PO.fixed(alpha, eps)
    assert aq == alpha * 2 ** 16 and thr == eps * 2 ** 30 and n == 600 and np.array_equal(deg, np.full(n, 5))
    A = np.zeros((n, n), dtype=np.int64)
    np.add.at(A, (np.repeat(np.arange(n), deg), ix), 1)
    assert np.array_equal(A, A.T)
    for root in (0, 5, 123, 300, 599):
        res = PO.push(ip, ix, root, aq, thr, 1024)
        assert res.stop == 0 and res.rounds >= 2
        pi = PO.exact_ppr(ip, ix, root, alpha)
        assert abs(pi.sum() - 1.0) < 1e-12
        p = np.zeros(n)
        for v, pv in res.p.items():
            p[v] = pv / ONE
        lost = ONE - sum(res.p.values()) - sum(res.r.values())
        assert lost >= 0
        assert (p <= pi).all(), float((p - pi).max())
        assert (pi - p <= eps * deg + lost / ONE).all(), float((pi - p - eps * deg).max())


# ---------------------------------------------------------------------------------------------------- the sampler, the trainer, the driver
def test_sampler_and_trainer_refuse_values_outside_the_rule():
    """The argument checks come before the graph is touched."""
    from grapes_amd.modules.shadow import ShaDow, ShaDowPPRSampler
    from grapes_amd.shadow import ShadowTrainer
    for kw, msg in ((dict(k=0), "k = 0 is not built"), (dict(k=1024), "k = 1024 is not built"), (dict(k=5, alpha=0.0), "alpha = 0.0 must lie"),
                    (dict(k=5, alpha=1.0), "alpha = 1.0 must lie"), (dict(k=5, alpha=1e-6), "alpha_q = 0 is outside"),
                    (dict(k=5, alpha=0.999999), "alpha_q = 65536 is outside"), (dict(k=5, eps=0.0), "eps = 0.0"),
                    (dict(k=5, eps=1.5), "eps = 1.5"), (dict(k=5, eps=float("nan")), "eps = nan"),
                    (dict(k=5, max_rounds=0), "max_rounds = 0 is outside"), (dict(k=5, max_rounds=1025), "max_rounds = 1025 is outside"),
                    (dict(k=5, e_cap=0), "n_cap and e_cap are at least 1")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            ShaDowPPRSampler(None, **kw)
    m = ShaDow(8, 16, 4, 2)
    with pytest.raises(ValueError, match="scope='ball' is not built"):
        ShadowTrainer(None, torch.zeros(3, 8), None, m, None, scope="ball")
    with pytest.raises(ValueError, match="k = 2000 is not built"):
        ShadowTrainer(None, torch.zeros(3, 8), None, m, None, scope="ppr", ppr_k=2000)


_KHOP = {'dataset': 'cora', 'batch_size': 512, 'hidden_dim': 256, 'num_layers': 3, 'lr': 0.001, 'max_epoch': 100,
         'eval_frequency': 1, 'dropout': 0.0, 'runs': 1, 'seed': None, 'depth': 2, 'num_neighbors': 10, 'conv': 'sage', 'pool': True}
_PPR = dict(_KHOP, scope="ppr", ppr_k=200, ppr_alpha=0.25, ppr_eps=2 ** -14, ppr_rounds=32)


def test_parsed_namespace():
    from grapes_amd import shadow
    assert vars(shadow.parse_args(["--dataset", "cora", "--scope", "khop"])) == _KHOP == vars(shadow.parse_args(["--dataset", "cora"]))
    got = vars(shadow.parse_args(["--dataset", "cora", "--scope", "ppr"]))
    assert got == _PPR and all(type(got[k]) is type(_PPR[k]) for k in _PPR)
    got = vars(shadow.parse_args(["--dataset", "cora", "--scope", "ppr", "--ppr_k", "32", "--ppr_alpha", "0.5", "--ppr_eps", "0.001",
                                  "--ppr_rounds", "7", "--depth", "9", "--num_neighbors", "64"]))      # (the k-hop cap is not PPR's)
    assert got == dict(_PPR, ppr_k=32, ppr_alpha=0.5, ppr_eps=0.001, ppr_rounds=7, depth=9, num_neighbors=64)


@pytest.mark.parametrize("argv,exc,message", [
    (["--scope", "ball"], SystemExit, None),
    (["--scope", "ppr", "--ppr_k", "1024"], ValueError, "shadow_ppr_sample: k = 1024 is not built"),
    (["--scope", "ppr", "--ppr_k", "0"], ValueError, "shadow_ppr_sample: k = 0 is not built"),
    (["--scope", "ppr", "--ppr_alpha", "1.0"], ValueError, "--ppr_alpha lies inside (0, 1) and --ppr_eps inside (0, 1]"),
    (["--scope", "ppr", "--ppr_eps", "0"], ValueError, "--ppr_alpha lies inside (0, 1) and --ppr_eps inside (0, 1]"),
    (["--scope", "ppr", "--ppr_rounds", "2000"], ValueError, "shadow_ppr_sample: max_rounds = 2000 is outside 1 .. 1024"),
    (["--scope", "ppr", "--batch_size", "5000"], ValueError, "--batch_size is 1 .. 4096"),
    (["--ppr_k", "32"], ValueError, "--ppr_k, --ppr_alpha, --ppr_eps and --ppr_rounds belong to --scope ppr"),
])
def test_command_line_refusals(argv, exc, message):
    from grapes_amd import shadow
    with pytest.raises(exc) as e:
        shadow.parse_args(["--dataset", "cora"] + argv)
    assert message is None or message in str(e.value)
