"""AS-GCN without a GPU: the C surface, the host oracle (tests/asgcn_oracle.py) against dense definitions, the two forms of the
variance, the analytic gradient to the sampler against central finite differences, the zero-sum identity of T, and the driver's
arguments."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import asgcn_oracle as AO
from tests import ladies_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("grapes_asgcn_importance", "grapes_asgcn_rows_workspace_bytes", "grapes_asgcn_variance", "grapes_asgcn_logq_bwd")
F32, F64 = np.float32, np.float64


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
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in grapes_hip.h"
        assert name in built_lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(prod, name) and hasattr(diag, name), f"{name} is not exported"
    assert built_lib.load().grapes_abi_version() == 304


def test_rows_workspace_is_a_host_call_that_grows(built_lib):
    lib = built_lib.load()
    sizes = [lib.grapes_asgcn_rows_workspace_bytes(m, n) for m, n in ((1, 1), (64, 100), (4096, 5000))]
    assert 0 < sizes[0] < sizes[1] < sizes[2] and sizes[2] >= 4 * (5000 + 3 * 4096)


# ---------------------------------------------------------------------------------------------------- graphs and batches
def _graphs():
    ip, ix, n = LO.hand_graph()
    rp, rx = LO.random_symmetric(64, 8, 11, loops=5)
    return {"hand": (ip, ix, n, np.array([5, 2, 11])), "random64": (rp, rx, 64, np.random.default_rng(1).permutation(64)[:12])}


def _sampler_params(n, F, seed):
    """x, w_g, b_g with no a_j within 1e-4 of 0 and both signs of a present (asserted on the input)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, F)).astype(F32)
    w_g, b_g = (rng.standard_normal(F) * 0.7).astype(F32), np.array([0.05], F32)
    a = x.astype(F64) @ w_g.astype(F64) + float(b_g[0])
    assert np.abs(a).min() > 1e-4 and (a > 0).any() and (a < 0).any()
    return x, w_g, b_g


@pytest.mark.parametrize("name", ["hand", "random64"])
def test_column_mass_is_the_column_sum_of_dense_p(name):
    ip, ix, n, targets = _graphs()[name]
    P = LO.dense_p(ip, ix, n)
    x, w_g, b_g = _sampler_params(n, 5, 3)
    b = AO.sample(ip, ix, n, targets, 4, 3, x, w_g, b_g, uniforms=[np.random.default_rng(d).random(n).astype(F32) for d in range(3)])
    prev = targets
    for L in b.layers:
        assert np.array_equal(L.prev, prev)
        c = P[prev].sum(0)
        assert np.allclose(L.imp.c, c, rtol=1e-13, atol=0)
        assert np.array_equal(L.candidates, np.nonzero(c > 0)[0]) and np.array_equal(L.imp.terms, (P[prev] > 0).sum(0))
        a = x.astype(F64) @ w_g.astype(F64) + float(b_g[0])
        assert np.allclose(L.imp.q, c * (np.maximum(a, 0) + 1), rtol=1e-13)
        l32 = AO.shifted_logits32(L.imp.logq[L.candidates].astype(F32))
        assert l32.max() == F32(-20.0) and (l32 <= -20.0).all()
        assert len(L.sampled) == min(len(L.candidates), 4) and np.isin(targets, L.after).all()
        # the weights: (P_ij / q_j) over the kept columns, row-normalised (D_i cancels)
        for i in prev:
            kept = [j for j in L.after if P[i, j] > 0]
            r = np.array([P[i, j] / L.imp.q[j] for j in kept])
            got = L.w[L.dst == i]
            assert np.array_equal(L.src[L.dst == i], kept) and np.allclose(got, r / r.sum(), rtol=1e-12)
        prev = L.after


def _fixed_batch(name, layers=2, samp_num=5, F=5, C=3, Hd=6, seed=7):
    ip, ix, n, targets = _graphs()[name]
    x, w_g, b_g = _sampler_params(n, F, seed)
    rng = np.random.default_rng(seed + 1)
    b = AO.sample(ip, ix, n, targets, samp_num, layers, x, w_g, b_g, uniforms=[rng.random(n).astype(F32) for _ in range(layers)])
    c_local = [np.where(L.imp.c[b.node_idx] > 0, L.imp.c[b.node_idx], 1.0) for L in b.layers]
    v = [AO.entry_v(ip, ix, L.src, L.dst) for L in b.layers]
    dims = [F] + [Hd] * (layers - 1) + [C]
    Ws = [rng.standard_normal((dims[i + 1], dims[i])) * 0.5 for i in range(layers)]
    bs = [rng.standard_normal(dims[i + 1]) * 0.1 for i in range(layers)]
    labels = rng.integers(0, C, len(targets))
    return SimpleBatch(b=b, xb=x[b.node_idx], w_g=w_g, b_g=b_g, c_local=c_local, v=v, Ws=Ws, bs=bs, labels=labels)


class SimpleBatch:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def step(self, w_g=None, b_g=None, var_coef=0.5, H_const=None):
        b = self.b
        return AO.train_step64(self.xb, self.Ws, self.bs, self.w_g if w_g is None else w_g, self.b_g if b_g is None else b_g,
                               b.edge_index, self.c_local, self.v, b.local_prev, b.local_targets, self.labels, var_coef,
                               H_const=H_const)


@pytest.mark.parametrize("name", ["hand", "random64"])
def test_variance_both_ways_and_not_negative(name):
    S = _fixed_batch(name)
    r = S.step()
    b = S.b
    for d in range(len(b.layers)):                                       # (the identity holds on any layer's list)
        H = np.random.default_rng(d).standard_normal((len(b.node_idx), 4)).astype(F32) if d else r.H0.astype(F32)
        var = AO.variance(b.edge_index[d][0], b.edge_index[d][1], r.w[d].astype(F32), b.local_prev[d], H)
        assert (np.abs(var.V - var.V_dev) <= 1e-12 * np.maximum(var.V_mag, 1e-300)).all()
        assert (var.V >= -1e-12 * var.V_mag).all() and (var.V_dev >= 0).all()
        assert np.isclose(var.L_var, var.V.mean(), rtol=1e-13)
    # the step's own L_var is the closed form over the fp64 weights
    H = r.H0
    w, (src, dst) = r.w[0], b.edge_index[0]
    tot = 0.0
    for i in b.local_prev[0]:
        k = np.nonzero(dst == i)[0]
        mu = (w[k, None] * H[src[k]]).sum(0)
        tot += ((len(k) * w[k, None] * H[src[k]] - mu) ** 2).sum() / len(k)
    assert np.isclose(r.L_var, tot / len(b.local_prev[0]), rtol=1e-12)


@pytest.mark.parametrize("name", ["hand", "random64"])
@pytest.mark.parametrize("var_coef", [0.0, 0.5])
def test_finite_differences_confirm_the_gradient_to_the_sampler(name, var_coef):
    """Central differences, step 1e-6, on every component of w_g and on b_g with the batch held fixed, against the oracle's
    analytic gradient of L_c + lambda L_var (H, a constant of L_var, held at the base point's value); and the closed form the device
    computes (T, then -[a > 0] / g) against autograd.  Agreement to 1e-6 is demanded twice: norm-wise, of every component against
    the largest one, and per component against its own size with the floor 1e-3 of the largest (a central difference of a loss of
    order 1 at step 1e-6 carries about 1e-16 / 1e-6 = 1e-10 of absolute noise, which is 1e-6 of a component of 1e-4)."""
    S = _fixed_batch(name)
    r = S.step(var_coef=var_coef)
    assert np.abs(r.a).min() > 1e-4                                      # no kink inside a difference
    h = 1e-6
    loss = lambda **kw: S.step(var_coef=var_coef, H_const=r.H0, **kw).loss
    fd_w = np.zeros(len(S.w_g))
    for f in range(len(S.w_g)):
        e = np.zeros(len(S.w_g)); e[f] = h
        fd_w[f] = (loss(w_g=S.w_g.astype(F64) + e) - loss(w_g=S.w_g.astype(F64) - e)) / (2 * h)
    fd_b = (loss(b_g=S.b_g.astype(F64) + h) - loss(b_g=S.b_g.astype(F64) - h)) / (2 * h)
    scale = max(np.abs(r.dw_g).max(), abs(float(r.db_g[0])))
    print(f"[asgcn] {name} lambda {var_coef}: |fd - analytic| / scale: w_g {np.abs(fd_w - r.dw_g).max() / scale:.2e}, "
          f"b_g {abs(fd_b - float(r.db_g[0])) / scale:.2e}")
    assert scale > 0
    assert np.abs(fd_w - r.dw_g).max() <= 1e-6 * scale and abs(fd_b - float(r.db_g[0])) <= 1e-6 * scale
    an, fd = np.append(r.dw_g, float(r.db_g[0])), np.append(fd_w, fd_b)
    assert (np.abs(fd - an) <= 1e-6 * np.maximum(np.abs(an), 1e-3 * scale)).all(), np.abs(fd - an) / np.maximum(np.abs(an), 1e-3 * scale)
    assert np.abs(r.da_T - r.da).max() <= 1e-12 * max(np.abs(r.da).max(), 1e-300)
    gx = r.da_T @ S.xb.astype(F64)
    assert np.allclose(gx, r.dw_g, rtol=1e-10, atol=1e-14 * scale) and np.isclose(r.da_T.sum(), float(r.db_g[0]), rtol=1e-10, atol=1e-14 * scale)


@pytest.mark.parametrize("name", ["hand", "random64"])
def test_t_sums_to_zero_per_layer(name):
    S = _fixed_batch(name, layers=3)
    r = S.step()
    b = S.b
    for d in range(3):
        G = r.G[d]
        T, Tm, _, terms = AO.logq_bwd(b.edge_index[d][0], b.edge_index[d][1], r.w[d], (G, np.abs(G), G), b.local_prev[d], len(b.node_idx))
        # logq_bwd rounds the weights to fp32, each by at most 2^-24 of itself: a row sums to 1 +- 2^-24, so |sum T| <= 2^-24 sum |Gbar|
        assert terms > 0 and abs(T.sum()) <= 2.0 ** -24 * terms
        assert abs(r.T[d].sum()) <= 1e-12 * terms                        # the fp64 weights: to rounding
        assert (np.abs(T) <= Tm * (1 + 1e-12)).all()


# ---------------------------------------------------------------------------------------------------- the driver
def test_cli_arguments():
    from grapes_amd import asgcn
    a = asgcn.parse_args(["--dataset", "cora"])
    assert (a.samp_num, a.batch_size, a.hidden_dim, a.num_layers, a.lr, a.var_coef) == (64, 512, 256, 2, 1e-3, 0.5)
    assert a.dropout == 0.0 and a.runs == 1 and a.seed is None and a.e_cap is None and a.eval_frequency == 1 and a.max_epoch == 100
    assert not hasattr(a, "sampler")
    b = asgcn.parse_args(["--dataset", "cora", "--samp_num", "8", "--num_layers", "3", "--e_cap", "100", "--max_epoch", "2",
                          "--seed", "7", "--dropout", "0.5", "--runs", "2", "--eval_frequency", "5", "--var_coef", "0.25"])
    assert (b.samp_num, b.num_layers, b.e_cap, b.max_epoch, b.seed, b.dropout, b.runs, b.eval_frequency, b.var_coef) == \
        (8, 3, 100, 2, 7, 0.5, 2, 5, 0.25)
    with pytest.raises(SystemExit):
        asgcn.parse_args(["--dataset", "cora", "--sampler", "ladies"])
    with pytest.raises(SystemExit):
        asgcn.parse_args([])
    with pytest.raises(ValueError):
        asgcn.parse_args(["--dataset", "cora", "--batch_size", "5000"])
    with pytest.raises(ValueError):
        asgcn.parse_args(["--dataset", "cora", "--var_coef", "-1"])


def test_the_ladies_driver_still_refuses_asgcn():
    from grapes_amd import ladies
    from grapes_amd.modules.ladies import KINDS, LayerWiseSampler
    assert KINDS == ("ladies", "fastgcn")
    with pytest.raises(SystemExit):
        ladies.parse_args(["--dataset", "cora", "--sampler", "asgcn"])
    with pytest.raises(ValueError, match="ladies, fastgcn"):
        LayerWiseSampler(object(), 4, 2, kind="asgcn")
