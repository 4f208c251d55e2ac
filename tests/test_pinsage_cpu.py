"""PinSAGE without a GPU: tests/pinsage_oracle.py against literal restatements (the walk step by step, the selection as a full sort of
(-count, id)), the stop rules on hand cases, the mean visit counts against the exact expectation from a dense fp64 matrix power, the
weights, the block chain, the C surface, the refusals, the command line, and the closed-form gradients of relu_l2norm and PinSAGEConv
(the modules' own autograd functions over host stand-ins for the kernels) against fp64 autograd of a plain-torch restatement."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pinsage_oracle as PS
from tests import pprgo_oracle as GO
from tests import shadow_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"grapes_pinsage_neighbors": 18, "grapes_relu_l2norm_fwd": 9, "grapes_relu_l2norm_bwd": 13}
FULL = 2 ** 32 - 1


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
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in grapes_hip.h as int or size_t"
        assert len([a for a in m.group(2).split(",") if a.strip()]) == nargs, name
        assert name in built_lib.SIGNATURES and len(built_lib.SIGNATURES[name][1]) == nargs, name
        assert built_lib.SIGNATURES[name][0] in (built_lib.I32, built_lib.SZ)
        assert hasattr(prod, name) and hasattr(diag, name), f"{name} is not exported"
    assert "#define GRAPES_ABI_VERSION 304" in text and built_lib.load().grapes_abi_version() == 304
    history = text[:text.index("#define GRAPES_ABI_VERSION")]
    assert "grapes_pinsage_neighbors" in history and "grapes_relu_l2norm_fwd" in history


def test_argument_checks_are_host_calls(built_lib):
    from grapes_amd import ops
    lib = built_lib.load()
    one = ctypes.c_void_p(16)                                            # a non-NULL aligned address that is never read

    def nb(m=4, R=10, L=2, T=3, N=10, nbr=one):
        return lib.grapes_pinsage_neighbors(one, one, N, one, m, None, R, L, 0, T, 0, 0, None, nbr, one, one, None, None)
    assert nb(R=0) == -1 and nb(L=0) == -1 and nb(R=1025, L=1) == -1 and nb(R=205, L=5) == -1 and nb(R=2 ** 20, L=2 ** 12) == -1
    assert nb(T=0) == -1 and nb(T=1024) == -1 and nb(m=0) == -1 and nb(N=0) == -1 and nb(nbr=None) == -1
    assert nb(m=2 ** 21, T=1023) == -1                                   # m K = 2^31

    def fwd(m=4, f=8, ld=8, eps=1e-12, s=one, out=ctypes.c_void_p(32)):
        return lib.grapes_relu_l2norm_fwd(s, ld, m, f, eps, out, ld, one, None)
    assert fwd(m=0) == -1 and fwd(f=0) == -1 and fwd(ld=7) == -1 and fwd(eps=0.0) == -1 and fwd(s=None) == -1
    assert fwd(f=257, ld=257) == -1 and fwd(f=1028, ld=1028) == -1
    assert fwd(f=260, ld=260, out=ctypes.c_void_p(20)) == -2 and fwd(f=260, ld=261) == -2      # a float4 width, rows not 16-byte aligned

    def bwd(m=4, f=8, ld=8, eps=1e-12, ds=ctypes.c_void_p(32)):
        return lib.grapes_relu_l2norm_bwd(one, ld, one, ld, one, one, ld, m, f, eps, ds, ld, None)
    assert bwd(m=0) == -1 and bwd(f=0) == -1 and bwd(ld=7) == -1 and bwd(eps=-1.0) == -1 and bwd(ds=None) == -1
    assert bwd(f=260, ld=260, ds=ctypes.c_void_p(20)) == -2

    assert ops.PINSAGE_MAX_VISITS == 1024 and ops.PINSAGE_MAX_NEIGHBORS == 1023 and ops.pinsage_args(256, 4, 1023) == 1024
    assert ops.pinsage_term_q(0.0) == 0 and ops.pinsage_term_q(0.5) == 2 ** 31 and ops.pinsage_term_q(1 - 2 ** -40) == FULL
    assert PS.term_q(0.25) == ops.pinsage_term_q(0.25) == 2 ** 30
    for R, L, T, msg in ((205, 5, 3, "R L <= 1024"), (0, 2, 3, "R L <= 1024"), (10, 2, 1024, "T = 1024 neighbours are not built"),
                         (10, 2, 0, "T = 0 neighbours are not built")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            ops.pinsage_args(R, L, T)
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="outside \\[0, 1\\)"):
            ops.pinsage_term_q(p)
    rowptr, col = torch.tensor([0, 2, 3, 3]), torch.tensor([1, 2, 0], dtype=torch.int32)
    with pytest.raises(built_lib.GrapesHipError):                        # no CPU path
        ops.pinsage_neighbors(rowptr, col, 3, torch.tensor([0, 1], dtype=torch.int32), 4, 2, 0, 2)
    with pytest.raises(built_lib.GrapesHipError):
        ops.relu_l2norm_fwd(torch.zeros(3, 4))
    with pytest.raises(built_lib.GrapesHipError):
        ops.relu_l2norm_bwd(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros(3), torch.zeros(3, 4))


# ---------------------------------------------------------------------------------------------------- the oracle
_HAND12 = SO.csr([[1, 2, 3], [0, 2], [0, 1, 3, 4], [0, 2, 5, 5], [2, 6], [3, 6, 7], [4, 5, 8], [5], [6, 9, 10], [8], [8, 11], []])


def _literal_counts(indptr, indices, v, R, L, tq, seed, off):
    """The rule read step by step from the header, with no helper shared with the oracle but the generator."""
    count = {}
    for j in range(R):
        c = v
        for t in range(L):
            P = SO.philox4x32_10_wide(v | (j << 32), off + (t >> 1), seed)
            a, s = P[2 * (t & 1)], P[2 * (t & 1) + 1]
            deg = int(indptr[c + 1] - indptr[c])
            if a < tq or deg == 0:
                break
            c = int(indices[int(indptr[c]) + ((s * deg) >> 32)])
            if c != v:
                count[c] = count.get(c, 0) + 1
    return count


def test_walk_against_a_literal_restatement_and_selection_against_a_full_sort():
    graphs = [_HAND12, SO.random_graph(60, 5, 71), SO.random_graph(7, 2, 72)]
    for gi, (ip, ix) in enumerate(graphs):
        n = len(ip) - 1
        for R, L, p, T in ((1, 1, 0.0, 1), (10, 2, 0.5, 3), (64, 3, 0.25, 5), (7, 5, 0.1, 50)):
            tq, seed, off = PS.term_q(p), 1000 + gi, 17 * gi + L
            roots = list(range(0, n, max(1, n // 6)))
            got = PS.neighbors(ip, ix, roots, R, L, tq, T, seed, off)
            assert not got.bad_index and got.nbr.shape == (len(roots), T + 1)
            for b, v in enumerate(roots):
                count = _literal_counts(ip, ix, v, R, L, tq, seed, off)
                assert count == PS.counts_of(ip, ix, v, R, L, tq, seed, off)[0] and v not in count
                order = sorted(count.items(), key=lambda uc: (-uc[1], uc[0]))[:T]
                c = 1 + len(order)
                assert got.cnt[b] == c and got.nbr[b, 0] == v and got.visits[b, 0] == 0
                assert got.nbr[b, 1:c].tolist() == [u for u, _ in order] and got.visits[b, 1:c].tolist() == [k for _, k in order]
                assert (got.nbr[b, c:] == v).all() and (got.visits[b, c:] == 0).all()
                assert sum(count.values()) <= R * L


def test_stop_rules_on_hand_cases():
    path2 = SO.csr([[1], [0]])
    never = PS.neighbors(*path2, [0, 1], 4, 5, 0, 3, seed=3)             # term_q = 0 never terminates: 0 -> 1 -> 0 -> 1 -> 0 -> 1
    assert never.cnt.tolist() == [2, 2] and never.nbr[:, 1].tolist() == [1, 0] and never.visits[:, 1].tolist() == [4 * 3, 4 * 3]
    always = PS.neighbors(*_HAND12, [0, 5, 11], 64, 3, FULL, 4, seed=3)    # a = 2^32 - 1 alone survives: no walk moves
    assert always.cnt.tolist() == [1, 1, 1] and (always.visits == 0).all() and (always.nbr == np.array([[0], [5], [11]])).all()
    dead = PS.neighbors(*SO.csr([[1], [2], []]), [0], 8, 6, 0, 4)        # 0 -> 1 -> 2, and row 2 is empty
    assert dead.cnt.tolist() == [3] and dead.nbr[0, :3].tolist() == [0, 1, 2] and dead.visits[0, :3].tolist() == [0, 8, 8]
    back = PS.neighbors(*path2, [0], 16, 2, 0, 4)                        # L = 2 on a two-node path: out and back, the return uncounted
    assert back.cnt.tolist() == [2] and back.nbr[0, :2].tolist() == [0, 1] and back.visits[0, :2].tolist() == [0, 16]
    iso = PS.neighbors(*SO.csr([[1], [0], []]), [2, 7, -1], 8, 2, 0, 2)  # an isolated root; two roots outside the graph
    assert iso.bad_index and iso.cnt.tolist() == [1, 0, 0] and iso.nbr.tolist() == [[2, 2, 2], [-1, -1, -1], [-1, -1, -1]]
    part = PS.neighbors(*path2, [0, 1], 2, 1, 0, 1, live=1)              # a root at or past *d_m: empty, without the bit
    assert not part.bad_index and part.cnt.tolist() == [2, 0] and part.nbr[1].tolist() == [-1, -1]


def test_mean_visit_counts_against_the_exact_expectation():
    """Over 500 consecutive offsets the mean visits per walk to every node lie within 6 L / (2 sqrt(500 R)) of the exact
    sum_{t = 1 .. L} (1 - p)^t [P^t]_{r, u}: a walk's visits to one node lie in [0, L], so its variance is at most L^2 / 4
    (Popoviciu), and the mean of 500 R walks has a standard deviation of at most L / (2 sqrt(500 R)); the bound is six of them."""
    ip, ix = _HAND12
    R, L, p, calls, seed = 64, 3, 0.25, 500, 20181
    bound = 6 * L / (2 * np.sqrt(calls * R))
    for r in (0, 8):                                                     # (8 sits beside the dead end 11 and the leaf 9)
        tot = np.zeros(12)
        for off in range(calls):
            for u, c in PS.counts_of(ip, ix, r, R, L, PS.term_q(p), seed, off)[0].items():
                tot[u] += c
        want = PS.expected_visits(ip, ix, r, R, L, p) / R
        err = np.abs(tot / (calls * R) - want)
        print(f"[pinsage] root {r}: max |mean - E| = {err.max():.4f}, bound {bound:.4f}")
        assert tot[r] == 0 and want[r] == 0 and want.sum() > 1.0 and (err <= bound).all()
    e = PS.expected_visits(*SO.csr([[1], [2], []]), 0, 1, 6, 0.5)        # the dead end absorbs: 0.5 at step 1, 0.25 at step 2, then nothing
    assert e.tolist() == [0.0, 0.5, 0.25]


def test_weights_sum_to_one_or_are_all_zero():
    from grapes_amd.modules.pinsage import visit_weights
    ip, ix = SO.random_graph(60, 5, 71)
    nb = PS.neighbors(ip, ix, list(range(60)), 50, 2, PS.term_q(0.5), 10, seed=5)
    nb.visits[7] = 0                                                     # a row without a visit
    w = PS.weights(nb.visits)
    assert w.dtype == np.float32 and np.array_equal(w, visit_weights(torch.as_tensor(nb.visits)).numpy())
    tot = w.astype(np.float64).sum(1)
    has = nb.visits.sum(1) > 0
    assert has.sum() >= 50 and not has[7] and (w[~has] == 0).all() and (np.abs(tot[has] - 1.0) <= 11 * PS.U).all()
    assert (w[:, 0] == 0).all() and (w[np.arange(11)[None, :] >= nb.cnt[:, None]] == 0).all()
    assert np.array_equal(w[has], (nb.visits[has].astype(np.float32).T / nb.visits[has].sum(1).astype(np.float32)).T)


def test_block_chain():
    ip, ix = SO.random_graph(200, 4, 73)
    R, L, T = 10, 3, 4
    blocks = PS.sample(ip, ix, [5, 190, 17], 3, R, L, PS.term_q(0.3), T, seed=9, off=100)
    assert len(blocks) == 3 and blocks[0].seeds.tolist() == [5, 190, 17]
    for d, b in enumerate(blocks):
        want = PS.neighbors(ip, ix, b.seeds, R, L, PS.term_q(0.3), T, 9, 100 + 2 * d)      # ceil(3 / 2) = 2 per block
        assert np.array_equal(b.nbr, want.nbr) and np.array_equal(b.visits, want.visits) and np.array_equal(b.cnt, want.cnt)
        live = np.arange(T + 1)[None, :] < b.cnt[:, None]
        assert np.array_equal(b.node_idx, np.unique(b.nbr[live])) and set(b.seeds.tolist()) <= set(b.node_idx.tolist())
        assert np.array_equal(b.node_idx[b.loc[:, 0]], b.seeds) and b.num_nodes == len(b.node_idx) <= len(b.seeds) * (T + 1)
        if d + 1 < len(blocks):
            assert np.array_equal(blocks[d + 1].seeds, b.node_idx)
    assert blocks[2].num_nodes > blocks[1].num_nodes > blocks[0].num_nodes > 3


# ---------------------------------------------------------------------------------------------------- gradients
def _rows(m, f, seed, eps):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((m, f))
    s[0] = -np.abs(s[0])                                                 # an all-negative row: nrm = 0
    if m > 2:
        s[1] = np.abs(s[1]) * 0.5 * eps / np.sqrt(f)                     # below eps
        s[2] = np.abs(s[2]) * 4.0 * eps + eps                            # above
    return s, rng.standard_normal((m, f))


@pytest.mark.parametrize("f", [1, 5, 64])
def test_relu_l2norm_closed_form_against_fp64_autograd(f):
    eps = 1e-3
    s, g = _rows(6, f, 40 + f, eps)
    st = torch.tensor(s, requires_grad=True)
    out = PS.torch_relu_l2norm(st, eps)
    out.backward(torch.tensor(g))
    o64, nrm = PS.relu_l2norm64(s, eps)
    ds, mag = PS.relu_l2norm_bwd64(g, s, eps)
    assert nrm[0] == 0 and (o64[0] == 0).all() and (f == 1 or nrm[1] < eps < nrm[2])
    assert np.abs(o64 - out.detach().numpy()).max() <= 1e-13 and (np.abs(ds - st.grad.numpy()) <= 1e-12 * np.maximum(mag, 1.0)).all()
    assert (np.abs(ds) <= mag * (1 + 1e-12)).all()


class _HostOps:
    """Host stand-ins for the kernels the modules call, in the tensors' own dtype: the closed forms of tests/pinsage_oracle.py and
    tests/pprgo_oracle.py."""

    @staticmethod
    def relu_l2norm_fwd(s, eps):
        out, nrm = PS.relu_l2norm64(s.numpy(), eps)
        return torch.as_tensor(out), torch.as_tensor(nrm)

    @staticmethod
    def relu_l2norm_bwd(g, out, nrm, s, eps):
        g, out, nrm, s = (t.numpy() for t in (g, out, nrm, s))
        d = np.maximum(nrm, eps)[:, None]
        return torch.as_tensor((s > 0) * (g - out * ((g * out).sum(1, keepdims=True) * (nrm >= eps)[:, None])) / d)

    @staticmethod
    def pprgo_aggregate_fwd(z, w, loc, cnt):
        return torch.as_tensor(GO.aggregate_fwd(z.numpy(), w.numpy(), loc.numpy(), cnt.numpy())[0])

    @staticmethod
    def pprgo_aggregate_bwd(g, w, tptr, tslot, n, e, item_cap=None):
        return torch.as_tensor(GO.aggregate_bwd(g.numpy(), w.numpy(), tptr.numpy(), tslot.numpy(), w.shape[1])[0])



class _HostGather(torch.autograd.Function):
    """target_batch._GatherX's contract on the host in the tensors' own dtype (that class allocates its gradient in fp32)."""

    @staticmethod
    def forward(ctx, X, ids, count, out, into_grad):
        ctx.save_for_backward(ids)
        ctx.shape = X.shape
        return X[ids.long()].clone()

    @staticmethod
    def backward(ctx, dx):
        g = torch.zeros(ctx.shape, dtype=dx.dtype)
        g[ctx.saved_tensors[0].long()] = dx
        return g, None, None, None, None


def test_conv_and_model_gradients_against_fp64_autograd(monkeypatch):
    from grapes_amd import ops
    from grapes_amd.modules import pinsage as MP
    for name in ("relu_l2norm_fwd", "relu_l2norm_bwd", "pprgo_aggregate_fwd", "pprgo_aggregate_bwd"):
        monkeypatch.setattr(ops, name, getattr(_HostOps, name))
    monkeypatch.setattr(MP, "_GatherX", _HostGather)
    ip, ix = SO.random_graph(60, 4, 75)
    roots = [3, 59, 20, 41]
    ob = PS.sample(ip, ix, roots, 2, 10, 2, PS.term_q(0.5), 3, seed=2)
    t = torch.as_tensor
    blocks = [SimpleNamespace(weight=t(b.weight.astype(np.float64)), loc=t(b.loc), self_loc=t(np.ascontiguousarray(b.loc[:, 0])),
                              cnt=t(b.cnt), tptr=t(b.tptr), tslot=t(b.tslot), num_nodes=b.num_nodes, item_cap=0) for b in ob]
    torch.manual_seed(5)
    model = MP.PinSAGE(6, [8, 7], 3).double()
    assert list(model.state_dict()) == ["convs.0.Q.weight", "convs.0.Q.bias", "convs.0.W.weight", "convs.0.W.bias", "convs.1.Q.weight",
                                        "convs.1.Q.bias", "convs.1.W.weight", "convs.1.W.bias", "lin.weight", "lin.bias"]
    assert list(MP.PinSAGEConv(6, 8, 5).state_dict()) == ["Q.weight", "Q.bias", "W.weight", "W.bias"]
    assert model.convs[0].W.weight.shape == (8, 14) and model.convs[1].Q.weight.shape == (7, 8) and model.out_channels == 3
    xb = torch.tensor(np.random.default_rng(6).standard_normal((ob[1].num_nodes, 6)), requires_grad=True)
    g = torch.tensor(np.random.default_rng(7).standard_normal((4, 3)))
    out = model(xb, SimpleNamespace(blocks=blocks))
    out.backward(g)
    last = model.convs[1](model.convs[0](xb, blocks[1]), blocks[0]).detach()
    assert ((last > 0).sum(1) >= 2).all()                                # (a row with one live column is a unit vector: no gradient passes)
    got = [xb.grad.clone()] + [p.grad.clone() for p in model.parameters()]
    xb.grad = None
    model.zero_grad()
    convs = [(c.Q.weight, c.Q.bias, c.W.weight, c.W.bias) for c in model.convs]
    want = PS.torch_model(xb, ob, convs, (model.lin.weight, model.lin.bias), MP.EPS)
    want.backward(g)
    assert out.shape == (4, 3) and torch.allclose(out, want, rtol=0, atol=1e-12)
    for a, p in zip(got, [xb] + list(model.parameters())):
        assert a.abs().max() > 0 and torch.allclose(a, p.grad, rtol=0, atol=1e-11)
    one = MP.PinSAGEConv(6, 8, 5).double()                               # one layer alone, on block 0 with the rows of its node_idx
    h = torch.tensor(np.random.default_rng(8).standard_normal((ob[0].num_nodes, 6)), requires_grad=True)
    a = one(h, blocks[0])
    b = PS.torch_conv(h, ob[0], one.Q.weight, one.Q.bias, one.W.weight, one.W.bias, MP.EPS)
    assert a.shape == (4, 5) and torch.allclose(a, b, rtol=0, atol=1e-13)
    assert torch.allclose(a.norm(dim=1)[a.abs().sum(1) > 0], torch.ones(1, dtype=torch.float64), atol=1e-12)
    with pytest.raises(ValueError, match="2 layers over a batch of 1 blocks"):
        model(xb, SimpleNamespace(blocks=blocks[:1]))
    with pytest.raises(ValueError, match="multiples of 4 up to 1024"):
        MP.PinSAGEConv(6, 258, 5)


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
    from grapes_amd.modules.pinsage import PinSAGE, PinSAGESampler
    from grapes_amd.pinsage import PinSAGETrainer
    for kw, msg in ((dict(num_random_walks=205, walk_length=5), "R L <= 1024"), (dict(num_random_walks=0), "R L <= 1024"),
                    (dict(walk_length=0), "R L <= 1024"), (dict(num_neighbors=1024), "T = 1024 neighbours are not built"),
                    (dict(num_neighbors=0), "T = 0 neighbours are not built"), (dict(termination_prob=1.0), "1.0 is outside [0, 1)"),
                    (dict(termination_prob=-0.5), "-0.5 is outside [0, 1)"), (dict(num_layers=0), "num_layers is at least 1")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            PinSAGESampler(None, **kw)
    with pytest.raises(ValueError, match="2\\^31 or more entries is not built"):
        PinSAGESampler(_fake_graph(2 ** 31))
    monkeypatch.setattr(ops, "csr_symmetric_check", lambda rowptr, col, n: 0)
    s = PinSAGESampler(_fake_graph())
    assert (s.K, s.term_q, s.seed, s.num_layers) == (11, 2 ** 31, 0, 2) and s.philox_offset.dtype == torch.int64
    with pytest.raises(ValueError, match="the roots are distinct"):
        s.sample(torch.tensor([0, 2, 0]))
    with pytest.raises(ValueError, match="at most 4096 roots per batch"):
        s.sample(torch.arange(4097))
    with pytest.raises(ValueError, match="a block of 4097 seeds is not built \\(at most 4096 = ops.PPRGO_MAX_ROOTS per block"):
        s.block(torch.zeros(4097, dtype=torch.int32))
    with pytest.raises(ValueError, match="no target"):
        s.sample(torch.tensor([], dtype=torch.int64))
    model = PinSAGE(8, [16, 16], 4)
    x = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="node features with a gradient are not built"):
        PinSAGETrainer(None, x.clone().requires_grad_(), None, model, None)
    with pytest.raises(TypeError, match="the model is a modules.pinsage.PinSAGE, not Linear"):
        PinSAGETrainer(None, x, None, torch.nn.Linear(8, 4), None)
    with pytest.raises(ValueError, match="batch_size is 1 .. 4096"):
        PinSAGETrainer(None, x, None, model, None, batch_size=5000)
    with pytest.raises(ValueError, match="2\\^31 or more entries is not built"):
        PinSAGETrainer(_fake_graph(2 ** 31), x, None, model, None)
    tr = PinSAGETrainer(_fake_graph(), x, None, model, None, num_neighbors=5, seed=77)
    assert tr.sampler.seed == 77 and tr.sampler.K == 6 == tr.eval_sampler.K and tr.eval_sampler.seed != 77 and tr.sampler.num_layers == 2
    assert tr.eval_sampler.graph is tr.sampler.graph and tr.eval_sampler.philox_offset is not tr.sampler.philox_offset
    with pytest.raises(ValueError, match="nothing to inject"):
        tr._sample(torch.tensor([0]), object())


_DEFAULT = {'dataset': 'cora', 'batch_size': 512, 'hidden_dim': 256, 'num_layers': 2, 'lr': 0.001, 'max_epoch': 100, 'eval_frequency': 1,
            'dropout': 0.0, 'runs': 1, 'seed': None, 'num_neighbors': 10, 'num_random_walks': 10, 'walk_length': 2,
            'termination_prob': 0.5}


def test_parsed_namespace():
    from grapes_amd import pinsage
    got = vars(pinsage.parse_args(["--dataset", "cora"]))
    assert got == _DEFAULT and all(type(got[k]) is type(_DEFAULT[k]) for k in _DEFAULT)
    line = "--dataset cora --num_neighbors 10 --num_random_walks 10 --walk_length 2 --termination_prob 0.5 --num_layers 2"
    assert line in pinsage.__doc__ and vars(pinsage.parse_args(line.split())) == _DEFAULT
    got = vars(pinsage.parse_args("--dataset cora --num_neighbors 50 --num_random_walks 200 --walk_length 5 --termination_prob 0".split()))
    assert got == dict(_DEFAULT, num_neighbors=50, num_random_walks=200, walk_length=5, termination_prob=0.0)
    for flag in ("--num_neighbors", "--num_random_walks", "--walk_length", "--termination_prob", "--batch_size", "--hidden_dim", "--seed"):
        assert flag in pinsage.__doc__
    assert "Not built" in pinsage.__doc__ and "returns to the root" in pinsage.__doc__


@pytest.mark.parametrize("argv,exc,message", [
    (["--walk_length", "x"], SystemExit, None),
    (["--num_random_walks", "205", "--walk_length", "5"], ValueError, "R L <= 1024"),
    (["--walk_length", "0"], ValueError, "R L <= 1024"),
    (["--num_neighbors", "1024"], ValueError, "T = 1024 neighbours are not built"),
    (["--termination_prob", "1.0"], ValueError, "outside [0, 1)"),
    (["--termination_prob", "-0.1"], ValueError, "outside [0, 1)"),
    (["--batch_size", "5000"], ValueError, "--batch_size is 1 .. 4096"),
    (["--num_layers", "0"], ValueError, "are at least 1"),
])
def test_command_line_refusals(argv, exc, message):
    from grapes_amd import pinsage
    with pytest.raises(exc) as e:
        pinsage.parse_args(["--dataset", "cora"] + argv)
    assert message is None or message in str(e.value)
