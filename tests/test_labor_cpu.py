"""LABOR without a GPU: the C surface, the host oracle (tests/labor_oracle.py) against the definitions it restates — the constraint
equation of c_s, the fixed point against the sorted solve, unbiasedness by exhaustive enumeration over shared variates — and the
driver's arguments and refusals."""
import ctypes
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import labor_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("grapes_labor_sample_layer", "grapes_labor_sample_layer_workspace_bytes", "grapes_labor_importance",
                "grapes_labor_importance_workspace_bytes")


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


def test_workspaces_and_argument_checks_are_host_calls(built_lib):
    """Sizes grow with their arguments; argument checks run before any launch and need no device."""
    from grapes_amd import ops
    lib = built_lib.load()
    assert lib.grapes_labor_sample_layer_workspace_bytes(4, 8) < lib.grapes_labor_sample_layer_workspace_bytes(400, 8) \
        < lib.grapes_labor_sample_layer_workspace_bytes(400, 800)
    assert lib.grapes_labor_sample_layer_workspace_bytes(400, 800) >= 800 * 16 + 401 * 4
    assert lib.grapes_labor_importance_workspace_bytes(1000) >= 4000
    one = ctypes.c_void_p(16)                                            # a non-NULL aligned address that is never read

    def sample(fanout=3, c=None, pi=None, item_cap=8, e_cap=16, ws=one):
        return lib.grapes_labor_sample_layer(one, one, 10, one, 4, None, fanout, None, 0, 0, c, pi, item_cap, e_cap, one, one, None,
                                             None, one, ws, None, None)
    assert sample(fanout=0) == -1 and sample(fanout=-1) == -1
    assert sample(c=one) == -1 and sample(pi=one) == -1                  # c and pi: both or neither
    assert sample(item_cap=0) == -1 and sample(e_cap=0) == -1 and sample(item_cap=(1 << 24) + 1) == -1
    assert sample(ws=ctypes.c_void_p(20)) == -2                          # 8-byte alignment
    for iters in (-1, 9):
        assert lib.grapes_labor_importance(one, one, 10, one, 4, None, 3, iters, one, one, one, None, None) == -1
    assert lib.grapes_labor_importance(one, one, 10, one, 4, None, 0, 1, one, one, one, None, None) == -1
    assert ops.LABOR_MAX_ITERS == 8 and ops.LABOR_CHUNK == 64
    assert ops.labor_item_cap(3, 0) == 1 and ops.labor_item_cap(3, 5) == 3 and ops.labor_item_cap(2, 1000) == 17


# ---------------------------------------------------------------------------------------------------- Philox and the integer rule
def test_the_oracles_philox_is_the_streams_of_the_other_oracles():
    from tests.saint_samplers_oracle import philox_words
    for seed, base, n in ((0, 0, 9), (12345678901234, 17, 40), (2 ** 63 + 5, 2 ** 33 + 1, 13)):
        assert np.array_equal(LO.node_words(seed, base, n), philox_words(seed, base, n).astype(np.uint32))


def _accepted_words(d, k):
    """How many of the 2^32 words LABOR-0 accepts for a row of d > k entries: the rule is monotone in the word, so the count is the
    first refused word, found by bisection over the oracle's own predicate."""
    lo, hi = 0, 2 ** 32                                                  # keep(lo - 1) holds (or lo = 0), keep(hi) fails (or hi = 2^32)
    while lo < hi:
        mid = (lo + hi) // 2
        if LO.keep_int(np.array([mid] + [0] * (d - 1), dtype=np.uint64), k)[0]:
            lo = mid + 1
        else:
            hi = mid
    return lo


def test_labor0_expected_kept_count_over_the_32_bit_threshold():
    """E[kept_s] = d T / 2^32 with T the accepted words.  T = ceil(k 2^32 / d): the expectation is min(d, k) EXACTLY whenever d divides
    k 2^32 and exceeds k by less than d 2^-32 otherwise (the threshold is an integer)."""
    for d, k in itertools.product((1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1000, 17375), (1, 3, 64)):
        if d <= k:
            assert LO.keep_int(np.full(d, 2 ** 32 - 1, dtype=np.uint64), k).all()        # kept whatever the word: d of d
            continue
        T = _accepted_words(d, k)
        assert T == -((-k << 32) // d)
        expected = Fraction(d * T, 2 ** 32)
        if (k << 32) % d == 0:
            assert expected == min(d, k)
        else:
            assert 0 < expected - k < Fraction(d, 2 ** 32)


# a 6-node graph whose rows with more than k entries hold 2 or 4: k 2^32 / d is an integer, and so is p G on the grid below
_G6_ROWS = [[1, 2, 3, 4], [0, 2], [0, 1, 3, 5], [0, 2, 2, 3], [5], []]           # a duplicate entry and a stored loop in row 3
_GRID = 4


def test_horvitz_thompson_is_unbiased_under_shared_variates_by_enumeration():
    """Every joint value of the six SHARED variates on a grid of _GRID points each (4^6 combinations): the mean over all of them of
    sum_kept x_t / (d_s p_st) is the row's plain mean, to 1e-12 — for LABOR-0's p = k / d through the 32-bit rule, and for a table of
    unequal p_st (multiples of 1 / _GRID) through the fp32 keep rule; the expected kept count of LABOR-0 is min(d, k) exactly."""
    rng = np.random.default_rng(0)
    x = rng.normal(size=6)
    combos = np.array(list(itertools.product(range(_GRID), repeat=6)), dtype=np.uint64)          # [4^6, 6]: u_t = j / _GRID
    words = (combos << np.uint64(32)) // np.uint64(_GRID)                                        # the 32-bit word of u_t
    assert len(combos) == _GRID ** 6
    for k in (1, 2):
        for s, nb in enumerate(_G6_ROWS):
            d = len(nb)
            if d == 0:
                continue
            kept = np.stack([LO.keep_int(w[nb], k) for w in words])                              # [combos, d]
            p = min(1.0, k / d)
            est = (kept * x[nb] / (d * p)).sum(1)
            assert abs(est.mean() - x[nb].mean()) < 1e-12
            assert Fraction(int(kept.sum()), len(combos)) == min(d, k)
    # unequal probabilities per (row, entry): c_s pi_t with c, pi chosen so that every product is a multiple of 1 / _GRID
    pi = np.array([1.0, 0.5, 2.0, 1.0, 0.5, 1.0], dtype=np.float32)
    for s, nb in enumerate(_G6_ROWS):
        d = len(nb)
        if d < 2:
            continue
        c = np.float32(0.5)
        kept_p = [LO.keep_f32(w[nb].astype(np.uint32), 1, c, pi[nb]) for w in words]
        kept, p = np.stack([q[0] for q in kept_p]), kept_p[0][1].astype(np.float64)
        assert ((p * _GRID) % 1 == 0).all() and len(set(p)) > 1
        est = (kept * x[nb] / (d * p)).sum(1)
        assert abs(est.mean() - x[nb].mean()) < 1e-12
    # rows that share a vertex decide alike at equal thresholds: rows 0 and 2 (d = 4) on vertex 3, for every combination
    k0 = np.stack([LO.keep_int(w[_G6_ROWS[0]], 1) for w in words])[:, _G6_ROWS[0].index(3)]
    k2 = np.stack([LO.keep_int(w[_G6_ROWS[2]], 1) for w in words])[:, _G6_ROWS[2].index(3)]
    assert np.array_equal(k0, k2) and 0 < k0.sum() < len(k0)


# ---------------------------------------------------------------------------------------------------- c_s
def _random_rows(rng):
    for trial in range(300):
        k = int(rng.integers(1, 20))
        d = k + 1 if trial % 5 == 0 else int(rng.integers(k + 1, 90))
        pi = rng.uniform(0.05, 2.0, d)
        if trial % 3 == 0:                                               # saturated entries: a few pi far above the rest
            pi[: max(1, d // 4)] *= rng.uniform(20.0, 200.0)
        yield pi, k


def test_sorted_solve_satisfies_the_constraint_and_the_fixed_point_agrees():
    """sum_t 1 / min(1, c pi_t) = d^2 / k to 1e-12 of its right-hand side, rows with saturated entries and rows with d = k + 1 included;
    the kernel's fixed point, in fp64 Python, finds the same c to 1e-12 and never takes more than d rounds."""
    rng = np.random.default_rng(1)
    saturated = 0
    for pi, k in _random_rows(rng):
        d = len(pi)
        c = LO.solve_c_sorted(pi, k)
        assert abs(LO.constraint(c, pi, k)) <= 1e-12 * d * d / k
        saturated += int((c * pi >= 1.0).any())
        c_fp, rounds = LO.solve_c_fixed_point(pi, k)
        assert abs(c_fp - c) <= 1e-12 * c and rounds <= d
    assert saturated >= 50                                               # (the saturated branch was taken)


def test_uniform_pi_gives_k_over_d():
    for d, k in ((2, 1), (11, 10), (65, 64), (500, 3), (17375, 25)):
        assert abs(LO.solve_c_sorted(np.ones(d), k) - k / d) <= 1e-15
        assert abs(LO.solve_c_fixed_point(np.ones(d), k)[0] - k / d) <= 1e-15
    # zero iterations: c = k / d on the long rows, 0 on the others, pi = 1
    indptr, indices = np.array([0, 3, 4, 4]), np.array([1, 2, 0, 0])
    c, pi = LO.importance(indptr, indices, [0, 1, 2], 2, 0, 3)
    assert np.allclose(c, [2 / 3, 0, 0]) and np.array_equal(pi, np.ones(3))


def test_importance_iterations_keep_the_variance_constraint_and_hajek_weights_sum_to_one():
    rng = np.random.default_rng(2)
    n = 40
    deg = rng.integers(0, 12, n)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = rng.integers(0, n, indptr[-1])
    rows = rng.permutation(n)[:25]
    for iters in (1, 3):
        c, pi = LO.importance(indptr, indices, rows, 3, iters, n)
        for cs, s in zip(c, rows):
            nb = indices[indptr[s]:indptr[s + 1]]
            if len(nb) > 3:
                assert abs(LO.constraint(cs, pi[nb], 3)) <= 1e-12 * len(nb) ** 2 / 3
            else:
                assert cs == 0
        words = LO.node_words(3, 0, n)
        src, dst, pos, p, w = LO.sample_layer(indptr, indices, rows, 3, words, c.astype(np.float32), pi.astype(np.float32))
        for s in set(dst):
            assert abs(w[dst == s].sum() - 1.0) < 1e-12
        assert np.array_equal(indices[pos], src)


# ---------------------------------------------------------------------------------------------------- the driver
_DEFAULTS = {'dataset': 'cora', 'batch_size': 512, 'hidden_dim': 256, 'num_layers': 2, 'lr': 0.001, 'max_epoch': 100,
             'eval_frequency': 1, 'dropout': 0.0, 'runs': 1, 'seed': None, 'fanouts': [10, 10], 'importance_iters': 0,
             'layer_dependency': False}
_SET_ARGV = ["--dataset", "arxiv", "--batch_size", "128", "--hidden_dim", "64", "--num_layers", "3", "--lr", "0.01", "--max_epoch", "5",
             "--eval_frequency", "2", "--dropout", "0.1", "--runs", "2", "--seed", "7", "--fanouts", "5,-1,3", "--importance_iters", "2",
             "--layer_dependency"]
_SET = {'dataset': 'arxiv', 'batch_size': 128, 'hidden_dim': 64, 'num_layers': 3, 'lr': 0.01, 'max_epoch': 5, 'eval_frequency': 2,
        'dropout': 0.1, 'runs': 2, 'seed': 7, 'fanouts': [5, -1, 3], 'importance_iters': 2, 'layer_dependency': True}


@pytest.mark.parametrize("argv,want", [(["--dataset", "cora"], _DEFAULTS), (_SET_ARGV, _SET)], ids=["defaults", "set"])
def test_parsed_namespace(argv, want):
    from grapes_amd import labor
    got = vars(labor.parse_args(argv))
    assert got == want
    assert all(type(got[k]) is type(want[k]) for k in want)


@pytest.mark.parametrize("argv,exc,message", [
    ([], SystemExit, "--dataset is required"),
    (["--dataset", "cora", "--fanouts", "65"], ValueError, "NeighborSampler: fanout 65 is not built (-1 for every neighbour, or 1 .. 64)"),
    (["--dataset", "cora", "--importance_iters", "9"], ValueError, "--importance_iters is 0 .. 8, not 9"),
    (["--dataset", "cora", "--importance_iters", "-1"], ValueError, "--importance_iters is 0 .. 8, not -1"),
    (["--dataset", "cora", "--fanouts", "10,10", "--num_layers", "3"], ValueError,
     "--fanouts holds one entry per layer: 2 given for --num_layers 3"),
    (["--dataset", "cora", "--batch_size", "5000"], ValueError,
     "--eval_frequency and --hidden_dim are at least 1, --batch_size is 1 .. 4096"),
])
def test_refusals(argv, exc, message):
    from grapes_amd import labor
    with pytest.raises(exc) as e:
        labor.parse_args(argv)
    assert str(e.value) == message


def test_there_is_no_aggr_flag_and_the_existing_drivers_are_as_they_were():
    from grapes_amd import graphsage, labor, ops
    with pytest.raises(SystemExit):
        labor.parse_args(["--dataset", "cora", "--aggr", "mean"])
    with pytest.raises(SystemExit):
        graphsage.parse_args(["--dataset", "cora", "--importance_iters", "1"])
    assert ops.SAGE_AGGRS == ("mean", "sum")


def test_host_tensors_are_refused(built_lib):
    from grapes_amd import ops
    from grapes_amd.labor import weighted_sage
    from grapes_amd.modules.gcn import SAGE
    rowptr, col = torch.tensor([0, 2, 3, 3]), torch.tensor([1, 2, 0], dtype=torch.int32)
    rows = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(built_lib.GrapesHipError):
        ops.labor_sample_layer(rowptr, col, 3, rows, 1, deg_sum=3)
    with pytest.raises(built_lib.GrapesHipError):
        ops.labor_importance(rowptr, col, 3, rows, 1, 2, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(built_lib.GrapesHipError):
        weighted_sage(SAGE(4, [8, 2]), torch.zeros(3, 4), [None, None], [None, None])


def test_sampler_and_trainer_refuse_what_is_not_built():
    """The argument checks come before the graph is touched."""
    from grapes_amd.modules.labor import LaborSampler
    with pytest.raises(ValueError, match="fanout 65 is not built"):
        LaborSampler(None, [65])
    with pytest.raises(ValueError, match="fanout 0 is not built"):
        LaborSampler(None, [10, 0])
    with pytest.raises(ValueError, match="importance_iters 9 is not built"):
        LaborSampler(None, [10], importance_iters=9)
    with pytest.raises(ValueError, match="importance_iters -1 is not built"):
        LaborSampler(None, [10], importance_iters=-1)
