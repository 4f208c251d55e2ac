"""The pair launches of the head-record gather-SpMM, driven directly through the rider calls (the way ops.gcn_aggregate_bwd
drives them): a recorded gather riding in another gather (gcn_aggregate_gather_head5_pair_k) or in a small graph's aggregation
(gcn_aggregate_gather_pair_k), over the local matrix and through a shard table, at 32 and 64 lanes per row.  A pair launch
runs the same body on the same arguments as the launch on its own, so every output is compared with torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS, N_X, NUM_IND, EPOCH = 300, 2000, 3, 9
WIDTHS = {32: 102, 64: 132}          # lanes per row: F  (102 sits in a 104-wide padded matrix: X-tail, indicator and padding lanes)
CUTS = [0, 700, 700, N_X]            # three uneven row shards, one of them empty


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _edges(rng, n, lens):
    """(src, dst) with lens[r] distinct sources other than r in by-target row r"""
    src = np.concatenate([(r + 1 + rng.permutation(n - 1)[:k]) % n for r, k in enumerate(lens)])
    dst = np.repeat(np.arange(n), lens)
    order = np.lexsort((dst, src))
    return _t(src[order], torch.int32), _t(dst[order], torch.int32)


class _Problem:
    """one local graph of N_ROWS rows built with head_ids: rows of 0, 1-4 and 5-16 entries and one hub row of 40 (GRAPES_HUB_ROW = 16)"""

    def __init__(self, seed, must=()):
        """must: feature-matrix rows that are to be among the head ids (they take the first local rows)"""
        from grapes_amd import ops
        rng = np.random.default_rng(seed)
        lens = rng.choice([0, 1, 2, 3, 4, 5, 9, 16], N_ROWS, p=[.1, .25, .2, .15, .1, .08, .07, .05])
        lens[:4] = [0, 4, 5, 16]
        lens[int(rng.integers(4, N_ROWS))] = 40
        ids = rng.permutation(N_X)
        self.ids = _t(np.concatenate([np.asarray(must, dtype=ids.dtype), ids[~np.isin(ids, must)]])[:N_ROWS], torch.int32)
        self.code = _t(((EPOCH << 8) | rng.integers(0, 1 << NUM_IND, N_X)).astype(np.int32))
        self.prep = ops.PreparedGraph(*_edges(rng, N_ROWS, lens), N_ROWS, head_ids=self.ids)
        got = (self.prep.rowptr_t[1:] - self.prep.rowptr_t[:-1]).cpu().numpy()
        assert self.prep.row_head is not None and np.array_equal(got, lens) and got.max() == 40

    def gather(self, X, F, out):
        from grapes_amd import ops
        return ops.gcn_aggregate_gather(X, self.ids, self.prep, self.code, EPOCH, NUM_IND, out=out, F=F)


class _Case:
    """What the cases share, computed once: per width the matrix, its shard table and the two problems' outputs on their own;
    the small aggregation that hosts a gather (f = 64, no head records: neither the item-scheduled nor the record form)."""

    def __init__(self):
        from grapes_amd import ops
        from grapes_amd.peer import PeerFeatures
        rng = np.random.default_rng(5)
        self.A, self.B = _Problem(11), _Problem(12)
        self.X, self.pf, self.solo = {}, {}, {}
        for lanes, F in WIDTHS.items():
            X = _t(rng.standard_normal((N_X, F)).astype(np.float32))
            self.X[lanes] = ops.pad_features(X)[0]
            self.pf[lanes] = PeerFeatures.from_shards([X[a:z].clone() for a, z in zip(CUTS, CUTS[1:])])
            self.solo[lanes] = tuple(p.gather(self.X[lanes], F, None) for p in (self.A, self.B))
            for p, ref in zip((self.A, self.B), self.solo[lanes]):       # the table path alone equals the local one
                assert torch.equal(p.gather(self.pf[lanes], F, None), ref)
        n = 200
        self.h = _t(rng.standard_normal((n, 64)).astype(np.float32))
        self.bias = _t(rng.standard_normal(64).astype(np.float32))
        self.gprep = ops.PreparedGraph(*_edges(rng, n, rng.integers(0, 7, n)), n)
        self.agg_solo = ops.gcn_aggregate_fwd(self.h, self.gprep, self.bias, True)
        torch.cuda.synchronize()

    def out(self, lanes):
        return torch.full_like(self.solo[lanes][0], float("nan"))

    def features(self, lanes, table):
        return self.pf[lanes] if table else self.X[lanes]


@pytest.fixture(scope="module")
def case():
    _cuda()
    return _Case()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(launch):
    """the launches `launch` issues, recorded as a rider program -> its handle"""
    from grapes_amd import _lib
    L = _lib.load()
    _lib.check(L.grapes_rider_record_begin(), "rider_record_begin")
    try:
        launch()
    finally:
        prog = int(L.grapes_rider_record_end())
    assert L.grapes_rider_count(prog) == 1
    return prog


def _ride(prog, host):
    """`host` issued with the program attached -> (records a host carried, records detach issued on their own)"""
    from grapes_amd import _lib
    L = _lib.load()
    paired = C.c_int32(-1)
    _lib.check(L.grapes_rider_attach(prog, 0, _stream()), "rider_attach")
    try:
        host()
    finally:
        alone = L.grapes_rider_detach(_stream(), C.byref(paired))
        L.grapes_rider_free(prog)
    return paired.value, alone


@pytest.mark.parametrize("table", [False, True], ids=["local", "shards"])
@pytest.mark.parametrize("lanes", [32, 64])
def test_gather_rides_in_gather(case, lanes, table):
    F, X = WIDTHS[lanes], case.features(lanes, table)
    out_a, out_b = case.out(lanes), case.out(lanes)
    prog = _record(lambda: case.B.gather(X, F, out_b))
    assert _ride(prog, lambda: case.A.gather(X, F, out_a)) == (1, 0)
    assert torch.equal(out_a, case.solo[lanes][0]) and torch.equal(out_b, case.solo[lanes][1])


@pytest.mark.parametrize("table", [False, True], ids=["local", "shards"])
@pytest.mark.parametrize("lanes", [32, 64])
def test_gather_rides_in_aggregation(case, lanes, table):
    """the host knows the rider's form from the record's variant alone"""
    from grapes_amd import ops
    F, X = WIDTHS[lanes], case.features(lanes, table)
    out_b, out_h = case.out(lanes), torch.full_like(case.agg_solo, float("nan"))
    prog = _record(lambda: case.B.gather(X, F, out_b))
    assert _ride(prog, lambda: ops.gcn_aggregate_fwd(case.h, case.gprep, case.bias, True, out=out_h)) == (1, 0)
    assert torch.equal(out_h, case.agg_solo) and torch.equal(out_b, case.solo[lanes][1])


def test_other_variant_does_not_ride(case):
    """a recorded 64-lane gather and a 32-lane host: the host runs alone, detach issues the record"""
    out_a, out_b = case.out(32), case.out(64)
    prog = _record(lambda: case.B.gather(case.X[64], WIDTHS[64], out_b))
    assert _ride(prog, lambda: case.A.gather(case.X[32], WIDTHS[32], out_a)) == (0, 1)
    assert torch.equal(out_a, case.solo[32][0]) and torch.equal(out_b, case.solo[64][1])


@pytest.mark.parametrize("table", [False, True], ids=["local", "shards"])
def test_program_on_its_own(case, table):
    from grapes_amd import _lib
    L = _lib.load()
    out_b = case.out(32)
    prog = _record(lambda: case.B.gather(case.features(32, table), WIDTHS[32], out_b))
    try:
        _lib.check(L.grapes_rider_launch(prog, _stream()), "rider_launch")
    finally:
        L.grapes_rider_free(prog)
    assert torch.equal(out_b, case.solo[32][1])


@pytest.mark.parametrize("lanes", [32, 64])
def test_eight_shards_with_empty_ends(lanes):
    """GRAPES_MAX_PEER_SHARDS shards, the first and the last of them empty, head ids on the first and the last row of every
    shard that has rows: the table path picks each row's shard by its bounds and equals the local gather bit for bit"""
    _cuda()
    from grapes_amd import ops
    from grapes_amd.peer import MAX_SHARDS, PeerFeatures
    cuts = [0, 0, 1, 400, 401, 1100, 1500, N_X, N_X]           # (shards of one row among them)
    assert len(cuts) == MAX_SHARDS + 1
    edge_rows = sorted({r for a, z in zip(cuts, cuts[1:]) if a < z for r in (a, z - 1)})
    prob = _Problem(13, must=edge_rows)
    assert set(edge_rows) <= set(prob.ids.cpu().tolist())
    F = WIDTHS[lanes]
    X = _t(np.random.default_rng(6).standard_normal((N_X, F)).astype(np.float32))
    pf = PeerFeatures.from_shards([X[a:z].clone() for a, z in zip(cuts, cuts[1:])], rank=1)
    assert pf.P == MAX_SHARDS and pf.bounds == cuts
    want = prob.gather(ops.pad_features(X)[0], F, None)
    got = torch.full_like(want, float("nan"))
    prob.gather(pf, F, got)
    assert torch.equal(got, want)
