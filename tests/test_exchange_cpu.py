"""The exchange's two CPU statements against each other and against the truth, on every case of tests/exchange_oracle.CASES:
the independent reference (exchange_oracle, written from include/grapes_hip.h) and the double the gloo tests run
(dist_worker.OracleLocalOps) must agree slot for slot — headers, columns, status words, code_pos and both overflow contracts
included — and what comes out of serve -> hand transpose -> recv / assemble must be get_neighborhoods on the full graph and
X[ids] plus the indicator columns.  No GPU; exact comparisons only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exchange_oracle as XO  # noqa: E402


def _ids(cases):
    return [c.id for c in cases]


def test_case_table_names_every_path():
    ids = _ids(XO.CASES)
    assert len(set(ids)) == len(ids)
    for path in ("serve<vec>", "serve<scalar>", "assemble<vload,vstore>", "assemble<vload,scalar-store>", "assemble<scalar,scalar>"):
        assert any(path in i and "+4B" not in i for i in ids), path
    for which, path in (("X_local", "serve<scalar>"), ("reply", "serve<scalar>"), ("back", "assemble<scalar,scalar>"),
                        ("out", "assemble<vload,scalar-store>")):
        assert any(f"{which}+4B" in i and path in i for i in ids), which            # the four scalar fallbacks of F = 8
    # the pairs the table must hold, on the paths the dispatch conditions give them
    for F, k, path in ((4, 0, "vload,vstore"), (8, 4, "vload,vstore"), (100, 4, "vload,vstore"), (8, 3, "vload,scalar-store"),
                       (4, 1, "vload,scalar-store"), (1, 0, "scalar,scalar"), (7, 3, "scalar,scalar"), (5, 8, "scalar,scalar")):
        assert XO.assemble_path(F, k, None) == path
        assert any(f"-F{F}-ind{k}-" in i and f"assemble<{path}>" in i for i in ids), (F, k)
    assert {k for k in range(9)} <= {c.part.num_ind for c in XO.FEAT_CASES}
    assert {1, 2, 3, 8, 64} <= {c.part.P for c in XO.ROWS_CASES} and {1, 2, 3, 8, 64} <= {c.part.P for c in XO.FEAT_CASES}
    assert {1023, 1024, 1025, 2049} <= {c.part.P * c.part.cap for c in XO.ROWS_CASES}
    assert {1, 1024, 1025} <= {c.part.cap for c in XO.ROWS_CASES}


@pytest.mark.parametrize("case", XO.ROWS_CASES, ids=_ids(XO.ROWS_CASES))
def test_adjacency_rows_reference_and_double(case):
    from dist_worker import OracleLocalOps
    part, dbl = case.part, OracleLocalOps()
    ref, P, cap = part.ref, part.P, part.cap
    req = torch.from_numpy(part.req.reshape(-1))
    b32 = torch.tensor(part.bounds, dtype=torch.int32)
    for o in range(P):
        rp, cl, lo, hi = part.shard(o)
        reply = torch.full((P * part.stride,), XO.FILL, dtype=torch.int32)
        st = torch.zeros(1, dtype=torch.int32)
        dbl.serve_rows(torch.from_numpy(rp), torch.from_numpy(cl), req, P, cap, lo, hi, reply, part.stride, part.e_slot, st)
        assert np.array_equal(reply.numpy().reshape(P, -1), ref["replies"][o]), f"owner {o}"
        assert int(st) == ref["serve_status"][o]
    overflow = False
    for r in range(P):
        nodes, m = part.req[r, :cap], part.counts[r]
        src, dst, d_e, eoff, status = ref["recv"][r]
        st = torch.zeros(1, dtype=torch.int32)
        got = dbl.recv_rows(torch.from_numpy(ref["backs"][r].reshape(-1)), part.stride, torch.from_numpy(nodes), b32, P, part.e_cap,
                            torch.tensor([int(part.req[r, cap])], dtype=torch.int32), st)
        true = XO.true_edges(part.indptr, part.indices, nodes, m)
        e = true.shape[1]
        k = min(e, part.e_cap)
        assert d_e == e == int(got[2]) and int(eoff[m]) == e == int(got[3][m])
        assert status == (XO.EDGE_OVERFLOW if e > part.e_cap else 0) == int(st)
        assert np.array_equal(eoff[:m + 1], got[3][:m + 1].numpy())
        assert np.array_equal(np.diff(eoff[:m + 1]), np.diff(part.indptr)[nodes[:m]])
        for mine, theirs, truth in ((src, got[0], true[0]), (dst, got[1], true[1])):
            assert np.array_equal(mine[:k], truth[:k]) and np.array_equal(theirs[:k].numpy(), truth[:k])
            assert (mine[k:] == XO.FILL).all()
        overflow |= e > part.e_cap
    assert overflow == ("overflow" in case.id) == any(ref["serve_status"])          # at a requester and at an owner
    if "fits_exactly" in case.id:
        assert max(rec[2] for rec in ref["recv"]) == part.e_cap


@pytest.mark.parametrize("case", XO.FEAT_CASES, ids=_ids(XO.FEAT_CASES))
def test_halo_rows_reference_and_double(case):
    from dist_worker import OracleLocalOps
    part, dbl = case.part, OracleLocalOps()
    ref, P, F, capf, n_slot, k = part.ref, part.P, part.F, part.capf, part.n_slot, part.num_ind
    req = torch.from_numpy(part.req.reshape(-1))
    b32 = torch.tensor(part.bounds, dtype=torch.int32)
    code = torch.from_numpy(part.code)
    for o in range(P):
        lo, hi = part.bounds[o], part.bounds[o + 1]
        reply = torch.full((P * n_slot * F,), float("nan"))
        st = torch.zeros(1, dtype=torch.int32)
        dbl.serve_features(torch.from_numpy(part.X[lo:hi]), req, P, capf, lo, hi, reply, n_slot, st)
        assert np.array_equal(XO.bits(reply.numpy().reshape(P, n_slot, F)), XO.bits(ref["replies"][o])), f"owner {o}"
        assert int(st) == ref["serve_status"][o]
    assert any(ref["serve_status"]) == ("overflow" in case.id)
    runs = [np.diff(np.searchsorted(part.req[r, :part.counts[r]], part.bounds)).max() for r in range(P)]
    assert max(runs) == n_slot + (1 if "one_short" in case.id else 0) or "legacy" in case.id
    d_ep = None if part.d_epoch is None else torch.tensor([part.d_epoch], dtype=torch.int64)
    for r in range(P):
        ids, n = part.req[r, :capf], part.counts[r]
        d_n = torch.tensor([int(part.req[r, capf])], dtype=torch.int32)
        back = torch.from_numpy(ref["backs"][r].reshape(-1))
        got = dbl.assemble_features(back, F, n_slot, torch.from_numpy(ids), b32, P, d_n, code if k else None, part.epoch, d_ep, k)
        out = ref["outs"][r]
        assert np.array_equal(XO.bits(got[:n].numpy()), XO.bits(out[:n]))
        assert np.isnan(out[n:]).all()                                               # rows past the count are not written
        assert np.array_equal(XO.bits(out[:n]), XO.bits(XO.true_rows_clamped(part, r)))
        ex = part.exact_rows(r)
        assert np.array_equal(XO.bits(out[:n][ex]), XO.bits(XO.true_rows(part.X, ids, n, part.code, part.epoch_live, k)[ex]))
        assert ex.all() or "overflow" in case.id
        # positions, with code_pos
        pos, cpos, shared = ref["positions"][r]
        gp, gc = torch.full((capf,), XO.FILL, dtype=torch.int32), torch.full((P * n_slot,), XO.FILL, dtype=torch.int32)
        dbl.halo_positions(torch.from_numpy(ids), b32, P, n_slot, d_n, code, gp, gc)
        keep = np.ones(P * n_slot, bool)
        keep[sorted(shared)] = False
        assert np.array_equal(gp.numpy(), pos) and np.array_equal(gc.numpy()[keep], cpos[keep])
        assert (pos[n:] == 0).all() and bool(shared) == (not ex.all())
        own = ex & ~np.isin(pos[:n], sorted(shared))                                  # (a position clamped rows share: unspecified)
        assert np.array_equal(cpos[pos[:n][own]], part.code[ids[:n][own]])           # every live position holds its id's word
        untouched = np.setdiff1d(np.arange(P * n_slot), pos[:n])
        assert (cpos[untouched] == XO.FILL).all()
        if n:   # the in-place view of the truth: back[pos[i]] is the row of ids[i]
            assert np.array_equal(XO.bits(ref["backs"][r].reshape(-1, F)[pos[:n]]), XO.bits(out[:n, :F]))
    with pytest.raises(ValueError):
        dbl.halo_positions(torch.from_numpy(part.req[0, :capf]), b32, P, n_slot, None, code, gp, None)
    # the n == 0 early return leaves pos alone
    gp.fill_(XO.FILL)
    dbl.halo_positions(torch.zeros(0, dtype=torch.int32), b32, P, n_slot, None, None, gp, None)
    assert bool((gp == XO.FILL).all())


NOTE_CASES = XO.NOTE_CASES


@pytest.mark.parametrize("case", NOTE_CASES, ids=_ids(NOTE_CASES))
def test_noted_rows_reference_and_double(case):
    from dist_worker import OracleLocalOps
    part, dbl = case.part, OracleLocalOps()
    s = XO.note_scenario(part)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    loc = t(s["loc0"].copy())
    dbl.note_rows(loc, t(s["ids_a"]), torch.tensor([s["count_a"]], dtype=torch.int32), t(s["pos"]), s["base"], t(s["node_map"]),
                  t(s["batch"]), torch.tensor([s["n_batch"]], dtype=torch.int32), None, None)
    assert np.array_equal(loc.numpy(), s["loc_a"])
    dbl.note_rows(loc, t(s["ids_b"]), torch.tensor([s["count_b"]], dtype=torch.int32), t(s["pos"]), s["base"], None, None, None,
                  t(s["idx_a"]), t(s["idx_b"]))
    assert np.array_equal(loc.numpy(), s["loc_b"])
    got = dbl.gather_noted(t(s["kept"]), loc, t(s["want"].astype(np.int32)), None)
    assert np.array_equal(XO.bits(got.numpy()), XO.bits(part.X[s["want"]]))
