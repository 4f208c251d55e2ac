#!/usr/bin/env python3
"""ShaDow-GNN's PPR scopes: ops.shadow_ppr_sample's three launches, the k-hop sampler beside them for scale, one eager training step
under each scope, and the k-hop sampler before and after its second half was factored out for both build kernels.

      python profiles/bench_shadow_ppr.py [--reps 21] [--inner 200] [--out profiles/shadow_ppr_bench.json]
      python profiles/bench_shadow_ppr.py --parent_lib <libgrapes_hip.so of the parent commit> [--out ...]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_shadow_ppr.py --trace_calls 200

The products-shaped synthetic graph, batch 512, everything in one process; the root sets are profiles/bench_shadow.py's: 512 training
nodes farther than two hops from the hub (the node of the most entries), and the same set with its first 64 roots replaced by the hub
and 63 nodes that store it.

Sampler.  ops.shadow_ppr_sample at alpha = 0.25 for k in {32, 200} and eps in {2^-12, 2^-14}, max_rounds 32, into preallocated
buffers, on both root sets, and ops.shadow_sample(depth 2, num_neighbors 10) in the same process — a neighbour for scale, not an equal:
it draws 10 entries of a row where the push walks all of them.  A repetition is `inner` calls between two device events, the variants
alternating in every repetition; the figure kept is the median over `reps` repetitions after a warm-up, with the quartiles beside it;
host launches are included.  Per case: the nodes and entries of the batch, and over the roots the rounds run, the stop codes, and the
touched nodes (recomputed on the host for a sample of the roots by the rule's own rounds, since the call does not return them).

Step.  ShadowTrainer.step under scope="ppr" (k = 200) beside scope="khop" (depth 2, num_neighbors 10): three SAGE layers of 256
columns, pooled readout, host wall time to a device synchronise, median of `reps` calls after 3.

--parent_lib times grapes_shadow_sample (depth 2, num_neighbors 10, both root sets) through the given library and through this tree's,
alternating in every repetition, the parent's library entered twice so that the spread of its own repeated runs stands beside the
difference.  --trace_calls N runs N calls of the k = 200, eps = 2^-14 case on the hub set and nothing else, for a kernel trace in a
run of its own.

Not measured: a captured step (none exists), other graphs, other alpha."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_shadow import BATCH, E_CAP, WIDTH, _alternate, _wall, root_sets, sampler_call  # noqa: E402

ALPHA, MAX_ROUNDS = 0.25, 32
KS, EPS = (32, 200), (2 ** -12, 2 ** -14)
TOUCHED_SAMPLE = 8                   # roots whose touched sets are recounted on the host


def ppr_call(ops, g, roots, k, eps):
    aq, thr = int(round(ALPHA * 2 ** 16)), max(1, int(round(eps * 2 ** 30)))
    out = ops.shadow_ppr_sample(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, MAX_ROUNDS, e_cap=E_CAP)
    n, e = int(out[6].item()), int(out[7].item())
    sizes = out[1][1:] - out[1][:-1]
    rounds, stop = out[9].cpu(), out[10].cpu()
    info = {"nodes": n, "entries": e, "largest_ego_net": int(sizes.max().item()), "smallest_ego_net": int(sizes.min().item()),
            "rounds_min_median_max": [int(rounds.min()), int(rounds.median()), int(rounds.max())],
            "stop_codes": {str(c): int((stop == c).sum()) for c in (0, 1, 2)}}
    return (lambda: ops.shadow_ppr_sample(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, MAX_ROUNDS, e_cap=E_CAP, out=out)), info


def touched(g, roots, eps):
    """[min, median, max] touched nodes over the first TOUCHED_SAMPLE roots, by the rule's rounds on the host."""
    aq, thr, T, ONE = int(round(ALPHA * 2 ** 16)), max(1, int(round(eps * 2 ** 30))), 4096, 1 << 30
    rowptr = g.rowptr.cpu()
    counts = []
    for root in roots[:TOUCHED_SAMPLE].tolist():
        r, deg, rows = {root: ONE}, {}, {}

        def row(v):
            if v not in rows:
                a, b = int(rowptr[v].item()), int(rowptr[v + 1].item())
                rows[v], deg[v] = g.col[a:b].tolist(), b - a
            return rows[v]
        for _ in range(MAX_ROUNDS):
            for v in r:
                row(v)
            front = [v for v in r if r[v] > 0 and r[v] >= thr * deg[v]]
            if not front or len(r) + sum(deg[v] for v in front) > T:
                break
            snap = [(v, r[v]) for v in front]
            for v, _ in snap:
                r[v] = 0
            for v, rv in snap:
                if deg[v]:
                    share = (rv - ((rv * aq) >> 16)) // deg[v]
                    for u in rows[v]:
                        r[u] = r.get(u, 0) + share
        counts.append(len(r))
    return [min(counts), int(statistics.median(counts)), max(counts)]


def raw_khop_call(torch, lib_path, g, roots, k=10, depth=2, seed=1):
    """grapes_shadow_sample through the library at lib_path (ctypes, this script's own buffers)."""
    from grapes_amd import _lib, ops
    lib = ctypes.CDLL(lib_path)
    res, args = _lib.SIGNATURES["grapes_shadow_sample"]
    lib.grapes_shadow_sample.restype, lib.grapes_shadow_sample.argtypes = res, args
    lib.grapes_shadow_sample_workspace_bytes.restype = ctypes.c_size_t
    B, C, dev = roots.numel(), ops.shadow_cap(depth, k), roots.device
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    n_id, ptr, batch, rid, ei, d_n, d_e = i32(B * C), i32(B + 1), i32(B * C), i32(B), i32(2, E_CAP), i32(1), i32(1)
    e_id = torch.empty(E_CAP, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.grapes_shadow_sample_workspace_bytes(B, depth, k), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = lib.grapes_shadow_sample(p(g.rowptr), p(g.col), g.num_nodes, p(roots), B, None, depth, k, None, seed, 0, None, B * C, E_CAP,
                                      p(n_id), p(ptr), p(batch), p(rid), p(ei[0]), p(ei[1]), p(e_id), p(d_n), p(d_e), p(ws), p(status),
                                      stream)
        assert rc == 0
    return fn, (n_id, ptr, ei, d_n, d_e)


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_shadow_ppr.py measures on the GPU; none is visible")
    from grapes_amd import _lib, ops, shadow
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.shadow import ShaDow
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    plain, with_hub, hub = root_sets(torch, g, train)
    sets = (("without_hub", plain), ("with_hub", with_hub))
    if a.trace_calls:
        fn, _ = ppr_call(ops, g, with_hub, 200, 2 ** -14)
        for _ in range(a.trace_calls):
            fn()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic)",
           "nodes": int(g.num_nodes), "entries": int(g.nnz), "batch_size": BATCH, "hub": hub,
           "hub_entries": int((g.rowptr[hub + 1] - g.rowptr[hub]).item()), "alpha": ALPHA, "max_rounds": MAX_ROUNDS,
           "units": {"sampler": "us per call (three launches, host launches included), median of reps",
                     "wall": "ms of host wall time to a device synchronise, host reads included"}}
    if a.parent_lib:
        calls, outs = {}, {}
        for name, roots in sets:
            for tag, path in (("parent_a", a.parent_lib), ("branch", _lib.LIB_PATH), ("parent_b", a.parent_lib)):
                calls[f"{name}/{tag}"], outs[f"{name}/{tag}"] = raw_khop_call(torch, path, g, roots)
        st = _alternate(torch, calls, a.reps, a.inner)
        for name, _ in sets:                                             # the two libraries computed the same batch
            pa, br = outs[f"{name}/parent_a"], outs[f"{name}/branch"]
            n, e = int(pa[3].item()), int(pa[4].item())
            assert n == int(br[3].item()) and e == int(br[4].item()) and torch.equal(pa[0][:n], br[0][:n]) and torch.equal(pa[1], br[1])
            assert torch.equal(pa[2][:, :e], br[2][:, :e])
        res["refactor_check"] = {"what": "grapes_shadow_sample(depth 2, num_neighbors 10): the parent commit's library (entered twice) "
                                         "against this tree's, alternating in every repetition of one process; same outputs asserted",
                                 **st}
    else:
        res["ppr"], seen = {}, {}
        for k in KS:
            for eps in EPS:
                calls, info = {}, {}
                for name, roots in sets:
                    calls[name], info[name] = ppr_call(ops, g, roots, k, eps)
                    if (name, eps) not in seen:                         # (the touched set does not depend on k)
                        seen[name, eps] = touched(g, roots, eps)
                    info[name][f"touched_min_median_max_first_{TOUCHED_SAMPLE}_roots"] = seen[name, eps]
                st = _alternate(torch, calls, a.reps, a.inner)
                entry = {name: {**info[name], **st[name]} for name in calls}
                res["ppr"][f"k={k},eps=2^{int(round(math.log2(eps)))}"] = entry
                print(json.dumps(entry), file=sys.stderr, flush=True)
        calls, info = {}, {}
        for name, roots in sets:
            calls[name], info[name] = sampler_call(ops, g, roots, 10, hub)
        st = _alternate(torch, calls, a.reps, a.inner)
        res["khop_depth2_k10"] = {name: {**info[name], **st[name]} for name in calls}
        # one eager step under each scope
        x, y = d.x.contiguous(), d.y
        torch.manual_seed(0)
        trainers = {}
        for name, kw in (("ppr", dict(scope="ppr", ppr_k=200, ppr_alpha=ALPHA, ppr_eps=2 ** -14, ppr_rounds=MAX_ROUNDS)),
                         ("khop", dict(depth=2, num_neighbors=10, seed=1))):
            m = ShaDow(x.shape[1], WIDTH, d.num_classes, 3, conv="sage", pool=True).to(g.device)
            trainers[name] = shadow.ShadowTrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), **kw)
        nodes = {}

        def step(name):
            def run():
                nodes[name] = int(trainers[name].step(plain)[1].num_nodes)
            return run
        steps = _wall(torch, {name: step(name) for name in trainers}, a.reps)
        for name in steps:
            steps[name]["batch_nodes_last_step"] = nodes[name]
        steps["ratio_ppr_to_khop"] = round(steps["ppr"]["median_ms"] / steps["khop"]["median_ms"], 3)
        res["step"] = steps
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--trace_calls", type=int, default=0)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
