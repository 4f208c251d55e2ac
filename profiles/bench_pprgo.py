#!/usr/bin/env python3
"""PPRGo: ops.pprgo_topk beside ops.shadow_ppr_sample (whose push and selection it shares), ops.pprgo_batch, the fused weighted
gathers beside their torch emulation, one eager PPRGoTrainer step, and the two ShaDow samplers before and after the push and the
selection were factored out of shadow_ppr_build_k.

      python profiles/bench_pprgo.py [--reps 21] [--inner 200] [--out profiles/pprgo_bench.json]
      python profiles/bench_pprgo.py --parent_lib <libgrapes_hip.so of the parent commit> [--out ...]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_pprgo.py --trace_calls 200

The products-shaped synthetic graph, batch 512, everything in one process; the root sets are profiles/bench_shadow.py's (512 training
nodes far from the hub, and the same set with the hub and 63 nodes that store it in front).  A repetition is `inner` calls between two
device events, the variants alternating in every repetition; the figure kept is the median over `reps` repetitions after a warm-up,
with the quartiles beside it; host launches are included.

topk.      ops.pprgo_topk and ops.shadow_ppr_sample at alpha = 0.25, (k, eps) in {32, 200} x {2^-12, 2^-14}, both root sets, into
           preallocated buffers.  topk does a strict subset of the other call's work; `lower_by_more_than_the_quartile_ranges` says
           whether its median lies below by more than the two quartile ranges together.
batch.     ops.pprgo_batch over the k = 32 and k = 200 slot tables (eps = 2^-14, the plain set).
gather.    ops.pprgo_aggregate_fwd, and forward + backward, at (k, C) = (32, 47), (200, 47), (200, 256), beside the torch emulation
           (w[..., None] * z[loc]).sum(1) with autograd (dead slots carry weight 0 there).  The equivalent edge list for
           ops.wgcn_aggregate_fwd / _bwd is not built here: that path wants a prepared graph over the n + m rows, which this script
           does not time.
step.      PPRGoTrainer.step (k = 32, two layers of 256 columns), with and without the precomputed tables, beside
           ShadowTrainer(scope="ppr", ppr_k=32) and SageTrainer(fanouts 10, 10): host wall time to a device synchronise, median of
           `reps` calls after 3 — neighbours for scale, not equals.

--parent_lib times grapes_shadow_sample (depth 2, num_neighbors 10) and grapes_shadow_ppr_sample (k = 200, eps = 2^-14) through the
given library and through this tree's, alternating in every repetition, the parent's library entered twice so that the spread of its
own repeated runs stands beside the difference; the outputs of the two libraries are asserted equal.  --trace_calls N runs N calls of
ops.pprgo_topk, ops.pprgo_batch and the gathers (k = 200, eps = 2^-14, the hub set, C = 47) and nothing else, for a kernel trace in a
run of its own.

Not measured: a captured step (none exists), other graphs, other alpha, the wgcn route."""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_shadow import BATCH, E_CAP, WIDTH, _alternate, _wall, root_sets  # noqa: E402
from bench_shadow_ppr import raw_khop_call  # noqa: E402

ALPHA, MAX_ROUNDS = 0.25, 32
KS, EPS = (32, 200), (2 ** -12, 2 ** -14)


def _fixed(eps):
    return int(round(ALPHA * 2 ** 16)), max(1, int(round(eps * 2 ** 30)))


def topk_call(ops, g, roots, k, eps):
    aq, thr = _fixed(eps)
    out = ops.pprgo_topk(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, MAX_ROUNDS)
    return (lambda: ops.pprgo_topk(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, MAX_ROUNDS, out=out)), out


def ppr_sample_call(ops, g, roots, k, eps):
    aq, thr = _fixed(eps)
    out = ops.shadow_ppr_sample(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, MAX_ROUNDS, e_cap=E_CAP)
    return (lambda: ops.shadow_ppr_sample(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, MAX_ROUNDS, e_cap=E_CAP, out=out)), out


def raw_ppr_call(torch, lib_path, g, roots, k=200, eps=2 ** -14):
    """grapes_shadow_ppr_sample through the library at lib_path (ctypes, this script's own buffers)."""
    from grapes_amd import _lib
    lib = ctypes.CDLL(lib_path)
    res, args = _lib.SIGNATURES["grapes_shadow_ppr_sample"]
    lib.grapes_shadow_ppr_sample.restype, lib.grapes_shadow_ppr_sample.argtypes = res, args
    lib.grapes_shadow_ppr_sample_workspace_bytes.restype = ctypes.c_size_t
    aq, thr = _fixed(eps)
    B, C, dev = roots.numel(), k + 1, roots.device
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    n_id, ptr, batch, rid, ei, d_n, d_e, score, rounds, stop = (i32(B * C), i32(B + 1), i32(B * C), i32(B), i32(2, E_CAP), i32(1), i32(1),
                                                                i32(B * C), i32(B), i32(B))
    e_id = torch.empty(E_CAP, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.grapes_shadow_ppr_sample_workspace_bytes(B, k), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = lib.grapes_shadow_ppr_sample(p(g.rowptr), p(g.col), g.num_nodes, p(roots), B, None, k, aq, thr, MAX_ROUNDS, B * C, E_CAP,
                                          p(n_id), p(ptr), p(batch), p(rid), p(ei[0]), p(ei[1]), p(e_id), p(score), p(rounds), p(stop),
                                          p(d_n), p(d_e), p(ws), p(status), stream)
        assert rc == 0
    return fn, (n_id, ptr, ei, d_n, d_e, score)


def gather_calls(torch, ops, b, C):
    """{name: fn} of the fused gathers and the torch emulation over batch b at width C, and the largest difference between them."""
    dev = b.loc.device
    torch.manual_seed(1)
    z = torch.randn(b.num_nodes, C, device=dev)
    g = torch.randn(b.loc.shape[0], C, device=dev)
    w, cnt, e = b.weight, b.cnt, int(b.tslot.numel())
    loc_l = b.loc.long().clamp(min=0)
    zt = z.clone().requires_grad_(True)

    def fused_fb():
        out = ops.pprgo_aggregate_fwd(z, w, b.loc, cnt)
        return out, ops.pprgo_aggregate_bwd(g, w, b.tptr, b.tslot, b.num_nodes, e, item_cap=b.item_cap)

    def torch_fb():
        zt.grad = None
        out = (w[..., None] * zt[loc_l]).sum(1)
        out.backward(g)
        return out, zt.grad
    (fo, fd), (to, td) = fused_fb(), torch_fb()
    diff = max(float((fo - to.detach()).abs().max()), float((fd - td).abs().max()))
    calls = {"fused_fwd": lambda: ops.pprgo_aggregate_fwd(z, w, b.loc, cnt), "fused_fwd_bwd": fused_fb,
             "torch_fwd": lambda: (w[..., None] * z[loc_l]).sum(1), "torch_fwd_bwd": torch_fb}
    return calls, diff


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pprgo.py measures on the GPU; none is visible")
    from grapes_amd import _lib, graphsage, ops, pprgo, shadow
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.pprgo import PPRGo, PPRGoSampler
    from grapes_amd.modules.shadow import ShaDow
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    plain, with_hub, hub = root_sets(torch, g, train)
    sets = (("without_hub", plain), ("with_hub", with_hub))
    if a.trace_calls:
        s = PPRGoSampler(g, k=200, alpha=ALPHA, eps=2 ** -14, max_rounds=MAX_ROUNDS)
        b = s.sample(with_hub)
        fused = gather_calls(torch, ops, b, 47)[0]["fused_fwd_bwd"]
        topk = topk_call(ops, g, with_hub, 200, 2 ** -14)[0]
        for _ in range(a.trace_calls):
            topk()
            ops.pprgo_batch(b.nbr, b.cnt, g.num_nodes, s._scratch)
            fused()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic)",
           "nodes": int(g.num_nodes), "entries": int(g.nnz), "batch_size": BATCH, "hub": hub,
           "hub_entries": int((g.rowptr[hub + 1] - g.rowptr[hub]).item()), "alpha": ALPHA, "max_rounds": MAX_ROUNDS,
           "units": {"calls": "us per call (host launches included), median of reps",
                     "wall": "ms of host wall time to a device synchronise, host reads included"}}
    if a.parent_lib:
        calls, outs = {}, {}
        for name, roots in sets:
            for tag, path in (("parent_a", a.parent_lib), ("branch", _lib.LIB_PATH), ("parent_b", a.parent_lib)):
                calls[f"khop/{name}/{tag}"], outs[f"khop/{name}/{tag}"] = raw_khop_call(torch, path, g, roots)
                calls[f"ppr/{name}/{tag}"], outs[f"ppr/{name}/{tag}"] = raw_ppr_call(torch, path, g, roots)
        st = _alternate(torch, calls, a.reps, a.inner)
        inside = {}
        for kind in ("khop", "ppr"):
            for name, _ in sets:                                         # the two libraries computed the same batch
                pa, br = outs[f"{kind}/{name}/parent_a"], outs[f"{kind}/{name}/branch"]
                n, e = int(pa[3].item()), int(pa[4].item())
                assert n == int(br[3].item()) and e == int(br[4].item()) and torch.equal(pa[0][:n], br[0][:n]) and torch.equal(pa[1], br[1])
                assert torch.equal(pa[2][:, :e], br[2][:, :e]) and (kind == "khop" or torch.equal(pa[5][:n], br[5][:n]))
                pq = [st[f"{kind}/{name}/{t}"] for t in ("parent_a", "parent_b")]
                lo, hi = min(q["q1_us"] for q in pq), max(q["q3_us"] for q in pq)
                inside[f"{kind}/{name}"] = bool(lo <= st[f"{kind}/{name}/branch"]["median_us"] <= hi)
        res["refactor_check"] = {"what": "grapes_shadow_sample(depth 2, num_neighbors 10) and grapes_shadow_ppr_sample(k 200, eps 2^-14): "
                                         "the parent commit's library (entered twice) against this tree's, alternating in every "
                                         "repetition of one process; same outputs asserted",
                                 "branch_median_inside_the_parents_quartiles": inside, **st}
    else:
        res["topk"] = {}
        for k in KS:
            for eps in EPS:
                calls = {}
                for name, roots in sets:
                    calls[f"{name}/pprgo_topk"], t = topk_call(ops, g, roots, k, eps)
                    calls[f"{name}/shadow_ppr_sample"], _ = ppr_sample_call(ops, g, roots, k, eps)
                st = _alternate(torch, calls, a.reps, a.inner)
                for name, _ in sets:
                    x, y = st[f"{name}/pprgo_topk"], st[f"{name}/shadow_ppr_sample"]
                    gap, spread = y["median_us"] - x["median_us"], (x["q3_us"] - x["q1_us"]) + (y["q3_us"] - y["q1_us"])
                    st[f"{name}/lower_by_more_than_the_quartile_ranges"] = bool(gap > spread)
                res["topk"][f"k={k},eps=2^{int(round(math.log2(eps)))}"] = st
                print(json.dumps(st), file=sys.stderr, flush=True)
        res["batch"], res["gather"] = {}, {}
        for k in KS:
            s = PPRGoSampler(g, k=k, alpha=ALPHA, eps=2 ** -14, max_rounds=MAX_ROUNDS)
            b = s.sample(plain)
            s.check()
            out = ops.pprgo_batch(b.nbr, b.cnt, g.num_nodes, s._scratch)
            st = _alternate(torch, {"pprgo_batch": lambda: ops.pprgo_batch(b.nbr, b.cnt, g.num_nodes, s._scratch, out=out)}, a.reps, a.inner)
            res["batch"][f"k={k}"] = {"nodes": b.num_nodes, "slots": b.num_slots, "longest_segment": int((b.tptr[1:] - b.tptr[:-1]).max().item()),
                                      **st["pprgo_batch"]}
            for C in ((47,) if k == 32 else (47, 256)):
                calls, diff = gather_calls(torch, ops, b, C)
                st = _alternate(torch, calls, a.reps, a.inner)
                st["largest_difference_fused_to_torch"] = diff
                st["ratio_torch_to_fused_fwd"] = round(st["torch_fwd"]["median_us"] / st["fused_fwd"]["median_us"], 2)
                st["ratio_torch_to_fused_fwd_bwd"] = round(st["torch_fwd_bwd"]["median_us"] / st["fused_fwd_bwd"]["median_us"], 2)
                res["gather"][f"k={k},C={C}"] = st
                print(json.dumps(st), file=sys.stderr, flush=True)
        # one eager step of each trainer
        x, y = d.x.contiguous(), d.y
        torch.manual_seed(0)
        trainers = {}
        for name in ("pprgo_uncached", "pprgo_cached"):
            m = PPRGo(x.shape[1], [WIDTH, d.num_classes]).to(g.device)
            trainers[name] = pprgo.PPRGoTrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), k=32, alpha=ALPHA, eps=2 ** -14,
                                                max_rounds=MAX_ROUNDS)
        trainers["pprgo_cached"].precompute(plain)
        m = ShaDow(x.shape[1], WIDTH, d.num_classes, 3, conv="sage", pool=True).to(g.device)
        trainers["shadow_ppr_k32"] = shadow.ShadowTrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), scope="ppr", ppr_k=32,
                                                          ppr_alpha=ALPHA, ppr_eps=2 ** -14, ppr_rounds=MAX_ROUNDS)
        m = graphsage.build_model(x.shape[1], WIDTH, d.num_classes, 2, 0.0, "mean", g.device)
        trainers["sage_10_10"] = graphsage.SageTrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), fanouts=[10, 10], seed=1)
        nodes = {}

        def step(name):
            def run():
                nodes[name] = int(trainers[name].step(plain)[1].num_nodes)
            return run
        steps = _wall(torch, {name: step(name) for name in trainers}, a.reps)
        for name in trainers:
            steps[name]["batch_nodes_last_step"] = nodes[name]
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
