#!/usr/bin/env python3
"""PinSAGE: ops.pinsage_neighbors beside a torch emulation of the same quantity and beside ops.pprgo_topk at the same K, the fused
relu + L2 normalisation beside the torch expression, and one eager PinSAGETrainer step beside its neighbours.

      python profiles/bench_pinsage.py [--reps 21] [--inner 200] [--out profiles/pinsage_bench.json]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_pinsage.py --trace_calls 200

The products-shaped synthetic graph, batch 512, everything in one process; the root sets are profiles/bench_shadow.py's (512 training
nodes far from the hub, and the same set with the hub and 63 nodes that store it in front).  A repetition is `inner` calls between two
device events, the variants alternating in every repetition; the figure kept is the median over `reps` repetitions after a warm-up,
with the quartiles beside it; host launches are included.

neighbors. ops.pinsage_neighbors at (R, L, T) = (10, 2, 3), (50, 2, 10), (200, 3, 50), (256, 4, 50), p = 0.5, both root sets, into
           preallocated buffers at a fixed host offset.  Beside it the cheapest torch form found of the same quantity on the device
           (torch_neighbors below: per step one torch.rand, a gather of rowptr and of col, then ONE sort of the [m, V] visits,
           unique_consecutive over the flattened rows, a scatter of the keys into a dense [m, V] table and topk — no Python loop over
           roots; its walks use torch's generator, so the figures compare cost, not bits), and ops.pprgo_topk at k = T (alpha 0.25,
           eps 2^-14): a neighbour for scale, not an equal.  `lower_by_more_than_the_quartile_ranges`: the fused median lies below the
           emulation's by more than the two interquartile ranges together.
norm.      ops.relu_l2norm_fwd, and forward + backward, on 5 000 rows of 64 and 256 columns beside relu(s) / clamp(norm, eps) with
           autograd.
step.      PinSAGETrainer.step (two layers of 256 columns, R = 10, L = 2, num_neighbors = 5: block 1 of 512 roots then holds at most
           3072 seeds, inside the batch structure's 4096) beside SageTrainer(fanouts 10, 10) and PPRGoTrainer(k = 32): host wall time
           to a device synchronise, median of `reps` calls after 3 — neighbours for scale, not equals.

--trace_calls N runs N calls of ops.pinsage_neighbors at (50, 2, 10) on the hub set and nothing else, for a kernel trace in a run of
its own.

Not measured: a captured step (none exists), other graphs, other termination probabilities."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_shadow import BATCH, WIDTH, _alternate, _wall, root_sets  # noqa: E402

POINTS = ((10, 2, 3), (50, 2, 10), (200, 3, 50), (256, 4, 50))
P_TERM = 0.5
NORM_ROWS, NORM_WIDTHS, EPS = 5000, (64, 256), 1e-12


def fused_call(ops, g, roots, R, L, T):
    tq = ops.pinsage_term_q(P_TERM)
    out = ops.pinsage_neighbors(g.rowptr, g.col, g.num_nodes, roots, R, L, tq, T, philox_seed=1, philox_offset=7)
    return (lambda: ops.pinsage_neighbors(g.rowptr, g.col, g.num_nodes, roots, R, L, tq, T, philox_seed=1, philox_offset=7, out=out)), out


def torch_neighbors(torch, g, roots, R, L, T):
    """The same quantity in torch on the device -> fn() -> (nbr [m, K], visits [m, K], cnt [m]).  Everything that does not depend on
    the draw (degrees, the repeated roots, the row bases) is prepared outside the timed call."""
    m, V, N, dev = roots.numel(), R * L, g.num_nodes, roots.device
    deg = (g.rowptr[1:] - g.rowptr[:-1]).contiguous()
    start = g.rowptr[:-1].contiguous()
    col = g.col
    root_rep = roots.long().repeat_interleave(R)
    base = (torch.arange(m, device=dev) * (N + 1))[:, None]
    rows = torch.arange(m, device=dev)
    big = torch.iinfo(torch.int64).max
    last = g.col.numel() - 1
    k = min(T, V)

    def fn():
        c, alive, vis = root_rep, torch.ones(m * R, dtype=torch.bool, device=dev), []
        for _ in range(L):
            u = torch.rand(2, m * R, device=dev)
            d = deg[c]
            alive = alive & (u[0] >= P_TERM) & (d > 0)
            idx = (start[c] + (u[1] * d).long().minimum(d - 1)).clamp_(0, last)
            c = torch.where(alive, col[idx].long(), c)
            vis.append(torch.where(alive & (c != root_rep), c, N))
        v = torch.stack(vis, 1).view(m, V)
        sv = v.sort(dim=1).values
        uq, cn = torch.unique_consecutive((sv + base).reshape(-1), return_counts=True)
        rb = torch.div(uq, N + 1, rounding_mode="floor")
        idn = uq - rb * (N + 1)
        key = torch.where(idn == N, big, ((V - cn) << 32) | idn)
        first = torch.searchsorted(rb, rows)
        dense = torch.full((m, V), big, dtype=torch.int64, device=dev)
        dense[rb, torch.arange(uq.numel(), device=dev) - first[rb]] = key
        top = dense.topk(k, dim=1, largest=False).values
        live = top != big
        nbr = torch.where(live, top & 0xFFFFFFFF, roots.long()[:, None])
        return nbr, torch.where(live, V - (top >> 32), 0), live.sum(1) + 1
    return fn


def topk_call(ops, g, roots, k):
    aq, thr = int(round(0.25 * 2 ** 16)), max(1, int(round(2 ** -14 * 2 ** 30)))
    out = ops.pprgo_topk(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, 32)
    return lambda: ops.pprgo_topk(g.rowptr, g.col, g.num_nodes, roots, k, aq, thr, 32, out=out)


def norm_calls(torch, ops, f):
    torch.manual_seed(2)
    s = torch.randn(NORM_ROWS, f, device="cuda")
    g = torch.randn(NORM_ROWS, f, device="cuda")
    st = s.clone().requires_grad_(True)
    out = ops.relu_l2norm_fwd(s, EPS)
    ds = torch.empty_like(s)

    def fused_fb():
        o, n = ops.relu_l2norm_fwd(s, EPS, out=out)
        return o, ops.relu_l2norm_bwd(g, o, n, s, EPS, ds=ds)

    def torch_f(x=s):
        z = torch.relu(x)
        return z / z.pow(2).sum(1, keepdim=True).sqrt().clamp(min=EPS)

    def torch_fb():
        st.grad = None
        o = torch_f(st)
        o.backward(g)
        return o, st.grad
    (fo, fd), (to, td) = fused_fb(), torch_fb()
    diff = max(float((fo - to.detach()).abs().max()), float((fd - td).abs().max()))
    return {"fused_fwd": lambda: ops.relu_l2norm_fwd(s, EPS, out=out), "fused_fwd_bwd": fused_fb, "torch_fwd": torch_f,
            "torch_fwd_bwd": torch_fb}, diff


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pinsage.py measures on the GPU; none is visible")
    from grapes_amd import graphsage, ops, pinsage, pprgo
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.pinsage import PinSAGE
    from grapes_amd.modules.pprgo import PPRGo
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    plain, with_hub, hub = root_sets(torch, g, train)
    sets = (("without_hub", plain), ("with_hub", with_hub))
    if a.trace_calls:
        fn = fused_call(ops, g, with_hub, 50, 2, 10)[0]
        for _ in range(a.trace_calls):
            fn()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic)",
           "nodes": int(g.num_nodes), "entries": int(g.nnz), "batch_size": BATCH, "hub": hub,
           "hub_entries": int((g.rowptr[hub + 1] - g.rowptr[hub]).item()), "termination_prob": P_TERM,
           "units": {"calls": "us per call (host launches included), median of reps",
                     "wall": "ms of host wall time to a device synchronise, host reads included"}}
    res["neighbors"] = {}
    for R, L, T in POINTS:
        calls, shapes = {}, {}
        for name, roots in sets:
            calls[f"{name}/pinsage_neighbors"], out = fused_call(ops, g, roots, R, L, T)
            calls[f"{name}/torch_emulation"] = torch_neighbors(torch, g, roots, R, L, T)
            calls[f"{name}/pprgo_topk"] = topk_call(ops, g, roots, T)
            e = calls[f"{name}/torch_emulation"]()
            shapes[name] = {"mean_kept_fused": round(float(out[2].float().mean()) - 1, 2), "mean_kept_torch": round(float(e[2].float().mean()) - 1, 2)}
        st = _alternate(torch, calls, a.reps, a.inner)
        for name, _ in sets:
            x, y = st[f"{name}/pinsage_neighbors"], st[f"{name}/torch_emulation"]
            gap, spread = y["median_us"] - x["median_us"], (x["q3_us"] - x["q1_us"]) + (y["q3_us"] - y["q1_us"])
            st[f"{name}/lower_by_more_than_the_quartile_ranges"] = bool(gap > spread)
            st[f"{name}/ratio_torch_to_fused"] = round(y["median_us"] / x["median_us"], 2)
            st[f"{name}/kept"] = shapes[name]
        res["neighbors"][f"R={R},L={L},T={T}"] = st
        print(json.dumps(st), file=sys.stderr, flush=True)
    res["norm"] = {}
    for f in NORM_WIDTHS:
        calls, diff = norm_calls(torch, ops, f)
        st = _alternate(torch, calls, a.reps, a.inner)
        st["largest_difference_fused_to_torch"] = diff
        st["ratio_torch_to_fused_fwd"] = round(st["torch_fwd"]["median_us"] / st["fused_fwd"]["median_us"], 2)
        st["ratio_torch_to_fused_fwd_bwd"] = round(st["torch_fwd_bwd"]["median_us"] / st["fused_fwd_bwd"]["median_us"], 2)
        res["norm"][f"rows={NORM_ROWS},f={f}"] = st
        print(json.dumps(st), file=sys.stderr, flush=True)
    # one eager step of each trainer
    x, y = d.x.contiguous(), d.y
    torch.manual_seed(0)
    trainers = {}
    m = PinSAGE(x.shape[1], [WIDTH, WIDTH], d.num_classes).to(g.device)
    trainers["pinsage_R10_L2_T5"] = pinsage.PinSAGETrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), num_neighbors=5,
                                                           num_random_walks=10, walk_length=2, termination_prob=P_TERM, seed=1)
    m = PPRGo(x.shape[1], [WIDTH, d.num_classes]).to(g.device)
    trainers["pprgo_k32"] = pprgo.PPRGoTrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), k=32, alpha=0.25, eps=2 ** -14,
                                               max_rounds=32)
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
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
