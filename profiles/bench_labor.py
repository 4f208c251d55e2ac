#!/usr/bin/env python3
"""LABOR: the layer-neighbour sampler's kernel against the node-wise sampler's on the same rows, the size of its batches against
NeighborSampler's, and one eager training step against GraphSAGE's.

      python profiles/bench_labor.py [--reps 21] [--inner 200] [--out profiles/labor_bench.json]

The products-shaped synthetic graph, batch 512, fanouts 25 / 10 and 10 / 10, everything in one process.

Kernel.  The rows of every layer of a NeighborSampler batch (the second layer of 25 / 10 holds the 17,375-entry hub row):
ops.labor_sample_layer (LABOR-0, four launches: a 64-entry chunk per wavefront, no selection pass) against ops.sage_sample_layer (two
launches, exact-k selection by one wavefront per row) into preallocated buffers.  A repetition is `inner` calls between two device
events, the variants alternating in every repetition; the figure kept is the median over `reps` repetitions after a warm-up, with the
quartiles beside it; host launches are included.

Batch.  num_nodes and the entry count of LaborSampler batches with importance_iters 0, 1 and 3 against NeighborSampler's at the same
fanouts and targets (one draw each, seed 1).

Step.  LaborTrainer.step (importance_iters 0, hidden 256) against SageTrainer.step on the same targets: host wall time to a device
synchronise, sampling with its host reads included; median of `reps` steps after 3.

Not measured: a captured step (none exists), other graphs or widths, the weighted route's step (importance_iters >= 1)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, BATCH = 256, 512
FANOUT_SETS = ((25, 10), (10, 10))
ITERS = (0, 1, 3)


def _stats(v):
    q = statistics.quantiles(v, n=4)
    return {"median_us": round(statistics.median(v), 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2)}


def _alternate(torch, variants, reps, inner):
    """{name: stats} of the callables in variants ({name: fn}), alternating between them in every repetition."""
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / inner)
    return {name: _stats(v) for name, v in times.items()}


def bench_kernels(torch, ops, g, b, a):
    Nn, dev = g.num_nodes, g.device
    layers = []
    for L in b.layers:
        rows, k = L.prev, L.fanout
        deg = g.rowptr[rows.long() + 1] - g.rowptr[rows.long()]
        deg_sum = int(deg.sum().item())
        e_sage = max(1, min(rows.numel() * k, deg_sum))
        out_sage = ops.sage_sample_layer(g.rowptr, g.col, Nn, rows, k, e_cap=e_sage, philox_seed=1)
        out_labor = ops.labor_sample_layer(g.rowptr, g.col, Nn, rows, k, philox_seed=1, deg_sum=deg_sum)
        item_cap = ops.labor_item_cap(rows.numel(), deg_sum)
        variants = {"labor_sample_layer": lambda: ops.labor_sample_layer(g.rowptr, g.col, Nn, rows, k, e_cap=deg_sum, item_cap=item_cap,
                                                                         philox_seed=1, out=out_labor),
                    "sage_sample_layer": lambda: ops.sage_sample_layer(g.rowptr, g.col, Nn, rows, k, e_cap=e_sage, philox_seed=1,
                                                                       out=out_sage)}
        st = _alternate(torch, variants, a.reps, a.inner)
        layers.append({"rows": int(rows.numel()), "fanout": k, "entries_of_the_rows": deg_sum, "max_row_entries": int(deg.max().item()),
                       "work_items": int(((deg + ops.LABOR_CHUNK - 1) // ops.LABOR_CHUNK).sum().item()),
                       "kept_labor": int(out_labor[4].item()), "kept_sage": int(out_sage[3].item()), **st,
                       "ratio_labor_to_sage": round(st["labor_sample_layer"]["median_us"] / st["sage_sample_layer"]["median_us"], 3)})
    return layers


def bench_batches(NeighborSampler, LaborSampler, g, targets, fanouts):
    def size(b):
        return {"num_nodes": int(b.num_nodes), "entries": [int(L.edge_src.numel()) for L in b.layers],
                "layer_sources": [int(L.after.numel()) for L in b.layers]}
    s = NeighborSampler(g, fanouts, seed=1)
    out = {"neighbor_sampler": size(s.sample(targets))}
    s.check()
    for it in ITERS:
        s = LaborSampler(g, fanouts, importance_iters=it, seed=1)
        out[f"labor_{it}"] = size(s.sample(targets))
        s.check()
        out[f"labor_{it}"]["nodes_ratio_to_neighbor_sampler"] = round(out[f"labor_{it}"]["num_nodes"] /
                                                                      out["neighbor_sampler"]["num_nodes"], 3)
    return out


def bench_steps(torch, trainers, targets, reps):
    wall, nodes = {name: [] for name in trainers}, {}
    for i in range(3 + reps):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, bb = tr.step(targets)
            torch.cuda.synchronize()
            if i >= 3:
                wall[name].append(1e3 * (time.perf_counter() - t0))
            nodes[name] = int(bb.num_nodes)
    steps = {}
    for name, v in wall.items():
        q = statistics.quantiles(v, n=4)
        steps[name] = {"median_ms": round(statistics.median(v), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3),
                       "batch_nodes_last_step": nodes[name]}
    steps["ratio_labor_to_sage"] = round(steps["labor"]["median_ms"] / steps["graphsage"]["median_ms"], 3)
    return steps


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_labor.py measures on the GPU; none is visible")
    from grapes_amd import graphsage, labor, ops
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.labor import LaborSampler
    from grapes_amd.modules.sage import NeighborSampler
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    targets = train[torch.randperm(train.numel(), device=train.device)[:BATCH]]
    x, y = d.x.contiguous(), d.y
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic)",
           "nodes": int(g.num_nodes), "entries": int(g.nnz), "batch_size": BATCH, "hidden_dim": WIDTH,
           "units": {"kernel": "us per call (host launches included), median of reps",
                     "step": "ms per eager step, host wall to a device synchronise"}, "fanouts": {}}
    for fanouts in FANOUT_SETS:
        s = NeighborSampler(g, fanouts, seed=1)
        b = s.sample(targets)
        s.check()
        entry = {"kernel_layers": bench_kernels(torch, ops, g, b, a),
                 "batch": bench_batches(NeighborSampler, LaborSampler, g, targets, fanouts)}
        models = {n: graphsage.build_model(x.shape[1], WIDTH, d.num_classes, 2, 0.0, "mean", g.device) for n in ("labor", "graphsage")}
        opt = {n: torch.optim.Adam(m.parameters(), lr=1e-3) for n, m in models.items()}
        trainers = {"labor": labor.LaborTrainer(g, x, y, models["labor"], opt["labor"], fanouts=fanouts, seed=1),
                    "graphsage": graphsage.SageTrainer(g, x, y, models["graphsage"], opt["graphsage"], fanouts=fanouts, seed=1)}
        entry["step"] = bench_steps(torch, trainers, targets, a.reps)
        res["fanouts"][",".join(str(k) for k in fanouts)] = entry
        print(json.dumps(entry), file=sys.stderr, flush=True)
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
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
