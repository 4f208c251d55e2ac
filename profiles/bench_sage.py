#!/usr/bin/env python3
"""GraphSAGE: the SAGEConv layer in both operand forms against the emulation it replaces, the node-wise sampler against reading
every entry of the same rows, and one eager training step against LADIES'.

      python profiles/bench_sage.py [--reps 21] [--inner 200] [--out profiles/sage_bench.json]

Layer.  The classifier's subgraph of the products workload as profiles/bench_gatv2.py builds it (1,024 nodes, 16,384 random edges),
100 -> 256.  One process times, alternating between them in every repetition: SAGEConv(100 -> 256, mean) transform-first and
aggregate-first; the emulation — GCNConv(normalize=False, bias=False) with edge_weight = 1 / deg of the target plus a root
Linear(100 -> 256) added to it; and GCNConv(100 -> 256).  Forward (no grad) and forward + backward (to x and every parameter).  A
repetition is `inner` calls between two device events; the figure kept is the median over `reps` repetitions after a warm-up of
every variant, with the quartiles beside it; host launches are included.

Sampler.  The products-shaped synthetic graph, batch 512, fanouts 25 / 10: per layer ops.sage_sample_layer (two launches) against
ops.frontier_offsets + ops.frontier_expand over the same rows (two launches: every entry read and written, nothing selected), and
frontier_expand alone on ready offsets; the same repetition scheme.

Step.  SageTrainer.step (fanouts 25 / 10, hidden 256) against LadiesTrainer.step (samp_num 64) on the same targets: host wall time
to a device synchronise, sampling with its host reads included; median of `reps` steps after 3.

Not measured: a captured step (none exists), other graphs or widths, aggr="sum" (the same kernels without the row scale)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, F_IN, N, E = 256, 100, 1024, 16384
FANOUTS, BATCH = (25, 10), 512


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


def bench_layer(torch, a):
    from grapes_amd.modules.gcn import GCNConv, Linear, SAGEConv
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(0)
    ei = torch.randint(0, N, (2, E), device=dev, generator=g, dtype=torch.int32)
    x = torch.randn(N, F_IN, device=dev, generator=g).requires_grad_(True)
    dout = torch.randn(N, WIDTH, device=dev, generator=g)
    deg = torch.bincount(ei[1].long(), minlength=N).clamp(min=1).to(torch.float32)
    w = (1.0 / deg)[ei[1].long()].contiguous()
    torch.manual_seed(0)
    sage = SAGEConv(F_IN, WIDTH).to(dev)
    emu_conv, emu_root = GCNConv(F_IN, WIDTH, normalize=False, bias=False).to(dev), Linear(F_IN, WIDTH).to(dev)
    gcn = GCNConv(F_IN, WIDTH).to(dev)
    emu_params = list(emu_conv.parameters()) + list(emu_root.parameters())
    calls = {"sage_transform_first": (lambda: sage(x, ei, _form="transform"), list(sage.parameters())),
             "sage_aggregate_first": (lambda: sage(x, ei, _form="aggregate"), list(sage.parameters())),
             "emulation_gcnconv_weighted_plus_linear": (lambda: emu_conv(x, ei, edge_weight=w) + emu_root(x), emu_params),
             "gcnconv": (lambda: gcn(x, ei), list(gcn.parameters()))}
    with torch.no_grad():                                     # the emulation computes the same map as the layer it is compared with
        emu_conv.lin.weight.copy_(sage.lin_l.weight); emu_root.weight.copy_(sage.lin_r.weight); emu_root.bias.copy_(sage.lin_l.bias)
        ref = calls["emulation_gcnconv_weighted_plus_linear"][0]()
        agree = {k: float((calls[k][0]() - ref).abs().max() / ref.abs().max()) for k in ("sage_transform_first", "sage_aggregate_first")}

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def fwd_bwd(fn, params):
        return lambda: torch.autograd.grad(fn(), [x] + params, dout)

    variants = {}
    for name, (fn, params) in calls.items():
        variants[(name, "fwd")] = fwd(fn)
        variants[(name, "fwd_bwd")] = fwd_bwd(fn, params)
    st = _alternate(torch, variants, a.reps, a.inner)
    layers = {name: {phase: st[(name, phase)] for phase in ("fwd", "fwd_bwd")} for name in calls}
    base = layers["emulation_gcnconv_weighted_plus_linear"]
    ratio = {name: {phase: round(r[phase]["median_us"] / base[phase]["median_us"], 3) for phase in ("fwd", "fwd_bwd")}
             for name, r in layers.items() if name != "emulation_gcnconv_weighted_plus_linear"}
    return {"shape": {"nodes": N, "edges": E, "f_in": F_IN, "width": WIDTH, "aggr": "mean"}, "default_form": sage.default_form(),
            "max_rel_difference_to_emulation": agree, "unit": "us per layer call (host launches included), median of reps",
            "layers": layers, "ratio_to_emulation": ratio}


def bench_sampler_and_step(torch, a):
    from grapes_amd import ops
    from grapes_amd.graph import DeviceGraph
    from grapes_amd import graphsage, ladies
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.sage import NeighborSampler
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    Nn = g.num_nodes
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    targets = train[torch.randperm(train.numel(), device=train.device)[:BATCH]]
    s = NeighborSampler(g, FANOUTS, seed=1)
    b = s.sample(targets)
    s.check()
    layers = []
    for L in b.layers:
        rows, k = L.prev, L.fanout
        eoff, d_e = ops.frontier_offsets(g.rowptr, rows)
        deg_sum = int(d_e.item())
        e_cap = max(1, min(rows.numel() * k, deg_sum))
        out = ops.sage_sample_layer(g.rowptr, g.col, Nn, rows, k, e_cap=e_cap, philox_seed=1)
        variants = {"sage_sample_layer": lambda: ops.sage_sample_layer(g.rowptr, g.col, Nn, rows, k, e_cap=e_cap, philox_seed=1, out=out),
                    "frontier_offsets_plus_expand": lambda: ops.frontier_expand(g.rowptr, g.col, rows, ops.frontier_offsets(g.rowptr, rows)[0],
                                                                                deg_sum),
                    "frontier_expand_alone": lambda: ops.frontier_expand(g.rowptr, g.col, rows, eoff, deg_sum)}
        st = _alternate(torch, variants, a.reps, a.inner)
        layers.append({"rows": int(rows.numel()), "fanout": k, "entries_of_the_rows": deg_sum, "kept": int(L.edge_src.numel()),
                       "max_row_entries": int((g.rowptr[rows.long() + 1] - g.rowptr[rows.long()]).max().item()), **st,
                       "ratio_to_offsets_plus_expand": round(st["sage_sample_layer"]["median_us"] /
                                                             st["frontier_offsets_plus_expand"]["median_us"], 3)})
    x, y = d.x.contiguous(), d.y
    steps = {}
    sage_model = graphsage.build_model(x.shape[1], WIDTH, d.num_classes, 2, 0.0, "mean", g.device)
    lad_model = ladies.build_model(x.shape[1], WIDTH, d.num_classes, 2, 0.0, g.device)
    trainers = {"graphsage_25_10": graphsage.SageTrainer(g, x, y, sage_model, torch.optim.Adam(sage_model.parameters(), lr=1e-3),
                                                          fanouts=FANOUTS, seed=1),
                "ladies_64": ladies.LadiesTrainer(g, x, y, lad_model, torch.optim.Adam(lad_model.parameters(), lr=1e-3), samp_num=64,
                                                  kind="ladies", seed=1)}
    wall = {name: [] for name in trainers}
    nodes = {}
    for i in range(3 + a.reps):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, bb = tr.step(targets)
            torch.cuda.synchronize()
            if i >= 3:
                wall[name].append(1e3 * (time.perf_counter() - t0))
            nodes[name] = int(bb.num_nodes)
    for name, v in wall.items():
        q = statistics.quantiles(v, n=4)
        steps[name] = {"median_ms": round(statistics.median(v), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3),
                       "batch_nodes": nodes[name]}
    steps["ratio_sage_to_ladies"] = round(steps["graphsage_25_10"]["median_ms"] / steps["ladies_64"]["median_ms"], 3)
    return {"dataset": "products (synthetic)", "nodes": int(Nn), "entries": int(g.nnz), "batch_size": BATCH, "fanouts": list(FANOUTS),
            "unit": "us per call (host launches included), median of reps", "layers": layers}, \
           {"unit": "ms per eager step, host wall to a device synchronise", "hidden_dim": WIDTH, "steps": steps}


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sage.py measures on the GPU; none is visible")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner}
    res["layer"] = bench_layer(torch, a)
    print(json.dumps(res["layer"]), file=sys.stderr, flush=True)
    res["sampler"], res["step"] = bench_sampler_and_step(torch, a)
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
