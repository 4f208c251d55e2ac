#!/usr/bin/env python3
"""GATv2Conv against GATConv at the same graph and total width: what the F-wide per-edge score and the per-head softmax cost
beside GAT's two per-node scalars.

      python profiles/bench_gatv2.py [--reps 21] [--inner 200] [--out profiles/gatv2_bench.json]

Shape: the classifier's subgraph of the products workload as profiles/bench_gat.py builds it (`sampled`: batch 256 + 3 hops x 256
samples = 1,024 nodes, 16,384 random edges), input width 100.  One process times, alternating between them in every repetition,
GATConv(100 -> 256) and GATv2Conv(100 -> H x C) for H x C = 1 x 256, 4 x 64 and 8 x 32: the layer's forward (GEMMs + aggregation)
and its forward + backward (to x, the weights, att and the bias).  A repetition is `inner` calls between two device events; the
figure kept is the median over `reps` repetitions, after a warm-up of every variant, with the quartiles beside it.  The same
rows of x_l are gathered as GAT gathers of H, plus one x_r row per destination; the extra work is F multiply-adds and H
reductions per edge, and a second GEMM (lin_r)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, F_IN, N, E = 256, 100, 1024, 16384
HEADS = ((1, 256), (4, 64), (8, 32))


def main(a):
    import torch
    from grapes_amd import ops
    from grapes_amd.modules.gcn import GATConv, GATv2Conv
    if not torch.cuda.is_available():
        raise SystemExit("bench_gatv2.py measures on the GPU; none is visible")
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(0)
    ei = torch.randint(0, N, (2, E), device=dev, generator=g, dtype=torch.int32)
    prep = ops.PreparedGraph(ei[0].contiguous(), ei[1].contiguous(), N)
    x = torch.randn(N, F_IN, device=dev, generator=g).requires_grad_(True)
    dout = torch.randn(N, WIDTH, device=dev, generator=g)
    torch.manual_seed(0)
    layers = {"gat_256": GATConv(F_IN, WIDTH).to(dev)}
    for h, c in HEADS:
        layers[f"gatv2_{h}x{c}"] = GATv2Conv(F_IN, c, heads=h).to(dev)

    def fwd(layer):
        with torch.no_grad():
            layer(x, prep)

    def fwd_bwd(layer):
        torch.autograd.grad(layer(x, prep), [x] + list(layer.parameters()), dout)

    variants = [(name, phase, fn, layer) for name, layer in layers.items() for phase, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd))]
    for _, _, fn, layer in variants:                         # warm-up: every variant, every shape of the timed window
        for _ in range(10):
            fn(layer)
    torch.cuda.synchronize()
    times = {(name, phase): [] for name, phase, _, _ in variants}
    for _ in range(a.reps):
        for name, phase, fn, layer in variants:              # (alternating: a drift of the machine reaches every variant alike)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.inner):
                fn(layer)
            t1.record()
            t1.synchronize()
            times[(name, phase)].append(t0.elapsed_time(t1) * 1e3 / a.inner)

    def stats(v):
        q = statistics.quantiles(v, n=4)
        return {"median_us": round(statistics.median(v), 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2)}
    res = {"device": torch.cuda.get_device_name(0), "shape": {"nodes": N, "edges": E, "f_in": F_IN, "width": WIDTH},
           "reps": a.reps, "inner": a.inner, "unit": "us per layer call (host launches included), median of reps",
           "layers": {name: {phase: stats(times[(name, phase)]) for phase in ("fwd", "fwd_bwd")} for name in layers}}
    base = res["layers"]["gat_256"]
    res["ratio_to_gat_256"] = {name: {phase: round(r[phase]["median_us"] / base[phase]["median_us"], 3) for phase in ("fwd", "fwd_bwd")}
                               for name, r in res["layers"].items() if name != "gat_256"}
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
