#!/usr/bin/env python3
"""VR-GCN: the fused control-variate aggregation against the same quantity assembled from existing ops, the cost of the long-row
split, and one eager training step against GraphSAGE's.

      python profiles/bench_vrgcn.py [--reps 21] [--inner 200] [--out profiles/vrgcn_bench.json]

Forward.  The products-shaped synthetic graph (loop-free copy), batch 512, fanouts 2 / 2, width 256: the rows are the output
layer's (the targets), H random on the batch's rows, the history random.  One process times, alternating in every repetition:
  fused                       ops.vrgcn_aggregate_fwd on the prepared kept entries (one launch; four with a long row among the rows)
  emulation_total             the same A from existing ops, everything a step would have to do for the full-neighbourhood term:
                              frontier_offsets + frontier_expand of the rows, the union with the rows (the 1-hop closure, with its
                              host reads), the local ids, gcn_prepare over the closure, gather_rows + scale_rows of the history on
                              the closure, gcn_aggregate_fwd_prescaled; and for the sampled term gather_rows of the history on the
                              batch, H - Hbar, wgcn_aggregate_fwd with the weights (d_u / k_u) dinv_u dinv_v (structure and weights
                              built once, outside the timing, as the fused call's preparation is), and the sum
  emulation_aggregations_only the gathers and aggregations alone on a ready closure and preparation
with and without the hub row (17 375 entries) among the rows.  A repetition is `inner` calls between two device events; the figure
kept is the median over `reps` repetitions after a warm-up of every variant, with the quartiles; host launches are included.  With
the hub among the rows emulation_total is the median of 5 single calls: its gcn_prepare ranks the hub row's entries against each
other in one wavefront (quadratic in the row), so 4 200 calls of it would run for many minutes.

Step.  VrgcnTrainer.step (fanouts 2 / 2, hidden 256) against SageTrainer.step (fanouts 25 / 10) on the same targets: host wall time
to a device synchronise, sampling with its host reads included; median of `reps` steps after 3.

Not measured: a captured step (none exists), other graphs or widths, the backward alone."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, BATCH, FANOUTS, SAGE_FANOUTS = 256, 512, (2, 2), (25, 10)


def _stats(v):
    q = statistics.quantiles(v, n=4)
    return {"median_us": round(statistics.median(v), 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2)}


def _alternate(torch, variants, reps, inner, warm=5):
    for fn in variants.values():
        for _ in range(warm):
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


def forward_case(torch, a, g, vg, targets, seed, total_single_calls=0):
    """The three variants on one batch whose output rows are `targets`.  total_single_calls > 0: emulation_total is the median of
    that many single calls instead of reps x inner (its gcn_prepare orders a row of the closure's by-target CSR by ranking every
    entry against every other in one wavefront: with the hub among the rows one call takes a large fraction of a second)."""
    from grapes_amd import ops
    from grapes_amd.modules.sage import NeighborSampler
    from grapes_amd.modules.sampling import union_of_lists
    from grapes_amd.modules.vrgcn import layer_inputs
    dev = g.device
    s = NeighborSampler(g, FANOUTS, seed=seed)
    b = s.sample(targets)
    s.check()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lay = layer_inputs(vg, b, 0, status)
    gen = torch.Generator(device=dev); gen.manual_seed(seed)
    n_local, N = b.num_nodes, g.num_nodes
    H = torch.randn(n_local, WIDTH, device=dev, generator=gen)
    hbar = torch.randn(N, WIDTH, device=dev, generator=gen)
    rows, rows_l = lay.rows_g, lay.rows_l
    out = torch.empty((rows.numel(), WIDTH), dtype=torch.float32, device=dev)

    def fused():
        return ops.vrgcn_aggregate_fwd(H, b.node_idx, hbar, vg.dinv, vg.rowptr, vg.col, rows, rows_l, lay.prep, item_cap=lay.item_cap,
                                       want_coef=False, out=out, status=status)[0]

    ei = b.edge_index[0]
    es, ed = ei[0].contiguous(), ei[1].contiguous()
    prep_k = ops.PreparedGraph(es, ed, n_local)
    ws_k = ops.WeightedStructure(prep_k, es, ed)
    deg = (vg.rowptr[1:] - vg.rowptr[:-1]).to(torch.float32)
    gu, gv = b.node_idx[ed.long()].long(), b.node_idx[es.long()].long()
    k_u = torch.bincount(ed.long(), minlength=n_local).to(torch.float32)[ed.long()]
    vals_k = ops.wgcn_weights(ws_k, (deg[gu] / k_u * vg.dinv[gu] * vg.dinv[gv]).contiguous(), mode=ops.WGCN_UNNORMALIZED)
    du = vg.dinv[rows.long()][:, None].contiguous()

    def structure():
        eoff, d_e = ops.frontier_offsets(g.rowptr, rows)
        deg_sum = int(d_e.item())
        row_e, nb_e, _ = ops.frontier_expand(g.rowptr, g.col, rows, eoff, deg_sum, status=status)
        closure = union_of_lists(g, [rows, nb_e], status)                # leaves node_map[id] = rank in the closure
        prep = ops.PreparedGraph(ops.tensormap_map(g.node_map, nb_e), ops.tensormap_map(g.node_map, row_e), closure.numel())
        return closure, prep, ops.tensormap_map(g.node_map, rows)

    def aggregations(closure, prep, rows_c):
        hs = ops.scale_rows(ops.gather_rows(hbar, closure), vg.dinv[closure.long()].contiguous())
        full = ops.gcn_aggregate_fwd_prescaled(hs, prep)                 # dinv_u (sum dinv_v Hbar[v] + dinv_u Hbar[u]) on the rows
        diff = H - ops.gather_rows(hbar, b.node_idx)
        kept = ops.wgcn_aggregate_fwd(diff, ws_k, vals_k)
        return full[rows_c.long()] + (kept[rows_l.long()] + du * du * diff[rows_l.long()])

    ready = structure()
    ref = aggregations(*ready)
    agree = float((fused() - ref).abs().max() / ref.abs().max())
    variants = {"fused": fused, "emulation_aggregations_only": lambda: aggregations(*ready)}
    total = lambda: aggregations(*structure())
    if total_single_calls:
        st = _alternate(torch, variants, a.reps, a.inner)
        st["emulation_total"] = _alternate(torch, {"t": total}, total_single_calls, 1, warm=1)["t"]
        st["emulation_total"]["form"] = f"median of {total_single_calls} single calls"
    else:
        st = _alternate(torch, dict(variants, emulation_total=total), a.reps, a.inner)
    d = g.rowptr[rows.long() + 1] - g.rowptr[rows.long()]
    return {"rows": int(rows.numel()), "batch_nodes": int(n_local), "kept_entries": int(es.numel()), "entries_of_the_rows": int(d.sum().item()),
            "max_row_entries": int(d.max().item()), "long_row_chunks": int(lay.item_cap), "closure_nodes": int(ready[0].numel()),
            "max_rel_difference_to_emulation": agree, **st,
            "ratio_fused_to_emulation_total": round(st["fused"]["median_us"] / st["emulation_total"]["median_us"], 4),
            "ratio_fused_to_aggregations_only": round(st["fused"]["median_us"] / st["emulation_aggregations_only"]["median_us"], 4)}


def bench_steps(torch, a, g0, d, targets):
    from grapes_amd import graphsage, vrgcn
    x, y = d.x.contiguous(), d.y
    vr_model = vrgcn.build_model(x.shape[1], WIDTH, d.num_classes, 2, g0.device)
    sage_model = graphsage.build_model(x.shape[1], WIDTH, d.num_classes, 2, 0.0, "mean", g0.device)
    trainers = {"vrgcn_2_2": vrgcn.VrgcnTrainer(g0, x, y, vr_model, torch.optim.Adam(vr_model.parameters(), lr=1e-3), fanouts=FANOUTS, seed=1),
                "graphsage_25_10": graphsage.SageTrainer(g0, x, y, sage_model, torch.optim.Adam(sage_model.parameters(), lr=1e-3),
                                                          fanouts=SAGE_FANOUTS, seed=1)}
    wall, nodes = {name: [] for name in trainers}, {}
    for i in range(3 + a.reps):
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
                       "batch_nodes": nodes[name]}
    steps["ratio_vrgcn_to_sage"] = round(steps["vrgcn_2_2"]["median_ms"] / steps["graphsage_25_10"]["median_ms"], 3)
    return {"unit": "ms per eager step, host wall to a device synchronise", "hidden_dim": WIDTH, "steps": steps}


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vrgcn.py measures on the GPU; none is visible")
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.vrgcn import VRGraph
    from grapes_amd.vrgcn import loop_free
    torch.manual_seed(0)                                                 # (the targets' permutation)
    d = synthetic_data("products", seed=0)
    g0 = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    g = loop_free(g0)
    vg = VRGraph(g)
    deg = g.rowptr[1:] - g.rowptr[:-1]
    hub = int(deg.argmax().item())
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    train = train[train != hub]
    targets = train[torch.randperm(train.numel(), device=train.device)[:BATCH]].to(torch.int32)
    with_hub = targets.clone()
    with_hub[0] = hub
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic), loop-free",
           "nodes": int(g.num_nodes), "entries": int(g.nnz), "hub_row_entries": int(deg.max().item()), "batch_size": BATCH,
           "fanouts": list(FANOUTS), "width": WIDTH, "unit": "us per call (host launches included), median of reps"}
    res["forward_without_hub"] = forward_case(torch, a, g, vg, targets, seed=1)
    print(json.dumps(res["forward_without_hub"]), file=sys.stderr, flush=True)
    res["forward_with_hub"] = forward_case(torch, a, g, vg, with_hub, seed=1, total_single_calls=5)
    print(json.dumps(res["forward_with_hub"]), file=sys.stderr, flush=True)
    res["hub_row_cost_us"] = round(res["forward_with_hub"]["fused"]["median_us"] - res["forward_without_hub"]["fused"]["median_us"], 2)
    res["step"] = bench_steps(torch, a, g0, d, targets)
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
