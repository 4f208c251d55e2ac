#!/usr/bin/env python3
"""GNNAutoScale: the resolve on its own, the fused aggregation beside the emulation it replaces, one eager training step beside
Cluster-GCN's and VR-GCN's, and the halo-to-in-batch entry ratio per partition.

      python profiles/bench_gas.py [--reps 21] [--inner 200] [--emu_reps 5] [--out profiles/gas_bench.json]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_gas.py --trace_calls 200

The products-shaped synthetic graph (loop-free copy), P = N // 160 clusters, q = 32 clusters per batch (about 5 000 rows), width
256, everything in one process; the `random`, `range` and `lp` (label propagation, 30 rounds, imbalance 0.1) partitions, for two
cluster lists each: 32 clusters without the hub (the node of the most entries), and the same list with its first cluster replaced
by the hub's.  The method is profiles/bench_cluster.py's: a repetition is `inner` calls between two device events, the variants
alternating in every repetition; the figure kept is the median over `reps` repetitions after a warm-up, host launches included.

(a) ops.gas_resolve into preallocated buffers, after the batch was built (its stamps stay valid: every batch has its own loader).
    in / halo entries and their ratio describe what the partitioner buys.
(b) ops.gas_aggregate_fwd (H and the history read in place) against the emulation it replaces, on the same batch:
      torch.unique of the halo ids, ops.gather_rows of their history rows, torch.cat behind H, ops.PreparedGraph (gcn_prepare) over
      the batch + halo entries, ops.gcn_aggregate_fwd over it
    — an ordinary convolution over batch + halo, as pyg_autoscale runs it; its normalisation is the subgraph's own, so its numbers
    differ from the rule's while its memory walk is the same plus the halo rows' self terms.  `emulation` is all of it,
    `emulation_aggregation_alone` the last call on ready buffers, timed as the fused call is; `emulation` is host wall time to a device
    synchronise over --emu_reps calls (gcn_prepare's rank sort of a by-target row is quadratic in the row, so the hub's row sets its
    time: the JSON has the figure).  The stated comparison: the fused forward against the
    emulation's aggregation alone.
(c) One eager GasTrainer.step against ClusterTrainer.step (same clusters, range partition, hub batch) and VrgcnTrainer.step
    (fanouts 2 / 2, 512 targets); host wall time to a device synchronise.  resolve_share = (a) / the GAS step.

Not measured: a membership test inside the gather instead of the resolve (not built), a captured step (none exists), other
graphs, other widths, partitions of METIS quality (none is built)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cluster import _alternate, _wall, cluster_lists              # noqa: E402

Q, ROWS_PER_CLUSTER, WIDTH = 32, 160, 256


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gas.py measures on the GPU; none is visible")
    from grapes_amd import clustergcn, gas, ops, vrgcn
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.cluster import ClusterData
    from grapes_amd.modules.gas import GasLoader
    from grapes_amd.modules.vrgcn import VRGraph
    d = synthetic_data("products", seed=0)
    g0 = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    g = vrgcn.loop_free(g0)
    dev, N = g.device, g.num_nodes
    deg = g.rowptr[1:] - g.rowptr[:-1]
    hub = int(torch.argmax(deg).item())
    P = N // ROWS_PER_CLUSTER
    vg = VRGraph(g)
    torch.manual_seed(0)
    hbar = torch.randn(N, WIDTH, device=dev)
    parts = {"random": ClusterData(g, P, method="random", seed=3), "range": ClusterData(g, P, method="range"),
             "lp": ClusterData(g, P, method="lp", seed=3)}
    batches = {}
    for m, cd in parts.items():
        for name, clusters in zip(("without_hub", "with_hub"), cluster_lists(torch, cd, hub, Q)):
            L = GasLoader(cd, Q)                                         # its own stamp table: the batch's stamps stay valid
            b = L.batch(clusters)
            L.check()
            batches[f"{m}/{name}"] = (L, b, clusters)

    def fused(b, h, out):
        return lambda: ops.gas_aggregate_fwd(h, hbar, vg.dinv, b.node_idx, b.rowptr_h, b.code, item_cap=b.item_cap, out=out)

    if a.trace_calls:
        _, b, _ = batches["range/with_hub"]
        fn = fused(b, torch.randn(b.num_nodes, WIDTH, device=dev), torch.empty(b.num_nodes, WIDTH, device=dev))
        for _ in range(a.trace_calls):
            fn()
        torch.cuda.synchronize()
        return

    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "emu_reps": a.emu_reps, "dataset": "products (synthetic, loop-free)",
           "nodes": int(N), "entries": int(g.nnz), "num_parts": P, "clusters_per_batch": Q, "width": WIDTH, "hub": hub,
           "hub_entries": int(deg[hub].item()), "lp": {k: parts["lp"].lp_info[k] for k in ("round", "max_size", "cap")},
           "lp_cut": [parts["lp"].lp_info["cuts"][0], parts["lp"].lp_info["cuts"][parts["lp"].lp_info["round"]]],
           "units": {"call": "us per call (host launches included), median of reps; min / max are the smallest and largest repetition",
                     "wall": "ms of host wall time to a device synchronise"},
           "not_measured": "a membership test inside the gather instead of the resolve; a captured step; other widths", "batch": {}}
    for key, (L, b, clusters) in batches.items():
        n, cd, ld = b.num_nodes, L.cluster_data, L.loader
        h = torch.randn(n, WIDTH, device=dev)
        out = torch.empty(n, WIDTH, device=dev)
        r_out = (torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(b.code.numel() + 1, dtype=torch.int32, device=dev),
                 torch.empty(2, dtype=torch.int64, device=dev))
        item_cap = min(max(1, int(cd.items[b.clusters.long()].sum().item())), ops.GAS_ITEM_CAP_MAX)
        serial = ld.serial

        def resolve():
            ops.gas_resolve(g.rowptr, g.col, N, b.node_idx, n, cd.where, ld.stamp, serial, r_out[1].numel(), item_cap=item_cap,
                            status=L.status, out=r_out)

        # the emulation it replaces
        row = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), (b.rowptr_h[1:] - b.rowptr_h[:-1]).long())

        def emulate(parts_only=False):
            out_of = b.code < 0
            halo = torch.unique(-1 - b.code[out_of])
            rows = ops.gather_rows(hbar, halo.to(torch.int32))
            cat = torch.cat([h, rows])
            src = b.code.clone()
            src[out_of] = (n + torch.searchsorted(halo, -1 - b.code[out_of])).to(torch.int32)
            prep = ops.PreparedGraph(src, row, n + halo.numel())
            if parts_only:
                return cat, prep
            return ops.gcn_aggregate_fwd(cat, prep)

        cat, prep = emulate(True)
        e_out = torch.empty_like(cat)
        variants = {"gas_resolve": resolve, "gas_aggregate_fwd": fused(b, h, out),
                    "emulation_aggregation_alone": lambda: ops.gcn_aggregate_fwd(cat, prep, out=e_out)}
        st = _alternate(torch, variants, a.reps, a.inner)
        # (the whole emulation by wall time, `emu_reps` calls: gcn_prepare puts a by-target row into canonical order with ONE
        # wavefront's rank sort, quadratic in the row — it was written for sampled rows — so the hub's row sets its time)
        emu = _wall(torch, {"emulation": emulate}, a.emu_reps)["emulation"]
        st["emulation"] = {k.replace("_ms", "_us"): round(1e3 * v, 1) for k, v in emu.items()}
        if not torch.equal(r_out[1][:b.code.numel()], b.code):
            raise SystemExit(f"bench_gas.py: {key}: the timed resolve wrote other codes than the batch's")
        res["batch"][key] = {"rows": n, "entries": int(b.code.numel()), "in_batch_entries": b.num_in, "halo_entries": b.num_halo,
                             "halo_to_in_batch": round(b.num_halo / max(b.num_in, 1), 2), "halo_nodes": int(cat.shape[0] - n),
                             "longest_row": int((b.rowptr_h[1:] - b.rowptr_h[:-1]).max().item()), "long_row_chunks": b.item_cap, **st,
                             "ratio_emulation_aggregation_alone_to_fused":
                                 round(st["emulation_aggregation_alone"]["median_us"] / st["gas_aggregate_fwd"]["median_us"], 3),
                             "ratio_emulation_to_fused": round(st["emulation"]["median_us"] / st["gas_aggregate_fwd"]["median_us"], 3)}
        print(json.dumps({key: res["batch"][key]}), file=sys.stderr, flush=True)
        del cat, prep, e_out
        L.check()

    # (c) one eager step beside Cluster-GCN's and VR-GCN's
    xs, y = d.x.contiguous(), d.y
    clusters = batches["range/with_hub"][2]
    m_gas = gas.build_model(xs.shape[1], WIDTH, d.num_classes, 2, dev)
    m_cl = clustergcn.build_model(xs.shape[1], WIDTH, d.num_classes, 2, 0.0, 0.0, dev)
    m_vr = vrgcn.build_model(xs.shape[1], WIDTH, d.num_classes, 2, dev)
    t_gas = gas.GasTrainer(g0, xs, y, m_gas, torch.optim.Adam(m_gas.parameters(), lr=1e-3), num_parts=P, batch_size=Q,
                           partition=parts["range"].part, seed=1, train_mask=d.train_mask)
    t_cl = clustergcn.ClusterTrainer(parts["range"], xs, y, d.train_mask, m_cl, torch.optim.Adam(m_cl.parameters(), lr=1e-3), batch_size=Q, seed=1)
    t_vr = vrgcn.VrgcnTrainer(g0, xs, y, m_vr, torch.optim.Adam(m_vr.parameters(), lr=1e-3), fanouts=(2, 2), seed=1)
    targets = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)[:512]
    nodes = {}

    def step(name, tr, arg):
        def run():
            nodes[name] = int(tr.step(arg)[1].num_nodes)
        return run
    steps = _wall(torch, {"gas": step("gas", t_gas, clusters), "cluster_gcn": step("cluster_gcn", t_cl, clusters),
                          "vrgcn": step("vrgcn", t_vr, targets)}, a.reps)
    for name in ("gas", "cluster_gcn", "vrgcn"):
        steps[name]["batch_nodes_last_step"] = nodes[name]
    steps["ratio_gas_to_cluster_gcn"] = round(steps["gas"]["median_ms"] / steps["cluster_gcn"]["median_ms"], 3)
    steps["ratio_gas_to_vrgcn"] = round(steps["gas"]["median_ms"] / steps["vrgcn"]["median_ms"], 3)
    steps["resolve_share_of_gas_step"] = round(res["batch"]["range/with_hub"]["gas_resolve"]["median_us"] / (1e3 * steps["gas"]["median_ms"]), 4)
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
    ap.add_argument("--emu_reps", type=int, default=5)
    ap.add_argument("--trace_calls", type=int, default=0)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
