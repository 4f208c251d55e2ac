#!/usr/bin/env python3
"""The label-propagation partitioner at graph scale: one round and its parts, the cut, a gather-only pass beside them, what thirty
rounds do to the cut and to a Cluster-GCN batch, and one trainer step before and after.

      python profiles/bench_partition.py [--reps 11] [--rounds 30] [--out profiles/partition_bench.json]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_partition.py --trace_rounds 5
      python profiles/bench_partition.py --merge_trace <dir> --out profiles/partition_bench.json

Two graphs of 2 449 029 nodes, P = N // 160 = 15 306 clusters, cap = ceil(N / P) + floor(0.1 N / P), a balanced random start:
the products-shaped synthetic (random endpoints under the benchmark's degree statistics: NO planted structure) and a planted graph
built on the device (node v in group v % P; 4 partners drawn inside its group and 1 anywhere, every pair stored in both rows).

(a) ops.partition_propose, ops.partition_admit (part and size put back before every call), ops.partition_cut on the start, and
    torch.index_select(part, 0, col) — the gather of part[col[j]] over every stored entry and nothing else, the memory floor of the
    proposal, except that it also WRITES 4 bytes per entry.  One call between two device events, the calls alternating in every
    repetition; the median over `reps` repetitions with quartiles, smallest and largest; host launches included.
(b) refine_partition(rounds): the cuts, the round kept, the largest cluster, host wall time.
(c) The kept-entry fraction of q = 32 batches — the first 8 batches of one seeded permutation of the clusters — under the start and
    under the refined assignment: edges kept / entries walked.
(d) One eager ClusterTrainer.step (2 layers, 256 hidden, the products features and labels on both graphs) on the same 32 clusters
    before and after; host wall time to a device synchronise.

--trace_rounds N runs N rounds (propose, admit, cut) from the random start on the products-shaped graph and nothing else, for a
kernel trace in a run of its own; --merge_trace DIR adds that run's per-kernel figures to the json.

Not measured: other cluster counts, other graphs, a captured form (none exists)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

Q, ROWS_PER_CLUSTER, BATCHES = 32, 160, 8


def _stats(v, unit="us", digits=2):
    q = statistics.quantiles(v, n=4)
    return {f"median_{unit}": round(statistics.median(v), digits), f"q1_{unit}": round(q[0], digits), f"q3_{unit}": round(q[2], digits),
            f"min_{unit}": round(min(v), digits), f"max_{unit}": round(max(v), digits)}


def _alternate(torch, variants, reps):
    """{name: stats} of (before, fn) pairs: `before` runs outside the timed span, one fn call between two device events."""
    times = {name: [] for name in variants}
    for i in range(3 + reps):
        for name, (before, fn) in variants.items():
            before()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if i >= 3:
                times[name].append(t0.elapsed_time(t1) * 1e3)
    return {name: _stats(v) for name, v in times.items()}


def planted_graph(torch, n, groups, intra, inter, seed, dev):
    gen = torch.Generator(device=dev); gen.manual_seed(seed)
    ar = torch.arange(n, device=dev)
    src = ar.repeat_interleave(intra)
    grp = src % groups
    per = (n - grp + groups - 1) // groups
    dst = grp + groups * (torch.randint(0, 1 << 40, (src.numel(),), device=dev, generator=gen) % per)
    s2 = ar.repeat_interleave(inter)
    d2 = torch.randint(0, n, (s2.numel(),), device=dev, generator=gen)
    a, b = torch.cat([src, s2]), torch.cat([dst, d2])
    keep = a != b
    a, b = a[keep], b[keep]
    rows, cols = torch.cat([a, b]), torch.cat([b, a])
    rows, order = torch.sort(rows, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return rowptr, cols[order].to(torch.int32).contiguous()


def kept_fraction(torch, loader, lists, deg):
    kept = walked = 0
    for clusters in lists:
        b = loader.batch(clusters)
        kept += int(b.edge_index.shape[1])
        walked += int(deg[b.node_idx.long()].sum().item())
    loader.check()
    return {"edges_kept": kept, "entries_walked": walked, "fraction": round(kept / max(walked, 1), 5)}


def step_time(torch, clustergcn, cd, d, clusters, reps):
    dev = cd.graph.device
    torch.manual_seed(0)
    model = clustergcn.build_model(d.x.shape[1], 256, d.num_classes, 2, 0.0, 0.0, dev)
    tr = clustergcn.ClusterTrainer(cd, d.x.contiguous(), d.y, d.train_mask, model, torch.optim.Adam(model.parameters(), lr=1e-3),
                                   batch_size=Q, seed=1)
    wall = []
    for i in range(3 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, b = tr.step(clusters)
        torch.cuda.synchronize()
        if i >= 3:
            wall.append(1e3 * (time.perf_counter() - t0))
    return {**_stats(wall, "ms", 3), "batch_nodes": int(b.num_nodes), "batch_edges": int(b.edge_index.shape[1])}


def merge_trace(a):
    rows = {}
    for f in sorted(glob.glob(os.path.join(a.merge_trace, "**", "*_kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            name = r["Name"].split("(")[0].replace(".kd", "")
            if name.startswith("part_") or name == "grapes_zero_k":
                rows[name] = {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    if not rows:
        raise SystemExit(f"no part_* kernel in a *_kernel_stats.csv under {a.merge_trace}")
    res = json.load(open(a.out))
    res["kernel_trace"] = {"what": "rocprofv3 --kernel-trace --stats over --trace_rounds rounds (propose, admit, cut) from the random start on "
                                   "the products-shaped graph, in a run of its own (kernel time only, no launch gaps)", "kernels": rows}
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def main(a):
    if a.merge_trace:
        return merge_trace(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_partition.py measures on the GPU; none is visible")
    from grapes_amd import clustergcn, ops
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.cluster import ClusterData, ClusterLoader, default_cap, make_partition, refine_partition
    d = synthetic_data("products", seed=0)
    dev = d.rowptr.device
    N = int(d.num_nodes)
    P = N // ROWS_PER_CLUSTER
    cap = default_cap(N, P, 0.1)
    start = make_partition(N, P, "random", 3).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    graphs = {"products (synthetic, no planted structure)": DeviceGraph(d.rowptr, d.col, N)}
    if a.trace_rounds:
        g = graphs["products (synthetic, no planted structure)"]
        part = start.to(torch.int32).contiguous()
        size = torch.bincount(start, minlength=P).to(torch.int32)
        for _ in range(a.trace_rounds):
            want, gain = ops.partition_propose(g.rowptr, g.col, N, part, P, status=status)
            ops.partition_admit(want, gain, part, size, cap, status=status)
            ops.partition_cut(g.rowptr, g.col, N, part, P, status=status)
        torch.cuda.synchronize()
        return
    graphs["planted (4 + 1 partners per node, groups = clusters)"] = DeviceGraph(*planted_graph(torch, N, P, 4, 1, 7, dev), N)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "nodes": N, "num_parts": P, "cap": cap, "clusters_per_batch": Q,
           "rounds": a.rounds,
           "units": {"round": "us per call (host launches included), median of reps", "wall": "ms of host wall time to a device synchronise"},
           "graphs": {}}
    gen = torch.Generator(); gen.manual_seed(5)
    order = torch.randperm(P, generator=gen)
    lists = [order[i * Q:(i + 1) * Q] for i in range(BATCHES)]
    for name, g in graphs.items():
        deg = g.rowptr[1:] - g.rowptr[:-1]
        part0 = start.to(torch.int32).contiguous()
        size0 = torch.bincount(start, minlength=P).to(torch.int32)
        part, size = part0.clone(), size0.clone()
        want, gain = ops.partition_propose(g.rowptr, g.col, N, part0, P, status=status)
        moved, cut = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
        gathered = torch.empty(g.nnz, dtype=torch.int32, device=dev)

        def restore():
            part.copy_(part0); size.copy_(size0)
        nothing = lambda: None                                              # noqa: E731
        variants = {
            "partition_propose": (nothing, lambda: ops.partition_propose(g.rowptr, g.col, N, part0, P, status=status, out=(want, gain))),
            "partition_admit": (restore, lambda: ops.partition_admit(want, gain, part, size, cap, status=status, moved=moved)),
            "partition_cut": (nothing, lambda: ops.partition_cut(g.rowptr, g.col, N, part0, P, status=status, out=cut)),
            "gather_only (index_select(part, col), writes 4 B per entry too)": (nothing, lambda: torch.index_select(part0, 0, g.col, out=gathered)),
        }
        entry = {"entries": int(g.nnz), "longest_row": int(deg.max().item()), "rows_above_64": int((deg > 64).sum().item()),
                 "rows_above_2048": int((deg > ops.PARTITION_LDS_ROW).sum().item()), **_alternate(torch, variants, a.reps)}
        entry["round_1"] = {"proposers": int((want >= 0).sum().item()), "moved": int(moved.item()), "cut_start": int(cut.item())}
        del gathered
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        refined, info = refine_partition(g, start, P, rounds=a.rounds, imbalance=0.1)
        torch.cuda.synchronize()
        entry["refine"] = {"wall_ms": round(1e3 * (time.perf_counter() - t0), 1), "rounds_run": len(info["moved"]), "round_kept": info["round"],
                           "cut_start": info["cuts"][0], "cut_final": info["cuts"][info["round"]],
                           "cut_fraction_start": round(info["cuts"][0] / g.nnz, 4),
                           "cut_fraction_final": round(info["cuts"][info["round"]] / g.nnz, 4), "moved_per_round": info["moved"],
                           "largest_cluster": info["max_size"]}
        cds = {"before": ClusterData(g, P, part=start), "after": ClusterData(g, P, part=refined)}
        entry["kept_entries_q32"] = {k: kept_fraction(torch, ClusterLoader(cd, Q, seed=1), lists, deg) for k, cd in cds.items()}
        entry["trainer_step"] = {k: step_time(torch, clustergcn, cd, d, lists[0], a.reps) for k, cd in cds.items()}
        if int(status.item()):
            raise SystemExit(f"bench_partition.py: status {int(status.item())} on {name}")
        res["graphs"][name] = entry
        print(json.dumps({name: entry}), file=sys.stderr, flush=True)
        del cds
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--trace_rounds", type=int, default=0)
    ap.add_argument("--merge_trace", default=None)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
