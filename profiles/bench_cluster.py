#!/usr/bin/env python3
"""Cluster-GCN: the cluster-union batch's six launches, the same node set through the existing induced-subgraph path, ClusterGCNConv
beside its emulation on SAGEConv's kernels, and one eager training step against GraphSAGE's.

      python profiles/bench_cluster.py [--reps 21] [--inner 200] [--out profiles/cluster_bench.json]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_cluster.py --trace_calls 200

The products-shaped synthetic graph, P = N // 160 clusters, q = 32 clusters per batch (about 5 000 rows), everything in one process.

(a) ops.cluster_batch into preallocated buffers under the `range` and the `random` partition, for two cluster lists each: 32 clusters
    without the hub (the node of the most entries), and the same list with its first cluster replaced by the hub's.  A repetition is
    `inner` calls between two device events, the configurations alternating in every repetition; the figure kept is the median over
    `reps` repetitions after a warm-up, with the quartiles, the smallest and the largest repetition beside it; host launches are
    included.  Every call takes a new serial and runs under ClusterLoader's capacities (the q largest clusters' rows and work
    items).  rows / entries walked / edges kept describe the batch.
(b) The same node set through the existing path: an N-sized node map filled with torch (node_map[node_idx] = arange(n)) plus
    ops.saint_subgraph with edge ids, timed the same way in the same alternation, wherever n <= ops.SAINT_MAX_IDS; a list of 128
    clusters (about 20 000 rows) shows where that path stops.  The stated comparison: on the hub batch cluster_batch must not be
    slower than this path's median by more than the larger of the two configurations' own max - min over their repetitions.
(c) ClusterGCNConv(100 -> 256) forward and forward + backward in both operand forms on the hub batch of the range partition,
    against the emulation — SAGEConv's aggregation kernels with loops = ones plus an elementwise diag_lambda term, the project's
    Linear around them — and against SAGEConv itself; host wall time to a device synchronise.
(d) One eager ClusterTrainer.step against SageTrainer.step (fanouts 10 / 10, 512 targets) in the same process, timed the same way.

--trace_calls N runs N cluster_batch calls on the hub batch of the range partition and nothing else, for a kernel trace in a run of
its own.

Not measured: a captured step (none exists), other graphs, partitions of METIS quality (none is built), other widths."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

Q, Q_LARGE, ROWS_PER_CLUSTER = 32, 128, 160
F_IN, F_OUT, LAMBDA = 100, 256, 0.5
E_CAP = 1 << 22                     # edge buffers: far above what a batch here holds (the status word is checked)


def _stats(v, unit="us", digits=2):
    q = statistics.quantiles(v, n=4)
    return {f"median_{unit}": round(statistics.median(v), digits), f"q1_{unit}": round(q[0], digits), f"q3_{unit}": round(q[2], digits),
            f"min_{unit}": round(min(v), digits), f"max_{unit}": round(max(v), digits)}


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


def _wall(torch, variants, reps):
    """{name: stats in ms} of host wall time to a device synchronise, in a shuffled order every round, after 3 calls each."""
    wall = {name: [] for name in variants}
    names, rng = list(variants), random.Random(0)
    for i in range(3 + reps):
        rng.shuffle(names)                                                # a new order every round: no variant always follows the same one
        for name in names:
            fn = variants[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 3:
                wall[name].append(1e3 * (time.perf_counter() - t0))
    return {name: _stats(v, "ms", 3) for name, v in wall.items()}


class Batcher:
    """ops.cluster_batch over one ClusterData into preallocated buffers, with a loader's membership table and serials."""

    def __init__(self, torch, ops, cd, q, status):
        top = lambda t: max(1, int(torch.sort(t, descending=True)[0][:q].sum().item()))       # ClusterLoader's capacities for q clusters
        self.torch, self.ops, self.cd, self.status = torch, ops, cd, status
        self.n_cap, self.item_cap = top(cd.sizes), top(cd.items)
        self.stamp = torch.zeros((cd.num_parts, 2), dtype=torch.int32, device=cd.graph.device)
        self.serial = 0

    def call(self, clusters, out=None):
        g, cd = self.cd.graph, self.cd
        self.serial += 1
        return self.ops.cluster_batch(g.rowptr, g.col, g.num_nodes, cd.perm, cd.partptr, cd.where, clusters, self.stamp, self.serial,
                                      self.n_cap, E_CAP, item_cap=self.item_cap, status=self.status, out=out)

    def closure(self, clusters):
        """(fn, info, node_idx [n]) of one cluster list."""
        out = self.call(clusters)
        n, e = int(out[5].item()), int(out[6].item())
        g = self.cd.graph
        deg = g.rowptr[1:] - g.rowptr[:-1]
        rows = out[1][:n].long()
        info = {"rows": n, "entries_walked": int(deg[rows].sum().item()), "edges_kept": e, "longest_row": int(deg[rows].max().item())}
        return (lambda: self.call(clusters, out)), info, out[1][:n].clone(), out[3][:, :e].clone()


def cluster_lists(torch, cd, hub, q):
    """(without_hub, with_hub): q clusters that leave the hub's out, and the same list with its first cluster replaced by the hub's."""
    c_hub = int(cd.part[hub].item())
    gen = torch.Generator(); gen.manual_seed(5)
    order = torch.randperm(cd.num_parts, generator=gen)
    plain = order[order != c_hub][:q].to(torch.int32)
    with_hub = plain.clone(); with_hub[0] = c_hub
    dev = cd.graph.device
    return plain.to(dev).contiguous(), with_hub.to(dev).contiguous()


def existing_path(torch, ops, g, node_idx, status):
    """The same node set through an N-sized node map and ops.saint_subgraph (edge ids formed, as cluster_batch forms them)."""
    n = node_idx.numel()
    count = torch.tensor([n], dtype=torch.int32, device=g.device)
    ar = torch.arange(n, dtype=torch.int32, device=g.device)
    idx = node_idx.long()
    out = ops.saint_subgraph(g.rowptr, g.col, node_idx, count, g.node_map, E_CAP, ids=True, status=status)

    def fn():
        g.node_map[idx] = ar
        ops.saint_subgraph(g.rowptr, g.col, node_idx, count, g.node_map, E_CAP, ids=True, status=status, out=out)
    fn()
    return fn, int(out[2].item())


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster.py measures on the GPU; none is visible")
    from grapes_amd import clustergcn, graphsage, ops
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.cluster import ClusterData
    from grapes_amd.modules.gcn import ClusterGCNConv, Linear, SAGEConv
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    dev = g.device
    deg = g.rowptr[1:] - g.rowptr[:-1]
    hub = int(torch.argmax(deg).item())
    P = g.num_nodes // ROWS_PER_CLUSTER
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    parts = {m: ClusterData(g, P, method=m, seed=3) for m in ("range", "random")}
    batchers = {m: Batcher(torch, ops, cd, Q, status) for m, cd in parts.items()}
    if a.trace_calls:
        fn = batchers["range"].closure(cluster_lists(torch, parts["range"], hub, Q)[1])[0]
        for _ in range(a.trace_calls):
            fn()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic)",
           "nodes": int(g.num_nodes), "entries": int(g.nnz), "num_parts": P, "clusters_per_batch": Q, "hub": hub,
           "hub_entries": int(deg[hub].item()), "saint_subgraph_stops_at_nodes": ops.SAINT_MAX_IDS,
           "units": {"batch": "us per call (host launches included), median of reps; min / max are the smallest and largest repetition",
                     "wall": "ms of host wall time to a device synchronise"}, "batch": {}}
    calls, info, keep = {}, {}, {}
    for m, cd in parts.items():
        for name, clusters in zip(("without_hub", "with_hub"), cluster_lists(torch, cd, hub, Q)):
            fn, inf, node_idx, ei = batchers[m].closure(clusters)
            calls[f"{m}/{name}/cluster_batch"], info[f"{m}/{name}"] = fn, inf
            old, e_old = existing_path(torch, ops, g, node_idx, status)
            assert e_old == inf["edges_kept"], (e_old, inf)
            calls[f"{m}/{name}/node_map+saint_subgraph"] = old
            keep[f"{m}/{name}"] = (clusters, node_idx, ei)
    st = _alternate(torch, calls, a.reps, a.inner)
    for key, inf in info.items():
        new, old = st[key + "/cluster_batch"], st[key + "/node_map+saint_subgraph"]
        res["batch"][key] = {**inf, "n_cap": batchers[key.split("/")[0]].n_cap, "item_cap": batchers[key.split("/")[0]].item_cap,
                             "cluster_batch": new, "node_map+saint_subgraph": old,
                             "ratio_existing_to_cluster_batch": round(old["median_us"] / new["median_us"], 3)}
    # the stated comparison, on the hub batches
    res["comparison"] = {}
    for m in parts:
        e = res["batch"][f"{m}/with_hub"]
        new, old = e["cluster_batch"], e["node_map+saint_subgraph"]
        margin = max(new["max_us"] - new["min_us"], old["max_us"] - old["min_us"])
        res["comparison"][m] = {"cluster_batch_median_us": new["median_us"], "existing_median_us": old["median_us"],
                                "margin_us": round(margin, 2), "holds": bool(new["median_us"] <= old["median_us"] + margin)}
    # past the existing path's limit
    cd = parts["range"]
    big = cluster_lists(torch, cd, hub, Q_LARGE)[1]
    large = Batcher(torch, ops, cd, Q_LARGE, status)
    fn, inf, node_idx, _ = large.closure(big)
    res["past_the_limit"] = {**inf, "clusters": Q_LARGE, "n_cap": large.n_cap, "item_cap": large.item_cap, "cluster_batch": _alternate(torch, {"x": fn}, a.reps, a.inner)["x"],
                             "node_map+saint_subgraph": f"not run: {inf['rows']} rows exceed its {ops.SAINT_MAX_IDS} ids"}
    if int(status.item()):
        raise SystemExit(f"bench_cluster.py: status {int(status.item())} after the batch calls")
    print(json.dumps({k: res[k] for k in ("batch", "comparison", "past_the_limit")}), file=sys.stderr, flush=True)

    # (c) the layer on the hub batch of the range partition
    _, node_idx, ei = keep["range/with_hub"]
    n = node_idx.numel()
    x = ops.gather_rows(d.x.contiguous(), node_idx)
    torch.manual_seed(0)
    conv, sage = ClusterGCNConv(F_IN, F_OUT, diag_lambda=LAMBDA).to(dev), SAGEConv(F_IN, F_OUT).to(dev)
    prep = ops.PreparedGraph(ei[0].contiguous(), ei[1].contiguous(), n)
    prep.loops = torch.ones(n, dtype=torch.int32, device=dev)
    dinv = (1.0 / (1 + (prep.rowptr_t[1:] - prep.rowptr_t[:-1]))).float()[:, None]
    lin_t, lin_a = Linear(F_IN, 2 * F_OUT).to(dev), Linear(2 * F_IN, F_OUT).to(dev)

    class SageAgg(torch.autograd.Function):
        @staticmethod
        def forward(ctx, src):
            return ops.sage_aggregate_fwd(src, prep, "mean")

        @staticmethod
        def backward(ctx, dout):
            return ops.sage_aggregate_bwd(dout.contiguous(), prep, "mean")[0]

    def emulate(form, xin):
        if form == "transform":
            h = lin_t(xin)
            hl = h[:, :F_OUT].contiguous()
            return torch.relu(SageAgg.apply(hl) + LAMBDA * dinv * hl + h[:, F_OUT:])
        return lin_a(torch.cat([SageAgg.apply(xin) + LAMBDA * dinv * xin, xin], 1), relu=True)

    gout = torch.randn(n, F_OUT, device=dev)

    def layer(f, train):
        def run():
            if not train:
                with torch.no_grad():
                    f(x)
                return
            xin = x.detach().requires_grad_(True)
            f(xin).backward(gout)
        return run
    variants = {}
    for train in (False, True):
        tag = "fwd+bwd" if train else "fwd"
        for form in ("transform", "aggregate"):
            variants[f"ClusterGCNConv/{form}/{tag}"] = layer(lambda t, form=form: conv(t, ei, relu=True, _form=form), train)
            variants[f"emulation/{form}/{tag}"] = layer(lambda t, form=form: emulate(form, t), train)
            variants[f"SAGEConv/{form}/{tag}"] = layer(lambda t, form=form: sage(t, ei, relu=True, _form=form), train)
    res["layer"] = {"rows": n, "edges": int(ei.shape[1]), "in": F_IN, "out": F_OUT, "diag_lambda": LAMBDA, **_wall(torch, variants, a.reps)}
    print(json.dumps(res["layer"]), file=sys.stderr, flush=True)

    # (d) one eager step beside GraphSAGE's
    xs, y = d.x.contiguous(), d.y
    m_cl = clustergcn.build_model(xs.shape[1], F_OUT, d.num_classes, 2, 0.0, 0.0, dev)
    m_sg = graphsage.build_model(xs.shape[1], F_OUT, d.num_classes, 2, 0.0, "mean", dev)
    t_cl = clustergcn.ClusterTrainer(parts["range"], xs, y, d.train_mask, m_cl, torch.optim.Adam(m_cl.parameters(), lr=1e-3), batch_size=Q, seed=1)
    t_sg = graphsage.SageTrainer(g, xs, y, m_sg, torch.optim.Adam(m_sg.parameters(), lr=1e-3), fanouts=(10, 10), seed=1)
    clusters = keep["range/with_hub"][0]
    targets = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)[:512]
    nodes = {}

    def step(name, tr, arg):
        def run():
            nodes[name] = int(tr.step(arg)[1].num_nodes)
        return run
    steps = _wall(torch, {"cluster_gcn": step("cluster_gcn", t_cl, clusters), "graphsage": step("graphsage", t_sg, targets)}, a.reps)
    for name in ("cluster_gcn", "graphsage"):
        steps[name]["batch_nodes_last_step"] = nodes[name]
    steps["ratio_cluster_to_sage"] = round(steps["cluster_gcn"]["median_ms"] / steps["graphsage"]["median_ms"], 3)
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
