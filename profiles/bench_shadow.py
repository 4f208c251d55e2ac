#!/usr/bin/env python3
"""ShaDow-GNN: the ego-net sampler's three launches, the nearest existing work beside them, and one eager training step against
GraphSAGE's.

      python profiles/bench_shadow.py [--reps 21] [--inner 200] [--out profiles/shadow_bench.json]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_shadow.py --trace_calls 200

The products-shaped synthetic graph, batch 512, depth 2, everything in one process.

Sampler.  ops.shadow_sample at num_neighbors 5, 10 and 25 into preallocated buffers, for two root sets: 512 random training nodes
whose ego-nets do not reach the hub (the node of the most entries), and the same set with its first 64 roots replaced by the hub and
63 nodes that store it — the hub is then a member of ego-nets, and its whole row is walked where their induced entries are counted
and written.  A repetition is `inner` calls between two device events, the root sets alternating in every repetition; the figure
kept is the median over `reps` repetitions after a warm-up, with the quartiles beside it; host launches are included.  "entries
walked" is the sum over every member of every ego-net of its row's entries: the count launch reads each once and the write launch
once more; the rate given is that sum over the call's time (both passes and the hops inside it).

The shared-scope analogue — not an equal: it builds ONE neighbourhood for the whole batch where the ego-net sampler builds 512 —
is a NeighborSampler batch at fanouts (k, k) plus ONE ops.saint_subgraph over its union where the union fits that call's
ops.SAINT_MAX_IDS ids; where it does not, the sampler is timed alone and the entry says so.  Both, and ShaDowKHopSampler.sample, are
timed as host wall time to a device synchronise, their host reads included; median of `reps` calls after 3.

Step.  ShadowTrainer.step (depth 2, num_neighbors 10, three SAGE layers of 256 columns, pooled readout) against SageTrainer.step
(fanouts 10 / 10, two layers) on the same targets, timed the same way.

--trace_calls N runs N sampler calls at num_neighbors 10 on the hub set and nothing else, for a kernel trace in a run of its own.

Not measured: a captured step (none exists), other graphs, depths or widths."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, BATCH, DEPTH = 256, 512, 2
FANOUTS = (5, 10, 25)
HUB_ROOTS = 64
E_CAP = 1 << 24                     # edge buffers: far above what a batch here holds (the status word is checked)


def _stats(v, unit="us", digits=2):
    q = statistics.quantiles(v, n=4)
    return {f"median_{unit}": round(statistics.median(v), digits), f"q1_{unit}": round(q[0], digits), f"q3_{unit}": round(q[2], digits)}


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
    """{name: stats in ms} of host wall time to a device synchronise, alternating, after 3 calls each."""
    wall = {name: [] for name in variants}
    for i in range(3 + reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 3:
                wall[name].append(1e3 * (time.perf_counter() - t0))
    return {name: _stats(v, "ms", 3) for name, v in wall.items()}


def root_sets(torch, g, train):
    """(plain, with_hub, hub): BATCH training nodes farther than DEPTH hops from the hub, whose ego-nets therefore never hold it, and
    the same list with its head replaced by the hub and nodes that store it."""
    deg = g.rowptr[1:] - g.rowptr[:-1]
    hub = int(torch.argmax(deg).item())
    cand = train[torch.randperm(train.numel(), device=train.device)[:8 * BATCH]]
    at = torch.nonzero(g.col == hub, as_tuple=False).reshape(-1)                          # entries that name the hub -> their rows
    storing = torch.unique(torch.searchsorted(g.rowptr, at, right=True) - 1)
    near = torch.zeros(g.num_nodes, dtype=torch.bool, device=g.device)                    # the hub and the nodes one hop from reaching it
    near[storing] = True
    near[hub] = True
    cdeg = deg[cand]
    owner = torch.repeat_interleave(torch.arange(cand.numel(), device=g.device), cdeg)
    first = torch.repeat_interleave(g.rowptr[cand] - (torch.cumsum(cdeg, 0) - cdeg), cdeg)
    entries = g.col[(torch.arange(owner.numel(), device=g.device) + first).long()].long()
    holds = near[cand].clone()
    holds[owner[near[entries]]] = True                                                    # within DEPTH = 2 hops of the hub: left out
    plain = cand[~holds][:BATCH].to(torch.int32).contiguous()
    if plain.numel() < BATCH:
        raise SystemExit("bench_shadow.py: too few training nodes far from the hub")
    storing = storing[storing != hub][:HUB_ROOTS - 1]
    with_hub = torch.cat([torch.tensor([hub], dtype=torch.int32, device=g.device), storing.to(torch.int32),
                          plain[HUB_ROOTS - 1 + 1:]])[:BATCH].contiguous()
    return plain, with_hub, hub


def sampler_call(ops, g, roots, k, hub, seed=1):
    """A closure over preallocated buffers, and what one call holds."""
    out = ops.shadow_sample(g.rowptr, g.col, g.num_nodes, roots, DEPTH, k, e_cap=E_CAP, philox_seed=seed, want_e_id=True)
    n, e = int(out[6].item()), int(out[7].item())
    deg = g.rowptr[1:] - g.rowptr[:-1]
    walked = int(deg[out[0][:n].long()].sum().item())
    sizes = (out[1][1:] - out[1][:-1])
    info = {"nodes": n, "entries": e, "largest_ego_net": int(sizes.max().item()), "member_row_entries": walked,
            "longest_member_row": int(deg[out[0][:n].long()].max().item()), "ego_nets_with_hub": int((out[0][:n] == hub).sum().item())}
    return (lambda: ops.shadow_sample(g.rowptr, g.col, g.num_nodes, roots, DEPTH, k, e_cap=E_CAP, philox_seed=seed, out=out)), info


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_shadow.py measures on the GPU; none is visible")
    from grapes_amd import graphsage, ops, shadow
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.sage import NeighborSampler
    from grapes_amd.modules.shadow import ShaDow, ShaDowKHopSampler
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    plain, with_hub, hub = root_sets(torch, g, train)
    if a.trace_calls:
        fn, _ = sampler_call(ops, g, with_hub, 10, hub)
        for _ in range(a.trace_calls):
            fn()
        torch.cuda.synchronize()
        return
    x, y = d.x.contiguous(), d.y
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic)",
           "nodes": int(g.num_nodes), "entries": int(g.nnz), "batch_size": BATCH, "depth": DEPTH, "hub": hub,
           "hub_entries": int((g.rowptr[hub + 1] - g.rowptr[hub]).item()), "hub_roots": HUB_ROOTS,
           "units": {"sampler": "us per ops.shadow_sample call (three launches, host launches included), median of reps",
                     "wall": "ms of host wall time to a device synchronise, host reads included"}, "num_neighbors": {}}
    for k in FANOUTS:
        calls, info = {}, {}
        for name, roots in (("without_hub", plain), ("with_hub", with_hub)):
            calls[name], info[name] = sampler_call(ops, g, roots, k, hub)
        st = _alternate(torch, calls, a.reps, a.inner)
        entry = {"cap": ops.shadow_cap(DEPTH, k)}
        for name in calls:
            t = st[name]["median_us"]
            entry[name] = {**info[name], **st[name], "member_row_entries_per_s": round(info[name]["member_row_entries"] / (t * 1e-6), 0)}
        # the shared-scope analogue and the sampler object, with their host reads
        ns, status = NeighborSampler(g, (k, k), seed=1), torch.zeros(1, dtype=torch.int32, device=g.device)
        sh = ShaDowKHopSampler(g, DEPTH, k, seed=1)

        fits = [True]                                   # saint_subgraph takes at most ops.SAINT_MAX_IDS ids

        def shared_scope():
            b = ns.sample(plain)
            if not fits[0]:
                return b, None
            count = torch.tensor([b.num_nodes], dtype=torch.int32, device=g.device)
            return b, ops.saint_subgraph(g.rowptr, g.col, b.node_idx, count, g.node_map, E_CAP, status=status)
        fits[0] = int(ns.sample(plain).num_nodes) <= ops.SAINT_MAX_IDS
        b, sub = shared_scope()
        entry["shared_scope_analogue"] = {
            "what": f"NeighborSampler(fanouts=({k}, {k})).sample" + (" + ONE saint_subgraph over its union" if fits[0] else
                                                                      f" ALONE: its union exceeds saint_subgraph's {ops.SAINT_MAX_IDS} ids, "
                                                                      "the induced subgraph is not measured"),
            "union_nodes": int(b.num_nodes), "induced_entries": int(sub[2].item()) if fits[0] else None}
        w = _wall(torch, {"shared_scope_analogue": shared_scope, "shadow_sampler_sample": lambda: sh.sample(plain)}, a.reps)
        entry["shared_scope_analogue"].update(w["shared_scope_analogue"])
        entry["shadow_sampler_sample"] = w["shadow_sampler_sample"]
        res["num_neighbors"][str(k)] = entry
        print(json.dumps(entry), file=sys.stderr, flush=True)
    # one eager step beside GraphSAGE's
    torch.manual_seed(0)
    m_sh = ShaDow(x.shape[1], WIDTH, d.num_classes, 3, conv="sage", pool=True).to(g.device)
    m_sg = graphsage.build_model(x.shape[1], WIDTH, d.num_classes, 2, 0.0, "mean", g.device)
    t_sh = shadow.ShadowTrainer(g, x, y, m_sh, torch.optim.Adam(m_sh.parameters(), lr=1e-3), depth=DEPTH, num_neighbors=10, seed=1)
    t_sg = graphsage.SageTrainer(g, x, y, m_sg, torch.optim.Adam(m_sg.parameters(), lr=1e-3), fanouts=(10, 10), seed=1)
    nodes = {}

    def step(name, tr):
        def run():
            nodes[name] = int(tr.step(plain)[1].num_nodes)
        return run
    steps = _wall(torch, {"shadow": step("shadow", t_sh), "graphsage": step("graphsage", t_sg)}, a.reps)
    for name in steps:
        steps[name]["batch_nodes_last_step"] = nodes[name]
    steps["ratio_shadow_to_sage"] = round(steps["shadow"]["median_ms"] / steps["graphsage"]["median_ms"], 3)
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
