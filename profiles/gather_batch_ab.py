#!/usr/bin/env python3
"""The aggregation calls whose gather loop moved into gather_batch (csrc/row_gather.h), timed under two builds of the library.

    GRAPES_LIB_PATH=<parent's libgrapes_hip.so> python profiles/gather_batch_ab.py --child parent_a.json
    python profiles/gather_batch_ab.py --child new.json
    GRAPES_LIB_PATH=<parent's libgrapes_hip.so> python profiles/gather_batch_ab.py --child parent_b.json
    python profiles/gather_batch_ab.py --summarize parent_a.json parent_b.json new.json [--round round1] --out profiles/gather_batch_ab.json

One child process per build, one at a time: parent, new, parent.  A child times every call with the method of
profiles/bench_vrgcn.py (_alternate: a repetition is `inner` calls between two device events, host launches included; the median
over `reps` repetitions after a warm-up), at the shapes of the bench scripts, width 256:
  sampled / fullbatch   profiles/bench_gcn2.py's and bench_gat.py's two graphs (1 024 nodes with 16 384 random edges; the
                        arxiv-sized synthetic graph): gcn2_propagate, sage_aggregate (mean), cluster_aggregate and gat_aggregate,
                        forward and backward.  (bench_sage.py and bench_cluster.py time their aggregations inside whole steps on
                        the products-shaped graph; here the two calls run alone on these two graphs.)
  vrgcn                 profiles/bench_vrgcn.py's batches: 512 targets of the products-shaped graph, fanouts (2, 2), layer 0, without
                        and with the hub among the targets; vrgcn_aggregate_fwd / _bwd.
  gas                   profiles/bench_gas.py's range-partition batches (32 clusters of 160 rows), without and with the hub's
                        cluster; gas_aggregate_fwd / _bwd.
The yardstick is the spread between the two parent children of the same call: a call whose new median is no higher than the larger
parent median by more than that spread is unchanged.  profiles/gather_batch_ab.json holds two such rounds side by side (round1,
round2; round2_row_load_first is a third child of round 2, on a build with the other shuffle order in gather_batch, run with
--label new)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WIDTH = 256


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gather_batch_ab.py measures on the GPU; none is visible")
    from bench_cluster import cluster_lists
    from bench_vrgcn import BATCH, FANOUTS, _alternate
    from grapes_amd import ops, synth
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.cluster import ClusterData
    from grapes_amd.modules.gas import GasLoader
    from grapes_amd.modules.sage import NeighborSampler
    from grapes_amd.modules.vrgcn import VRGraph, layer_inputs
    from grapes_amd.vrgcn import loop_free
    dev, f = "cuda", WIDTH
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    res = {}

    def timed(tag, variants):
        for name, st in _alternate(torch, variants, a.reps, a.inner).items():
            res[f"{name}/{tag}"] = st
            print(f"{name}/{tag}: {st['median_us']} us", flush=True)

    for shape in ("sampled", "fullbatch"):
        if shape == "sampled":
            n = 1024
            ei = torch.randint(0, n, (2, 16384), device=dev, generator=gen, dtype=torch.int32)
            prep = ops.PreparedGraph(ei[0].contiguous(), ei[1].contiguous(), n)
            ops.gcn2_attach_loops(prep, ei[0].contiguous(), ei[1].contiguous())
        else:
            n, deg, maxdeg = synth.CONFIGS["arxiv"][:3]
            rowptr, col = synth.synth_graph_device(n, deg, maxdeg, seed=0, device=dev)
            dg = DeviceGraph(rowptr, col, n)
            prep = dg.gcn_prepared()
            prep.loops = ops.gcn2_loop_counts_csr(dg.rowptr, dg.col, n)
        x, x0, g = (torch.randn(n, f, device=dev, generator=gen) for _ in range(3))
        a_s, a_d, b = (0.2 * torch.randn(f, device=dev, generator=gen) for _ in range(3))
        s_src, s_dst = ops.gat_scores(x, a_s, a_d)
        out, row_ms = ops.gat_aggregate_fwd(x, s_src, s_dst, prep, b, False)
        timed(shape, {
            "gcn2_propagate_fwd": lambda: ops.gcn2_propagate_fwd(x, x0, prep, 0.1),
            "gcn2_propagate_bwd": lambda: ops.gcn2_propagate_bwd(g, prep, 0.1),
            "sage_aggregate_fwd": lambda: ops.sage_aggregate_fwd(x, prep, "mean"),
            "sage_aggregate_bwd": lambda: ops.sage_aggregate_bwd(g, prep, "mean"),
            "cluster_aggregate_fwd": lambda: ops.cluster_aggregate_fwd(x, prep, 0.5),
            "cluster_aggregate_bwd": lambda: ops.cluster_aggregate_bwd(g, prep, 0.5),
            "gat_aggregate_fwd": lambda: ops.gat_aggregate_fwd(x, s_src, s_dst, prep, b, False),
            "gat_aggregate_bwd": lambda: ops.gat_aggregate_bwd(g, out, x, s_src, s_dst, row_ms, a_s, a_d, prep, b, False)})
        assert prep.status is None or int(prep.status.item()) == 0

    # the products-shaped graph of bench_vrgcn.py and bench_gas.py
    torch.manual_seed(0)
    d = synthetic_data("products", seed=0)
    g0 = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    gr = loop_free(g0)
    vg = VRGraph(gr)
    N = gr.num_nodes
    deg = gr.rowptr[1:] - gr.rowptr[:-1]
    hub = int(deg.argmax().item())
    hbar = torch.randn(N, f, device=dev, generator=gen)
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    train = train[train != hub]
    targets = train[torch.randperm(train.numel(), device=train.device)[:BATCH]].to(torch.int32)
    with_hub = targets.clone()
    with_hub[0] = hub
    for name, tg in (("without_hub", targets), ("with_hub", with_hub)):
        bt = NeighborSampler(gr, FANOUTS, seed=11).sample(tg)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lay = layer_inputs(vg, bt, 0, status)
        H = torch.randn(bt.num_nodes, f, device=dev, generator=gen)
        m = lay.rows_g.numel()
        out = torch.empty((m, f), dtype=torch.float32, device=dev)
        da = torch.randn(m, f, device=dev, generator=gen)
        _, coef = ops.vrgcn_aggregate_fwd(H, bt.node_idx, hbar, vg.dinv, vg.rowptr, vg.col, lay.rows_g, lay.rows_l, lay.prep,
                                          item_cap=lay.item_cap, status=status)
        timed(f"vrgcn_{name}", {
            "vrgcn_aggregate_fwd": lambda: ops.vrgcn_aggregate_fwd(H, bt.node_idx, hbar, vg.dinv, vg.rowptr, vg.col, lay.rows_g, lay.rows_l,
                                                                   lay.prep, item_cap=lay.item_cap, want_coef=False, out=out, status=status),
            "vrgcn_aggregate_bwd": lambda: ops.vrgcn_aggregate_bwd(da, coef, lay.pos, bt.node_idx, vg.dinv, lay.prep, status=status)})
        assert int(status.item()) == 0
    Q, P = 32, N // 160
    cd = ClusterData(gr, P, method="range")
    for name, clusters in zip(("without_hub", "with_hub"), cluster_lists(torch, cd, hub, Q)):
        L = GasLoader(cd, Q)
        bt = L.batch(clusters)
        L.check()
        n = bt.num_nodes
        h, da = (torch.randn(n, f, device=dev, generator=gen) for _ in range(2))
        out = torch.empty(n, f, device=dev)
        timed(f"gas_range_{name}", {
            "gas_aggregate_fwd": lambda: ops.gas_aggregate_fwd(h, hbar, vg.dinv, bt.node_idx, bt.rowptr_h, bt.code, item_cap=bt.item_cap,
                                                               out=out),
            "gas_aggregate_bwd": lambda: ops.gas_aggregate_bwd(da, bt.node_idx, vg.dinv, bt.prep)})
    torch.cuda.synchronize()
    with open(a.child, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "library": a.label or (os.environ.get("GRAPES_LIB_PATH") and "parent" or "new"),
                   "reps": a.reps, "inner": a.inner, "calls": res}, fh, indent=1)
    print(json.dumps({"written": a.child, "calls": len(res)}))


def summarize(a):
    """One line per call: [q1, median, q3] of each child, and whether the new median is inside the parents' spread.  The round is
    added to --out under --round, beside the rounds already there."""
    pa, pb, new = (json.load(open(p)) for p in a.summarize)
    assert pa["library"] == pb["library"] == "parent" and new["library"] == "new"
    tri = lambda st: [st["q1_us"], st["median_us"], st["q3_us"]]
    calls, above = {}, []
    for k in sorted(new["calls"]):
        ma, mb, mn = pa["calls"][k]["median_us"], pb["calls"][k]["median_us"], new["calls"][k]["median_us"]
        ok = mn <= max(ma, mb) + abs(ma - mb)
        calls[k] = {"parent_a": tri(pa["calls"][k]), "parent_b": tri(pb["calls"][k]), "new": tri(new["calls"][k]), "inside": ok}
        if not ok:
            above.append(k)
        print(f"{k:45s} parent {ma:9.2f} {mb:9.2f}  new {mn:9.2f}  {'ok' if ok else 'ABOVE'}")
    out = json.load(open(a.out)) if os.path.exists(a.out) else {
        "what": __doc__.split("\n\n")[0], "order": "a round is parent, new, parent: one child process at a time",
        "unit": "us per call (host launches included): [first quartile, median, third quartile] over reps repetitions of inner calls",
        "criterion": "inside: new median <= the larger parent median + |parent_a - parent_b|", "device": new["device"],
        "reps": new["reps"], "inner": new["inner"]}
    out[a.round] = {"above_parent_spread": above, "calls": calls}
    with open(a.out, "w") as fh:                                         # (a scalar, a list of names or a call per line)
        lines = []
        for k, v in out.items():
            if isinstance(v, dict):
                rows = ",\n".join(f"   {json.dumps(c)}: {json.dumps(st)}" for c, st in v["calls"].items())
                lines.append(f' {json.dumps(k)}: {{\n  "above_parent_spread": {json.dumps(v["above_parent_spread"])},\n  "calls": {{\n{rows}\n  }}\n }}')
            else:
                lines.append(f" {json.dumps(k)}: {json.dumps(v)}")
        fh.write("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"{a.round}: {len(calls)} calls, {len(above)} above the parents' spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--summarize", nargs=3)
    ap.add_argument("--out", default="profiles/gather_batch_ab.json")
    ap.add_argument("--round", default="round1")
    ap.add_argument("--label", help="what the child's library is called (default: parent with GRAPES_LIB_PATH set, else new)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=100)
    a = ap.parse_args()
    summarize(a) if a.summarize else child(a)
