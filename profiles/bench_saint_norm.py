"""Wall time of GraphSAINT's coverage estimate (modules/saint.py: estimate_norm) on a synthetic stand-in graph, for rw
(walk_length 2), node and edge at --batch_size and --sample_coverage: ONE call per sampler, timed on the host from before the call
to after a device synchronise (the call reads the running total once per pass, so it is host-paced); the edge sampler's weight
table is built before the clock starts.  Also the passes, batches and sampled nodes of the estimate, the two norm launches timed
with device events, and how many entries took each special value.

Writes one JSON document (--out, else stdout).  One measurement each: no repeats, no spread."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="products")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--num_steps", type=int, default=30)
    ap.add_argument("--sample_coverage", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grapes_amd import ops
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.saint import make_sampler
    d = synthetic_data(a.dataset, seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    res = {"device": torch.cuda.get_device_name(0), "dataset": a.dataset, "nodes": int(d.num_nodes), "entries": int(g.nnz),
           "batch_size": a.batch_size, "num_steps": a.num_steps, "sample_coverage": a.sample_coverage,
           "note": "one call per sampler, host wall time", "samplers": {}}
    for kind in ("rw", "node", "edge"):
        ld = make_sampler(kind, g, a.batch_size, 2, num_steps=a.num_steps, seed=1)
        ld.weights()
        ld.sample()                                        # first launches of the process / the sampler
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ld.estimate_norm(a.sample_coverage)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ld.check()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.saint_norms(g.rowptr, g.num_nodes, ld.node_count, ld.edge_count, ld.num_samples)
        e.record(); e.synchronize()
        en = ld.edge_norm
        r = dict(n_cap=ld.n_cap, estimate_wall_s=round(wall, 4), passes=ld.num_samples // a.num_steps, batches=ld.num_samples,
                 total_sampled_nodes=ld.total_sampled_nodes, ms_per_batch=round(1e3 * wall / ld.num_samples, 4),
                 norms_launch_ms=round(s.elapsed_time(e), 4), nodes_never_sampled=int((ld.node_count == 0).sum().item()),
                 entries_never_counted=int((ld.edge_count[: g.nnz] == 0).sum().item()),
                 edge_norm_at_1e4=int((en[: g.nnz] == 1e4).sum().item()), edge_norm_at_0_1=int((en[: g.nnz] == 0.1).sum().item()))
        res["samplers"][kind] = r
        print(json.dumps({kind: r}), file=sys.stderr)
        del ld
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
