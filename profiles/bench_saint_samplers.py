"""GraphSAINT's three samplers side by side on the synthetic products-shaped graph (grapes_amd/modules/saint.py, saint.py):

  * the edge sampler's one-time weight table: build time (median / min / max over --builds, device events) and bytes;
  * per-batch sampling time — the draw, the node set and the induced subgraph (sampler.sample()) — for rw (walk_length 2), node
    and edge at --batch_size, median / min / max over --steps calls after --warmup, each call timed alone with device events;
  * the captured trainer's step (GCN(F, [256, C]), lr 0.01): median / min / max over --steps replays after --warmup;
  * batch nodes and induced edges of the last batch.

Writes one JSON document (--out, else stdout).  All three samplers are measured in the same process, one after the other."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, n):
    out = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def _stats(ms, prefix):
    return {f"{prefix}_ms_median": round(statistics.median(ms), 4), f"{prefix}_ms_min": round(min(ms), 4),
            f"{prefix}_ms_max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="products")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--builds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grapes_amd import ops, saint
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.saint import make_sampler
    d = synthetic_data(a.dataset, seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    B = a.batch_size
    res = {"device": torch.cuda.get_device_name(0), "dataset": a.dataset, "nodes": int(d.num_nodes), "entries": int(g.nnz),
           "batch_size": B, "steps": a.steps, "warmup": a.warmup, "samplers": {}}
    ops.saint_edge_weights(g.rowptr, g.col, g.num_nodes)
    ms = _timed(lambda: ops.saint_edge_weights(g.rowptr, g.col, g.num_nodes), a.builds)
    w = ops.saint_edge_weights(g.rowptr, g.col, g.num_nodes)
    res["edge_weight_table"] = dict(_stats(ms, "build"), builds=a.builds, bytes=int(sum(t.numel() * t.element_size() for t in w)),
                                    total_weight=int(w[2][-1].item()))
    del w
    x, y = d.x.contiguous(), d.y
    for kind in ("rw", "node", "edge"):
        ld = make_sampler(kind, g, B, 2, seed=1)
        for _ in range(a.warmup):
            ld.sample()
        ms = _timed(ld.sample, a.steps)
        ld.check()
        r = dict(n_cap=ld.n_cap, e_cap=ld.e_cap, **_stats(ms, "sample"))
        del ld
        torch.manual_seed(0)
        model = saint.build_model(x.shape[1], 256, d.num_classes, "cuda")
        tr = saint.make_trainer("graph", g, x, y, d.train_mask, model, 0.01, batch_size=B, walk_length=2, seed=1, sampler=kind)
        for _ in range(a.warmup + 1):
            tr.step()
        ms = _timed(tr.step, a.steps)
        tr.check()
        r.update(_stats(ms, "graph_step"), batch_nodes=int(tr.draw_out[2].item()), batch_edges=int(tr.sub_out[2].item()))
        res["samplers"][kind] = r
        print(json.dumps({kind: r}), file=sys.stderr)
        del tr, model
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
