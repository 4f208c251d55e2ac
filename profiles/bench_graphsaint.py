"""GraphSAINT random-walk training (grapes_amd/saint.py; reference graphsaint.py:104-121): per-step and per-epoch-evaluation
times on the synthetic stand-ins of cora, arxiv, Reddit and products (GCN(F, [256, C]), lr 0.01).

Per dataset and batch shape (B x L = 256 x 2, the reference's, and 4000 x 2, past the 2048-node small-graph build):
  * captured step: median / min / max over --steps replays after --warmup, each replay timed alone with device events;
  * eager step (modules.saint loader, GCN autograd, torch.optim.Adam; two host reads per step): median over --eager_steps;
  * batch nodes and induced edges of the last batch;
and per dataset the full-graph evaluation (one forward, val + test metric) time, median over --evals.
Launches per step and kernel times: run under rocprofv3 --kernel-trace --stats with --steps / --warmup small and divide the
kernel call counts by the replays.  Writes one JSON document (--out, else stdout)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, n):
    out = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def _case(name, d, g, B, L, a):
    from grapes_amd import saint
    x, y = d.x.contiguous(), d.y
    res = {"dataset": name, "batch_size": B, "walk_length": L}
    torch.manual_seed(0)
    model = saint.build_model(x.shape[1], 256, d.num_classes, "cuda")
    tr = saint.make_trainer("graph", g, x, y, d.train_mask, model, 0.01, batch_size=B, walk_length=L, seed=1)
    t0 = time.time()
    tr.step(); torch.cuda.synchronize()
    res["capture_s"] = round(time.time() - t0, 3)
    for _ in range(a.warmup):
        tr.step()
    ms = _timed(tr.step, a.steps)
    tr.check()
    res.update(graph_step_ms_median=round(statistics.median(ms), 4), graph_step_ms_min=round(min(ms), 4),
               graph_step_ms_max=round(max(ms), 4), graph_steps=a.steps,
               batch_nodes=int(tr.walk_out[2].item()), batch_edges=int(tr.sub_out[2].item()))
    del tr, model
    if not a.graph_only:
        torch.manual_seed(0)
        model = saint.build_model(x.shape[1], 256, d.num_classes, "cuda")
        tr = saint.make_trainer("eager", g, x, y, d.train_mask, model, 0.01, batch_size=B, walk_length=L, seed=1)
        for _ in range(3):
            tr.step()
        ms = _timed(tr.step, a.eager_steps)
        res["eager_step_ms_median"] = round(statistics.median(ms), 4)
        del tr, model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="cora,arxiv,reddit,products")
    ap.add_argument("--shapes", default="256x2,4000x2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--eager_steps", type=int, default=30)
    ap.add_argument("--evals", type=int, default=5)
    ap.add_argument("--graph_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grapes_amd import saint
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.graphsaint import evaluate
    from grapes_amd.main import synthetic_data
    results = {"device": torch.cuda.get_device_name(0), "cases": [], "evaluation": []}
    for name in a.datasets.split(","):
        d = synthetic_data(name, seed=0)
        g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
        for shp in a.shapes.split(","):
            B, L = (int(v) for v in shp.split("x"))
            results["cases"].append(_case(name, d, g, B, L, a))
            print(json.dumps(results["cases"][-1]), file=sys.stderr)
        if a.evals:
            torch.manual_seed(0)
            model = saint.build_model(d.x.shape[1], 256, d.num_classes, "cuda")
            evaluate(model, d.x, g, d.y, d.val_mask, d.test_mask, None)
            ms = _timed(lambda: evaluate(model, d.x, g, d.y, d.val_mask, d.test_mask, None), a.evals)
            results["evaluation"].append({"dataset": name, "nodes": int(d.num_nodes), "entries": int(g.nnz),
                                          "eval_ms_median": round(statistics.median(ms), 3)})
            print(json.dumps(results["evaluation"][-1]), file=sys.stderr)
            del model
        del d, g
        torch.cuda.empty_cache()
    text = json.dumps(results, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
