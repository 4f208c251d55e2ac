"""LADIES / FastGCN on a synthetic stand-in graph (default: products-shaped): per layer the device time of the importance launch,
the draw (ops.gumbel_topk on the shifted logits) and the layer kernel's three launches, each timed with device events on the inputs
one sampled batch produced (the bitmaps marked outside the clock); FastGCN's one-time global importance; and the eager training
step (LadiesTrainer.step: sampling with its host reads, forward, backward, Adam) as host wall time to a device synchronise.

Medians over --repeats runs after --warmup runs, with the minimum and maximum beside them.  Writes one JSON document (--out, else
stdout).  Not measured: a captured step (none exists), other graphs, the set work between the kernels on its own."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def _events(fn, warmup, repeats):
    """ms per call of fn() by device events."""
    out = []
    for i in range(warmup + repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record(); e.synchronize()
        if i >= warmup:
            out.append(s.elapsed_time(e))
    return _stat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="products")
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--samp_num", type=int, default=64)
    ap.add_argument("--num_layers", type=int, default=2)
    ap.add_argument("--hidden_dim", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grapes_amd import ops
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.ladies import LadiesTrainer, build_model
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.ladies import LayerWiseSampler
    d = synthetic_data(a.dataset, seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    N = g.num_nodes
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    targets = train[torch.randperm(train.numel(), device=train.device)[: a.batch_size]]
    res = {"device": torch.cuda.get_device_name(0), "dataset": a.dataset, "nodes": int(N), "entries": int(g.nnz),
           "batch_size": a.batch_size, "samp_num": a.samp_num, "num_layers": a.num_layers, "hidden_dim": a.hidden_dim,
           "warmup": a.warmup, "repeats": a.repeats, "unit": "ms", "samplers": {}}
    for kind in ("ladies", "fastgcn"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = LayerWiseSampler(g, a.samp_num, a.num_layers, kind=kind, seed=1)
        torch.cuda.synchronize()
        r = {"symmetric": bool(s.symmetric), "construct_wall_ms": round(1e3 * (time.perf_counter() - t0), 3), "layers": []}
        if kind == "fastgcn":
            r["global_importance"] = _events(lambda: ops.ladies_importance(g.rowptr, s.rowptr_t, s.col_t, N, pi_table=s.pi_table),
                                             a.warmup, a.repeats)
        b = s.sample(targets)
        s.check()
        for L in b.layers:
            m, row = L.prev.numel(), {"rows": int(L.prev.numel()), "after": int(L.after.numel()), "entries": int(L.weight.numel())}
            if kind == "ladies":
                n = L.candidates.numel()
                row["candidates"] = int(n)
                ops.bitmap_mark_lists(g.prev_bits, None, [(L.prev, None)], N)
                row["importance"] = _events(lambda: ops.ladies_importance(g.rowptr, s.rowptr_t, s.col_t, N, ids=L.candidates,
                                                                          prev_bits=g.prev_bits, m=m, pi_table=s.pi_table),
                                            a.warmup, a.repeats)
                ops.bitmap_clear(g.prev_bits, L.prev)
                cand = L.candidates
            else:
                n, cand = N, s._all_ids()
            if n > a.samp_num:
                u = ops.philox_uniform(n, 1, 0, g.device)
                row["draw"] = _events(lambda: ops.gumbel_topk(L.logit, a.samp_num, uniforms=u, candidate_ids=cand, n=n, mode=0,
                                                              want_log_prob=False, want_stats=False), a.warmup, a.repeats)
            ops.bitmap_mark_lists(g.bits, None, [(L.after, None)], N)
            e_cap = max(1, L.weight.numel())
            row["layer"] = _events(lambda: ops.ladies_layer(g.rowptr, g.col, N, L.prev, g.bits, s.pi_table, e_cap), a.warmup, a.repeats)
            ops.bitmap_clear(g.bits, L.after)
            r["layers"].append(row)
        x, y = d.x.contiguous(), d.y
        model = build_model(x.shape[1], a.hidden_dim, d.num_classes, a.num_layers, 0.0, g.device)
        tr = LadiesTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=1e-3), samp_num=a.samp_num, kind=kind, seed=1)
        wall = []
        for i in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(targets)
            torch.cuda.synchronize()
            if i >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
        r["eager_step_wall"] = _stat(wall)
        res["samplers"][kind] = r
        print(json.dumps({kind: r}), file=sys.stderr)
        del s, tr, model
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
