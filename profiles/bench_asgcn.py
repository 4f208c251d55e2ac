#!/usr/bin/env python3
"""AS-GCN on a synthetic stand-in graph (default: products-shaped), one process, two comparisons:

      python profiles/bench_asgcn.py [--reps 21] [--inner 200] [--out profiles/asgcn_bench.json]

* the importance of one layer's candidates (the layer of one sampled batch that has the most): ops.asgcn_importance — column mass,
  feature dot product, g, q, logq in one launch and the shift in a second — against the unfused form of the same quantities'
  inputs: ops.ladies_importance (the same transpose-row walk) + ops.gather_rows of the candidates' feature rows + the 1-wide
  ops.linear_fwd.  The unfused form stops there: it has not yet formed q, logq or the shifted logits.
* one AsgcnTrainer.step against one LadiesTrainer.step on the same graph, targets, model shape and samp_num (eager steps: sampling
  with its host reads, forward, backward, Adam).

A repetition is `inner` calls (`inner_step` steps) between two device events, the variants alternating inside every repetition; the
figure kept is the median over `reps` repetitions after a warm-up of every variant, with the quartiles beside it (the method of
profiles/bench_gatv2.py).  Not measured here: other graphs and shapes, a captured step (none exists); the kernels one by one are in
profiles/asgcn_kernel_stats.txt, from a rocprofv3 --kernel-trace --stats run of its own over the same layer."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(a):
    import torch
    from grapes_amd import ops
    from grapes_amd.asgcn import AsgcnTrainer
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.ladies import LadiesTrainer, build_model
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.asgcn import AdaptiveSampler
    if not torch.cuda.is_available():
        raise SystemExit("bench_asgcn.py measures on the GPU; none is visible")
    d = synthetic_data(a.dataset, seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    N = g.num_nodes
    x, y = d.x.contiguous(), d.y
    F = x.shape[1]
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    torch.manual_seed(0)
    targets = train[torch.randperm(train.numel(), device=train.device)[: a.batch_size]]
    sampler = AdaptiveSampler(g, a.samp_num, a.num_layers, F, seed=1)
    b = sampler.sample(targets, x)
    sampler.check()
    L = max(b.layers, key=lambda l: l.candidates.numel())
    cand, m = L.candidates, L.prev.numel()
    w_g, b_g = sampler.w_g.detach(), sampler.b_g.detach()
    w_row = w_g.reshape(1, -1).contiguous()
    ops.bitmap_mark_lists(g.prev_bits, None, [(L.prev, None)], N)

    def fused():
        ops.asgcn_importance(g.rowptr, sampler.rowptr_t, sampler.col_t, N, x, w_g, b_g, ids=cand, prev_bits=g.prev_bits, m=m,
                             q_table=sampler.pi_table, a_table=sampler.a_table)

    def unfused():
        ops.ladies_importance(g.rowptr, sampler.rowptr_t, sampler.col_t, N, ids=cand, prev_bits=g.prev_bits, m=m,
                              pi_table=sampler.pi_table)
        ops.linear_fwd(ops.gather_rows(x, cand), w_row)

    def timed(variants, inner):
        for fn in variants.values():                          # warm-up: every variant, every shape of the timed window
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():                    # (alternating: a drift of the machine reaches every variant alike)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(inner):
                    fn()
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1) * 1e3 / inner)
        out = {}
        for k, v in times.items():
            q = statistics.quantiles(v, n=4)
            out[k] = {"median_us": round(statistics.median(v), 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2)}
        return out

    imp = timed({"asgcn_importance": fused, "ladies_importance+gather_rows+linear_fwd": unfused}, a.inner)
    ops.bitmap_clear(g.prev_bits, L.prev)

    model_a = build_model(F, a.hidden_dim, d.num_classes, a.num_layers, 0.0, g.device)
    model_l = build_model(F, a.hidden_dim, d.num_classes, a.num_layers, 0.0, g.device)
    opt = torch.optim.Adam(list(model_a.parameters()) + list(sampler.parameters()), lr=1e-3)
    tr_a = AsgcnTrainer(g, x, y, model_a, sampler, opt, var_coef=0.5)
    tr_l = LadiesTrainer(g, x, y, model_l, torch.optim.Adam(model_l.parameters(), lr=1e-3), samp_num=a.samp_num, kind="ladies", seed=1)
    steps = timed({"asgcn_step": lambda: tr_a.step(targets), "ladies_step": lambda: tr_l.step(targets)}, a.inner_step)
    tr_a.check(); tr_l.check()

    res = {"device": torch.cuda.get_device_name(0), "dataset": a.dataset, "nodes": int(N), "entries": int(g.nnz), "features": int(F),
           "batch_size": a.batch_size, "samp_num": a.samp_num, "num_layers": a.num_layers, "hidden_dim": a.hidden_dim,
           "reps": a.reps, "inner": a.inner, "inner_step": a.inner_step,
           "unit": "us per call (host launches included), median of reps",
           "layer": {"rows": int(m), "candidates": int(cand.numel()), "batch_nodes": int(b.num_nodes),
                     "entries": [int(l.weight.numel()) for l in b.layers]},
           "importance": imp, "step": steps,
           "ratio": {"importance_fused_over_unfused": round(imp["asgcn_importance"]["median_us"] /
                                                            imp["ladies_importance+gather_rows+linear_fwd"]["median_us"], 3),
                     "asgcn_step_over_ladies_step": round(steps["asgcn_step"]["median_us"] / steps["ladies_step"]["median_us"], 3)}}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="products")
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--samp_num", type=int, default=64)
    ap.add_argument("--num_layers", type=int, default=2)
    ap.add_argument("--hidden_dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--inner_step", type=int, default=20)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
