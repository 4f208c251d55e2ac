#!/usr/bin/env python3
"""LINKX: ops.bag_batch, ops.bag_fwd and the fused row-sparse Adam ops.bag_bwd_adam beside two torch forms of the same update, and one
eager LinkxTrainer step beside PPRGoTrainer and SageTrainer.

      python profiles/bench_linkx.py [--reps 21] [--inner 200] [--out profiles/linkx_bench.json]
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/bench_linkx.py --trace_calls 50

The products-shaped synthetic graph, batch 512, H in {64, 256}, everything in one process; the root sets are profiles/bench_shadow.py's
(512 training nodes far from the hub, and the same set with the hub and 63 nodes that store it in front).  A repetition is `inner` calls
between two device events, the variants alternating in every repetition; the figure kept is the median over `reps` repetitions after
a warm-up, with the quartiles beside it; host launches are included.

bag_batch.   ops.bag_batch into preallocated tables at capacities that fit.
bag_fwd.     ops.bag_fwd with the item capacity the batch's counts give.
adam.        the backward + optimiser step of the table from a fixed d out [512, H]:
               fused         ops.bag_bwd_adam
               torch_sparse  nn.EmbeddingBag(mode="sum", sparse=True): forward, backward (a sparse gradient), torch.optim.SparseAdam —
                             minus the time of its forward alone, measured beside it
               torch_dense   index_add_ of d out's rows into a dense [N, H] gradient + torch.optim.Adam over the table
             `fused_lower_than_torch_sparse_by_more_than_both_iqrs` says whether the fused median lies below the sparse form's
             (forward subtracted) by more than the interquartile ranges together — the fused form's, the sparse form's and that
             of the forward-only run that was subtracted.
step.        LinkxTrainer.step (hidden 256, fused) beside PPRGoTrainer(k=32) and SageTrainer(10/10): host wall time to a device
             synchronise — neighbours for scale, not equals.

--trace_calls N runs N LinkxTrainer steps (hidden 256, the hub set) and nothing else, for a kernel trace in a run of its own.
Not measured: a captured step (none exists), other graphs, multi-GPU forms."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_shadow import BATCH, WIDTH, _alternate, _wall, root_sets  # noqa: E402

WIDTHS = (64, 256)


def main(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_linkx.py measures on the GPU; none is visible")
    from grapes_amd import graphsage, linkx, ops, pprgo
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    from grapes_amd.modules.linkx import LINKX, BagBatcher
    from grapes_amd.modules.pprgo import PPRGo
    d = synthetic_data("products", seed=0)
    g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
    N, dev = g.num_nodes, g.device
    train = torch.nonzero(d.train_mask, as_tuple=False).reshape(-1)
    plain, with_hub, hub = root_sets(torch, g, train)
    sets = (("without_hub", plain), ("with_hub", with_hub))
    x, y = d.x.contiguous(), d.y

    def linkx_trainer():
        torch.manual_seed(0)
        m = LINKX(N, x.shape[1], WIDTH, d.num_classes).to(dev)
        return linkx.LinkxTrainer(g, x, y, m, torch.optim.Adam(m.dense_parameters(), lr=1e-3), bag_lr=1e-3)
    if a.trace_calls:
        tr = linkx_trainer()
        for _ in range(a.trace_calls):
            tr.step(with_hub)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "dataset": "products (synthetic)", "nodes": int(N),
           "entries": int(g.nnz), "batch_size": BATCH, "hub": hub, "hub_entries": int((g.rowptr[hub + 1] - g.rowptr[hub]).item()),
           "units": {"calls": "us per call (host launches included), median of reps",
                     "wall": "ms of host wall time to a device synchronise, host reads included"}}
    bb = BagBatcher(g)
    batches = {name: bb.batch(roots) for name, roots in sets}
    bb.check()
    res["bag_batch"] = {}
    for name, roots in sets:
        b = batches[name]
        r32 = b.rows
        uc, ec = b.num_unique + 16, b.num_entries + 16
        out = ops.bag_batch(g.rowptr, g.col, N, r32, bb._scratch, uc, ec)
        st = _alternate(torch, {"bag_batch": lambda: ops.bag_batch(g.rowptr, g.col, N, r32, bb._scratch, uc, ec, out=out)}, a.reps, a.inner)
        res["bag_batch"][name] = {"distinct_columns": b.num_unique, "entries": b.num_entries, "longest_segment": b.seg_max,
                                  "longest_row": b.row_max, **st["bag_batch"]}
    res["bag_fwd"], res["adam"] = {}, {}
    for H in WIDTHS:
        torch.manual_seed(H)
        W = torch.randn(N, H, device=dev) * 0.01
        bias = torch.zeros(H, device=dev)
        ea, eas = torch.zeros_like(W), torch.zeros_like(W)
        emb = torch.nn.EmbeddingBag(N, H, mode="sum", sparse=True).to(dev)
        sp_opt = torch.optim.SparseAdam(emb.parameters(), lr=1e-3)
        Wd = torch.nn.Parameter(W.clone())
        Wd.grad = torch.zeros_like(Wd)
        de_opt = torch.optim.Adam([Wd], lr=1e-3)
        G = torch.randn(BATCH, H, device=dev)
        for name, _ in sets:
            b = batches[name]
            ic_f, ic_b = ops.bag_fwd_item_cap(b.num_entries, b.row_max), ops.bag_bwd_item_cap(b.num_entries, b.seg_max)
            out = ops.bag_fwd(g.rowptr, g.col, N, b.rows, W, bias, item_cap=ic_f)
            st = _alternate(torch, {"bag_fwd": lambda: ops.bag_fwd(g.rowptr, g.col, N, b.rows, W, bias, item_cap=ic_f, out=out)}, a.reps,
                            a.inner)
            res["bag_fwd"][f"H={H}/{name}"] = st["bag_fwd"]
            r = b.rows.long().clamp(0, N - 1)
            deg = g.rowptr[r + 1] - g.rowptr[r]
            ent = torch.cat([g.col[g.rowptr[i]:g.rowptr[i + 1]] for i in r.tolist()]).long()
            offs = (torch.cumsum(deg, 0) - deg).contiguous()
            brow = torch.repeat_interleave(torch.arange(BATCH, device=dev), deg)
            step = [0]

            def fused():
                step[0] += 1
                ops.bag_bwd_adam(G, b.tptr, b.trow, b.uniq, b.num_unique, b.num_entries, W, ea, eas, 1e-3, 0.9, 0.999, 1e-8, step[0],
                                 item_cap=ic_b)

            def torch_sparse():
                sp_opt.zero_grad()
                emb(ent, offs).backward(G)
                sp_opt.step()

            def torch_sparse_forward_only():
                with torch.no_grad():
                    emb(ent, offs)

            def torch_dense():
                Wd.grad.zero_()
                Wd.grad.index_add_(0, ent, G[brow])
                de_opt.step()
            st = _alternate(torch, {"fused": fused, "torch_sparse": torch_sparse, "torch_sparse_forward_only": torch_sparse_forward_only,
                                    "torch_dense": torch_dense}, a.reps, a.inner)
            f, s, s0 = st["fused"], st["torch_sparse"], st["torch_sparse_forward_only"]
            net = s["median_us"] - s0["median_us"]
            spread = (f["q3_us"] - f["q1_us"]) + (s["q3_us"] - s["q1_us"]) + (s0["q3_us"] - s0["q1_us"])   # (the subtracted forward's too)
            st["torch_sparse_minus_forward_us"] = round(net, 2)
            st["fused_lower_than_torch_sparse_by_more_than_both_iqrs"] = bool(net - f["median_us"] > spread)
            st["ratio_torch_sparse_to_fused"] = round(net / f["median_us"], 2)
            st["ratio_torch_dense_to_fused"] = round(st["torch_dense"]["median_us"] / f["median_us"], 2)
            res["adam"][f"H={H}/{name}"] = st
            print(json.dumps({f"H={H}/{name}": st}), file=sys.stderr, flush=True)
        del W, ea, eas, emb, sp_opt, Wd, de_opt
        torch.cuda.empty_cache()
    trainers = {"linkx_fused": linkx_trainer()}
    torch.manual_seed(0)
    m = PPRGo(x.shape[1], [WIDTH, d.num_classes]).to(dev)
    trainers["pprgo_k32"] = pprgo.PPRGoTrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), k=32, alpha=0.25, eps=2 ** -14)
    m = graphsage.build_model(x.shape[1], WIDTH, d.num_classes, 2, 0.0, "mean", dev)
    trainers["sage_10_10"] = graphsage.SageTrainer(g, x, y, m, torch.optim.Adam(m.parameters(), lr=1e-3), fanouts=[10, 10], seed=1)
    res["step"] = _wall(torch, {name: (lambda t=t: t.step(plain)) for name, t in trainers.items()}, a.reps)
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
