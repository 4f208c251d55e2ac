"""Full-batch evaluation over papers100M at its real shape (N1 above 2^31 entries; grapes_amd/full_graph.py): the CLI's
classifier GCN(128, [256, 172]) evaluated on a mask of --mask rows through the row-blocked 64-bit path.  Prints one JSON line:
the evaluation pass (device-synchronised, after a warm-up pass that also builds the graph's plan), each layer's aggregation
timed on its own with events over the same row blocks, their algorithmic bytes — (4F + 4) B per aggregated entry + (8F + 12) B
per row, as DESIGN.md counts the int32 kernels' — and the fraction of 8 TB/s, and the peak HBM the pass allocated beyond what
was resident.  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mask", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grapes_amd import full_graph, ops, synth
    from grapes_amd.eval import evaluate
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    import types
    N, deg, maxdeg, F, C, *_ = synth.CONFIGS["papers100m"]
    t0 = time.time()
    rowptr, col = synth.synth_graph_device_chunked(N, deg, maxdeg, seed=0, device="cuda")
    g = DeviceGraph(rowptr, col, N)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    X = synth.randn_rows_(torch.empty(N, F, device="cuda"), generator=gen)
    y = torch.randint(0, C, (N,), device="cuda", generator=gen)
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[torch.randperm(N, device="cuda", generator=gen)[:a.mask]] = True
    torch.manual_seed(0)
    c = GCN(F, [256, C]).cuda()
    data = types.SimpleNamespace(x=X, y=y)
    args = types.SimpleNamespace(sampling_hops=3, num_samples=256, use_indicators=True)
    torch.cuda.synchronize()
    setup_s = time.time() - t0
    t0 = time.time()
    plan = g.full_graph_plan()
    torch.cuda.synchronize()
    plan_s = time.time() - t0
    evaluate(c, None, data, args, g, mask=mask, full_batch=True)             # warm-up
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize(); t = time.time()
        acc, _ = evaluate(c, None, data, args, g, mask=mask, full_batch=True)
        torch.cuda.synchronize(); times.append(time.time() - t)
    peak = torch.cuda.max_memory_allocated() - base
    # the first pass after empty_cache (times[0]) against the warm ones: how much of the difference is T2's allocation itself —
    # a fresh N x C buffer timed through hipMalloc, its first write and a second write
    del_t = {}
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    t = time.time(); buf = torch.empty((N, C), dtype=torch.float32, device="cuda"); torch.cuda.synchronize(); del_t["alloc_s"] = time.time() - t
    t = time.time(); buf.fill_(0.0); torch.cuda.synchronize(); del_t["first_write_s"] = time.time() - t
    t = time.time(); buf.fill_(1.0); torch.cuda.synchronize(); del_t["second_write_s"] = time.time() - t
    del buf
    # each layer's aggregation alone, over the row blocks the pass uses
    nnz = g.nnz
    B = full_graph.DEFAULT_BLOCK_ROWS
    rows = torch.nonzero(mask).reshape(-1).to(torch.int32)
    T2 = torch.empty((N, C), dtype=torch.float32, device="cuda")            # (172 % 4 == 0: no padding)
    T2.normal_(generator=gen)
    layers = []
    for name, h, pre, sel in (("layer1_aggregate_X", X, False, None), ("layer2_aggregate_T2_mask_rows", T2, True, rows)):
        total = N if sel is None else sel.numel()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(2):
            ev0.record()
            for i0 in range(0, total, B):
                m = min(B, total - i0)
                ops.gcn_large_aggregate(h, plan, pre, r0=i0 if sel is None else 0, m=m, rows=None if sel is None else sel[i0:i0 + m])
            ev1.record(); torch.cuda.synchronize()
        ms = ev0.elapsed_time(ev1)
        f = h.shape[1]
        if sel is None:
            entries = nnz
        else:
            entries = int((rowptr[sel.long() + 1] - rowptr[sel.long()]).sum())
        byts = (4 * f + 4) * entries + (8 * f + 12) * total
        layers.append({"name": name, "rows": total, "entries": entries, "width": f, "ms": round(ms, 2),
                       "algorithmic_bytes": byts, "tb_per_s": round(byts / ms / 1e9, 3), "fraction_of_8tbps": round(byts / ms / 1e9 / 8.0, 3)})
    res = {"workload": "papers100m full-batch evaluation", "N": N, "nnz": nnz, "F": F, "C": C, "model": "GCN(128,[256,172])",
           "mask_rows": int(rows.numel()), "block_rows": B, "hub_items": plan.item_cap, "symmetric": plan.symmetric,
           "eval_pass_s": [round(t, 3) for t in times], "eval_pass_s_min": round(min(times), 3),
           "first_pass_note": "eval_pass_s[0] follows torch.cuda.empty_cache(): its N-sized operand is allocated afresh",
           "t2_sized_buffer": {k: round(v, 3) for k, v in del_t.items()}, "accuracy": acc,
           "peak_extra_gib": round(peak / 2 ** 30, 2), "t2_gib": round(N * C * 4 / 2 ** 30, 2),
           "plan_build_s": round(plan_s, 2), "setup_s": round(setup_s, 1), "aggregation": layers,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
