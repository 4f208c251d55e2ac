#!/usr/bin/env python3
"""The weighted GCN aggregation (ops.wgcn_*) beside the unweighted one (ops.gcn_aggregate_fwd / _bwd) of the same build, on the
same graph, in the same process: the weight pass, the forward, the backward without and with the edge-weight gradient.

  measure (device events; medians with min - max over --repeats windows of --iters calls, the two forms alternating):
      python profiles/bench_wgcn.py [--out profiles/wgcn_bench.json]
  kernel times (a run of its own, no counters alongside):
      rocprofv3 --kernel-trace --stats -d DIR -- python profiles/bench_wgcn.py --trace fwd|bwd --shape hop --width 256

Shapes: `hop` = a products-shaped hop graph (37,500 nodes, 38,000 random directed entries; f = 256 and f = 104); `classifier` = the
classifier's sampled subgraph (1,024 nodes, 16,384 entries; f = 256).  The weighted forward moves 4 more bytes per entry (val_t)
than the unweighted one, and reads lw per row."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"hop": (37500, 38000, (256, 104)), "classifier": (1024, 16384, (256,))}


def _setup(shape, f):
    import torch
    from grapes_amd import ops
    n, e, _ = SHAPES[shape]
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    ei = torch.randint(0, n, (2, e), device="cuda", generator=g, dtype=torch.int32)
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    prep = ops.PreparedGraph(src, dst, n)
    ws = ops.WeightedStructure(prep, src, dst)
    w = torch.rand(e, device="cuda", generator=g) * 2
    vals = ops.wgcn_weights(ws, w)
    h = torch.randn(n, f, device="cuda", generator=g)
    dout = torch.randn(n, f, device="cuda", generator=g)
    bias = torch.zeros(f, device="cuda")
    calls = {
        "weights": lambda: ops.wgcn_weights(ws, w),
        "fwd_weighted": lambda: ops.wgcn_aggregate_fwd(h, ws, vals, bias, True),
        "fwd_unweighted": lambda: ops.gcn_aggregate_fwd(h, prep, bias, True),
        "bwd_weighted": lambda: ops.wgcn_aggregate_bwd(dout, ws, vals),
        "bwd_weighted_dw": lambda: ops.wgcn_aggregate_bwd(dout, ws, vals, h=h, want_dw=True),
        "bwd_unweighted": lambda: ops.gcn_aggregate_bwd(dout, prep),
    }
    return prep, calls


def _time(calls, iters, repeats):
    """{name: [us per call, one value per window]}: every window times `iters` calls of one form between two events; the forms
    take turns inside a repeat, so a drift of the machine reaches all of them."""
    import torch
    for fn in calls.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / iters)
    return out


def measure(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_wgcn: no GPU (there is no CPU path to time)")
    rows = []
    for shape, (n, e, widths) in SHAPES.items():
        for f in widths:
            prep, calls = _setup(shape, f)
            t = _time(calls, a.iters, a.repeats)
            row = {"shape": shape, "n": n, "entries": e, "aggregated_entries": int(prep.num_edges_no_loops), "f": f,
                   "iters_per_window": a.iters, "windows": a.repeats, "us_per_call": {}}
            for k, v in t.items():
                row["us_per_call"][k] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
            med = lambda k: row["us_per_call"][k]["median"]
            # ratio of the medians, and the spread of the per-repeat ratios (the two forms of a repeat run back to back)
            for tag in ("fwd", "bwd"):
                per = [w / u for w, u in zip(t[tag + "_weighted"], t[tag + "_unweighted"])]
                row[tag + "_weighted_over_unweighted"] = {"median": round(med(tag + "_weighted") / med(tag + "_unweighted"), 3),
                                                          "min": round(min(per), 3), "max": round(max(per), 3)}
            rows.append(row)
            print(json.dumps(row))
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events around windows of calls on one stream (launch gaps inside)",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


def trace(a):
    import torch
    _, calls = _setup(a.shape, a.width)
    names = ("fwd_weighted", "fwd_unweighted") if a.trace == "fwd" else ("bwd_weighted_dw", "bwd_unweighted")
    for _ in range(a.iters):
        for k in names:
            calls[k]()
    torch.cuda.synchronize()
    print(f"{a.shape} width={a.width} trace={a.trace} iters={a.iters}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgcn_bench.json"))
    ap.add_argument("--iters", type=int, default=2000)     # a window of 2000 calls: 15 - 180 ms of device time
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--trace", choices=["fwd", "bwd"])
    ap.add_argument("--shape", choices=list(SHAPES), default="hop")
    ap.add_argument("--width", type=int, default=256)
    a = ap.parse_args()
    trace(a) if a.trace else measure(a)
