#!/usr/bin/env python3
"""GAT aggregation against the GCN aggregation at the same graph and width (the comparison point: the one-pass GAT forward reads
the same rows of H plus 4 bytes of s_src per edge and 8 bytes per row).

  run (under `rocprofv3 --kernel-trace --stats -d DIR --`, one process per shape, width and phase, no counters alongside):
      python profiles/bench_gat.py --shape sampled|fullbatch --width W --phase fwd|bwd [--iters 50]
  summarise the runs' *_kernel_stats.csv into the table kept in profiles/gat_kernel_stats.txt:
      python profiles/bench_gat.py --summarize DIR [DIR ...]

Shapes: `sampled` = the classifier's subgraph of the products workload (batch 256 + 3 hops x 256 samples: 1,024 nodes, 16,384
random edges); `fullbatch` = the arxiv-sized synthetic graph (169,343 nodes, mean degree 13.7, hub rows up to 13,161).  Kernels
named gat_* belong to the GAT call (scores included in the forward); every other kernel launched once per iteration or more
belongs to the GCN call."""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(a):
    import torch
    from grapes_amd import ops, synth
    from grapes_amd.graph import DeviceGraph
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(0)
    if a.shape == "sampled":
        n, e = 1024, 16384
        ei = torch.randint(0, n, (2, e), device=dev, generator=g, dtype=torch.int32)
        prep = ops.PreparedGraph(ei[0].contiguous(), ei[1].contiguous(), n)
    else:
        N, deg, maxdeg = synth.CONFIGS["arxiv"][:3]
        rowptr, col = synth.synth_graph_device(N, deg, maxdeg, seed=0, device=dev)
        prep = DeviceGraph(rowptr, col, N).gcn_prepared()
        n = N
    f = a.width
    h = torch.randn(n, f, device=dev, generator=g)
    dout = torch.randn(n, f, device=dev, generator=g)
    bias = torch.zeros(f, device=dev)
    a_src = torch.randn(f, device=dev, generator=g) * 0.1
    a_dst = torch.randn(f, device=dev, generator=g) * 0.1
    s_src, s_dst = ops.gat_scores(h, a_src, a_dst)
    out, row_ms = ops.gat_aggregate_fwd(h, s_src, s_dst, prep, bias)
    for it in range(a.iters + 5):                      # (5 extra iterations of each: warm-up, counted by the summary's divisor)
        if a.phase == "fwd":
            ops.gcn_aggregate_fwd(h, prep, bias, False)
            s_src, s_dst = ops.gat_scores(h, a_src, a_dst)
            ops.gat_aggregate_fwd(h, s_src, s_dst, prep, bias)
        else:
            ops.gcn_aggregate_bwd(dout, prep)
            ops.gat_aggregate_bwd(dout, out, h, s_src, s_dst, row_ms, a_src, a_dst, prep, bias)
    torch.cuda.synchronize()
    print(f"{a.shape} n={n} edges={int(prep.num_edges_no_loops)} width={f} phase={a.phase} iters={a.iters + 5}")


def _kernel_totals(d):
    """[(kernel name, calls, total ns)] from the run's *_kernel_stats.csv, or from its rocpd database."""
    csvs = sorted(glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True))
    if csvs:
        return [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(csvs[0]))]
    import sqlite3
    per = {}
    for name, dur in sqlite3.connect(sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True))[0]).execute(
            "select name, duration from kernels"):
        c, t = per.get(name, (0, 0.0))
        per[name] = (c + 1, t + float(dur))
    return sorted(((k, c, t) for k, (c, t) in per.items()), key=lambda r: -r[2])


def summarize(dirs):
    print("# rocprofv3 --kernel-trace --stats, MI355X; one process per row; us per call = sum over the call's kernels of total / iterations")
    print(f"{'shape':10s} {'width':>5s} {'phase':>5s} {'GCN us':>9s} {'GAT us':>9s} {'GAT/GCN':>8s}   kernels (us per iteration)")
    for d in dirs:
        tag = os.path.basename(os.path.normpath(d)).split("_")            # <shape>_<width>_<phase>
        shape, width, phase = tag[0], tag[1], tag[2]
        iters = int(open(os.path.join(d, "run.log")).read().split("iters=")[1].split()[0])
        gat, gcn, names = 0.0, 0.0, []
        for name, calls, tot in _kernel_totals(d):
            name = name.split("(")[0]
            if name.startswith("void "):
                name = name[5:]
            if name.startswith("gat_"):
                # (the set-up runs the scores and the forward once more)
                k = calls - 1 if (name.startswith("gat_scores") or name.startswith("gat_fwd")) and phase == "bwd" else calls
                if k < iters:
                    continue
                gat += tot / calls * (k // iters)
                names.append(f"{name.split('<')[0]} {tot / calls / 1e3:.1f}")
            elif calls >= iters and calls % iters == 0:
                gcn += tot / calls * (calls // iters)
                names.append(f"{name.split('<')[0]} {tot / calls / 1e3:.1f}")
        print(f"{shape:10s} {width:>5s} {phase:>5s} {gcn / 1e3:9.1f} {gat / 1e3:9.1f} {gat / gcn if gcn else float('nan'):8.2f}   " + ", ".join(names))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["sampled", "fullbatch"], default="sampled")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--phase", choices=["fwd", "bwd"], default="fwd")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--summarize", nargs="+")
    a = ap.parse_args()
    summarize(a.summarize) if a.summarize else run(a)
