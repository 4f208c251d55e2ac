#!/usr/bin/env python3
"""GCN2Conv's propagation (grapes_gcn2_propagate_fwd / _bwd) against the GCN aggregation (grapes_gcn_aggregate_fwd / _bwd) on the
same graph and width in the same run, and one whole conv (propagation + the identity-mapping GEMMs + the blend).

  run (under `rocprofv3 --kernel-trace --stats -d DIR --`, one process per shape and phase, no counters alongside):
      python profiles/bench_gcn2.py --shape sampled|fullbatch --width W --phase fwd|bwd [--iters 50]
  summarise the runs' *_kernel_stats.csv into the table kept in profiles/gcn2_kernel_stats.txt:
      python profiles/bench_gcn2.py --summarize DIR [DIR ...]
  the whole job (each GPU step under its own timeout, chained with &&):
      python profiles/bench_gcn2.py --print-job OUTDIR | bash

Shapes: `sampled` = the classifier's subgraph of the products workload (batch 256 + 3 hops x 256 samples: 1,024 nodes, 16,384
random edges); `fullbatch` = the arxiv-sized synthetic graph (169,343 nodes, mean degree 13.7, hub rows up to 13,161).

The yardstick is the GCN aggregation, not the code under test.  Algorithmic bytes per call (fp32, e aggregated edges, n rows,
width f; gathered rows counted once per edge, as the kernels request them):
    GCN fwd   e (4 f + 4 + 4)  [row of H, column index, dinv of the source]  + n (4 f [own row] + 4 f [out] + 8 [rowptr, dinv])
    GCN2 fwd  e (4 f + 4)      [row of x, column index]                      + n (4 f [x0] + 4 f [S] + 8 [rowptr, loops])
    GCN bwd   e (4 f + 8) + n (4 f + 4 f + 8);   GCN2 bwd  e (4 f + 4) + n (4 f [dS own row] + 4 f [dx] + 4 f [dx0] + 8)
The expectation printed by --summarize: propagate time <= GCN time x byte ratio x the GCN kernel's own run-to-run spread
(max / min of its per-call time over the repeats of the run, from the kernel trace)."""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def algorithmic_bytes(n, e, f):
    return {"gcn_fwd": e * (4 * f + 8) + n * (8 * f + 8), "gcn2_fwd": e * (4 * f + 4) + n * (8 * f + 8),
            "gcn_bwd": e * (4 * f + 8) + n * (8 * f + 8), "gcn2_bwd": e * (4 * f + 4) + n * (12 * f + 8)}


def run(a):
    import torch
    from grapes_amd import ops, synth
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN2Conv
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(0)
    if a.shape == "sampled":
        n, e = 1024, 16384
        ei = torch.randint(0, n, (2, e), device=dev, generator=g, dtype=torch.int32)
        prep = ops.PreparedGraph(ei[0].contiguous(), ei[1].contiguous(), n)
        ops.gcn2_attach_loops(prep, ei[0].contiguous(), ei[1].contiguous())
    else:
        N, deg, maxdeg = synth.CONFIGS["arxiv"][:3]
        rowptr, col = synth.synth_graph_device(N, deg, maxdeg, seed=0, device=dev)
        dg = DeviceGraph(rowptr, col, N)
        prep = dg.gcn_prepared()
        prep.loops = ops.gcn2_loop_counts_csr(dg.rowptr, dg.col, N)
        n = N
    f = a.width
    x = torch.randn(n, f, device=dev, generator=g)
    x0 = torch.randn(n, f, device=dev, generator=g)
    dout = torch.randn(n, f, device=dev, generator=g)
    bias = torch.zeros(f, device=dev)
    conv = GCN2Conv(f, 0.1, 0.5, 2).to(dev)
    xr, x0r = x.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    for it in range(a.iters + 5):                      # (5 extra iterations of each: warm-up, counted by the summary's divisor)
        if a.phase == "fwd":
            ops.gcn_aggregate_fwd(x, prep, bias, False)
            ops.gcn2_propagate_fwd(x, x0, prep, 0.1)
            with torch.no_grad():
                conv(x, x0, prep, relu=True)
        else:
            ops.gcn_aggregate_bwd(dout, prep)
            ops.gcn2_propagate_bwd(dout, prep, 0.1)
            out = conv(xr, x0r, prep, relu=True)
            torch.autograd.grad(out, [xr, x0r, conv.weight1], dout)
    torch.cuda.synchronize()
    e = int(prep.num_edges_no_loops)
    print(f"{a.shape} n={n} edges={e} loops={int(prep.loops[:n].sum())} width={f} phase={a.phase} iters={a.iters + 5}")


def _kernel_rows(d):
    """[(kernel name, duration ns)] per launch from the run's kernel trace (csv or rocpd database), in launch order."""
    csvs = sorted(glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True))
    if csvs:
        rows = [(r["Kernel_Name"], float(r["End_Timestamp"]) - float(r["Start_Timestamp"]), float(r["Start_Timestamp"]))
                for r in csv.DictReader(open(csvs[0]))]
        return [(k, t) for k, t, _ in sorted(rows, key=lambda r: r[2])]
    import sqlite3
    db = sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True))[0]
    return [(k, float(t)) for k, t in sqlite3.connect(db).execute("select name, duration from kernels order by start")]


def _short(name):
    name = name.split("(")[0]
    return (name[5:] if name.startswith("void ") else name).split("<")[0]


def summarize(dirs):
    print("# rocprofv3 --kernel-trace --stats, MI355X; one process per row; us per call = sum over the call's kernels of their mean time")
    print("# spread = max / min over the run's repeats of the GCN aggregation's main kernel (its own run-to-run variation)")
    print("# prop = row_sum_rows_k + row_sum_chunks_k + row_sum_combine_k once; a bwd run's mean of those kernels is over the bare backward call")
    print("# and the conv's forward and backward calls (the same kernels over the two CSRs)")
    print(f"{'shape':10s} {'width':>5s} {'phase':>5s} {'GCN us':>8s} {'prop us':>8s} {'prop/GCN':>8s} {'bytes':>6s} {'spread':>6s} {'bound':>6s} "
          f"{'met':>4s} {'conv us':>8s}   kernels (us per call x calls per iteration)")
    for d in dirs:
        shape, width, phase = os.path.basename(os.path.normpath(d)).split("_")[:3]
        log = open(os.path.join(d, "run.log")).read()
        iters = int(log.split("iters=")[1].split()[0])
        n, e = int(log.split("n=")[1].split()[0]), int(log.split("edges=")[1].split()[0])
        per = {}
        for name, t in _kernel_rows(d):
            per.setdefault(_short(name), []).append(t)
        gcn = prop = conv = 0.0
        names, spread = [], float("nan")
        for k, ts in sorted(per.items(), key=lambda kv: -sum(kv[1])):
            if len(ts) < iters:
                continue                                          # (set-up kernels: the graph build, the generators)
            mean, per_it = sum(ts) / len(ts), len(ts) // iters
            names.append(f"{k} {mean / 1e3:.1f} x{per_it}")
            if k.startswith("row_sum_"):
                prop += mean                                     # (one call of the bare propagation; the conv's call is the second)
                conv += mean * (per_it - 1)
            elif k.startswith("gcn2_"):
                conv += mean * per_it
            elif k.startswith("gcn_aggregate") or k.startswith("colsum"):
                gcn += mean * per_it
                if k.startswith("gcn_aggregate") and not ("chunks" in k or "combine" in k):
                    steady = ts[5 * per_it:]
                    spread = max(steady) / min(steady)
            else:
                conv += mean * per_it                            # the GEMMs of the conv
        b = algorithmic_bytes(n, e, int(width))
        ratio = b[f"gcn2_{phase}"] / b[f"gcn_{phase}"]
        bound = gcn * ratio * spread
        print(f"{shape:10s} {width:>5s} {phase:>5s} {gcn / 1e3:8.1f} {prop / 1e3:8.1f} {prop / gcn if gcn else float('nan'):8.2f} {ratio:6.3f} "
              f"{spread:6.2f} {bound / 1e3:6.1f} {'yes' if prop <= bound else 'NO':>4s} {conv / 1e3:8.1f}   " + ", ".join(names))


def print_job(out):
    steps = []
    for shape in ("fullbatch", "sampled"):
        for phase in ("fwd", "bwd"):
            d = f"{out}/{shape}_256_{phase}"
            steps.append(f"mkdir -p {d} && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d {d} -- "
                         f"python profiles/bench_gcn2.py --shape {shape} --width 256 --phase {phase} > {d}/run.log 2>&1")
    dirs = " ".join(f"{out}/{s}_256_{p}" for s in ("fullbatch", "sampled") for p in ("fwd", "bwd"))
    steps.append(f"python profiles/bench_gcn2.py --summarize {dirs} > {out}/gcn2_kernel_stats.txt")
    print(" && \\\n".join(steps) + " || exit 1")          # (a failed or timed-out step ends the job: nothing starts after it)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["sampled", "fullbatch"], default="sampled")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--phase", choices=["fwd", "bwd"], default="fwd")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--summarize", nargs="+")
    ap.add_argument("--print-job")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.print_job:
        print_job(a.print_job)
    else:
        run(a)
