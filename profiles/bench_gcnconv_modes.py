#!/usr/bin/env python3
"""GCNConv's modes (improved, add_self_loops=False, normalize=False: ops.wgcn_* with a mode) beside the weighted-normalised path of
the default layer (ops.wgcn_* as before: "parent") and the unweighted default (ops.gcn_aggregate_*), on the graphs of
profiles/bench_wgcn.py, same build, same process: the weight pass, the forward, the backward with and without the edge-weight
gradient.

  measure (device events; medians with min - max over --repeats windows of --iters calls, the forms taking turns inside a repeat):
      python profiles/bench_gcnconv_modes.py [--out profiles/gcnconv_modes_ab.txt]

The expectation it checks: normalize=False ("plain") is no slower than the parent path beyond the spread the windows show — it
does strictly less (no dinv[col] read per gathered entry, no by-source / by-target sums, no q)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_wgcn import SHAPES, _time      # noqa: E402  (the same graphs, the same alternating windows)


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
    h = torch.randn(n, f, device="cuda", generator=g)
    dout = torch.randn(n, f, device="cuda", generator=g)
    bias = torch.zeros(f, device="cuda")
    modes = {"parent": (ops.WGCN_LOOP_FILL, 1.0), "improved": (ops.WGCN_LOOP_FILL, 2.0), "no_loops": (ops.WGCN_LOOP_SUM, 1.0),
             "plain": (ops.WGCN_UNNORMALIZED, 1.0)}
    calls = {"fwd_unweighted": lambda: ops.gcn_aggregate_fwd(h, prep, bias, True),
             "bwd_unweighted": lambda: ops.gcn_aggregate_bwd(dout, prep)}
    for name, (mode, fill) in modes.items():
        vals = ops.wgcn_weights(ws, w, mode, fill)
        calls["weights_" + name] = lambda mode=mode, fill=fill: ops.wgcn_weights(ws, w, mode, fill)
        calls["fwd_" + name] = lambda vals=vals: ops.wgcn_aggregate_fwd(h, ws, vals, bias, True)
        calls["bwd_" + name] = lambda vals=vals: ops.wgcn_aggregate_bwd(dout, ws, vals)
        calls["bwd_dw_" + name] = lambda vals=vals: ops.wgcn_aggregate_bwd(dout, ws, vals, h=h, want_dw=True)
    calls["weights_plain_no_edge_weight"] = lambda: ops.wgcn_weights(ws, None, ops.WGCN_UNNORMALIZED)
    return prep, calls


def measure(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gcnconv_modes: no GPU (there is no CPU path to time)")
    lines = [f"# {torch.cuda.get_device_name(0)}; device events around windows of {a.iters} calls on one stream (launch gaps inside), "
             f"{a.repeats} windows per form, the forms taking turns inside a repeat; us per call: median (min - max)",
             "# parent = the weighted-normalised path of the default layer; ratio = form / parent per repeat: median (min - max)"]
    for shape, (n, e, widths) in SHAPES.items():
        for f in widths:
            prep, calls = _setup(shape, f)
            t = _time(calls, a.iters, a.repeats)
            lines.append(f"{shape}: n = {n}, entries = {e}, aggregated = {int(prep.num_edges_no_loops)}, f = {f}")
            for k, v in t.items():
                stage = k.split("_")[0] if not k.startswith("bwd_dw") else "bwd_dw"
                ref = t.get(stage + "_parent")
                ratio = ""
                if ref is not None and k != stage + "_parent":
                    per = [x / y for x, y in zip(v, ref)]
                    ratio = f"   / parent {statistics.median(per):.3f} ({min(per):.3f} - {max(per):.3f})"
                lines.append(f"  {k:32s} {statistics.median(v):8.2f} ({min(v):.2f} - {max(v):.2f}){ratio}")
            print(json.dumps({"shape": shape, "f": f, "median_us": {k: round(statistics.median(v), 2) for k, v in t.items()}}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "gcnconv_modes_ab.txt"))
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    measure(ap.parse_args())
