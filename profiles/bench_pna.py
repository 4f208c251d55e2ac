#!/usr/bin/env python3
"""PNAConv's fused aggregation (grapes_pna_aggregate_fwd / _bwd) and one whole conv against the same layer composed from torch ops
on the GPU (index_select, cat, F.linear, scatter_reduce x4, the scalers), in one process on one device.

    python profiles/bench_pna.py [--out profiles/pna_bench.json] [--iters 30] [--repeats 7]

Shape: the classifier's subgraph of the products workload as profiles/bench_gcn2.py takes it (batch 256 + 3 hops x 256 samples:
1,024 nodes, 16,384 random edges), at F = 100 (products' input width) and F = 256 (hidden layers), C = 256; aggregators mean, min,
max, std and scalers identity, amplification, attenuation.

Method: device events around `iters` back-to-back calls, after a warm-up of the same length; `repeats` such timings per form,
the forms interleaved (fused, torch, fused, ...) so that clock drift hits both; reported: the median and the min .. max of the
per-call time.  The yardstick is the torch composition, not the code under test:
    gather-and-reduce part (what the fused forward replaces)  = index_select x2, cat, F.linear (pre_nn on e x 2F), 4 scatter_reduce,
                                                                 the std arithmetic, the scalers and the cat into post_nn's operand
    fused forward                                              = the [a | b] GEMM + grapes_pna_aggregate_fwd
Acceptance: fused forward (GEMM included) <= the torch gather-and-reduce part, medians, no margin; likewise forward + backward.
Everything else is recorded, not gated: us per launch, the algorithmic bytes (each b_j row once per edge, the 13F output row, the
6F statistics, x, a: e (4F + 4) + n (4 (13 + 6 + 2) F + 8)) against the time as a fraction of 8 TB/s.  Registers and occupancy of
the kernels come from profiles/kernel_regs.sh (static, from the code object)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AGG, SCAL = ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"]


def timed(fn, iters):
    import torch
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def torch_aggregate(x, w_pre, b_pre, src, dst, n, sc):
    """PyG's message / aggregate / scale steps with torch ops: post_nn's operand [n, 13 F]."""
    import torch
    import torch.nn.functional as Fn
    m = Fn.linear(torch.cat([x.index_select(0, dst), x.index_select(0, src)], 1), w_pre, b_pre)
    idx = dst[:, None].expand_as(m)
    zero = torch.zeros((n, m.shape[1]), dtype=m.dtype, device=m.device)
    mean = zero.scatter_reduce(0, idx, m, "mean", include_self=False)
    mn = zero.scatter_reduce(0, idx, m, "amin", include_self=False)
    mx = zero.scatter_reduce(0, idx, m, "amax", include_self=False)
    msq = zero.scatter_reduce(0, idx, m * m, "mean", include_self=False)
    std = (torch.relu(msq - mean * mean) + 1e-5).sqrt()
    A = torch.cat([mean, mn, mx, std], 1)
    return torch.cat([x] + [A * sc[:, k:k + 1] for k in range(sc.shape[1])], 1)


def run(a):
    import torch
    import torch.nn.functional as Fn
    from grapes_amd import ops
    from grapes_amd.modules.gcn import PNAConv, pna_degree_histogram
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(0)
    n, e, C = 1024, 16384, 256
    ei = torch.randint(0, n, (2, e), device=dev, generator=g, dtype=torch.int32)
    prep = ops.gcn2_attach_loops(ops.PreparedGraph(ei[0].contiguous(), ei[1].contiguous(), n), ei[0].contiguous(), ei[1].contiguous())
    src, dst = ei[0].long(), ei[1].long()
    deg = pna_degree_histogram(ei.long(), n)
    d = torch.bincount(dst, minlength=n).float()
    results = {"shape": {"n": n, "e": e, "C": C, "aggregators": AGG, "scalers": SCAL}, "iters": a.iters, "repeats": a.repeats,
               "device": torch.cuda.get_device_name(0), "widths": {}}
    for F in (100, 256):
        conv = PNAConv(F, C, AGG, SCAL, deg).to(dev)
        cfg = conv.cfg
        sc = torch.stack([torch.ones_like(d), (d + 1).log() / cfg.avg_log, cfg.avg_log / (d.clamp(min=1) + 1).log()], 1)
        x = torch.randn(n, F, device=dev, generator=g)
        w_pre, b_pre = conv.pre_nn.weight.detach(), conv.pre_nn.bias.detach()
        w2 = torch.cat([w_pre[:, :F], w_pre[:, F:]], 0).contiguous()
        bias2 = torch.cat([b_pre, torch.zeros_like(b_pre)])
        ab = ops.linear_bias_act_fwd(x, w2, bias2, False)
        z, stats = ops.pna_aggregate_fwd(x, ab, prep, cfg)
        zt = torch_aggregate(x, w_pre, b_pre, src, dst, n, sc)
        check = float((z - zt).abs().max())
        dz = torch.randn(z.shape, device=dev, generator=g)
        dout = torch.randn(n, C, device=dev, generator=g)
        xr = x.clone().requires_grad_(True)
        params = [conv.pre_nn.weight, conv.pre_nn.bias, conv.post_nn.weight, conv.post_nn.bias, conv.lin.weight, conv.lin.bias]

        def torch_agg_fb():
            xl, wl, bl = xr.detach().requires_grad_(True), w_pre.clone().requires_grad_(True), b_pre.clone().requires_grad_(True)
            torch.autograd.grad(torch_aggregate(xl, wl, bl, src, dst, n, sc), [xl, wl, bl], dz)

        def torch_conv_fb():
            zz = torch_aggregate(xr, conv.pre_nn.weight, conv.pre_nn.bias, src, dst, n, sc)
            out = torch.relu(Fn.linear(Fn.linear(zz, conv.post_nn.weight, conv.post_nn.bias), conv.lin.weight, conv.lin.bias))
            torch.autograd.grad(out, [xr] + params, dout)

        def fused_conv_fb():
            torch.autograd.grad(conv(xr, prep, relu=True), [xr] + params, dout)

        def fused_agg_fb():
            ab_ = ops.linear_bias_act_fwd(x, w2, bias2, False)
            z_, st_ = ops.pna_aggregate_fwd(x, ab_, prep, cfg)
            dab = ops.pna_aggregate_bwd(dz, ab_, st_, prep, cfg)
            ops.linear_bwd_weight_gated(dab, x)
            ops.linear_bwd_input(dab, w2)

        forms = {
            "fused_aggregate_fwd_launch": lambda: ops.pna_aggregate_fwd(x, ab, prep, cfg),
            "fused_aggregate_bwd_launches": lambda: ops.pna_aggregate_bwd(dz, ab, stats, prep, cfg),
            "fused_fwd_with_gemm": lambda: ops.pna_aggregate_fwd(x, ops.linear_bias_act_fwd(x, w2, bias2, False), prep, cfg),
            "torch_gather_reduce_fwd": lambda: torch_aggregate(x, w_pre, b_pre, src, dst, n, sc),
            "fused_fwd_bwd_with_gemms": fused_agg_fb,
            "torch_gather_reduce_fwd_bwd": torch_agg_fb,
            "fused_conv_fwd_bwd": fused_conv_fb,
            "torch_conv_fwd_bwd": torch_conv_fb,
        }
        times = {k: [] for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():                     # interleaved
                times[k].append(timed(fn, a.iters))
        row = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
        bytes_fwd = e * (4 * F + 4) + n * (4 * (13 + 6 + 2) * F + 8)
        t = row["fused_aggregate_fwd_launch"]["median_us"] * 1e-6
        row["fwd_algorithmic_bytes"] = bytes_fwd
        row["fwd_fraction_of_8TBps"] = bytes_fwd / t / 8e12
        row["max_abs_difference_fused_vs_torch_operand"] = check
        row["accept_fwd"] = row["fused_fwd_with_gemm"]["median_us"] <= row["torch_gather_reduce_fwd"]["median_us"]
        row["accept_fwd_bwd"] = row["fused_fwd_bwd_with_gemms"]["median_us"] <= row["torch_gather_reduce_fwd_bwd"]["median_us"]
        results["widths"][str(F)] = row
        print(f"F={F}: " + ", ".join(f"{k} {v['median_us']:.1f} us" for k, v in row.items() if isinstance(v, dict)))
        print(f"F={F}: accept fwd {row['accept_fwd']}, fwd+bwd {row['accept_fwd_bwd']}, operand difference {check:.2e}, "
              f"fwd launch at {100 * row['fwd_fraction_of_8TBps']:.2f} % of 8 TB/s")
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "pna_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    run(ap.parse_args())
