"""Full-batch training (grapes_amd/full_graph.py train_step; reference full-batch.py:100-107): milliseconds per epoch — one
train_step plus torch Adam's step — on synthetic ogbn-products through the int32 autograd path and the forced row-blocked path,
and on synthetic papers100M (GCN(128, [256, 172]), the row-blocked 64-bit path) at the synthetic split (10 % train) and at OGB's
label counts (1,207,179 train / 125,265 valid / 214,338 test as random masks).

Each case: one warm-up epoch, then --reps repetitions of --epochs epochs timed with device events (the spread across
repetitions is reported), then one profiled epoch for the per-phase times (device events at the phase boundaries), the size of
the source set S and of the train rows' entries, the transposed gather's algorithmic bytes — (4C + 4) B per entry + (8C + 12) B
per source, the formula DESIGN.md's kernel table uses — and its fraction of 8 TB/s, and the peak HBM the epoch allocated beyond
what was resident.  Writes one JSON document (--out, else stdout).  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OGB = (1_207_179, 125_265, 214_338)


def _case(name, g, x, y, train, valid, F, C, large, epochs, reps, hidden=256):
    from grapes_amd import full_graph
    from grapes_amd.modules.gcn import GCN
    torch.manual_seed(0)
    c = GCN(F, [hidden, C]).cuda()
    opt = torch.optim.Adam(c.parameters(), lr=1e-3)
    valid_idx = valid.nonzero().squeeze(1)

    def epoch(i):
        opt.zero_grad()
        ev = valid_idx if (i + 1) % 5 == 0 else None                      # full-batch.py:116 at the default eval_frequency
        full_graph.train_step(c, x, g, y, train, eval_rows=ev, large_graph=large)
        opt.step()

    epoch(0)                                                                # warm-up (builds the graph's plan / int32 CSR)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(epochs):
            epoch(i)
        e.record(); torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / epochs)
    peak = torch.cuda.max_memory_allocated() - base
    out = {"case": name, "path": "row-blocked 64-bit" if large or (large is None and g.nnz >= full_graph.LARGE_NNZ) else
           "int32 autograd", "ms_per_epoch_reps": [round(v, 3) for v in ms], "ms_per_epoch_min": round(min(ms), 3),
           "ms_per_epoch_max": round(max(ms), 3), "epochs_per_rep": epochs, "peak_extra_hbm_gib": round(peak / 2 ** 30, 3),
           "train_rows": int(train.sum()), "valid_rows": int(valid.sum())}
    if full_graph.use_large_path(g, large):
        full_graph.PROFILE = {}
        try:
            opt.zero_grad()
            full_graph.train_step(c, x, g, y, train, eval_rows=valid_idx, large_graph=large)
            torch.cuda.synchronize()
            prof = full_graph.PROFILE
        finally:
            full_graph.PROFILE = None
        ph = prof["phases"]
        out["phases_ms"] = {ph[i][0]: round(ph[i - 1][1].elapsed_time(ph[i][1]), 3) for i in range(1, len(ph))}
        out["sources"], out["entries"] = prof["sources"], prof["entries"]
        cp = (C + 3) // 4 * 4
        nbytes = (4 * cp + 4) * prof["entries"] + (8 * cp + 12) * prof["sources"]
        t = out["phases_ms"]["transposed_gather"] / 1e3
        out["transposed_gather_bytes"] = nbytes
        out["transposed_gather_tb_s"] = round(nbytes / t / 1e12, 3)
        out["transposed_gather_of_8tb_s"] = round(nbytes / t / 8e12, 3)
        out["whole_graph_transposed_spmm_bytes"] = (4 * cp + 4) * int(g.nnz) + (8 * cp + 12) * int(g.num_nodes)
    del c, opt
    torch.cuda.empty_cache()
    return out


def _masks(N, counts, gen):
    perm = torch.randperm(N, device="cuda", generator=gen)
    ms = []
    o = 0
    for k in counts:
        m = torch.zeros(N, dtype=torch.bool, device="cuda"); m[perm[o:o + k]] = True
        ms.append(m); o += k
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="products,papers100m")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grapes_amd import synth
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.main import synthetic_data
    results = {"device": torch.cuda.get_device_name(0), "cases": []}
    cases = a.cases.split(",")
    if "products" in cases:
        d = synthetic_data("products", seed=0)
        g = DeviceGraph(d.rowptr, d.col, d.num_nodes)
        for large in (False, True):
            results["cases"].append(_case("products", g, d.x, d.y, d.train_mask, d.val_mask, d.num_features, d.num_classes,
                                          large, a.epochs, a.reps))
            print(json.dumps(results["cases"][-1]), file=sys.stderr)
        del d, g
        torch.cuda.empty_cache()
    if "papers100m" in cases:
        t0 = time.time()
        N, deg, maxdeg, F, C, *_ = synth.CONFIGS["papers100m"]
        rowptr, col = synth.synth_graph_device_chunked(N, deg, maxdeg, seed=0, device="cuda")
        g = DeviceGraph(rowptr, col, N)
        gen = torch.Generator(device="cuda"); gen.manual_seed(1)
        X = synth.randn_rows_(torch.empty(N, F, device="cuda"), generator=gen)
        y = torch.randint(0, C, (N,), device="cuda", generator=gen)
        torch.cuda.synchronize()
        results["papers100m_setup_s"] = round(time.time() - t0, 1)
        tr, va, _ = _masks(N, (int(0.10 * N), int(0.05 * N), 0), gen)
        results["cases"].append(_case("papers100m synthetic split", g, X, y, tr, va, F, C, None, max(1, a.epochs // 2), a.reps))
        print(json.dumps(results["cases"][-1]), file=sys.stderr)
        del tr, va
        tr, va, _ = _masks(N, OGB, gen)
        results["cases"].append(_case("papers100m OGB label counts", g, X, y, tr, va, F, C, None, a.epochs, a.reps))
        print(json.dumps(results["cases"][-1]), file=sys.stderr)
    text = json.dumps(results, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
