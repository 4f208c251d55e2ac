#!/usr/bin/env python3
"""Bit-level record of the eight row-gather aggregation entry points (GAT, GCN2, PNA and SAGE, forward and backward), to compare
two builds of the library: every output array of one fixed-seed run is hashed (SHA-256 of its bytes) into a JSON file.

    python profiles/row_gather_dump.py --out A.json             (on each build, on the GPU)
    python profiles/row_gather_dump.py --compare A.json B.json  (anywhere)

Graphs: n = 3000 with a hub row as target (in-degree > 2000), and n = 2600 with one hub as target AND source, so the long-row
chunk and combine kernels run on both CSRs.  Widths: one per instantiated template shape <VEC, LPR, NS> — f = 24, 64, 100, 256,
512 for GAT, GCN2 and SAGE, f = 32, 100, 256 for PNA — each with 16-byte-aligned operands (the float4 shapes) and, where the scalar
shape covers the width, with operands one float off alignment (the scalar shapes).  SAGE: mean and sum, with the long-row work
items and without them, plain (contiguous operands, nothing fused) and with add, bias and ReLU on column blocks of wider matrices.
Every input is finite."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def graphs():
    import numpy as np
    from tests.gat_oracle import random_graph
    one = random_graph(3000, seed=1, mean_deg=6, hub=17, hub_deg=2100, n_dup=60, n_loops=40, n_isolated=25, directed_block=30)
    n, hub = 2600, 5
    rng = np.random.default_rng(71)
    base = random_graph(n, seed=72, mean_deg=4, hub=hub, hub_deg=900, n_dup=20, n_loops=30, n_isolated=10)
    out_edges = np.stack([np.full(700, hub), rng.integers(0, n - 10, 700)])
    both = np.concatenate([base, out_edges, np.array([[hub, hub], [hub, hub]]).T.reshape(2, -1)], axis=1).astype(np.int64)
    return {"n3000_hub": (3000, one), "n2600_hub_both": (n, both)}


def dump(path):
    import torch
    from grapes_amd import ops
    dev = "cuda"
    rec = {}

    def put(key, *arrays):
        for k, t in enumerate(arrays):
            rec[f"{key}/{k}"] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    def rand(gen, *shape, off=0):
        """A contiguous fp32 tensor whose first element sits `off` floats past a 16-byte boundary."""
        numel = 1
        for s in shape:
            numel *= s
        buf = torch.empty(numel + 4, device=dev)
        t = buf[off:off + numel].view(*shape)
        t.copy_(torch.randn(*shape, generator=gen).to(dev))
        assert t.data_ptr() % 16 == 4 * off
        return t

    for gname, (n, ei) in graphs().items():
        src, dst = (torch.from_numpy(ei[k]).int().to(dev).contiguous() for k in (0, 1))
        prep = ops.gcn2_attach_loops(ops.PreparedGraph(src, dst, n), src, dst)
        assert int(prep.n_items_t.item()) > 8
        gen = torch.Generator().manual_seed(1234)
        for f in (24, 64, 100, 256, 512):
            for off in (0, 1):
                key = f"{gname}/f{f}/off{off}"
                if not (off and f > 256):                                    # GAT: scalar columns up to 256
                    h, G = rand(gen, n, f, off=off), rand(gen, n, f, off=off)
                    a_s, a_d, b = (rand(gen, f) * 0.2 for _ in range(3))
                    s_src, s_dst = ops.gat_scores(h, a_s, a_d)
                    put(key + "/gat_scores", s_src, s_dst)
                    for relu in (False, True):
                        out, row_ms = ops.gat_aggregate_fwd(h, s_src, s_dst, prep, b, relu)
                        put(key + f"/gat_fwd/relu{int(relu)}", out, row_ms)
                        put(key + f"/gat_bwd/relu{int(relu)}", *ops.gat_aggregate_bwd(G, out, h, s_src, s_dst, row_ms, a_s, a_d, prep, b, relu))
                x, x0, ds, ds2 = (rand(gen, n, f, off=off) for _ in range(4))
                put(key + "/gcn2_fwd", *ops.gcn2_propagate_fwd(x, x0, prep, 0.3, want_p=True))
                put(key + "/gcn2_bwd", *ops.gcn2_propagate_bwd(ds, prep, 0.3))
                put(key + "/gcn2_bwd_two", *ops.gcn2_propagate_bwd(ds, prep, 0.3, ds_add=ds2, add_is_p=True, dx0=x0.clone()))
                if off and f > 256:                                          # SAGE: scalar columns up to 256
                    continue
                wide, dwide, bias = rand(gen, n, 3 * f, off=off), rand(gen, n, 3 * f, off=off), rand(gen, f, off=off)
                for aggr in ("mean", "sum"):
                    for long_rows in (True, False):
                        k2 = key + f"/sage_{aggr}/long{int(long_rows)}"
                        out = ops.sage_aggregate_fwd(x, prep, aggr, long_rows=long_rows)
                        put(k2 + "/fwd_plain", out)
                        put(k2 + "/bwd_plain", ops.sage_aggregate_bwd(ds, prep, aggr, long_rows=long_rows)[0])
                        # column blocks of wider matrices: src and add in, out and the root copy out; add, bias and ReLU fused
                        o2, d2 = torch.zeros(n, 2 * f, device=dev), torch.zeros(n, 2 * f, device=dev)
                        ops.sage_aggregate_fwd(wide[:, f:2 * f], prep, aggr, add=wide[:, 2 * f:], bias=bias, relu=True, out=o2[:, f:],
                                               copy_out=o2[:, :f], long_rows=long_rows)
                        _, _, dbias = ops.sage_aggregate_bwd(dwide[:, :f], prep, aggr, relu_out=o2[:, f:], add=dwide[:, 2 * f:],
                                                             dsrc=d2[:, :f], dadd=d2[:, f:], want_bias=True, long_rows=long_rows)
                        put(k2 + "/fwd_blocks", o2)
                        put(k2 + "/bwd_blocks", d2, dbias)
        for f in (32, 100, 256):
            for off in (0, 1):
                key = f"{gname}/f{f}/off{off}"
                avg_log, avg_lin = 1.9, 6.5
                cfg = ops.PNAConfig(["mean", "min", "max", "std", "var", "sum"], ["identity", "amplification", "attenuation", "linear",
                                                                                   "inverse_linear"], avg_log, avg_lin)
                x, ab = rand(gen, n, f, off=off), rand(gen, n, 2 * f, off=off)
                z, stats = ops.pna_aggregate_fwd(x, ab, prep, cfg)
                dz = rand(gen, n, cfg.blocks * f, off=off)
                put(key + "/pna_fwd", z, stats)
                put(key + "/pna_bwd", ops.pna_aggregate_bwd(dz, ab, stats, prep, cfg))
        assert prep.status is None or int(prep.status.item()) == 0
    torch.cuda.synchronize()
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
    print(json.dumps({"written": path, "arrays": len(rec)}))


def compare(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    print(f"{len(ra)} arrays in {a}, {len(rb)} in {b}: {len(diff)} differ")
    for k in diff:
        print("  differs:", k)
    return 1 if diff or not ra else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.out))
