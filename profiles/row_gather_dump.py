#!/usr/bin/env python3
"""Bit-level record of the row-gather aggregation entry points (GAT, GCN2, PNA and SAGE; Cluster-GCN, weighted GCN, GATv2, VR-GCN
and GAS; forward and backward), to compare two builds of the library (GRAPES_LIB_PATH selects the build): every output array of one fixed-seed run is hashed (SHA-256 of its bytes) into a JSON file.

    python profiles/row_gather_dump.py --out A.json [--full A_full.json]   (on each build, on the GPU)
    python profiles/row_gather_dump.py --compare A.json B.json              (anywhere)

--out holds one line per entry point: the number of its arrays and the SHA-256 over their hashes in key order (digest below);
--full one hash per array, to find WHICH array differs when two digests do.  --digest-of FULL.json rewrites a full record as --out.

Graphs: n = 3000 with a hub row as target (in-degree > 2000), and n = 2600 with one hub as target AND source, so the long-row
chunk and combine kernels run on both CSRs.  Widths: one per instantiated template shape <VEC, LPR, NS> — f = 24, 64, 100, 256,
512 for GAT, GCN2 and SAGE, f = 32, 100, 256 for PNA — each with 16-byte-aligned operands (the float4 shapes) and, where the scalar
shape covers the width, with operands one float off alignment (the scalar shapes).  SAGE: mean and sum, with the long-row work
items and without them, plain (contiguous operands, nothing fused) and with add, bias and ReLU on column blocks of wider matrices.
Cluster-GCN (the loop-free copy of each graph, with the long-row items and without), weighted GCN (symmetric normalisation, with
the edge-weight gradient) and GATv2 (4 heads, concatenated and averaged) run at the same five widths and alignments.  VR-GCN and
GAS take the loop-free by-target CSR of each graph as the global graph, at the same widths and alignments, with the long-row items
and without: VR-GCN lists the first 700 nodes (the hub among them) of a batch that is the whole graph and keeps the first two
entries of a row; GAS runs a batch of 1 500 shuffled nodes with the hub, the others being halo.  Every input is finite."""
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


def dump(path, full=None):
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
        more(ops, gname, n, ei, rand, put)
    torch.cuda.synchronize()
    if full:
        with open(full, "w") as fh:
            json.dump(rec, fh, indent=0, sort_keys=True)
    write_digest(rec, path)


def digest(rec):
    """{entry point: "<arrays> <SHA-256 over the arrays' hashes in key order>"} of a full record {graph/f/off/entry point/.../k: hash};
    SAGE's and Cluster-GCN's keys name the pass further down (fwd_* / bwd*)."""
    groups = {}
    for key in sorted(rec):
        parts = key.split("/")
        name = parts[3] + "".join("_" + p[:3] for p in parts[4:] if p[:3] in ("fwd", "bwd"))
        groups.setdefault(name, []).append(rec[key])
    return {name: f"{len(h)} {hashlib.sha256(''.join(h).encode()).hexdigest()}" for name, h in groups.items()}


def write_digest(rec, path):
    d = digest(rec)
    with open(path, "w") as fh:
        json.dump(d, fh, indent=0, sort_keys=True)
    print(json.dumps({"written": path, "arrays": len(rec), "entry_points": len(d)}))


def more(ops, gname, n, ei, rand, put):
    """Cluster-GCN, weighted GCN, GATv2, VR-GCN and GAS on the graph (n, ei)."""
    import numpy as np
    import torch
    dev = "cuda"
    gen = torch.Generator().manual_seed(4321)
    flat = ei[:, ei[0] != ei[1]]                                             # loop-free; by target, the stored order inside a row
    flat = flat[:, np.argsort(flat[1], kind="stable")]
    src, dst = (torch.from_numpy(flat[k]).int().to(dev).contiguous() for k in (0, 1))
    prep = ops.PreparedGraph(src, dst, n)
    wst = ops.WeightedStructure(prep, src, dst)
    vals = ops.wgcn_weights(wst, torch.rand(src.numel(), generator=gen).to(dev) + 0.5)
    # the history aggregations: the same entries as the global CSR
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(flat[1], minlength=n))]).astype(np.int64)).to(dev)
    col = src
    deg = (rowptr[1:] - rowptr[:-1]).float()
    dinv = (deg + 1.0).rsqrt().contiguous()
    hub = int(torch.argmax(deg).item())
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    m = 700
    assert hub < m and int(deg[hub].item()) > 8 * 64
    rows = ids[:m].contiguous()
    first = rowptr[:m, None] + torch.arange(2, device=dev)[None, :]                       # the first two entries of a listed row
    keep = first < rowptr[1:m + 1, None]
    kprep = ops.PreparedGraph(col[first[keep]].contiguous(), rows.long()[:, None].expand(m, 2)[keep].int().contiguous(), n)
    pos = torch.full((n,), -1, dtype=torch.int32, device=dev)
    pos[:m] = ids[:m]
    perm = torch.randperm(n, generator=gen)[:1500]
    if hub not in perm.tolist():
        perm[0] = hub
    node_idx = perm.int().to(dev).contiguous()
    loc = torch.full((n,), -1, dtype=torch.int64, device=dev)
    loc[node_idx.long()] = torch.arange(1500, device=dev)
    cnt = (rowptr[1:] - rowptr[:-1])[node_idx.long()]
    rowptr_h = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0)])
    row_of = torch.repeat_interleave(torch.arange(1500, device=dev), cnt)
    at = rowptr[node_idx.long()][row_of] + (torch.arange(int(rowptr_h[-1].item()), device=dev) - rowptr_h[row_of])
    v = col[at].long()
    code = torch.where(loc[v] >= 0, loc[v], -1 - v).int().contiguous()
    gprep = ops.PreparedGraph(code[code >= 0].contiguous(), row_of[code >= 0].int().contiguous(), 1500)
    rowptr_h = rowptr_h.int().contiguous()
    assert int((code < 0).sum().item()) > 0 and int((code >= 0).sum().item()) > 0
    for f in (24, 64, 100, 256, 512):
        for off in (0, 1):
            if off and f > 256:                                              # scalar columns up to 256
                continue
            key = f"{gname}/f{f}/off{off}"
            x, g, add = (rand(gen, n, f, off=off) for _ in range(3))
            bias = rand(gen, f, off=off)
            for long_rows in (True, False):
                k2 = key + f"/cluster/long{int(long_rows)}"
                out = ops.cluster_aggregate_fwd(x, prep, 0.5, add=add, bias=bias, relu=True, long_rows=long_rows)
                put(k2 + "/fwd", out, ops.cluster_aggregate_fwd(x, prep, 0.0, long_rows=long_rows))
                put(k2 + "/bwd", *ops.cluster_aggregate_bwd(g, prep, 0.5, relu_out=out, add=add, want_add=True, want_bias=True,
                                                             long_rows=long_rows))
            out = ops.wgcn_aggregate_fwd(x, wst, vals, bias, True)
            put(key + "/wgcn_fwd", out, ops.wgcn_aggregate_fwd(x, wst, vals))
            put(key + "/wgcn_bwd", *ops.wgcn_aggregate_bwd(g, wst, vals, h=x, relu_out=out, want_dw=True))
            x_r, att = rand(gen, n, f, off=off), rand(gen, f, off=off) * 0.2
            for concat in (True, False):
                b2 = bias if concat else rand(gen, f // 4, off=off)
                g2 = g if concat else rand(gen, n, f // 4, off=off)
                out, agg, row_ms = ops.gatv2_aggregate_fwd(x, x_r, att, prep, 4, concat, 0.2, b2, True)
                put(key + f"/gatv2_fwd/concat{int(concat)}", out, row_ms, *([] if concat else [agg]))
                put(key + f"/gatv2_bwd/concat{int(concat)}", *ops.gatv2_aggregate_bwd(g2, out, agg, x, x_r, att, row_ms, prep, 4, concat, 0.2,
                                                                                       bias=b2, relu=True))
            hbar, da = rand(gen, n, f, off=off), rand(gen, m, f, off=off)
            st = torch.zeros(1, dtype=torch.int32, device=dev)
            for item_cap in (None, 0):
                A, coef = ops.vrgcn_aggregate_fwd(x, ids, hbar, dinv, rowptr, col, rows, rows, kprep, item_cap=item_cap, status=st)
                put(key + f"/vrgcn_fwd/items{int(item_cap is None)}", A, coef)
            put(key + "/vrgcn_bwd", ops.vrgcn_aggregate_bwd(da, coef, pos, ids, dinv, kprep, status=st))
            h, dg = rand(gen, 1500, f, off=off), rand(gen, 1500, f, off=off)
            for item_cap in (None, 0):
                put(key + f"/gas_fwd/items{int(item_cap is None)}",
                    ops.gas_aggregate_fwd(h, hbar, dinv, node_idx, rowptr_h, code, item_cap=item_cap, status=st))
            put(key + "/gas_bwd", ops.gas_aggregate_bwd(dg, node_idx, dinv, gprep, status=st))
            assert int(st.item()) == 0
    assert prep.status is None or int(prep.status.item()) == 0


def compare(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    print(f"{len(ra)} records in {a}, {len(rb)} in {b}: {len(diff)} differ")
    for k in diff:
        print("  differs:", k)
    return 1 if diff or not ra else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--full")
    ap.add_argument("--digest-of")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.digest_of:
        sys.exit(write_digest(json.load(open(a.digest_of)), a.out))
    sys.exit(compare(*a.compare) if a.compare else dump(a.out, a.full))
