#!/usr/bin/env python3
"""Bit-level record of the five operations whose twin entry points were folded into one (ABI 303): wgcn_weights,
wgcn_aggregate_fwd / _bwd, saint_subgraph and saint_masked_loss — to compare the build before the fold with the build after it
(block_prims_dump.py's sibling: same JSON of SHA-256 digests, compared with row_gather_dump.py --compare).  An operation is reached
under whichever name the tree has (getattr(ops, ...)), so the one script runs on both.

    python profiles/twin_fold_dump.py --out A.json               (on each build, on the GPU; seconds)
    python profiles/row_gather_dump.py --compare A.json B.json   (anywhere)

wgcn: graph A — 2,304 nodes (just past ops._SMALL_GRAPH: the long-row items exist), about 8,000 entries, a hub (node 3) with in- and
out-degree 200 (four chunks of GRAPES_LONG_ROW), node 5 with two stored self-loops, one duplicated entry, an isolated last node — and
graph B, 40 nodes (rows only); widths 7, 50, 130, 128, 256, 260 (one per branch of ROW_LAUNCH); LOOP_FILL with fill 1 and 2,
LOOP_SUM, UNNORMALIZED, each with edge weights and, where ops.wgcn_weights takes it, without; forward with bias + ReLU and bare;
backward with the ReLU gate and the weight gradient.
saint loss: 40 rows (37 live) over N = 300; C = 1, 7, 65; single- and multi-label; with and without node_norm; with and without
d_train; 9 and 0 training rows.
saint subgraph: plain, with ids, with ids and a table; at an e_cap that fits and at one that overflows (the status bit; the buffers
are longer than e_cap and prefilled, so a write at or past e_cap shows in the digest)."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(path):
    import numpy as np
    import torch
    from grapes_amd import ops
    dev = "cuda"
    rec = {}
    i32, i64 = torch.int32, torch.int64

    def put(key, *arrays):
        for k, t in enumerate(arrays):
            a = np.zeros(0) if t is None else t.detach().contiguous().cpu().numpy()
            rec[f"{key}/{k}"] = hashlib.sha256(a.tobytes()).hexdigest()

    # ------------------------------------------------------------------------------------------------ GCNConv with edge weights
    rng = np.random.default_rng(303)
    gen = torch.Generator().manual_seed(303)

    def graph_a():
        n, hub = 2304, 3
        s, d = rng.integers(0, n - 1, 7600), rng.integers(0, n - 1, 7600)
        keep = (s != hub) & (d != hub) & (s != d)
        s, d = s[keep], d[keep]
        others = rng.permutation(np.setdiff1d(np.arange(n - 1), [hub]))
        s = np.concatenate([s, np.full(200, hub), others[:200], [5, 5], s[:1]])          # hub out, hub in, two loops, a duplicate
        d = np.concatenate([d, others[200:400], np.full(200, hub), [5, 5], d[:1]])
        return n, s, d

    def graph_b():
        n = 40
        s, d = rng.integers(0, n - 1, 150), rng.integers(0, n - 1, 150)
        s[-3:], d[-3:] = [7, 7, s[0]], [7, 7, d[0]]
        return n, s, d

    modes = (("fill1", ops.WGCN_LOOP_FILL, 1.0), ("fill2", ops.WGCN_LOOP_FILL, 2.0), ("sum", ops.WGCN_LOOP_SUM, 1.0),
             ("unnorm", ops.WGCN_UNNORMALIZED, 1.0))
    for gname, (n, s, d) in (("A", graph_a()), ("B", graph_b())):
        order = rng.permutation(len(s))
        src, dst = (torch.from_numpy(v[order]).to(i32).to(dev).contiguous() for v in (s, d))
        st = torch.zeros(1, dtype=i32, device=dev)
        prep = ops.PreparedGraph(src, dst, n, status=st)
        ws = ops.WeightedStructure(prep, src, dst)
        if gname == "A":
            assert n > ops._SMALL_GRAPH and int(prep.n_items_t.item()) > 0 and int(prep.n_items_s.item()) > 0
        ew = (torch.rand(len(s), generator=gen) * 2 + 0.05).to(dev)
        for mname, mode, fill in modes:
            for wname, w in (("w", ew), ("ones", None)):
                if w is None and mname == "fill1":
                    continue                                                 # ops.wgcn_weights refuses it
                key = f"wgcn/{gname}/{mname}/{wname}"
                vals = ops.wgcn_weights(ws, w, mode, fill)
                put(key + "/weights", vals.val_t, vals.val_s, vals.lw, vals.dinv)
                for f in (7, 50, 130, 128, 256, 260):
                    h, dout = torch.randn(n, f, generator=gen).to(dev), torch.randn(n, f, generator=gen).to(dev)
                    bias = torch.randn(f, generator=gen).to(dev)
                    out = ops.wgcn_aggregate_fwd(h, ws, vals, bias=bias, relu=True)
                    put(key + f"/f{f}/fwd_bias_relu", out)
                    put(key + f"/f{f}/fwd", ops.wgcn_aggregate_fwd(h, ws, vals))
                    put(key + f"/f{f}/bwd", *ops.wgcn_aggregate_bwd(dout, ws, vals, h=h, relu_out=out, want_dw=True))
        assert int(st.item()) == 0

    # ------------------------------------------------------------------------------------------------ GraphSAINT's masked loss
    weighted = getattr(ops, "saint_masked_loss" + "_weighted", None)     # the twin's name, in the tree before the fold

    def masked_loss(z, C, ids, count, mask, lab, node_norm, **kw):
        if node_norm is None:
            return ops.saint_masked_loss(z, C, ids, count, mask, lab, **kw)
        if weighted is not None:
            return weighted(z, C, ids, count, mask, node_norm, lab, **kw)
        return ops.saint_masked_loss(z, C, ids, count, mask, lab, node_norm=node_norm, **kw)

    N, n_rows = 300, 40
    for C in (1, 7, 65):
        logits = (torch.randn(n_rows, C, generator=gen) * 3).contiguous()
        logits[0] = 0.75
        logits[1] = torch.linspace(-80.0, 80.0, C) if C > 1 else torch.tensor([80.0])
        logits = logits.to(dev)
        labels = {"single": torch.randint(0, C, (N,), generator=gen).to(dev), "multi": (torch.rand(N, C, generator=gen) < 0.4).float().to(dev)}
        perm = torch.randperm(N, generator=gen)[:n_rows]
        ids = perm.to(i32).to(dev)
        norm = (torch.rand(N, generator=gen) * 3 + 0.01).to(dev)
        count = torch.tensor([n_rows - 3], dtype=i32, device=dev)            # three rows past the count: zero gradient
        for kind, lab in labels.items():
            for T in (0, 9):
                mask = torch.zeros(N, dtype=torch.bool)
                mask[perm[:T]] = True
                mask = mask.to(dev)
                for nname, node_norm in (("mean", None), ("norm", norm)):
                    for with_train in (True, False):
                        st = torch.zeros(1, dtype=i32, device=dev)
                        d_train = torch.full((1,), -1, dtype=i32, device=dev) if with_train else None
                        loss, g = masked_loss(logits, C, ids, count, mask, lab, node_norm, d_train=d_train, status=st)
                        put(f"saint_loss/C{C}/{kind}/T{T}/{nname}/train{int(with_train)}", loss, g, d_train, st)

    # ------------------------------------------------------------------------------------------------ GraphSAINT's subgraph
    with_ids = getattr(ops, "saint_subgraph" + "_ids", None)              # the twin's name, in the tree before the fold

    def subgraph(*a, ids=False, edge_norm=None, **kw):
        if not ids and edge_norm is None:
            return ops.saint_subgraph(*a, **kw)
        if with_ids is not None:
            return with_ids(*a, edge_norm=edge_norm, **kw)
        return ops.saint_subgraph(*a, edge_norm=edge_norm, ids=True, **kw)

    n, e = 5000, 60000
    ei = np.stack([rng.integers(0, n - 1, e), rng.integers(0, n - 1, e)]).astype(np.int64)
    ei[0, :3000] = 3
    ei[1, 3000:6000] = 3
    ei[:, -50:] = ei[:, :50]
    ei = ei[:, np.lexsort((ei[1], ei[0]))]                                    # a CSR with a fixed entry order: built on the host
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]).astype(np.int64)).to(dev)
    col = torch.from_numpy(ei[1].astype(np.int32)).to(dev)
    table = torch.rand(col.numel(), generator=gen).to(dev)
    node_map = torch.zeros(n, dtype=i32, device=dev)
    _, node_idx, count = ops.saint_walk_nodes(rowptr, col, n, 700, 2, philox_seed=9, philox_offset=2, node_map=node_map)
    n_cap = node_idx.numel()
    edges = int(ops.saint_subgraph(rowptr, col, node_idx, count, node_map, 1 << 17)[2])
    assert 200 < edges < (1 << 17)
    for cname, e_cap in (("fits", 1 << 17), ("overflows", edges // 2)):
        for fname, kw in (("plain", {}), ("ids", dict(ids=True)), ("table", dict(edge_norm=table))):
            size = e_cap + 64                                                # a guard region behind every edge buffer
            bufs = (torch.full((size,), -7, dtype=i32, device=dev), torch.full((size,), -7, dtype=i32, device=dev),
                    torch.zeros(1, dtype=i32, device=dev), torch.zeros(n_cap + 1, dtype=i32, device=dev))
            if kw:
                bufs += (torch.full((size,), -7, dtype=i64, device=dev),
                         torch.full((size,), -7.0, device=dev) if "edge_norm" in kw else None)
            st = torch.zeros(1, dtype=i32, device=dev)
            out = subgraph(rowptr, col, node_idx, count, node_map, e_cap, status=st, out=bufs, **kw)
            k = int(out[2])
            assert k == min(edges, e_cap) and (int(st.item()) & 1) == (edges > e_cap)
            put(f"saint_subgraph/{cname}/{fname}", *out, st)              # (the whole buffers: written or still the prefill)

    torch.cuda.synchronize()
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
    print(json.dumps({"written": path, "arrays": len(rec)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    sys.exit(dump(ap.parse_args().out))
