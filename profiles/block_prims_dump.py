#!/usr/bin/env python3
"""Bit-level record of the entry points whose kernels take their scans, searches and row losses from csrc/block_prims.h and
csrc/row_loss.h, to compare two builds of the library (row_gather_dump.py's sibling: same JSON of SHA-256 digests, same --compare).

    python profiles/block_prims_dump.py --out A.json             (on each build, on the GPU; seconds)
    python profiles/row_gather_dump.py --compare A.json B.json   (anywhere)

Losses (classifier_loss, step_losses in both forms, rowlist_loss with and without dropout, saint_masked_loss): C = 1, 2, 7, 63,
64, 65, 200 — across the one-value-per-lane pass and the 64-lane stride — single- and multi-label, 1 and 9 target rows (and 0
training rows for the masked loss: NaN with a zero gradient; the other entry points refuse an empty row list); row 0 of the
logits is all-equal, row 1 spreads over +-80.
Scans, sort and search: node sets of 1 id, of one id many times, of SAINT_MAX_IDS ids; draws below the first entry, on a row
boundary and on the last entry; the edge sampler's table over more rows than one round of its scan; frontiers that are empty,
that fill exactly 256 / 1024 / 4096 words, and a scattered one, in the small- and the large-bitmap forms; PreparedGraph and
csr_build of a graph with a hub, duplicates and an isolated last node (entries whose order inside a row is left to atomics are
sorted inside the row first); the row exchange and the halo rows of two peers."""
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
            a = t.detach().contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
            rec[f"{key}/{k}"] = hashlib.sha256(a.tobytes()).hexdigest()

    def rows_sorted(rowptr, vals):
        """vals with every CSR row's entries in ascending order (rows filled through atomic cursors)"""
        rp, v = rowptr.cpu().numpy().astype(np.int64), vals.cpu().numpy()[: int(rowptr[-1])].copy()
        for a, b in zip(rp[:-1], rp[1:]):
            v[a:b].sort()
        return v

    # ------------------------------------------------------------------------------------------------ losses
    gen = torch.Generator().manual_seed(20261)
    N = 300
    for C in (1, 2, 7, 63, 64, 65, 200):
        n_rows = 40
        logits = (torch.randn(n_rows, C, generator=gen) * 3).contiguous()
        logits[0] = 0.75
        logits[1] = torch.linspace(-80.0, 80.0, C) if C > 1 else torch.tensor([80.0])
        logits = logits.to(dev)
        labels = {"single": torch.randint(0, C, (N,), generator=gen).to(dev),
                  "multi": (torch.rand(N, C, generator=gen) < 0.4).float().to(dev)}
        perm = torch.randperm(N, generator=gen)[:n_rows].to(i32)
        node_map = torch.full((N,), -1, dtype=i32)
        node_map[perm.long()] = torch.arange(n_rows, dtype=i32)
        node_map, ids = node_map.to(dev), perm.to(dev)
        hop_stats = torch.randn(2, 8, generator=gen).to(dev)
        z_out = torch.randn(70, generator=gen).to(dev)
        dinv = (torch.rand(N, generator=gen) + 0.1).to(dev)
        mask_all = torch.zeros(N, dtype=torch.bool)
        for kind, lab in labels.items():
            for B in (1, 9):
                key = f"loss/C{C}/{kind}/B{B}"
                tgt = ids[:B].contiguous()
                local = node_map[tgt.long()].contiguous()
                put(key + "/classifier_loss", *ops.classifier_loss(logits, local, tgt, lab))
                for many in (True, False):
                    put(key + f"/step_losses/mb{int(many)}", *ops.step_losses(logits, node_map, tgt, lab, hop_stats, 0.5, z_out=z_out,
                                                                             log_z_init=0.25, many_workgroups=many))
                for p in (0.0, 0.5):
                    put(key + f"/rowlist_loss/p{p}", *ops.rowlist_loss(logits[:B].contiguous(), C, tgt, lab, dinv, p=p, seed=11, offset=3))
            for T in (0, 1, 9):
                mask = mask_all.clone()
                mask[perm[:T].long()] = True
                count = torch.tensor([n_rows - 3], dtype=i32, device=dev)          # three rows past the count: zero gradient
                st, d_train = torch.zeros(1, dtype=i32, device=dev), torch.zeros(1, dtype=i32, device=dev)
                put(f"loss/C{C}/{kind}/T{T}/saint_masked_loss", *ops.saint_masked_loss(logits, C, ids, count, mask.to(dev), lab,
                                                                                     d_train=d_train, status=st), d_train, st)

    # ------------------------------------------------------------------------------------------------ graphs
    rng = np.random.default_rng(77)

    def graph(n, e, hub_deg):
        """directed edges among nodes 0 .. n - 2 (the last node is isolated), a hub (node 3), duplicates and self loops"""
        s, d = rng.integers(0, n - 1, e), rng.integers(0, n - 1, e)
        s[:hub_deg] = 3
        d[hub_deg:2 * hub_deg] = 3
        s[-50:], d[-50:] = s[:50], d[:50]
        d[-80:-50] = s[-80:-50]
        return np.stack([s, d]).astype(np.int64)

    for n, e, hub in ((3, 2, 0), (5000, 60000, 3000), (20001, 200000, 5000)):
        ei = graph(n, e, hub) if n > 3 else np.array([[0, 1], [1, 0]], dtype=np.int64)
        rowptr, col = ops.csr_build(torch.from_numpy(ei).to(dev), n)
        put(f"csr_build/n{n}", rowptr, col)
        src, dst = (torch.from_numpy(ei[k]).to(i32).to(dev).contiguous() for k in (0, 1))
        st = torch.zeros(1, dtype=i32, device=dev)
        g = ops.PreparedGraph(src, dst, n, status=st)
        nt, ns = int(g.n_items_t), int(g.n_items_s)
        items = [np.sort(t[: 2 * k].cpu().numpy().reshape(-1, 2).astype(np.int64) @ np.array([1 << 32, 1]))
                 for t, k in ((g.items_t, nt), (g.items_s, ns))]
        put(f"prepared/n{n}", g.rowptr_t, g.rowptr_s, g.dinv, rows_sorted(g.rowptr_t, g.csr_src), rows_sorted(g.rowptr_s, g.csr_dst),
            g.n_long[:2], *items, st)
        if n == 3:
            continue
        # ---- GraphSAINT samplers on this graph
        for name, B, L, roots in (("one", 1, 0, [n - 1]), ("dups", 700, 0, [5] * 700), ("full", 4096, 3, None), ("wide", 16384, 0, None)):
            node_map = torch.zeros(n, dtype=i32, device=dev)
            r = None if roots is None else torch.tensor(roots, dtype=i32, device=dev)
            st = torch.zeros(1, dtype=i32, device=dev)
            walks, node_idx, count = ops.saint_walk_nodes(rowptr, col, n, B, L, roots=r, philox_seed=9, philox_offset=2,
                                                          node_map=node_map, status=st)
            k = int(count)
            put(f"saint_walk/n{n}/{name}", walks, node_idx[:k], count, node_map[node_idx[:k].long()], st)
            sub = ops.saint_subgraph(rowptr, col, node_idx, count, node_map, 1 << 17, status=st)
            put(f"saint_subgraph/n{n}/{name}", sub[0][: int(sub[2])], sub[1][: int(sub[2])], sub[2], sub[3], st)
        weights = ops.saint_edge_weights(rowptr, col, n)
        put(f"saint_edge_weights/n{n}", *weights)
        nnz, total_w = int(rowptr[-1]), int(weights[2][-1])
        rp = rowptr.cpu().numpy()
        for sampler, w, total, cdf in (("node", None, nnz, rp), ("edge", weights, total_w, weights[2].cpu().numpy())):
            # below / on the first entry, on row boundaries, one below them, the last entry; then one value many times
            t = np.concatenate([[0, 1, total - 1], cdf[1:40], cdf[1:40] - 1, cdf[-3:] - 1]).astype(np.int64)
            t = np.unique(t[(t >= 0) & (t < total)])
            for name, draws in (("edges", t), ("dups", np.full(600, t[len(t) // 2])), ("one", t[:1])):
                node_map = torch.zeros(n, dtype=i32, device=dev)
                st = torch.zeros(1, dtype=i32, device=dev)
                out = ops.saint_draw_nodes(rowptr, col, n, len(draws), weights=w, draws=torch.from_numpy(draws).to(dev),
                                           node_map=node_map, status=st)
                k = int(out[2])
                put(f"saint_draw/n{n}/{sampler}/{name}", out[0], out[1][:k], out[2], out[3], node_map[out[1][:k].long()], st)
            B = 16384 if w is None else 8192
            node_map = torch.zeros(n, dtype=i32, device=dev)
            out = ops.saint_draw_nodes(rowptr, col, n, B, weights=w, philox_seed=5, philox_offset=7, node_map=node_map)
            k = int(out[2])
            put(f"saint_draw/n{n}/{sampler}/philox", out[0], out[1][:k], out[2], out[3], node_map[out[1][:k].long()])

    # ------------------------------------------------------------------------------------------------ frontier compaction
    for n in (64 * 1024 + 1, 64 * 8192 + 7):                                 # <= 4096 words: the small-bitmap form; above: the large one
        W = (n + 63) // 64
        fronts = {"empty": np.zeros(0, np.int64), "w256": np.arange(64 * 256), "w1024": np.arange(64 * 1024),
                  "w4096": np.arange(min(64 * 4096, n)), "scattered": np.unique(rng.integers(0, n, 5000)), "last": np.array([n - 1])}
        for name, ids in fronts.items():
            for one in (True, False):
                bits, pbits = torch.zeros(W, dtype=i64, device=dev), torch.zeros(W, dtype=i64, device=dev)
                node_map = torch.full((n,), -1, dtype=i32, device=dev)
                st = torch.zeros(1, dtype=i32, device=dev)
                if len(ids):
                    t = torch.from_numpy(ids).to(i32).to(dev)
                    ops.bitmap_mark(bits, None, t, n)
                    ops.bitmap_mark(pbits, None, t[::3].contiguous(), n)
                n_cap = len(ids) + 8
                b, nb, nbl, c = ops.frontier_compact(bits, None, pbits, n, n_cap, node_map=node_map, status=st, one_launch=one)
                cb, cn = int(c[0]), int(c[1])
                put(f"frontier_compact/n{n}/{name}/one{int(one)}", b[:cb], nb[:cn], nbl[:cn], c, node_map, bits, st)

    # ------------------------------------------------------------------------------------------------ exchange (two peers)
    n, P, cap, e_cap = 5000, 2, 300, 40000
    ei = graph(n, 60000, 3000)
    rowptr, col = ops.csr_build(torch.from_numpy(ei).to(dev), n)
    bounds = [0, 2400, n]
    bounds32 = torch.tensor(bounds, dtype=i32, device=dev)
    stride = 2 * cap + e_cap
    queries = [np.concatenate([[3, n - 1, 3, 0, 2399, 2400], rng.permutation(n)[: cap - 6]]).astype(np.int32) for _ in range(P)]
    counts = [cap, cap - 11]
    req = torch.cat([torch.cat([torch.from_numpy(q), torch.tensor([m], dtype=i32)]) for q, m in zip(queries, counts)]).to(dev)
    st = torch.zeros(1, dtype=i32, device=dev)
    replies = []
    for o in range(P):
        lo, hi = bounds[o], bounds[o + 1]
        rp = (rowptr[lo:hi + 1] - rowptr[lo]).contiguous()
        cl = col[int(rowptr[lo]):int(rowptr[hi])].contiguous()
        reply = torch.zeros(P * stride, dtype=i32, device=dev)
        ops.exchange_serve_rows(rp, cl, req, P, cap, lo, hi, reply, stride, e_cap, status=st)
        replies.append(reply.view(P, stride))
    for r in range(P):
        back = torch.stack([replies[o][r] for o in range(P)]).reshape(-1).contiguous()
        d_m = torch.tensor([counts[r]], dtype=i32, device=dev)
        src, dst, d_e, eoff = ops.exchange_recv_rows(back, stride, torch.from_numpy(queries[r]).to(dev), bounds32, P, e_cap, d_m=d_m, status=st)
        put(f"exchange_recv_rows/r{r}", src[: int(d_e)], dst[: int(d_e)], d_e, eoff[: counts[r] + 1], st)
    # halo rows: ascending request lists with ids below the owner's range, on both of its ends and above it
    F, n_slot = 12, 64
    X = torch.randn(bounds[1] - bounds[0], F, generator=gen).to(dev)
    for name, lst in (("inside", [5, 6, 900, 2399]), ("around", [0, 2399, 2400, 2401, 4999]), ("above", [2400, 3000]), ("none", [])):
        reqf = torch.zeros(P * (cap + 1), dtype=i32).view(P, cap + 1)
        for p in range(P):
            reqf[p, : len(lst)] = torch.tensor(lst, dtype=i32)
            reqf[p, cap] = len(lst)
        reply = torch.zeros(P * n_slot * F, device=dev)
        st = torch.zeros(1, dtype=i32, device=dev)
        ops.exchange_serve_features(X, reqf.reshape(-1).to(dev), P, cap, bounds[0], bounds[1], reply, n_slot, status=st)
        put(f"exchange_serve_features/{name}", reply, st)

    torch.cuda.synchronize()
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
    print(json.dumps({"written": path, "arrays": len(rec)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    sys.exit(dump(ap.parse_args().out))
