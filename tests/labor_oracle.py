"""TEST INFRASTRUCTURE — LABOR, the layer-neighbour sampler, restated on the host in NumPy / pure Python [Balin and Catalyurek, NeurIPS
2023; LABOR-recall: DGL's LaborSampler].  The rule of include/grapes_hip.h (grapes_labor_sample_layer / grapes_labor_importance) is the
contract; this file states it a second time, with DIFFERENT algorithms where the kernel's could be wrong:

  philox4x32_10 / node_words   Philox4x32-10 in uint64 NumPy arithmetic: r_t = word t & 3 of philox4x32_10(base + (t >> 2), seed)
  keep_int                     LABOR-0: d <= k keeps everything, else r_t d < k << 32 in Python integers
  keep_f32                     LABOR-i: (r_t >> 8) 2^-24 < fminf(1, c pi_t), ONE fp32 multiply, given fp32 c and pi
  solve_c_sorted               c_s (fp64) by SORTING pi and trying every saturated prefix — not the kernel's fixed point
  solve_c_fixed_point          the kernel's monotone fixed point, in any dtype (fp64 to compare with the sorted solve, fp32 to measure
                               what fp32 alone costs)
  importance                   the pi iterations for one layer, in any dtype
  hajek                        w_st = (1 / p_st) / sum over the row's kept entries of 1 / p_st
  sample_layer / sample        one layer; the layers chained from the targets inward as modules/labor.py chains them
Only tests import this module; it imports nothing of the product.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, seed):
    """uint32 [n, 4]: the four words of Philox4x32-10 at the 64-bit counters ctr (c2 = c3 = 0) under the 64-bit key seed."""
    ctr = np.asarray(ctr, dtype=np.uint64).reshape(-1)
    c0, c1 = ctr & _M32, ctr >> np.uint64(32)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & _M32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & _M32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def node_words(seed, base, num_nodes):
    """uint32 [N]: r_t of every node t for the layer whose base counter is `base`."""
    n4 = (int(num_nodes) + 3) // 4
    ctr = (np.arange(n4, dtype=np.uint64) + np.uint64(int(base) & (2 ** 64 - 1)))
    return philox4x32_10(ctr, seed).reshape(-1)[:int(num_nodes)]


def layer_base(philox_offset, d, num_nodes, layer_dependency):
    return int(philox_offset) + (0 if layer_dependency else d * ((int(num_nodes) + 3) // 4))


def offset_advance(num_layers, num_nodes):
    return int(num_layers) * ((int(num_nodes) + 3) // 4)


# --------------------------------------------------------------------------------------------- the keep rules
def keep_int(words_row, fanout):
    """bool [d]: LABOR-0 over the words of one row's entries, in Python integers."""
    d = len(words_row)
    if d <= fanout:
        return np.ones(d, dtype=bool)
    return np.array([int(w) * d < (int(fanout) << 32) for w in words_row], dtype=bool)


def p_f32(c_s, pi_row):
    """fp32 [d]: p_st = fminf(1, c_s pi_t), one fp32 multiply."""
    return np.minimum(F32(1.0), F32(c_s) * np.asarray(pi_row, dtype=F32)).astype(F32)


def keep_f32(words_row, fanout, c_s, pi_row):
    """(bool [d], fp32 [d] p): LABOR-i over one row given fp32 c_s and pi."""
    d = len(words_row)
    if d <= fanout:
        return np.ones(d, dtype=bool), np.ones(d, dtype=F32)
    u = (np.asarray(words_row, dtype=np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    p = p_f32(c_s, pi_row)
    return u < p, p


def hajek(p_kept, dtype=F64):
    """w = (1 / p) / sum(1 / p) over one row's kept entries."""
    inv = 1.0 / np.asarray(p_kept, dtype=dtype)
    return inv / inv.sum(dtype=dtype) if len(inv) else inv


# --------------------------------------------------------------------------------------------- c_s
def constraint(c, pi_row, fanout):
    """sum_t 1 / min(1, c pi_t) - d^2 / k in fp64: zero at the solution."""
    pi_row = np.asarray(pi_row, dtype=F64)
    d = len(pi_row)
    return float(np.sum(1.0 / np.minimum(1.0, c * pi_row)) - d * d / fanout)


def solve_c_sorted(pi_row, fanout, dtype=F64):
    """c_s with sum_t 1 / min(1, c pi_t) = d^2 / k, d > k, by sorting (fp64 unless dtype says otherwise): with the j largest pi
    saturated, c_j = (sum of 1 / pi over the rest) / (d^2 / k - j); c_j never decreases in j while the j-th largest is saturated by
    c_{j - 1}, so the solution is the first j whose c_j leaves the next entry unsaturated."""
    pi = np.sort(np.asarray(pi_row, dtype=dtype))[::-1]
    d = len(pi)
    assert d > fanout
    D = dtype(dtype(d) * dtype(d)) / dtype(fanout)
    inv = dtype(1.0) / pi
    tail = np.concatenate([np.cumsum(inv[::-1], dtype=dtype)[::-1], np.zeros(1, dtype)])     # tail[j] = sum_{q >= j} 1 / pi_(q)
    for j in range(d):
        c = tail[j] / (D - dtype(j))
        if c * pi[j] < dtype(1.0):
            return dtype(c)
    raise AssertionError("no solution: d > k guarantees one")


def solve_c_fixed_point(pi_row, fanout, dtype=F64):
    """The kernel's algorithm in `dtype`: J = {}, c = (sum_{t not in J} 1 / pi_t) / (d^2 / k - |J|), J <- {t : c pi_t >= 1}, until J stops
    growing.  Returns (c, rounds)."""
    pi = np.asarray(pi_row, dtype=dtype)
    d = len(pi)
    D = dtype(dtype(d) * dtype(d)) / dtype(fanout)
    one = dtype(1.0)
    c = (one / pi).sum(dtype=dtype) / D
    nJ, rounds = 0, 0
    for rounds in range(1, d + 1):
        sat = c * pi >= one
        j = int(sat.sum())
        if j <= nJ:
            break
        nJ = j
        c = (one / pi[~sat]).sum(dtype=dtype) / (D - dtype(nJ))
    return dtype(c), rounds


def importance(indptr, indices, rows, fanout, iters, num_nodes, dtype=F64, solve=None):
    """(c [m], pi [N]) of one layer: from pi = 1, `iters` times pi_t <- pi_t max_{s listed, d_s > k, t in N(s)} c_s(pi), then c_s once
    more.  c is 0 for a row with d_s <= k; pi is 1 where no such row reaches.  solve(pi_row, fanout) -> c (default: the sorted solve
    in `dtype`)."""
    if solve is None:
        solve = lambda p, k: solve_c_sorted(p, k, dtype)
    pi = np.ones(int(num_nodes), dtype=dtype)
    nbrs = [np.asarray(indices[int(indptr[s]):int(indptr[s + 1])], dtype=np.int64) for s in rows]

    def all_c():
        return np.array([solve(pi[nb], fanout) if len(nb) > fanout else 0.0 for nb in nbrs], dtype=dtype)

    for _ in range(int(iters)):
        c = all_c()
        mx = np.zeros(int(num_nodes), dtype=dtype)
        for cs, nb in zip(c, nbrs):
            if len(nb) > fanout:
                np.maximum.at(mx, nb, cs)
        touched = mx > 0
        pi[touched] = pi[touched] * mx[touched]
    return all_c(), pi


# --------------------------------------------------------------------------------------------- layers
def sample_layer(indptr, indices, rows, fanout, words, c=None, pi=None):
    """(src, dst, pos int64, p fp32, w fp64) of one layer over the per-NODE words (uint32 [N]); c, pi (fp32) select the importance
    rule.  fanout -1 keeps everything.  Rows in list order, within a row in CSR order."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    words = np.asarray(words).view(np.uint32)
    src, dst, pos, ps, ws = [], [], [], [], []
    for r, s in enumerate(np.asarray(rows, dtype=np.int64)):
        a, b = int(indptr[s]), int(indptr[s + 1])
        nb = indices[a:b]
        k = len(nb) if fanout == -1 else fanout
        if c is None:
            kept = keep_int(words[nb], k)
            p = np.full(len(nb), 1.0 if len(nb) <= k else k / max(len(nb), 1), dtype=F32)
        else:
            kept, p = keep_f32(words[nb], k, c[r], pi[nb])
        t = np.nonzero(kept)[0]
        if len(t):
            src.append(nb[t]); dst.append(np.full(len(t), s, np.int64)); pos.append(a + t); ps.append(p[t])
            ws.append(hajek(p[t]))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(src, np.int64), cat(dst, np.int64), cat(pos, np.int64), cat(ps, F32), cat(ws, F64)


def sample(indptr, indices, targets, fanouts, seed=0, philox_offset=0, layer_dependency=False, keys=None, cpi=None):
    """One batch of modules.labor.LaborSampler with LABOR-0, or with the importance rule when cpi gives per layer the (c, pi) to use.
    keys: per layer a table of N words or None."""
    targets = np.asarray(targets, dtype=np.int64)
    n = len(indptr) - 1
    prev, layers = targets, []
    for d, k in enumerate(fanouts):
        kd = keys[d] if keys is not None and d < len(keys) else None
        words = np.asarray(kd).view(np.uint32) if kd is not None else node_words(seed, layer_base(philox_offset, d, n, layer_dependency), n)
        c, pi = cpi[d] if cpi is not None and cpi[d] is not None else (None, None)
        src, dst, pos, p, w = sample_layer(indptr, indices, prev, k, words, c, pi)
        after = np.union1d(prev, src)
        layers.append(SimpleNamespace(prev=prev, after=after, src=src, dst=dst, pos=pos, p=p, w=w, words=words))
        prev = after
    node_idx = np.unique(prev)
    local = np.full(n, -1, np.int64)
    local[node_idx] = np.arange(len(node_idx))
    return SimpleNamespace(node_idx=node_idx, targets=targets, local_targets=local[targets], layers=layers,
                           philox_offset=philox_offset + offset_advance(len(fanouts), n),
                           edge_index=[np.stack([local[L.src], local[L.dst]]) for L in layers])


def independent_source_count(indptr, indices, rows, fanout, seed):
    """The number of distinct sources of one LABOR-0 layer drawn with INDEPENDENT per-entry variates at the same thresholds (what
    per-row sampling does): the count the shared variates are to beat."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    total = int(sum(indptr[s + 1] - indptr[s] for s in rows))
    words = philox4x32_10(np.arange((total + 3) // 4, dtype=np.uint64), seed).reshape(-1)
    out, p = set(), 0
    for s in rows:
        nb = indices[int(indptr[s]):int(indptr[s + 1])]
        kept = keep_int(words[p:p + len(nb)], fanout)
        p += len(nb)
        out.update(int(t) for t in nb[kept])
    return len(out)


# --------------------------------------------------------------------------------------------- graphs
SPECIAL_DEGREES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 192, 193, 64, 64)


def hand_graph(n, seed, special=SPECIAL_DEGREES, max_deg=12):
    """(indptr int64, indices int32, degrees): rows 0 .. len(special) - 1 have exactly the special degrees — 0, 1, k and k + 1 for the
    fanouts 1, 3 and 64, one entry below, at and above the 64-entry chunk, two and three chunks and one more — with columns drawn WITH
    replacement in any order (duplicates are separate entries); row len(special) stores duplicates and its own loop twice; the other
    rows hold 0 .. max_deg random entries, every fifth one its loop too.  Not symmetric: the sampler reads rows only."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, n, d).tolist() for d in special]
    s = len(rows)
    rows.append([s, s, 3, 3, 9, 3])
    for i in range(s + 1, n):
        r = rng.integers(0, n, int(rng.integers(0, max_deg + 1))).tolist()
        if i % 5 == 0:
            r.insert(len(r) // 2, i)
        rows.append(r)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.asarray([c for r in rows for c in r], dtype=np.int32)
    return indptr, indices, np.diff(indptr)
