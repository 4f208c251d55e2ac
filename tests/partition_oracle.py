"""The label-propagation partitioner on a CPU (numpy int64), written from the rule in include/grapes_hip.h: propose, admit, cut and
the driver's refine — and a seeded planted-partition generator.  Nothing here imports the product."""
import numpy as np

BAD = 4                                                                  # GRAPES_STATUS_BAD_INDEX


def csr(rows):
    """(indptr int64, indices int32) of per-row column lists, kept exactly as given (order, duplicates, loops)."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.asarray([c for r in rows for c in r], dtype=np.int32).reshape(-1)


def planted(n, groups, intra, inter, seed, hub=None, hub_degree=0, dups=0, loops=0):
    """A symmetric planted-partition graph -> (indptr, indices, group int64 [n]).  Node v is in group v % groups; it draws `intra`
    partners inside its group and `inter` anywhere, every pair stored in both rows (about 2 (intra + inter) entries per row).  hub:
    that row also gets hub_degree random columns (one direction).  dups: that many stored entries are stored once more; loops: that
    many rows store themselves.  The stored order of a row is shuffled."""
    rng = np.random.default_rng(seed)
    group = np.arange(n, dtype=np.int64) % groups
    src = np.repeat(np.arange(n, dtype=np.int64), intra)
    per = (n - group[src] + groups - 1) // groups                           # the members of src's group
    dst = group[src] + groups * (rng.integers(0, 1 << 40, src.size) % per)
    s2 = np.repeat(np.arange(n, dtype=np.int64), inter)
    d2 = rng.integers(0, n, s2.size)
    a, b = np.concatenate([src, s2]), np.concatenate([dst, d2])
    keep = a != b
    a, b = a[keep], b[keep]
    rows, cols = np.concatenate([a, b]), np.concatenate([b, a])
    if hub is not None and hub_degree:
        rows = np.concatenate([rows, np.full(hub_degree, hub, dtype=np.int64)])
        cols = np.concatenate([cols, rng.integers(0, n, hub_degree)])
    if dups:
        pick = rng.integers(0, rows.size, dups)
        rows, cols = np.concatenate([rows, rows[pick]]), np.concatenate([cols, cols[pick]])
    if loops:
        pick = rng.permutation(n)[:loops]
        rows, cols = np.concatenate([rows, pick]), np.concatenate([cols, pick])
    order = np.lexsort((rng.random(rows.size), rows))
    rows, cols = rows[order], cols[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return indptr, cols.astype(np.int32), group


def balanced_random(n, P, seed):
    """A balanced random start: a seeded permutation, position i going to cluster i * P // n."""
    part = np.empty(n, dtype=np.int64)
    part[np.random.default_rng(seed).permutation(n)] = np.arange(n, dtype=np.int64) * P // n
    return part


def default_cap(n, P, imbalance_num=1, imbalance_den=10):
    """ceil(n / P) + floor(imbalance n / P) in integers, imbalance = num / den."""
    return -(-n // P) + (imbalance_num * n) // (imbalance_den * P)


def _entries(indptr, indices, part, P):
    """(row, column, label of the column, status) of the entries that count: no stored loop, no bad column or label."""
    indptr, indices, part = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(part, dtype=np.int64)
    n = len(indptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    ok = (indices >= 0) & (indices < n)
    status = 0 if ok.all() else BAD
    lab = np.where(ok, part[np.where(ok, indices, 0)], 0)
    okl = (lab >= 0) & (lab < P)
    if not okl[ok].all():
        status |= BAD
    keep = ok & okl & (indices != row)
    return row[keep], indices[keep], lab[keep], status


def propose(indptr, indices, part, P):
    """(want int64 [n] (-1: stays), gain int64 [n] (0: stays), status)."""
    part = np.asarray(part, dtype=np.int64)
    n = len(indptr) - 1
    row, _, lab, status = _entries(indptr, indices, part, P)
    want, gain = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    cur_ok = (part >= 0) & (part < P)
    if not cur_ok.all():
        status |= BAD
    pair, count = np.unique(row * P + lab, return_counts=True)             # ascending: by row, then by label
    prow, plab = pair // P, pair % P
    m = np.zeros(n, dtype=np.int64)
    np.maximum.at(m, prow, count)
    ccur = np.zeros(n, dtype=np.int64)
    mine = plab == part[prow]
    ccur[prow[mine]] = count[mine]
    at_max = count == m[prow]
    first = np.full(n, P, dtype=np.int64)
    np.minimum.at(first, prow[at_max], plab[at_max])                       # the smallest label with count m
    go = cur_ok & (m > 0) & (ccur != m)
    want[go], gain[go] = first[go], (m - ccur)[go]
    return want, gain, status


def propose_dense(indptr, indices, part, P):
    """The same by brute force: the dense n x P count matrix, a Python loop over the entries."""
    n = len(indptr) - 1
    counts = np.zeros((n, P), dtype=np.int64)
    for v in range(n):
        for j in range(int(indptr[v]), int(indptr[v + 1])):
            u = int(indices[j])
            if u != v:
                counts[v, int(part[u])] += 1
    want, gain = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for v in range(n):
        m = counts[v].max()
        if m == 0 or counts[v, int(part[v])] == m:
            continue
        want[v] = int(np.argmax(counts[v]))                                 # (argmax: the first = smallest label at the maximum)
        gain[v] = m - counts[v, int(part[v])]
    return want, gain


def keys_of(want, gain):
    v = np.nonzero(np.asarray(want) >= 0)[0]
    return v, ((0x7fffffff - np.asarray(gain, dtype=np.int64)[v]) << 32) | v


def admit(want, gain, part, size, cap):
    """(part, size, moved) after the admission; the inputs are left as they are."""
    want, part, size = np.asarray(want, dtype=np.int64), np.array(part, dtype=np.int64), np.array(size, dtype=np.int64)
    free = np.maximum(cap - size, 0)
    v, key = keys_of(want, gain)
    moved = 0
    for c in np.unique(want[v]):
        sel = want[v] == c
        vc = v[sel][np.argsort(key[sel], kind="stable")][:free[c]]
        np.subtract.at(size, part[vc], 1)
        size[c] += len(vc)
        part[vc] = c
        moved += len(vc)
    return part, size, moved


def admit_by_full_sort(want, gain, part, size, cap):
    """The same by ONE sort of all proposers by (destination, key) and a rank inside the destination."""
    want, part, size = np.asarray(want, dtype=np.int64), np.array(part, dtype=np.int64), np.array(size, dtype=np.int64)
    free = np.maximum(cap - size, 0)
    v, key = keys_of(want, gain)
    order = np.lexsort((key, want[v]))
    v, dest = v[order], want[v][order]
    start = np.concatenate([[0], np.cumsum(np.bincount(dest, minlength=len(size)))])
    rank = np.arange(len(v)) - start[dest]
    ok = rank < free[dest]
    for node, c in zip(v[ok], dest[ok]):
        size[part[node]] -= 1
        size[c] += 1
        part[node] = c
    return part, size, int(ok.sum())


def cut(indptr, indices, part, P):
    part = np.asarray(part, dtype=np.int64)
    row, _, lab, _ = _entries(indptr, indices, part, P)
    return int((part[row] != lab).sum())


def refine(indptr, indices, part, P, cap, rounds, trace=None):
    """(part of the earliest round with the smallest cut, info) — info: cuts (the start's first), moved (per round run), round (the
    chosen one, 0 = the start), max_size (of the returned assignment).  trace: a list that receives (part, size) after every round."""
    part = np.array(part, dtype=np.int64)
    size = np.bincount(part, minlength=P).astype(np.int64)
    if size.max() > cap:
        raise ValueError("cap is below the largest starting cluster")
    cuts, moved = [cut(indptr, indices, part, P)], []
    best, best_round = part.copy(), 0
    for r in range(1, rounds + 1):
        want, gain, _ = propose(indptr, indices, part, P)
        part, size, mv = admit(want, gain, part, size, cap)
        moved.append(mv)
        if trace is not None:
            trace.append((part.copy(), size.copy()))
        if mv == 0:
            break
        cuts.append(cut(indptr, indices, part, P))
        if cuts[-1] < cuts[best_round]:
            best, best_round = part.copy(), r
    return best, dict(cuts=cuts, moved=moved, round=best_round, max_size=int(np.bincount(best, minlength=P).max()))
