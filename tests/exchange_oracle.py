"""Plain-numpy reference of the 1-D partition exchange, written from the contracts in include/grapes_hip.h ("1-D node partition":
message layouts, live counts, the two overflow contracts) — one query, one id, one row at a time, no scan and no binary search —
and the case table that tests/test_exchange_cpu.py (the CPU double of tests/dist_worker.py) and tests/test_exchange_gpu.py (the
kernels of csrc/exchange_kernels.hip, P simulated ranks on one GPU) share.  Everything is integer work or bit copies of fp32
rows: every comparison made against this file is exact.

Buffers are passed in PRE-FILLED and written in place, so a word the contract says is not written keeps its fill and a stray
write shows up in a word-for-word comparison."""
import functools

import numpy as np

EDGE_OVERFLOW, NODE_OVERFLOW = 1, 2
FILL = -7                                  # pre-fill of every int32 buffer (no valid length, offset, id or position)
FILL_F = np.float32(np.nan)                # ... and of every fp32 buffer (compared as bit patterns)


# ------------------------------------------------------------------------------------------------ per-call restatements
def owner_of(bounds, v):
    """the rank p with bounds[p] <= v < bounds[p + 1] (empty shards own nothing)"""
    for p in range(len(bounds) - 1):
        if bounds[p] <= v < bounds[p + 1]:
            return p
    raise ValueError(f"id {v} outside [0, {bounds[-1]})")


def live_count(raw, cap):
    """a message's live count: clamped to [0, cap]; None = the whole list"""
    return cap if raw is None else min(max(int(raw), 0), cap)


def serve_rows(rowptr, col, req, cap, lo, hi, reply, e_slot):
    """owner: reply[p] = [len[cap] | off[cap] | columns[e_slot] | ...] for every peer's query list req[p] = [cap ids | count].
    -> status"""
    status = 0
    for p in range(req.shape[0]):
        m, t = live_count(req[p, cap], cap), 0
        for j in range(cap):
            v = int(req[p, j])
            row = col[rowptr[v - lo]:rowptr[v - lo + 1]] if (j < m and lo <= v < hi) else col[:0]
            reply[p, j], reply[p, cap + j] = len(row), t
            k = min(max(e_slot - t, 0), len(row))                   # the columns whose in-slot index is below e_slot
            reply[p, 2 * cap + t:2 * cap + t + k] = row[:k]
            t += len(row)
        if t > e_slot:
            status |= EDGE_OVERFLOW
    return status


def recv_rows(back, nodes, count, bounds, e_cap):
    """requester: -> (src[e_cap], dst[e_cap], d_e, eoff[cap + 1], status); what is not written keeps FILL"""
    cap = len(nodes)
    m, t = live_count(count, cap), 0
    src, dst, eoff = np.full(e_cap, FILL, np.int32), np.full(e_cap, FILL, np.int32), np.full(cap + 1, FILL, np.int32)
    for i in range(m):
        slot = back[owner_of(bounds, int(nodes[i]))]
        n_col, off = int(slot[i]), int(slot[cap + i])
        eoff[i] = t
        k = min(max(e_cap - t, 0), n_col)                           # the exact prefix of the true list
        src[t:t + k] = nodes[i]
        dst[t:t + k] = slot[2 * cap + off:2 * cap + off + k]
        t += n_col
    eoff[m] = t
    return src, dst, t, eoff, (EDGE_OVERFLOW if t > e_cap else 0)


def serve_features(X_local, req, cap, lo, hi, reply, n_slot):
    """owner: reply[p, 0 .. run) = the rows of the ids of [lo, hi) in peer p's ascending list.  -> status"""
    status = 0
    for p in range(req.shape[0]):
        lst = req[p, :live_count(req[p, cap], cap)].astype(np.int64)
        run = lst[(lst >= lo) & (lst < hi)]
        if len(run) > n_slot:
            status |= NODE_OVERFLOW
            run = run[:n_slot]
        reply[p, :len(run)] = X_local[run - lo]
    return status


def indicators(words, epoch, num_ind):
    """fp32[n, num_ind]: bit j of an indicator word whose bits 8..31 equal `epoch`, else 0"""
    w = np.asarray(words).astype(np.int64) & 0xffffffff
    live = (w >> 8) == (int(epoch) & 0xffffffff)
    return np.stack([((w >> j) & 1) * live for j in range(num_ind)], axis=1).astype(np.float32).reshape(len(w), num_ind)


def _slot_rows(ids, n, bounds, n_slot):
    """for the live rows of an ascending list: (owner, row inside the owner's slot, position inside the run) — the position is
    the number of earlier entries with the same owner, clamped to the slot"""
    seen, out = {}, []
    for i in range(n):
        p = owner_of(bounds, int(ids[i]))
        r = seen.get(p, 0)
        seen[p] = r + 1
        out.append((p, min(r, n_slot - 1), r))
    return out


def assemble_features(back, ids, count, bounds, out, code=None, epoch=0, num_ind=0):
    """requester: out[i] = [row of ids[i] from back[n_peers, n_slot, F] | indicators] for the live rows; the rest keeps its fill"""
    n_slot, F = back.shape[1], back.shape[2]
    n = live_count(count, len(ids))
    for i, (p, r, _) in enumerate(_slot_rows(ids, n, bounds, n_slot)):
        out[i, :F] = back[p, r]
    if num_ind and n:
        out[:n, F:] = indicators(code[ids[:n].astype(np.int64)], epoch, num_ind)
    return out


def halo_positions(ids, count, bounds, n_slot, pos, code=None, code_pos=None):
    """pos[i] = row of ids[i] in back viewed as [n_peers * n_slot, F] (0 past the count), code_pos[pos[i]] = code[ids[i]].
    -> the positions several clamped rows share (an overflowing run: whose word stays there is unspecified)"""
    if len(ids) == 0:
        return set()
    n = live_count(count, len(ids))
    pos[:] = 0
    writers = {}
    for i, (p, r, _) in enumerate(_slot_rows(ids, n, bounds, n_slot)):
        pos[i] = p * n_slot + r
        writers.setdefault(int(pos[i]), []).append(i)
    shared = {q for q, w in writers.items() if len(w) > 1}
    if code_pos is not None:
        for q, w in writers.items():
            if q not in shared:
                code_pos[q] = code[int(ids[w[0]])]
    return shared


def note_rows(loc, ids, count, pos, base, node_map=None, batch=None, n_batch=None, idx_a=None, idx_b=None):
    """loc[ids[i]] = base + pos[row(i)]: row(i) = node_map[ids[i]] where that is a live row of `batch` holding ids[i] (else loc is
    left alone), or idx_b[idx_a[i]]"""
    for i in range(live_count(count, len(ids))):
        v = int(ids[i])
        if node_map is not None:
            row = int(node_map[v])
            if not (0 <= row < live_count(n_batch, len(batch))) or int(batch[row]) != v:
                continue
        else:
            row = int(idx_b[int(idx_a[i])])
        loc[v] = base + int(pos[row])
    return loc


# ------------------------------------------------------------------------------------------------ the end-to-end truths
def true_edges(indptr, indices, queries, count):
    """after serve -> transpose -> recv: get_neighborhoods of the live queries on the FULL graph (int64[2, e])"""
    from oracle import grapes_oracle as O
    return O.get_neighborhoods(np.asarray(queries[:count], dtype=np.int64), indptr, indices)


def true_rows(X, ids, n, code=None, epoch=0, num_ind=0):
    """after serve -> transpose -> assemble: [X[ids[:n]] | indicator columns]"""
    rows = X[np.asarray(ids[:n], dtype=np.int64)]
    if not num_ind:
        return rows
    return np.concatenate([rows, indicators(code[np.asarray(ids[:n], dtype=np.int64)], epoch, num_ind)], axis=1)


def true_rows_clamped(part, r):
    """true_rows under the node-overflow contract: a live row past the first n_slot of its run carries the features of the run's
    row n_slot - 1 (the slot's last row) — and its OWN indicator columns.  Without an overflow this is true_rows."""
    ids, n = part.req[r, :part.capf].astype(np.int64), part.counts[r]
    src = ids[:n].copy()
    for i, (_, rs, pr) in enumerate(_slot_rows(ids, n, part.bounds, part.n_slot)):
        src[i] = ids[i - pr + rs]
    rows = part.X[src]
    if not part.num_ind:
        return rows
    return np.concatenate([rows, indicators(part.code[ids[:n]], part.epoch_live, part.num_ind)], axis=1)


def note_scenario(part, r=0):
    """Inputs and expected result of both forms of note_rows over requester r's exchanged rows, kept as dist._kept_buffer lays
    them out: [slot 0: P * n_slot rows (never fetched: NaN) | slot 1: back of requester r | the isolated nodes' rows].
    node-map form (base = slot 1): ids that are batch rows; ids whose map entry points at a live row of ANOTHER id; a negative
    row; a row >= *d_n_batch that would pass the batch check (the batch's padding holds that very id); a row past the batch; an
    isolated node (stale entry: keeps its static location); and, past *d_n, ids that would be noted.
    index form: kept position -> candidate -> batch row, count below the list length."""
    P, n_slot, N, capf = part.P, part.n_slot, part.N, part.capf
    rng = np.random.default_rng(99)
    ids, n = part.req[r, :capf].astype(np.int64), part.counts[r]
    pos = part.ref["positions"][r][0]
    live = np.unique(ids[:n])
    others = np.setdiff1d(np.arange(N), live)
    assert capf > n >= 8 and len(others) >= capf - n + 12
    batch = ids.copy()
    batch[n:] = others[:capf - n]                                    # valid ids in the padding rows [n, capf)
    free = others[capf - n:]
    iso, stale, negative, past = free[:3], free[3:6], free[6:9], free[9:12]
    node_map = np.full(N, 12345, np.int64)                           # stale everywhere (a row past any batch) ...
    node_map[ids[:n]] = np.arange(n)                                 # ... but on the live batch rows
    node_map[batch[n:]] = np.arange(n, capf)                         # row >= *d_n_batch, and batch[row] == id
    node_map[stale] = rng.integers(0, n, 3)
    node_map[negative] = [-1, -5, -2 ** 31]
    sel = rng.permutation(live)
    noted, unseen = sel[:len(sel) // 2], sel[len(sel) // 2:][:5]
    ids_a = np.concatenate([rng.permutation(np.concatenate([noted, stale, negative, past, batch[n:], iso[:1]])), unseen])
    base = P * n_slot
    first = np.unique(ids[:n], return_index=True)[1]                 # (one row per id: two rows of one id are two right answers)
    idx_b = rng.permutation(first)[:40]                              # candidate -> batch row
    idx_a = np.sort(rng.permutation(len(idx_b))[:16])                # kept position -> candidate
    ids_b = batch[idx_b[idx_a]]
    assert len(idx_a) == 16
    loc0 = np.full(N, FILL, np.int32)
    loc0[iso] = 2 * base + np.arange(3)
    kept = np.concatenate([np.full((base, part.F), FILL_F, np.float32), part.ref["backs"][r].reshape(base, part.F), part.X[iso]])
    i32 = lambda a: np.asarray(a).astype(np.int32)
    s = dict(batch=i32(batch), n_batch=n, node_map=i32(node_map), ids_a=i32(ids_a), count_a=len(ids_a) - 5, pos=pos, base=base,
             idx_a=i32(idx_a), idx_b=i32(idx_b), ids_b=i32(ids_b), count_b=12, loc0=loc0, kept=kept, iso=i32(iso))
    loc = loc0.copy()
    note_rows(loc, s["ids_a"], s["count_a"], pos, base, node_map=s["node_map"], batch=s["batch"], n_batch=n)
    s["loc_a"] = loc.copy()
    note_rows(loc, s["ids_b"], s["count_b"], pos, base, idx_a=s["idx_a"], idx_b=s["idx_b"])
    s["loc_b"] = loc
    s["want"] = np.unique(np.concatenate([noted, ids_b[:12], iso]))
    # the truth this is all for: the noted nodes' rows are found in the kept buffer
    assert set(np.flatnonzero(s["loc_a"] != FILL)) == set(noted) | set(iso)
    assert np.array_equal(bits(kept[loc[s["want"]]]), bits(part.X[s["want"]]))
    return s


def bits(a):
    """fp32 array -> its bit patterns (NaN fill compares equal to itself)"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the case table
def _bounds(kind, N, P):
    from grapes_amd.dist import partition_bounds
    if kind == "even":
        return partition_bounds(N, P)
    b = partition_bounds(N, P - 1)                                  # hand-made: P - 1 even shards and one EMPTY shard
    k = {"empty_first": 0, "empty_middle": P // 2, "empty_last": P - 1}[kind]
    return b[:k + 1] + b[k:]


@functools.lru_cache(maxsize=None)
def graph(N):
    """(indptr int64, indices int32, hub | None): symmetric; every node v with v % 7 == 0 has degree 0; with N > 1300 node 17 is a
    hub of 1100 neighbours — a row longer than the 1024-thread chunk of the scans"""
    from oracle import grapes_oracle as O
    rng = np.random.default_rng(1000 + N)
    live = np.flatnonzero(np.arange(N) % 7 != 0)
    ei = live[rng.integers(0, len(live), (2, min(1500, 2 * N)))]
    hub = 17 if N > 1300 else None
    if hub is not None:
        nb = rng.permutation(live[live != hub])[:1100]
        ei = np.concatenate([ei, np.stack([np.full(1100, hub), nb])], axis=1)
    indptr, indices = O.build_csr(np.concatenate([ei, ei[::-1]], axis=1), N)
    assert hub is None or indptr[hub + 1] - indptr[hub] > 1024
    return indptr, indices, hub


def _pad(N, k):
    """padding of a list beyond its count: ids no table has a row for.  Nothing may read them."""
    return np.resize(np.array([-1, N, 2 ** 31 - 1], dtype=np.int64), k)


class RowsPart:
    """adjacency rows of one case: every rank's query message, the reference's replies / backs / requester outputs"""

    def __init__(self, N, bounds, cap, req, e_cap, graph_=None):
        self.N, self.bounds, self.P, self.cap, self.req = N, list(bounds), len(bounds) - 1, cap, req
        self.indptr, self.indices = (graph_ or graph(N))[:2]
        self.e_slot = self.e_cap = e_cap                            # as dist.expand: stride = 2 cap + e_cap
        self.stride = 2 * cap + e_cap + 3                           # (three words of slack: nothing may write them)
        self.counts = [live_count(req[r, cap], cap) for r in range(self.P)]

    def shard(self, o):
        lo, hi = self.bounds[o], self.bounds[o + 1]
        return ((self.indptr[lo:hi + 1] - self.indptr[lo]).astype(np.int64),
                self.indices[self.indptr[lo]:self.indptr[hi]].astype(np.int32), lo, hi)

    @functools.cached_property
    def ref(self):
        P = self.P
        replies, sstat = [], []
        for o in range(P):
            rp, cl, lo, hi = self.shard(o)
            reply = np.full((P, self.stride), FILL, np.int32)
            sstat.append(serve_rows(rp, cl, self.req, self.cap, lo, hi, reply, self.e_slot))
            replies.append(reply)
        backs = [transpose(replies, r) for r in range(P)]
        recv = [recv_rows(backs[r], self.req[r, :self.cap], self.req[r, self.cap], self.bounds, self.e_cap) for r in range(P)]
        return dict(replies=replies, serve_status=sstat, backs=backs, recv=recv)


class FeatPart:
    """halo feature rows of one case"""

    def __init__(self, N, bounds, X, num_ind, capf, req, n_slot, code, epoch, d_epoch=None, misalign=None):
        self.N, self.bounds, self.P, self.X, self.F, self.num_ind = N, list(bounds), len(bounds) - 1, X, X.shape[1], num_ind
        self.capf, self.req, self.n_slot, self.code = capf, req, n_slot, code
        self.epoch, self.d_epoch, self.misalign = epoch, d_epoch, misalign
        self.epoch_live = epoch if d_epoch is None else (d_epoch & 0xffffff)      # the device word wins, masked to 24 bits
        self.counts = [live_count(req[r, capf], capf) for r in range(self.P)]

    @functools.cached_property
    def ref(self):
        P, F = self.P, self.F
        replies, sstat = [], []
        for o in range(P):
            lo, hi = self.bounds[o], self.bounds[o + 1]
            reply = np.full((P, self.n_slot, F), FILL_F, np.float32)
            sstat.append(serve_features(self.X[lo:hi], self.req, self.capf, lo, hi, reply, self.n_slot))
            replies.append(reply)
        backs = [transpose(replies, r) for r in range(P)]
        outs, poss = [], []
        for r in range(P):
            ids = self.req[r, :self.capf]
            out = np.full((self.capf, F + self.num_ind), FILL_F, np.float32)
            outs.append(assemble_features(backs[r], ids, self.req[r, self.capf], self.bounds, out, self.code, self.epoch_live,
                                          self.num_ind))
            pos, cpos = np.full(self.capf, FILL, np.int32), np.full(P * self.n_slot, FILL, np.int32)
            shared = halo_positions(ids, self.req[r, self.capf], self.bounds, self.n_slot, pos, self.code, cpos)
            poss.append((pos, cpos, shared))
        return dict(replies=replies, serve_status=sstat, backs=backs, outs=outs, positions=poss)

    def exact_rows(self, r):
        """the live rows of requester r that sit among the first n_slot of their run (all of them without an overflow)"""
        return np.array([pr < self.n_slot for _, _, pr in _slot_rows(self.req[r], self.counts[r], self.bounds, self.n_slot)], bool)


def transpose(replies, r):
    """the all-to-all, by hand: rank r receives slot r of every owner's reply"""
    return np.stack([rep[r] for rep in replies])


class Case:
    def __init__(self, id, make):
        self.id, self._make = id, make

    @functools.cached_property
    def part(self):
        return self._make()

    def __repr__(self):
        return self.id


def _rows_queries(rng, N, bounds, cap, hub, r):
    """requester r's queries: the hub twice, then ids ON the shard edges (lo, hi - 1 and hi of every shard, starting at shard r), a
    degree-0 row, the first and the last node, then random ids (repeats included).  Requester 1 asks ONE owner for everything,
    requester 2 asks the first non-empty shard's owner for nothing."""
    P = len(bounds) - 1
    full = [s for s in range(P) if bounds[s] < bounds[s + 1]]
    if r == 1 and P > 1:
        s = owner_of(bounds, hub) if hub is not None else full[len(full) // 2]
        lo, hi = bounds[s], bounds[s + 1]
        q = np.concatenate([[lo, hi - 1] + ([hub, hub] if hub is not None else []), rng.integers(lo, hi, cap)])[:cap]
        return q
    special = [hub, hub] if hub is not None else []
    for s in full[r % len(full):] + full[:r % len(full)]:
        special += [bounds[s], bounds[s + 1] - 1] + ([bounds[s + 1]] if bounds[s + 1] < N else [])
    special = special[:max(cap - 3, 0)] + [0, min(7, N - 1), N - 1]
    q = np.concatenate([special, rng.integers(0, N, cap)]).astype(np.int64)[:cap]
    if r == 2 and P > 2:
        lo, hi = bounds[full[0]], bounds[full[0] + 1]
        q[(q >= lo) & (q < hi)] = N - 1
    return q


def _rows_case(N, P, kind, cap, counts=None, short=0, hub_last=False):
    """counts: the RAW count words per requester (default: too large, cap, 2/3, 0, negative, then cap - r).  e_slot = e_cap = the
    largest requester total - short: it fits exactly, or (short = 1) is one short of it."""
    def make():
        indptr, indices, hub = graph(N)
        bounds = _bounds(kind, N, P)
        rng = np.random.default_rng(7 * N + 31 * P + cap)
        raw = counts or [[cap + 5, cap, (2 * cap + 2) // 3, 0, -3][r] if r < 5 else max(cap - r, 0) for r in range(P)]
        req = np.empty((P, cap + 1), np.int64)
        for r in range(P):
            q = _rows_queries(rng, N, bounds, cap, hub, r)
            m = live_count(raw[r], cap)
            if hub_last and r == 1:
                q[m - 1] = hub
            q[m:] = _pad(N, cap - m)
            req[r, :cap], req[r, cap] = q, raw[r]
        req = req.astype(np.int32)
        deg = np.diff(indptr)
        totals = [int(deg[req[r, :live_count(raw[r], cap)]].sum()) for r in range(P)]
        part = RowsPart(N, bounds, cap, req, max(max(totals) - short, 1))
        if hub_last:        # the hub row straddles the slot's edge, at the owner and at the requester
            assert totals[1] == max(totals) and totals[1] - deg[hub] < part.e_slot < totals[1]
        return part
    return make


def serve_path(F, misalign):
    """grapes_exchange_serve_features: serve_rows_k<VEC> when F % 4 == 0 and X_local and reply are both 16-byte aligned"""
    return "vec" if F % 4 == 0 and misalign not in ("X_local", "reply") else "scalar"


def assemble_path(F, num_ind, misalign):
    """grapes_exchange_assemble_features: VLOAD = F % 4 == 0 and back 16-byte aligned; VSTORE = VLOAD and (F + num_ind) % 4 == 0
    and out 16-byte aligned -> halo_assemble_k<VLOAD, VSTORE>"""
    vload = F % 4 == 0 and misalign != "back"
    vstore = vload and (F + num_ind) % 4 == 0 and misalign != "out"
    return "vload,vstore" if vstore else ("vload,scalar-store" if vload else "scalar,scalar")


def _feat_list(rng, N, bounds, n, r):
    """requester r's ascending list of n live ids, with repeats: requester 0 holds every shard's first id and the id before it,
    requester 1's list lies wholly in the largest shard, requester 2's run is empty for the first two non-empty shards."""
    P = len(bounds) - 1
    full = [s for s in range(P) if bounds[s] < bounds[s + 1]]
    lo, hi = 0, N
    if r == 1 and P > 1:
        s = max(full, key=lambda s: bounds[s + 1] - bounds[s])
        lo, hi = bounds[s], bounds[s + 1]
    elif r == 2 and len(full) > 2:
        lo = bounds[full[2]]
    ids = rng.integers(lo, hi, n)
    ids[1::3] = ids[0::3][:len(ids[1::3])]                          # every third id twice
    if r == 0:
        edges = [v for s in full for v in (bounds[s], bounds[s] - 1, bounds[s + 1] - 1) if 0 <= v < N]
        ids[:len(edges)] = edges[:n]
    return np.sort(ids)


def _feat_case(N, P, kind, F, num_ind, capf, epoch=5, d_epoch=None, misalign=None, short=0):
    """counts: capf - 3 (a live count below the list length), capf, 2/3, then capf - r; with P >= 4 the last requester sends 0.
    n_slot = the longest run of any list in any shard - short: it fits exactly, or (short = 1) is one short of it.  Indicator
    words: all 8 low bits random whatever num_ind is, a third of them with a stale epoch."""
    def make():
        bounds = _bounds(kind, N, P)
        rng = np.random.default_rng(11 * N + 13 * P + 17 * F + num_ind + capf)
        X = rng.standard_normal((N, F)).astype(np.float32)
        req = np.empty((P, capf + 1), np.int64)
        for r in range(P):
            n = [capf - 3, capf, (2 * capf + 2) // 3][r] if r < 3 else capf - r
            n = 0 if (P >= 4 and r == P - 1) else max(n, 0)
            req[r, :n], req[r, n:capf], req[r, capf] = _feat_list(rng, N, bounds, n, r), _pad(N, capf - n), n
        req = req.astype(np.int32)
        runs = [np.diff(np.searchsorted(req[r, :req[r, capf]], bounds)).max() for r in range(P)]
        live = epoch if d_epoch is None else d_epoch & 0xffffff
        ep = np.where(rng.integers(0, 3, N) > 0, live, (live - 1) & 0xffffff).astype(np.int64)
        code = ((ep << 8) | rng.integers(0, 256, N)).astype(np.uint32).view(np.int32)
        assert max(runs) - short >= 1
        return FeatPart(N, bounds, X, num_ind, capf, req, int(max(runs)) - short, code, epoch, d_epoch, misalign)
    return make


def _legacy(P, F, num_ind):
    """the three cases tests/test_exchange_gpu.py had before this table: N = 5003, 120000 entries, cap 300, e_cap 40000, counts
    cap - 11 r; lists of 1200 distinct ids, counts 1200 - 37 r, n_slot = 2 * 1200 / P, a third of the indicator words stale"""
    @functools.lru_cache(maxsize=None)
    def both():
        from grapes_amd.dist import partition_bounds
        from oracle import grapes_oracle as O
        N = 5003
        rng = np.random.default_rng(3)
        ei = rng.integers(0, N, (2, 60000))
        ei[0, :5000] = 17
        ei[0, 5000:5200] = N - 1
        g = O.build_csr(np.concatenate([ei, ei[::-1]], axis=1), N)
        rng = np.random.default_rng(4)
        X = rng.standard_normal((N, F)).astype(np.float32)
        b = partition_bounds(N, P)
        cap, e_cap = 300, 40000
        req = np.empty((P, cap + 1), np.int32)
        for r in range(P):
            req[r, :cap] = rng.permutation(N)[:cap]
            req[r, :4] = [17, N - 1, 17, 0]
            req[r, cap] = cap - 11 * r
        capf = 1200
        reqf = np.empty((P, capf + 1), np.int32)
        for r in range(P):
            reqf[r, :capf], reqf[r, capf] = np.sort(rng.permutation(N)[:capf]), capf - 37 * r
        epoch = 5
        code = ((epoch << 8) | rng.integers(0, 1 << max(num_ind, 1), N)).astype(np.int32)
        code[::3] = (4 << 8) | 0xf
        return (RowsPart(N, b, cap, req, e_cap, graph_=g),
                FeatPart(N, b, X, num_ind, capf, reqf, capf if P == 1 else 2 * capf // P, code, epoch))
    return both


def _cases():
    rows, feat = [], []

    def R(name, *a, **k):
        rows.append(Case("rows-" + name, _rows_case(*a, **k)))

    def Ft(N, P, kind, F, num_ind, capf, tag="", **k):
        name = (f"feat-P{P}-F{F}-ind{num_ind}" + (f"-{kind}" if kind != "even" else "") + (f"-{tag}" if tag else "") +
                (f"-{k['misalign']}+4B" if k.get("misalign") else "") +
                f"-serve<{serve_path(F, k.get('misalign'))}>-assemble<{assemble_path(F, num_ind, k.get('misalign'))}>")
        feat.append(Case(name, _feat_case(N, P, kind, F, num_ind, capf, **k)))

    # ---- adjacency rows.  serve_offsets_k scans the P * cap owner-side lengths, recv_offsets_k the requester's cap lengths, in
    # chunks of 1024 threads with a carry: P * cap (and cap) on, one below and one above a chunk edge, and past two chunks.
    R("P3-cap341-M1023-below_chunk", 2003, 3, "even", 341)
    R("P8-cap128-M1024-exact_chunk", 2003, 8, "even", 128)
    R("P1-cap1025-M1025-carry-recv_carry-fits_exactly", 2003, 1, "even", 1025, counts=[1025])
    R("P1-cap1025-count_below_cap", 2003, 1, "even", 1025, counts=[700])
    R("P3-cap683-M2049-two_carries", 2003, 3, "even", 683)
    R("P2-cap1-recv_one_query", 2003, 2, "even", 1, counts=[1, 1])
    R("P2-cap1024-M2048-recv_exact_chunk", 2003, 2, "even", 1024)
    R("P64-cap16-M1024-max_peers", 2003, 64, "even", 16)
    R("P8-N5-fewer_nodes_than_ranks", 5, 8, "even", 7)
    R("P3-empty_first_shard", 2003, 3, "empty_first", 40)
    R("P3-empty_middle_shard", 2003, 3, "empty_middle", 40)
    R("P3-empty_last_shard", 2003, 3, "empty_last", 40)
    R("P8-empty_middle_shard", 2003, 8, "empty_middle", 150)
    R("P3-cap341-edge_overflow-hub_straddles_slot_edge", 2003, 3, "even", 341, short=1, hub_last=True)
    R("P1-cap1025-edge_overflow-one_short", 2003, 1, "even", 1025, counts=[1025], short=1)

    # ---- halo rows.  The path in a case's name is DERIVED from the dispatch conditions of grapes_exchange_serve_features /
    # grapes_exchange_assemble_features (serve_path / assemble_path above restate them); the GPU test checks the alignment of
    # the four tensors it passes, so the name is what the call takes.
    Ft(2003, 2, "even", 4, 0, 257)
    Ft(2003, 3, "even", 8, 4, 300, tag="epoch_bits_8_to_31", epoch=0xabcdef)
    Ft(2003, 8, "even", 100, 4, 130, tag="device_epoch_wins", epoch=6, d_epoch=(0x5a << 24) | 0x80c0de)
    Ft(2003, 3, "empty_middle", 8, 3, 300)
    Ft(2003, 64, "even", 4, 1, 80, tag="max_peers")
    Ft(2003, 1, "even", 1, 0, 300)
    Ft(2003, 8, "empty_first", 7, 3, 130)
    Ft(2003, 3, "empty_last", 7, 3, 130)
    Ft(5, 8, "even", 5, 8, 12, tag="N5_fewer_nodes_than_ranks")
    for which in ("X_local", "reply", "back", "out"):               # one float into the allocation: the scalar fallbacks
        Ft(2003, 3, "even", 8, 4, 200, misalign=which)
    for num_ind in (2, 5, 6, 7, 8):
        Ft(2003, 2, "even", 8, num_ind, 64)
    Ft(2003, 3, "even", 8, 4, 300, tag="node_overflow_one_short", short=1)
    Ft(2003, 8, "even", 7, 3, 130, tag="node_overflow_one_short", short=1)

    for P, F, num_ind in ((1, 8, 0), (3, 100, 4), (8, 7, 3)):       # the suite's first three cases, as they were
        both = _legacy(P, F, num_ind)
        rows.append(Case(f"rows-legacy-P{P}-F{F}-ind{num_ind}", lambda both=both: both()[0]))
        feat.append(Case(f"feat-legacy-P{P}-F{F}-ind{num_ind}-serve<{serve_path(F, None)}>-assemble<{assemble_path(F, num_ind, None)}>",
                         lambda both=both: both()[1]))
    return rows, feat


ROWS_CASES, FEAT_CASES = _cases()
CASES = ROWS_CASES + FEAT_CASES
# note_scenario needs an exchange without overflow, padding rows in requester 0's list and ids to spare
NOTE_CASES = [c for c in FEAT_CASES if not any(w in c.id for w in ("overflow", "N5", "legacy"))]
