// ShaDow-GNN's sampler [Zeng et al., NeurIPS 2021; PyG-recall: ShaDowKHopSampler over torch_sparse's ego_k_hop_sample_adj]: every root
// gets its OWN small sampled ego-net, the batch is the disjoint union of the ego-nets, and a GNN of any depth runs on the union.  The
// rule written in include/grapes_hip.h (grapes_shadow_sample) is the contract; tests/shadow_oracle.py reproduces it bit for bit.
//
// B independent problems of at most SHADOW_MAX_NODES = 1024 nodes each: one workgroup per root holds its whole ego-net in LDS.
//   shadow_build_k   a workgroup per root.  A hop is three memory round trips whatever the frontier's size: every thread fetches the
//                    row pointers of one frontier node into LDS; a wavefront per frontier node then chooses positions without
//                    touching memory — a row of more than k entries by Floyd's algorithm ACROSS the wavefront: lane s holds word
//                    w_s and, in the end, the s-th chosen position; step s broadcasts its candidate and a ballot answers "already
//                    chosen?" — k steps whatever the degree, no pass over a hub row; every thread then loads one chosen entry.
//                    New ids go through an LDS hash (integer LDS atomics; which lane wins changes nothing: the result is
//                    a set) onto the node list, whose tail is the next frontier.  Then ONE bitonic sort of the list in LDS, and the
//                    induced entries are counted per member: a wavefront strides over a member's row, the whole workgroup over a
//                    row of more than SHADOW_LONG_ROW entries; membership is a binary search of the sorted set.  Leaves the sorted
//                    set and the per-member counts in a fixed [B, C] staging area, with n_b and e_b.
//   shadow_scan_k    ONE workgroup: ptr and the edge offsets (clamped to n_cap / e_cap), *d_n, *d_e, the overflow bits, and the
//                    stream offset's advance.  B <= 4096 counts that the launch before left in one table: a thread walks its own
//                    span on block_excl_scan_u64 and the tail is list_scan_finish (row_list.h, "which scan when").
//   shadow_write_k   a workgroup per root: n_id, batch, root_n_id, and the edges compacted in order within each row
//                    (wave_compact_slot; a long row by the whole workgroup, 1024 entries per trip).
// Integer code only, no float, no global atomic beyond the status OR, no kernel waits on another workgroup: the outputs do not
// depend on scheduling and two runs give the same bits.
//
// The sort / count / staging half of shadow_build_k is shadow_stage, a __device__ function: the PPR scopes further down
// (grapes_shadow_ppr_sample: shadow_ppr_build_k, then the same scan and write) build their member list another way and enter it too.
//
// The segment mean at the end of the file is the model's readout over an ego-net's rows (grapes_segment_mean_fwd / _bwd).
#include "philox.h"
#include "row_list.h"

#define SHADOW_THREADS 1024             // 16 wavefronts: a workgroup is bound by its dependent memory trips, and each wavefront keeps one in flight
#define SHADOW_WAVES (SHADOW_THREADS / 64)
#define SHADOW_MAX_NODES 1024          // the ego-net cap C: the sorted set of one root lives in LDS
#define SHADOW_MAX_ROOTS 4096
#define SHADOW_MAX_FANOUT 64           // one chosen position per lane
#define SHADOW_HASH 2048               // LDS hash slots: twice the cap, so a probe always ends
#define SHADOW_LONG_ROW 256            // a member row with more entries is walked by the whole workgroup, SHADOW_THREADS per trip
#define SHADOW_EMPTY (-1)
#define SHADOW_PER (SHADOW_MAX_NODES / SHADOW_THREADS)   // member counts a thread of shadow_write_k scans
static_assert(SHADOW_MAX_NODES == SHADOW_PER * SHADOW_THREADS, "shadow_write_k scans SHADOW_PER member counts per thread");
static_assert(SHADOW_HASH >= 2 * SHADOW_MAX_NODES && (SHADOW_HASH & (SHADOW_HASH - 1)) == 0, "hash slots");

// C = 1 + k + ... + k^depth, or 0 when it exceeds the cap (or the arguments are outside the rule)
static inline int shadow_cap(int depth, int fanout) {
    if (depth < 1 || fanout < 1 || fanout > SHADOW_MAX_FANOUT) return 0;
    long long c = 1, p = 1;
    for (int h = 0; h < depth; ++h) {
        p *= fanout;
        c += p;
        if (c > SHADOW_MAX_NODES) return 0;
    }
    return (int)c;
}

// id -> the node list, once: the lane whose compare-and-swap takes the empty slot appends it
__device__ __forceinline__ void shadow_insert(int* hash, int* nodes, int* n_nodes, int c) {
    unsigned slot = ((unsigned)c * 0x9E3779B1u) >> 21;                          // 11 bits
    for (int probe = 0; probe < SHADOW_HASH; ++probe) {
        const int old = atomicCAS(&hash[slot], SHADOW_EMPTY, c);
        if (old == SHADOW_EMPTY) {
            const int idx = atomicAdd(n_nodes, 1);
            if (idx < SHADOW_MAX_NODES) nodes[idx] = c;                          // (always: |S_h| <= 1 + k + ... + k^h <= C)
            return;
        }
        if (old == c) return;
        slot = (slot + 1) & (SHADOW_HASH - 1);
    }
}

// The row starts and the degrees of ids[i0 .. i1) into LDS: one memory round trip for the whole list, where a wavefront that walked
// the list alone would pay one per node.  A degree is clamped to [0, 2^31): the graph holds fewer than 2^31 entries.
__device__ __forceinline__ void shadow_rows(const int64_t* __restrict__ rowptr, const int* ids, int i0, int i1, int64_t* ra, int* rdeg) {
    for (int i = i0 + (int)threadIdx.x; i < i1; i += SHADOW_THREADS) {
        const int v = ids[i];
        const int64_t a = rowptr[v], d = rowptr[v + 1] - a;
        ra[i] = a;
        rdeg[i] = d < 0 ? 0 : (d > 0x7fffffffll ? 0x7fffffff : (int)d);
    }
}

// the rank of id c in the sorted set, or -1
__device__ __forceinline__ int shadow_rank(const int* set, int n, int c) {
    const int i = lower_bound<int, int, int>(set, n, c);
    return (i < n && set[i] == c) ? i : -1;
}

// The second half of a build kernel, shared by shadow_build_k and shadow_ppr_build_k: the member list nodes[0 .. n) of root b (any order,
// n <= C <= SHADOW_MAX_NODES, in LDS, complete and behind a barrier) -> the sorted set, the induced entries counted per member, and
// both in the [B, C] staging area with nb[b] and eb[b].  The caller hands over its LDS: nodes and cnt of SHADOW_MAX_NODES ints, longs
// (the list of long member rows; *n_long = 0 on entry) SHADOW_MAX_NODES ints, ra / rdeg of SHADOW_MAX_NODES entries, scan_lds of 17
// ints.  `bad`: the thread met a column outside [0, N) before.  Every thread of the workgroup calls it; nodes stays sorted in LDS.
__device__ __forceinline__ void shadow_stage(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N, int b, int C, int n,
                                             int* nodes, int* cnt, int* longs, int64_t* ra, int* rdeg, int* scan_lds, int* n_long,
                                             int32_t* __restrict__ set_out, int32_t* __restrict__ cnt_out, int32_t* __restrict__ nb,
                                             int32_t* __restrict__ eb, int32_t* status, bool bad) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // ---- the sorted set: one bitonic sort of the list, padded to a power of two
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += SHADOW_THREADS) nodes[i] = 0x7fffffff;
    for (int i = tid; i < n; i += SHADOW_THREADS) cnt[i] = 0;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += SHADOW_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const int u = nodes[i], w = nodes[x];
                    if ((u > w) == ((i & kk) == 0)) { nodes[i] = w; nodes[x] = u; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += SHADOW_THREADS) set_out[(size_t)b * C + i] = nodes[i];

    // ---- the induced entries of every member: a wavefront per short row
    shadow_rows(rowptr, nodes, 0, n, ra, rdeg);
    __syncthreads();
    for (int i = wid; i < n; i += SHADOW_WAVES) {
        const int64_t a = ra[i];
        const long long deg = rdeg[i];
        if (deg > SHADOW_LONG_ROW) {
            if (lane == 0) longs[atomicAdd(n_long, 1)] = i;
            continue;
        }
        int c = 0;
        for (long long t0 = 0; t0 < deg; t0 += 64) {
            const long long t = t0 + lane;
            const int cj = t < deg ? col[a + t] : -1;
            const bool valid = (unsigned)cj < (unsigned)N;
            if (t < deg && !valid) bad = true;
            c += __popcll(__ballot(valid && shadow_rank(nodes, n, cj) >= 0));
        }
        if (lane == 0) cnt[i] = c;
    }
    __syncthreads();
    // the long rows, each by the whole workgroup (their order in the list changes nothing: a row's count is its own)
    const int nl = *n_long;
    for (int q = 0; q < nl; ++q) {
        const int i = longs[q];
        const int64_t a = ra[i];
        const long long deg = rdeg[i];
        int c = 0;
        for (long long t0 = 0; t0 < deg; t0 += SHADOW_THREADS) {
            const long long t = t0 + tid;
            const int cj = t < deg ? col[a + t] : -1;
            const bool valid = (unsigned)cj < (unsigned)N;
            if (t < deg && !valid) bad = true;
            c += __popcll(__ballot(valid && shadow_rank(nodes, n, cj) >= 0));
        }
        if (lane == 0) atomicAdd(&cnt[i], c);
    }
    __syncthreads();
    int s = 0;
    for (int i = tid; i < n; i += SHADOW_THREADS) { const int c = cnt[i]; cnt_out[(size_t)b * C + i] = c; s += c; }
    int total;
    block_excl_scan(s, scan_lds, &total);
    if (tid == 0) { nb[b] = n; eb[b] = total; }
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
}

__global__ __launch_bounds__(SHADOW_THREADS) void shadow_build_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                                 const int32_t* __restrict__ roots, int m_host,
                                                                 const int32_t* __restrict__ d_m, int depth, int fanout, int C,
                                                                 const uint32_t* __restrict__ words, uint64_t seed,
                                                                 uint64_t philox_offset, const uint64_t* __restrict__ d_philox_offset,
                                                                 int32_t* __restrict__ set_out, int32_t* __restrict__ cnt_out,
                                                                 int32_t* __restrict__ nb, int32_t* __restrict__ eb, int32_t* status) {
    __shared__ int nodes[SHADOW_MAX_NODES];
    __shared__ int cnt[SHADOW_MAX_NODES];
    __shared__ int hash[SHADOW_HASH];                                           // after the hops: the list of long member rows
    __shared__ int64_t ra[SHADOW_MAX_NODES];                                    // row starts: of the frontier, then of the members
    __shared__ int rdeg[SHADOW_MAX_NODES];                                      // and their degrees
    __shared__ int64_t cpos[SHADOW_MAX_NODES];                                  // a hop's chosen positions in col
    __shared__ int scan_lds[17];
    __shared__ int n_nodes, n_long, n_cand;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int live = eff_count(d_m, m_host);
    const int root = b < live ? roots[b] : -1;
    if ((unsigned)root >= (unsigned)N) {                                        // (workgroup-uniform) an empty ego-net
        if (tid == 0) {
            nb[b] = 0; eb[b] = 0;
            if (b < live && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        }
        return;
    }
    for (int i = tid; i < SHADOW_HASH; i += SHADOW_THREADS) hash[i] = SHADOW_EMPTY;
    __syncthreads();
    if (tid == 0) {
        nodes[0] = root; n_nodes = 1; n_long = 0;
        hash[((unsigned)root * 0x9E3779B1u) >> 21] = root;
    }
    __syncthreads();
    const uint64_t off = d_philox_offset ? *d_philox_offset : philox_offset;
    bool bad = false;

    // ---- the hops: F_{h-1} = nodes[f0 .. f1), F_h is appended behind it
    int f0 = 0;
    for (int h = 1; h <= depth; ++h) {
        const int f1 = n_nodes < SHADOW_MAX_NODES ? n_nodes : SHADOW_MAX_NODES;
        __syncthreads();                                                        // (every wavefront holds f1 before the list grows)
        const uint64_t hi = off + (uint64_t)b * (uint64_t)depth + (uint64_t)(h - 1);
        if (tid == 0) n_cand = 0;
        shadow_rows(rowptr, nodes, f0, f1, ra, rdeg);                           // one round trip for the frontier's row pointers
        __syncthreads();
        // a wavefront per frontier node: its chosen positions onto the hop's candidate list (no memory access in this loop)
        for (int i = f0 + wid; i < f1; i += SHADOW_WAVES) {
            const int v = nodes[i];
            const int64_t a = ra[i];
            const unsigned long long deg = (unsigned long long)rdeg[i];
            long long pos = -1;
            if (deg <= (unsigned long long)fanout) {
                if ((unsigned long long)lane < deg) pos = lane;
            } else {
                uint32_t w = 0u;
                if (lane < fanout) {
                    if (words) {
                        w = words[((size_t)b * depth + (h - 1)) * fanout + lane];
                    } else {
                        const Philox4 p = philox4x32_10_wide(((uint64_t)(uint32_t)v << 4) | (uint64_t)(lane >> 2), hi, seed);
                        const int q = lane & 3;
                        w = q == 0 ? p.v[0] : (q == 1 ? p.v[1] : (q == 2 ? p.v[2] : p.v[3]));
                    }
                }
                unsigned long long chosen = ~0ull;                              // lane s < the step: the s-th chosen position
                for (int s = 0; s < fanout; ++s) {
                    const unsigned long long j = deg - (unsigned long long)fanout + (unsigned long long)s;
                    const uint32_t ws = (uint32_t)__shfl((int)w, s, 64);
                    const unsigned long long t = ((unsigned long long)ws * (j + 1ull)) >> 32;
                    const bool present = __any(lane < s && chosen == t);
                    if (lane == s) chosen = present ? j : t;                    // (j itself is new: every earlier choice is below it)
                }
                if (lane < fanout) pos = (long long)chosen;
            }
            const int kept = deg <= (unsigned long long)fanout ? (int)deg : fanout;
            int cb = 0;
            if (lane == 0 && kept) cb = atomicAdd(&n_cand, kept);
            cb = __shfl(cb, 0, 64);
            if (pos >= 0 && cb + lane < SHADOW_MAX_NODES) cpos[cb + lane] = a + pos;   // (always: |F_{h-1}| k <= k^h < C)
        }
        __syncthreads();
        // the candidates' ids in one round trip, every thread loading; the list's order changes nothing: the result is a set
        const int nc = n_cand < SHADOW_MAX_NODES ? n_cand : SHADOW_MAX_NODES;
        for (int q = tid; q < nc; q += SHADOW_THREADS) {
            const int c = col[cpos[q]];
            if ((unsigned)c < (unsigned)N) shadow_insert(hash, nodes, &n_nodes, c); else bad = true;
        }
        __syncthreads();
        f0 = f1;
    }
    int n = n_nodes < SHADOW_MAX_NODES ? n_nodes : SHADOW_MAX_NODES;
    n = n < C ? n : C;

    shadow_stage(rowptr, col, N, b, C, n, nodes, cnt, hash, ra, rdeg, scan_lds, &n_long, set_out, cnt_out, nb, eb, status, bad);
}

// ONE workgroup.  ptr[b] = min(nodes of the ego-nets before b, n_cap), eoff[b] the same for the entries and e_cap; ptr[m], eoff[m],
// *d_n, *d_e = the clamped totals; more raise GRAPES_STATUS_NODE_OVERFLOW / GRAPES_STATUS_EDGE_OVERFLOW.  *d_philox_offset advances.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void shadow_scan_k(const int32_t* __restrict__ nb, const int32_t* __restrict__ eb,
                                                                   int m_host, const int32_t* __restrict__ d_m, int depth, int n_cap,
                                                                   int e_cap, int32_t* __restrict__ ptr, int32_t* __restrict__ eoff,
                                                                   int32_t* __restrict__ d_n, int32_t* __restrict__ d_e,
                                                                   uint64_t* d_philox_offset, int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int per = (m_host + LIST_SCAN_THREADS - 1) / LIST_SCAN_THREADS;
    const int lo = (int)threadIdx.x * per, hi = min(lo + per, m_host);
    unsigned long long sn = 0ull, se = 0ull;
    for (int i = lo; i < hi; ++i) { sn += (unsigned long long)nb[i]; se += (unsigned long long)eb[i]; }
    unsigned long long tn, te;
    unsigned long long rn = block_excl_scan_u64(sn, lds, &tn);
    unsigned long long re = block_excl_scan_u64(se, lds, &te);
    for (int i = lo; i < hi; ++i) {
        ptr[i] = (int)(rn < (unsigned long long)n_cap ? rn : (unsigned long long)n_cap);
        eoff[i] = (int)(re < (unsigned long long)e_cap ? re : (unsigned long long)e_cap);
        rn += (unsigned long long)nb[i]; re += (unsigned long long)eb[i];
    }
    if (threadIdx.x == 0) {
        const int t = tn < (unsigned long long)n_cap ? (int)tn : n_cap;
        ptr[m_host] = t;
        *d_n = t;
        if (tn > (unsigned long long)n_cap && status) atomicOr(status, GRAPES_STATUS_NODE_OVERFLOW);
        if (d_philox_offset) *d_philox_offset += (uint64_t)eff_count(d_m, m_host) * (uint64_t)depth;
    }
    list_scan_finish(te, e_cap, eoff + m_host, d_e, status);
}

// A workgroup per root: its rows of n_id / batch, root_n_id, and its edges behind eoff[b] — local row ascending, within a row in the
// CSR's order.  Nothing is written at or past n_cap / e_cap.  score_in (optional): the staged [B, C] scores of the members, copied
// to score beside n_id; with NULL nothing more is read or written.  SCORES = false compiles the copy out for the k-hop
// sampler's launch, which never has scores: a run-time NULL test there measured 0.8 - 1.2 us on its 175 us call
// (profiles/shadow_ppr_bench.json, refactor_check).
template <bool SCORES>
__global__ __launch_bounds__(SHADOW_THREADS) void shadow_write_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                                 const int32_t* __restrict__ roots, int C,
                                                                 const int32_t* __restrict__ set_in, const int32_t* __restrict__ cnt_in,
                                                                 const int32_t* __restrict__ nb, const int32_t* __restrict__ ptr,
                                                                 const int32_t* __restrict__ eoff, int n_cap, int e_cap,
                                                                 int32_t* __restrict__ n_id, int32_t* __restrict__ batch,
                                                                 int32_t* __restrict__ root_n_id, int32_t* __restrict__ edge_src,
                                                                 int32_t* __restrict__ edge_dst, int64_t* __restrict__ e_id,
                                                                 const uint32_t* __restrict__ score_in, uint32_t* __restrict__ score) {
    __shared__ int nodes[SHADOW_MAX_NODES];
    __shared__ int roff[SHADOW_MAX_NODES];
    __shared__ int longs[SHADOW_MAX_NODES];
    __shared__ int64_t ra[SHADOW_MAX_NODES];
    __shared__ int rdeg[SHADOW_MAX_NODES];
    __shared__ int scan_lds[17];
    __shared__ int wc[SHADOW_WAVES];
    __shared__ int n_long;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int n = nb[b];
    n = n < C ? n : C;
    if (n <= 0) {                                                               // (workgroup-uniform)
        if (tid == 0) root_n_id[b] = -1;
        return;
    }
    const int nbase = ptr[b], ebase = eoff[b];
    if (tid == 0) n_long = 0;
    int v[SHADOW_PER], s = 0;
#pragma unroll
    for (int q = 0; q < SHADOW_PER; ++q) {
        const int i = SHADOW_PER * tid + q;
        v[q] = i < n ? cnt_in[(size_t)b * C + i] : 0;
        if (i < n) nodes[i] = set_in[(size_t)b * C + i];
        s += v[q];
    }
    int total;
    int run = block_excl_scan(s, scan_lds, &total);
#pragma unroll
    for (int q = 0; q < SHADOW_PER; ++q) {
        if (SHADOW_PER * tid + q < n) roff[SHADOW_PER * tid + q] = run;
        run += v[q];
    }
    __syncthreads();
    for (int i = tid; i < n; i += SHADOW_THREADS) {
        if (nbase + i < n_cap) { n_id[nbase + i] = nodes[i]; batch[nbase + i] = b; }
    }
    if (SCORES && score_in) {                                                   // (the PPR scopes: a member's staged score beside its id)
        for (int i = tid; i < n; i += SHADOW_THREADS)
            if (nbase + i < n_cap) score[nbase + i] = score_in[(size_t)b * C + i];
    }
    if (tid == 0) root_n_id[b] = nbase + shadow_rank(nodes, n, roots[b]);       // (the root is a member)
    if (ebase >= e_cap) return;                                                 // (workgroup-uniform) every slot is past the capacity

    shadow_rows(rowptr, nodes, 0, n, ra, rdeg);
    __syncthreads();
    for (int i = wid; i < n; i += SHADOW_WAVES) {
        const int64_t a = ra[i];
        const long long deg = rdeg[i];
        if (deg > SHADOW_LONG_ROW) {
            if (lane == 0) longs[atomicAdd(&n_long, 1)] = i;
            continue;
        }
        int base = ebase + roff[i];
        for (long long t0 = 0; t0 < deg; t0 += 64) {
            const long long t = t0 + lane;
            const int cj = t < deg ? col[a + t] : -1;
            const int r = (unsigned)cj < (unsigned)N ? shadow_rank(nodes, n, cj) : -1;
            const int p = wave_compact_slot(r >= 0, lane, base);
            if (r >= 0 && p < e_cap) {
                edge_src[p] = nbase + r; edge_dst[p] = nbase + i;
                if (e_id) e_id[p] = (int64_t)(a + t);
            }
        }
    }
    __syncthreads();
    const int nl = n_long;
    for (int q = 0; q < nl; ++q) {
        const int i = longs[q];
        const int64_t a = ra[i];
        const long long deg = rdeg[i];
        int base = ebase + roff[i];
        for (long long t0 = 0; t0 < deg; t0 += SHADOW_THREADS) {
            const long long t = t0 + tid;
            const int cj = t < deg ? col[a + t] : -1;
            const int r = (unsigned)cj < (unsigned)N ? shadow_rank(nodes, n, cj) : -1;
            const unsigned long long bal = __ballot(r >= 0);
            if (lane == 0) wc[wid] = __popcll(bal);
            __syncthreads();
            int pre = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < SHADOW_WAVES; ++w) { const int x = wc[w]; tot += x; pre += w < wid ? x : 0; }
            const int p = base + pre + __popcll(bal & ((1ull << lane) - 1ull));
            if (r >= 0 && p < e_cap) {
                edge_src[p] = nbase + r; edge_dst[p] = nbase + i;
                if (e_id) e_id[p] = (int64_t)(a + t);
            }
            base += tot;
            __syncthreads();                                                    // (wc is rewritten by the next trip)
        }
    }
}

// set int32[m * C] | cnt int32[m * C] | nb int32[m] | eb int32[m] | eoff int32[m + 1]
extern "C" size_t grapes_shadow_sample_workspace_bytes(int32_t m, int32_t depth, int32_t fanout) {
    const int C = shadow_cap(depth, fanout);
    if (m < 1 || m > SHADOW_MAX_ROOTS || C == 0) return 0;
    return ((size_t)2 * m * C + (size_t)3 * m + 1) * 4 + 16;
}

extern "C" int grapes_shadow_sample(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m,
                                    const int32_t* d_m, int32_t depth, int32_t fanout, const uint32_t* words, uint64_t philox_seed,
                                    uint64_t philox_offset, uint64_t* d_philox_offset, int32_t n_cap, int32_t e_cap, int32_t* n_id,
                                    int32_t* ptr, int32_t* batch, int32_t* root_n_id, int32_t* edge_src, int32_t* edge_dst,
                                    int64_t* e_id, int32_t* d_n, int32_t* d_e, void* workspace, int32_t* status,
                                    grapes_stream_t stream) {
    const int C = shadow_cap(depth, fanout);
    if (num_nodes <= 0 || m < 1 || m > SHADOW_MAX_ROOTS || C == 0 || n_cap <= 0 || e_cap <= 0) return GRAPES_EINVAL;
    if (!rowptr || !col || !roots || !n_id || !ptr || !batch || !root_n_id || !edge_src || !edge_dst || !d_n || !d_e || !workspace)
        return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* set = (int32_t*)workspace;
    int32_t* cnt = set + (size_t)m * C;
    int32_t* nb = cnt + (size_t)m * C;
    int32_t* eb = nb + m;
    int32_t* eoff = eb + m;
    hipLaunchKernelGGL(shadow_build_k, dim3(m), dim3(SHADOW_THREADS), 0, s, rowptr, col, num_nodes, roots, m, d_m, depth, fanout, C,
                       words, philox_seed, philox_offset, (const uint64_t*)d_philox_offset, set, cnt, nb, eb, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(shadow_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, (const int32_t*)nb, (const int32_t*)eb, m, d_m, depth,
                       n_cap, e_cap, ptr, eoff, d_n, d_e, d_philox_offset, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(shadow_write_k<false>, dim3(m), dim3(SHADOW_THREADS), 0, s, rowptr, col, num_nodes, roots, C, (const int32_t*)set,
                       (const int32_t*)cnt, (const int32_t*)nb, (const int32_t*)ptr, (const int32_t*)eoff, n_cap, e_cap, n_id, batch,
                       root_n_id, edge_src, edge_dst, e_id, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the PPR scopes
// grapes_shadow_ppr_sample: the scope of a root is the k best nodes of an approximate personalised PageRank from it, by synchronous
// forward push in FIXED POINT (the rule in include/grapes_hip.h; tests/shadow_ppr_oracle.py reproduces it bit for bit).
//   shadow_ppr_build_k   a workgroup per root, the touched table in LDS: an open-addressing hash of PPR_HASH = 8192 id slots with the
//                    residual r beside it (the one array other nodes' pushes add into: integer LDS atomics), at most half full, so
//                    a probe always ends; per TOUCHED INDEX (insertion order, at most PPR_T = 4096) the slot, the row start, the
//                    degree and p — p is only ever written by its own node's push, so it needs no slot and no atomic.
//                    A round is two dependent memory trips whatever the frontier's size: (1) every thread fetches the row pointers of
//                    one newly touched node (degrees and row starts stay cached in LDS for the rest of the call); (2) after the
//                    workgroup scan that counts the frontier and its entries — the three stops are workgroup-uniform decisions on
//                    its totals — the frontier's entries are walked FLAT: the stop-2 rule bounds a round that runs to
//                    sum deg <= PPR_T entries, so a thread takes at most PPR_PER = 4 of them, finds each one's frontier row by a
//                    binary search of the rows' offsets in LDS, and requests its columns together.  A hub row is spread over the
//                    workgroup like any other, so the push itself needs no long-row path (the induced-entry count in
//                    shadow_stage keeps its own).  Then CAS to insert, add to r.
//                    Selection: one 64-bit key per touched node, (2^32 - 1 - score) << 32 | id — ascending keys are score
//                    descending, then id ascending; the root and zero scores get the largest key — over the dead row-start / degree
//                    arrays, and ONE bitonic sort.  Bitonic and not a radix select: the sort is the network shadow_stage already
//                    runs, has one path for every size, and is 78 LDS passes of 4 keys per thread at the most; a radix select over
//                    64-bit keys is 8 histogram passes with LDS atomics plus a compaction that must still resolve the ties at the
//                    k-th key by id.  (Neither has been timed against the other.)  The first k keys and the root enter
//                    shadow_stage; each member's score is staged at its rank in the sorted set.
//   shadow_scan_k / shadow_write_k as above (depth 0: there is no stream to advance); the write copies the staged scores.
// Integer code only, no float, no global atomic beyond the status OR, no kernel waits on another workgroup.  Which lane wins a slot or
// which touched index a node gets changes nothing: r and p are sums of integers, and the keys are distinct.
//
// The rounds and the selection are ppr_push_select, a __device__ function (as shadow_stage is the other half): PPRGo's
// grapes_pprgo_topk (pprgo_topk_k, below the build kernel) enters it too and then writes the sorted keys' prefix straight out in rank
// order — no sort by id, no induced-entry count, no scan, no edge write: one launch.  Compiler's remarks for gfx950
// (-Rpass-analysis=kernel-resource-usage): shadow_ppr_build_k 155 868 B LDS, 56 VGPRs, occupancy 4 waves per SIMD (one workgroup of 16
// wavefronts per CU, bound by the LDS block), 2 890 instructions (2 889 before the function was cut out; shadow_build_k 1 147 both
// times); pprgo_topk_k 155 864 B LDS, 50 VGPRs, occupancy 4, 2 090 instructions.
#define PPR_T 4096                      // the touched-set capacity: part of the rule
#define PPR_HASH 8192
#define PPR_ONE (1u << 30)
#define PPR_MAX_K (SHADOW_MAX_NODES - 1)
#define PPR_MAX_ROUNDS 1024
#define PPR_PER (PPR_T / SHADOW_THREADS)
static_assert(PPR_T == PPR_PER * SHADOW_THREADS && PPR_HASH == 2 * PPR_T && PPR_T <= 65536, "a thread takes PPR_PER touched nodes; 16-bit lists");
// one LDS block, carved by hand so that the selection's keys and the stage's arrays can lie over what is dead by then
#define PPR_O_HKEY 0                               // int      [PPR_HASH]  ids; after the selection: shadow_stage's arrays
#define PPR_O_HR (PPR_O_HKEY + 4 * PPR_HASH)       // uint32   [PPR_HASH]  r, by slot
#define PPR_O_TRA (PPR_O_HR + 4 * PPR_HASH)        // uint32   [PPR_T]     row start (fewer than 2^31 entries)   } after the rounds: the
#define PPR_O_TDEG (PPR_O_TRA + 4 * PPR_T)         // int      [PPR_T]     degree                                } PPR_T 64-bit keys
#define PPR_O_TP (PPR_O_TDEG + 4 * PPR_T)          // uint32   [PPR_T]     p
#define PPR_O_FR (PPR_O_TP + 4 * PPR_T)            // uint32   [PPR_T]     the frontier's snapshot of r
#define PPR_O_TSLOT (PPR_O_FR + 4 * PPR_T)         // uint16   [PPR_T]     touched index -> slot
#define PPR_O_FT (PPR_O_TSLOT + 2 * PPR_T)         // uint16   [PPR_T]     frontier position -> touched index
#define PPR_O_FOFF (PPR_O_FT + 2 * PPR_T)          // uint16   [PPR_T]     frontier position -> its first entry in the flat walk
#define PPR_LDS_BYTES (PPR_O_FOFF + 2 * PPR_T)     // 152 KiB of the CU's 160
static_assert(PPR_O_TDEG == PPR_O_TRA + 4 * PPR_T && 8 * PPR_T == 2 * 4 * PPR_T, "the keys lie over tra and tdeg");
static_assert(4 * PPR_HASH >= SHADOW_MAX_NODES * (4 + 4 + 4 + 8 + 4), "the stage's arrays lie over the id slots");

// id -> its slot (-1: no free slot, which the rule's capacity check excludes); the lane that takes an empty slot appends the touched index
__device__ __forceinline__ int ppr_insert(int* hkey, unsigned short* tslot, int* n_touched, int c) {
    unsigned slot = ((unsigned)c * 0x9E3779B1u) >> 19;                          // 13 bits
    for (int probe = 0; probe < PPR_HASH; ++probe) {
        const int old = atomicCAS(&hkey[slot], SHADOW_EMPTY, c);
        if (old == SHADOW_EMPTY) {
            const int idx = atomicAdd(n_touched, 1);
            if (idx < PPR_T) tslot[idx] = (unsigned short)slot;                  // (always: |S| + sum deg <= PPR_T before the round ran)
            return (int)slot;
        }
        if (old == c) return (int)slot;
        slot = (slot + 1) & (PPR_HASH - 1);
    }
    return -1;
}

// The first half of a PPR kernel, shared by shadow_ppr_build_k and pprgo_topk_k: the rounds of root `root` (inside [0, N)) and the
// selection.  Leaves the sorted keys at lds + PPR_O_TRA — key i < n_valid is the i-th best node, (2^32 - 1 - score) << 32 | id — and
// returns min(n_valid, k); rounds, stop and the root's score go to the caller's variables, `bad` is set by a thread that met a column
// outside [0, N).  The caller hands over the carved LDS block, block_excl_scan3's 51 ints and the three shared words (n_long = 0 is
// the stage's and is set here with the others).  Every thread of the workgroup calls it and leaves it behind a barrier.
__device__ __forceinline__ int ppr_push_select(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N, int root, int k,
                                               uint32_t alpha_q, uint32_t thr, int max_rounds, unsigned char* lds, int* scan_lds,
                                               int& n_touched, int& n_long, int& n_valid, uint32_t& root_score, int& rounds_ret,
                                               int& stop_ret, bool& bad) {
    int* hkey = (int*)(lds + PPR_O_HKEY);
    uint32_t* hr = (uint32_t*)(lds + PPR_O_HR);
    uint32_t* tra = (uint32_t*)(lds + PPR_O_TRA);
    int* tdeg = (int*)(lds + PPR_O_TDEG);
    uint32_t* tp = (uint32_t*)(lds + PPR_O_TP);
    uint32_t* fr = (uint32_t*)(lds + PPR_O_FR);
    unsigned short* tslot = (unsigned short*)(lds + PPR_O_TSLOT);
    unsigned short* ft = (unsigned short*)(lds + PPR_O_FT);
    unsigned short* foff = (unsigned short*)(lds + PPR_O_FOFF);
    const int tid = threadIdx.x;
    for (int i = tid; i < PPR_HASH; i += SHADOW_THREADS) { hkey[i] = SHADOW_EMPTY; hr[i] = 0u; }
    for (int i = tid; i < PPR_T; i += SHADOW_THREADS) tp[i] = 0u;
    __syncthreads();
    if (tid == 0) {
        const unsigned slot = ((unsigned)root * 0x9E3779B1u) >> 19;
        hkey[slot] = root; hr[slot] = PPR_ONE; tslot[0] = (unsigned short)slot;    // touched index 0 is the root
        n_touched = 1; n_long = 0; n_valid = 0;
    }
    __syncthreads();

    // ---- the rounds
    int known = 0, rounds = 0, stop = 0;
    for (;;) {
        const int nT = n_touched < PPR_T ? n_touched : PPR_T;
        for (int t = known + tid; t < nT; t += SHADOW_THREADS) {                // one round trip for the newly touched nodes' row pointers
            const int v = hkey[tslot[t]];
            const int64_t a = rowptr[v], d = rowptr[v + 1] - a;
            tra[t] = (uint32_t)a;
            tdeg[t] = d < 0 ? 0 : (d > 0x7fffffffll ? 0x7fffffff : (int)d);
        }
        known = nT;
        __syncthreads();
        // F, |F| and sum deg: a thread looks at PPR_PER consecutive touched indices.  A degree counts as at most PPR_T + 1 in the sum:
        // the sum then stays in an int, and "more than PPR_T" is decided as by the exact sum.
        uint32_t rv[PPR_PER];
        int dg[PPR_PER], c = 0, ds = 0, z = 0;
#pragma unroll
        for (int q = 0; q < PPR_PER; ++q) {
            const int t = PPR_PER * tid + q;
            rv[q] = 0u; dg[q] = 0;
            if (t < nT) {
                const uint32_t r = hr[tslot[t]];
                const int deg = tdeg[t];
                if (r > 0u && (unsigned long long)r >= (unsigned long long)thr * (unsigned long long)deg) {
                    rv[q] = r; dg[q] = deg;
                    ++c; ds += deg < PPR_T + 1 ? deg : PPR_T + 1;
                }
            }
        }
        int nF, E, zz;
        block_excl_scan3(c, ds, z, scan_lds, &nF, &E, &zz);
        if (nF == 0) { stop = 0; break; }                                       // (workgroup-uniform, all three)
        if (rounds == max_rounds) { stop = 1; break; }
        if (nT + E > PPR_T) { stop = 2; break; }
        // the snapshot: (touched index, r, first entry) at the frontier position, and r = 0 (every deg <= PPR_T here: E is exact)
#pragma unroll
        for (int q = 0; q < PPR_PER; ++q) {
            if (rv[q]) {
                const int t = PPR_PER * tid + q;
                ft[c] = (unsigned short)t; fr[c] = rv[q]; foff[c] = (unsigned short)ds;
                hr[tslot[t]] = 0u;
                ++c; ds += dg[q];
            }
        }
        __syncthreads();
        // p: a thread per frontier node (its own p: no atomic)
        for (int f = tid; f < nF; f += SHADOW_THREADS) {
            const int t = ft[f];
            const uint32_t r = fr[f];
            tp[t] += tdeg[t] == 0 ? r : (uint32_t)(((unsigned long long)r * alpha_q) >> 16);
        }
        // the push: the frontier's E <= PPR_T entries flat over the workgroup, a thread's columns requested together
        int cj[PPR_PER];
        uint32_t sh[PPR_PER];
#pragma unroll
        for (int q = 0; q < PPR_PER; ++q) {
            const int e = tid + q * SHADOW_THREADS;
            cj[q] = 0; sh[q] = 0u;
            if (e < E) {
                int lo = 0, hi = nF;                                            // the last frontier position with foff <= e: empty rows
                while (lo < hi) {                                               // share their successor's offset and are skipped
                    const int mid = (lo + hi) >> 1;
                    if ((int)foff[mid] <= e) lo = mid + 1; else hi = mid;
                }
                const int f = lo - 1, t = ft[f];
                const uint32_t r = fr[f], keep = (uint32_t)(((unsigned long long)r * alpha_q) >> 16);
                sh[q] = (r - keep) / (uint32_t)tdeg[t];
                cj[q] = col[(size_t)tra[t] + (size_t)(e - (int)foff[f])];
            }
        }
#pragma unroll
        for (int q = 0; q < PPR_PER; ++q) {
            if (tid + q * SHADOW_THREADS < E) {
                if ((unsigned)cj[q] < (unsigned)N) {
                    const int slot = ppr_insert(hkey, tslot, &n_touched, cj[q]);
                    if (slot >= 0) atomicAdd(&hr[slot], sh[q]);
                } else {
                    bad = true;                                                 // dropped: its share is lost
                }
            }
        }
        __syncthreads();
        ++rounds;
    }
    // (every thread left the loop behind block_excl_scan3's last barrier: the tables are final and tra / tdeg are dead)

    // ---- the selection: one key per touched node, sorted ascending
    const int nT = n_touched < PPR_T ? n_touched : PPR_T;
    unsigned long long* keys = (unsigned long long*)(lds + PPR_O_TRA);
    int P = 1;
    while (P < nT) P <<= 1;
    for (int t = tid; t < P; t += SHADOW_THREADS) {
        unsigned long long key = ~0ull;
        if (t < nT) {
            const int slot = tslot[t];
            const uint32_t sc = tp[t] + (uint32_t)(((unsigned long long)hr[slot] * alpha_q) >> 16);
            if (t == 0) root_score = sc;
            else if (sc > 0u) key = ((unsigned long long)(0xffffffffu - sc) << 32) | (unsigned long long)(uint32_t)hkey[slot];
        }
        keys[t] = key;
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += SHADOW_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long u = keys[i], w = keys[x];
                    if ((u > w) == ((i & kk) == 0)) { keys[i] = w; keys[x] = u; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < P; i += SHADOW_THREADS)                               // the candidates are the keys in front of the first ~0
        if (keys[i] != ~0ull && (i + 1 == P || keys[i + 1] == ~0ull)) n_valid = i + 1;
    __syncthreads();
    rounds_ret = rounds; stop_ret = stop;
    return n_valid < k ? n_valid : k;
}

__global__ __launch_bounds__(SHADOW_THREADS) void shadow_ppr_build_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                     int N, const int32_t* __restrict__ roots, int m_host,
                                                                     const int32_t* __restrict__ d_m, int k, uint32_t alpha_q,
                                                                     uint32_t thr, int max_rounds, int C,
                                                                     int32_t* __restrict__ set_out, int32_t* __restrict__ cnt_out,
                                                                     uint32_t* __restrict__ score_out, int32_t* __restrict__ nb,
                                                                     int32_t* __restrict__ eb, int32_t* __restrict__ rounds_out,
                                                                     int32_t* __restrict__ stop_out, int32_t* status) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[PPR_LDS_BYTES];
    __shared__ int scan_lds[51];
    __shared__ int n_touched, n_long, n_valid;
    __shared__ uint32_t root_score;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int live = eff_count(d_m, m_host);
    const int root = b < live ? roots[b] : -1;
    if ((unsigned)root >= (unsigned)N) {                                        // (workgroup-uniform) an empty ego-net
        if (tid == 0) {
            nb[b] = 0; eb[b] = 0;
            if (rounds_out) rounds_out[b] = 0;
            if (stop_out) stop_out[b] = 0;
            if (b < live && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        }
        return;
    }
    bool bad = false;
    int rounds, stop;
    const int n_sel = ppr_push_select(rowptr, col, N, root, k, alpha_q, thr, max_rounds, lds, scan_lds, n_touched, n_long, n_valid, root_score,
                                      rounds, stop, bad);
    const int n = 1 + n_sel;
    const unsigned long long* keys = (const unsigned long long*)(lds + PPR_O_TRA);

    // ---- the members enter the shared stage, whose arrays lie over the id slots (dead: the keys carry the ids)
    int* nodes = (int*)(lds + PPR_O_HKEY);
    int* cnt = nodes + SHADOW_MAX_NODES;
    int* longs = cnt + SHADOW_MAX_NODES;
    int64_t* ra = (int64_t*)(longs + SHADOW_MAX_NODES);
    int* rdeg = (int*)(ra + SHADOW_MAX_NODES);
    for (int i = tid; i < n; i += SHADOW_THREADS) nodes[i] = i == 0 ? root : (int)(uint32_t)keys[i - 1];
    __syncthreads();
    shadow_stage(rowptr, col, N, b, C, n, nodes, cnt, longs, ra, rdeg, scan_lds, &n_long, set_out, cnt_out, nb, eb, status, bad);
    // a member's score at its rank in the sorted set
    for (int i = tid; i < n; i += SHADOW_THREADS) {
        const int v = i == 0 ? root : (int)(uint32_t)keys[i - 1];
        const uint32_t sc = i == 0 ? root_score : 0xffffffffu - (uint32_t)(keys[i - 1] >> 32);
        const int rk = shadow_rank(nodes, n, v);
        if (rk >= 0) score_out[(size_t)b * C + rk] = sc;
    }
    if (tid == 0) {
        if (rounds_out) rounds_out[b] = rounds;
        if (stop_out) stop_out[b] = stop;
    }
}

// grapes_pprgo_topk: the same push and selection WITHOUT the ego-net — a workgroup per root writes the root and the sorted keys'
// prefix straight into the fixed slots nbr / score [m][K], K = k + 1, in rank order: no sort by id, no induced-entry count, no scan
// and no edge write, so one launch and no workspace.  Slots at or past cnt[b] hold (root, 0); a root that names no node leaves
// (-1, 0) and cnt = 0.
__global__ __launch_bounds__(SHADOW_THREADS) void pprgo_topk_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                               const int32_t* __restrict__ roots, int m_host,
                                                               const int32_t* __restrict__ d_m, int k, uint32_t alpha_q, uint32_t thr,
                                                               int max_rounds, int32_t* __restrict__ nbr, uint32_t* __restrict__ score,
                                                               int32_t* __restrict__ cnt_out, int32_t* __restrict__ rounds_out,
                                                               int32_t* __restrict__ stop_out, int32_t* status) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[PPR_LDS_BYTES];
    __shared__ int scan_lds[51];
    __shared__ int n_touched, n_long, n_valid;
    __shared__ uint32_t root_score;
    const int b = blockIdx.x, tid = threadIdx.x, K = k + 1;
    const int live = eff_count(d_m, m_host);
    const int root = b < live ? roots[b] : -1;
    if ((unsigned)root >= (unsigned)N) {                                        // (workgroup-uniform) no node: empty slots
        for (int i = tid; i < K; i += SHADOW_THREADS) { nbr[(size_t)b * K + i] = -1; score[(size_t)b * K + i] = 0u; }
        if (tid == 0) {
            cnt_out[b] = 0;
            if (rounds_out) rounds_out[b] = 0;
            if (stop_out) stop_out[b] = 0;
            if (b < live && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        }
        return;
    }
    bool bad = false;
    int rounds, stop;
    const int n_sel = ppr_push_select(rowptr, col, N, root, k, alpha_q, thr, max_rounds, lds, scan_lds, n_touched, n_long, n_valid, root_score,
                                      rounds, stop, bad);
    const unsigned long long* keys = (const unsigned long long*)(lds + PPR_O_TRA);
    for (int i = tid; i < K; i += SHADOW_THREADS) {
        int v = root;
        uint32_t sc = 0u;
        if (i == 0) sc = root_score;
        else if (i <= n_sel) { const unsigned long long key = keys[i - 1]; v = (int)(uint32_t)key; sc = 0xffffffffu - (uint32_t)(key >> 32); }
        nbr[(size_t)b * K + i] = v; score[(size_t)b * K + i] = sc;
    }
    if (tid == 0) {
        cnt_out[b] = 1 + n_sel;
        if (rounds_out) rounds_out[b] = rounds;
        if (stop_out) stop_out[b] = stop;
    }
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
}

extern "C" int grapes_pprgo_topk(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m,
                                 const int32_t* d_m, int32_t k, uint32_t alpha_q, uint32_t thr, int32_t max_rounds, int32_t* nbr,
                                 uint32_t* score, int32_t* cnt, int32_t* rounds, int32_t* stop, int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || m < 1 || m > SHADOW_MAX_ROOTS || k < 1 || k > PPR_MAX_K) return GRAPES_EINVAL;
    if (alpha_q < 1u || alpha_q > 65535u || thr < 1u || thr > PPR_ONE || max_rounds < 1 || max_rounds > PPR_MAX_ROUNDS) return GRAPES_EINVAL;
    if (!rowptr || !col || !roots || !nbr || !score || !cnt) return GRAPES_EINVAL;
    hipLaunchKernelGGL(pprgo_topk_k, dim3(m), dim3(SHADOW_THREADS), 0, (hipStream_t)stream, rowptr, col, num_nodes, roots, m, d_m, k,
                       alpha_q, thr, max_rounds, nbr, score, cnt, rounds, stop, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// set int32[m * C] | cnt int32[m * C] | score uint32[m * C] | nb int32[m] | eb int32[m] | eoff int32[m + 1], C = k + 1
extern "C" size_t grapes_shadow_ppr_sample_workspace_bytes(int32_t m, int32_t k) {
    if (m < 1 || m > SHADOW_MAX_ROOTS || k < 1 || k > PPR_MAX_K) return 0;
    return ((size_t)3 * m * (k + 1) + (size_t)3 * m + 1) * 4 + 16;
}

extern "C" int grapes_shadow_ppr_sample(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m,
                                        const int32_t* d_m, int32_t k, uint32_t alpha_q, uint32_t thr, int32_t max_rounds,
                                        int32_t n_cap, int32_t e_cap, int32_t* n_id, int32_t* ptr, int32_t* batch, int32_t* root_n_id,
                                        int32_t* edge_src, int32_t* edge_dst, int64_t* e_id, uint32_t* score, int32_t* rounds,
                                        int32_t* stop, int32_t* d_n, int32_t* d_e, void* workspace, int32_t* status,
                                        grapes_stream_t stream) {
    if (num_nodes <= 0 || m < 1 || m > SHADOW_MAX_ROOTS || k < 1 || k > PPR_MAX_K || n_cap <= 0 || e_cap <= 0) return GRAPES_EINVAL;
    if (alpha_q < 1u || alpha_q > 65535u || thr < 1u || thr > PPR_ONE || max_rounds < 1 || max_rounds > PPR_MAX_ROUNDS) return GRAPES_EINVAL;
    if (!rowptr || !col || !roots || !n_id || !ptr || !batch || !root_n_id || !edge_src || !edge_dst || !d_n || !d_e || !workspace)
        return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int C = k + 1;
    int32_t* set = (int32_t*)workspace;
    int32_t* cnt = set + (size_t)m * C;
    uint32_t* sc = (uint32_t*)(cnt + (size_t)m * C);
    int32_t* nb = (int32_t*)(sc + (size_t)m * C);
    int32_t* eb = nb + m;
    int32_t* eoff = eb + m;
    hipLaunchKernelGGL(shadow_ppr_build_k, dim3(m), dim3(SHADOW_THREADS), 0, s, rowptr, col, num_nodes, roots, m, d_m, k, alpha_q, thr,
                       max_rounds, C, set, cnt, sc, nb, eb, rounds, stop, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(shadow_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, (const int32_t*)nb, (const int32_t*)eb, m, d_m, 0, n_cap,
                       e_cap, ptr, eoff, d_n, d_e, (uint64_t*)nullptr, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(shadow_write_k<true>, dim3(m), dim3(SHADOW_THREADS), 0, s, rowptr, col, num_nodes, roots, C, (const int32_t*)set,
                       (const int32_t*)cnt, (const int32_t*)nb, (const int32_t*)ptr, (const int32_t*)eoff, n_cap, e_cap, n_id, batch,
                       root_n_id, edge_src, edge_dst, e_id, score ? (const uint32_t*)sc : (const uint32_t*)nullptr, score);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the segment mean
// out[b, :] = the mean of h[ptr[b] .. ptr[b + 1], :] (0 for an empty segment).  A workgroup per segment, a thread per column: the rows
// are added in row order and the sum is divided once, so every element is n_b - 1 additions and one division in a fixed order.
#define SEGMEAN_THREADS 256
#define SEGMEAN_MAX_WIDTH 1024

// the rows [a, e) of segment b, or false (and the bad-index bit) when ptr does not describe a run inside [0, n_rows]
__device__ __forceinline__ bool segment_rows(const int32_t* __restrict__ ptr, int b, int n_rows, int& a, int& e, int32_t* status) {
    a = ptr[b]; e = ptr[b + 1];
    if (a < 0 || e < a || e > n_rows) {
        if (threadIdx.x == 0 && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        a = e = 0;
        return false;
    }
    return true;
}

__global__ __launch_bounds__(SEGMEAN_THREADS) void segment_mean_fwd_k(const float* __restrict__ h, const int32_t* __restrict__ ptr,
                                                                      int n_rows, int f, float* __restrict__ out, int32_t* status) {
    const int b = blockIdx.x;
    int a, e;
    segment_rows(ptr, b, n_rows, a, e, status);
    const float n = (float)(e - a);
    for (int c = threadIdx.x; c < f; c += SEGMEAN_THREADS) {
        float s = 0.f;
        for (int r = a; r < e; ++r) s += h[(size_t)r * f + c];
        out[(size_t)b * f + c] = e > a ? s / n : 0.f;
    }
}

// dh[r, :] = g[b, :] / n_b for the rows of segment b; rows in front of the first segment and behind the last get 0
__global__ __launch_bounds__(SEGMEAN_THREADS) void segment_mean_bwd_k(const float* __restrict__ g, const int32_t* __restrict__ ptr,
                                                                      int num_segments, int n_rows, int f, float* __restrict__ dh,
                                                                      int32_t* status) {
    const int b = blockIdx.x;
    int a, e;
    const bool ok = segment_rows(ptr, b, n_rows, a, e, status);
    const float n = (float)(e - a);
    for (int c = threadIdx.x; c < f; c += SEGMEAN_THREADS) {
        const float v = e > a ? g[(size_t)b * f + c] / n : 0.f;
        for (int r = a; r < e; ++r) dh[(size_t)r * f + c] = v;
        if (ok && b == 0)
            for (int r = 0; r < a; ++r) dh[(size_t)r * f + c] = 0.f;
        if (ok && b == num_segments - 1)
            for (int r = e; r < n_rows; ++r) dh[(size_t)r * f + c] = 0.f;
    }
}

static int segment_mean_check(const float* x, const int32_t* ptr, int32_t num_segments, int32_t n_rows, int32_t f, const float* y) {
    if (num_segments < 1 || n_rows < 0 || f < 1 || f > SEGMEAN_MAX_WIDTH || !x || !ptr || !y) return GRAPES_EINVAL;
    return 0;
}

extern "C" int grapes_segment_mean_fwd(const float* h, const int32_t* ptr, int32_t num_segments, int32_t n_rows, int32_t f, float* out,
                                       int32_t* status, grapes_stream_t stream) {
    if (segment_mean_check(h, ptr, num_segments, n_rows, f, out)) return GRAPES_EINVAL;
    hipLaunchKernelGGL(segment_mean_fwd_k, dim3(num_segments), dim3(SEGMEAN_THREADS), 0, (hipStream_t)stream, h, ptr, n_rows, f, out,
                       status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_segment_mean_bwd(const float* g, const int32_t* ptr, int32_t num_segments, int32_t n_rows, int32_t f, float* dh,
                                       int32_t* status, grapes_stream_t stream) {
    if (segment_mean_check(g, ptr, num_segments, n_rows, f, dh)) return GRAPES_EINVAL;
    hipLaunchKernelGGL(segment_mean_bwd_k, dim3(num_segments), dim3(SEGMEAN_THREADS), 0, (hipStream_t)stream, g, ptr, num_segments,
                       n_rows, f, dh, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
