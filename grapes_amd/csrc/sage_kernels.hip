// GraphSAGE [Hamilton et al., NeurIPS 2017; PyG-recall: torch_geometric 2.5.2 SAGEConv, NeighborLoader]: the node-wise uniform
// neighbour sampler over the DeviceGraph CSR.
//
// ---- the sampler (grapes_sage_sample_layer): for every list row r keep min(deg, fanout) of the entries of CSR row rows[r],
// uniformly without replacement.  The rule, bit-reproducible on a CPU (tests/sage_oracle.py):
//   off_r = the exclusive prefix over r, in list order, of deg(rows[r]);  entry t of list row r has stream position p = off_r + t;
//   its key is keys[p] when keys are given, else raw 32-bit word p of the Philox stream (seed, off) — word p & 3 of
//   philox4x32_10(off + p / 4, seed), as grapes_saint_draw_nodes indexes words;
//   row r keeps the min(deg, fanout) entries with the smallest composite (key << 32) | t: unique, so a tie in the word goes to the
//   lower position and nothing depends on scheduling;  kept entries are written for r ascending and within a row for t ascending.
// A row with deg <= fanout keeps everything; its words are skipped all the same, so p is the same on every path.  A row listed
// twice draws twice (its p differs).
//
//   sage_scan_k    ONE workgroup: the rows' degrees, both exclusive prefixes (list_scan_tiles of row_list.h), the edge count, the overflow
//                  bit, the stream's base offset for the write kernel and its advance by ceil(sum deg / 4)
//   sage_write_k   one wavefront per list row.  deg <= fanout: a copy.  deg <= 64: a key per lane, its rank by 64 broadcast
//                  compares, the kept lanes compacted by a ballot.  Longer rows: a lane takes four stream positions (one Philox
//                  call) per trip; an 8-bit radix select on the 32-bit word counts one digit per pass, of the entries that match the
//                  prefix found so far, in a wavefront-private 256-bin LDS histogram; once the candidates (at or below the prefix)
//                  fit 128 slots — after the first pass for a row of up to ~ 16 000 entries — one more pass lists them in order and
//                  the row ends in registers like a short one; words that tie beyond that take four passes and a fifth that writes
//                  word < T and the first positions with word == T.  Two to five generations of the keys: linear in deg, no sort,
//                  nothing through global memory.  Integer arithmetic only.
//
// SAGEConv's aggregation is grapes_rootsum_aggregate_fwd / _bwd (rootsum_kernels.hip).
#include "philox.h"
#include "row_list.h"

#define SAGE_MAX_FANOUT 64
#define SAGE_CAND 128                 // candidates a long row finishes in registers with (two per lane; half the histogram's LDS each for words and positions)

// ------------------------------------------------------------------------------------------------------------ the sampler

// key of stream position p
__device__ __forceinline__ uint32_t sage_key(const uint32_t* __restrict__ keys, long long n_keys, uint64_t seed, uint64_t off,
                                             long long p, int32_t* status) {
    if (keys) {
        if (p < n_keys) return keys[p];
        if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);                // (a key list shorter than the rows' entries)
        return 0xffffffffu;
    }
    return philox_word_at(seed, off, p);
}

// ONE workgroup.  off_p[r] = sum of deg over the list rows before r, off_e[r] = min(sum of min(deg, fanout) before r, e_cap);
// *d_e = min(total, e_cap); *base_off = the stream offset of this call; *d_philox_offset += ceil(sum deg / 4).
// A row id outside [0, N) counts as an empty row and raises GRAPES_STATUS_BAD_INDEX.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void sage_scan_k(const int64_t* __restrict__ rowptr, int N,
                                                                 const int32_t* __restrict__ rows, int m_host,
                                                                 const int32_t* __restrict__ d_m, int fanout, int e_cap,
                                                                 uint64_t philox_offset, uint64_t* d_philox_offset,
                                                                 long long* __restrict__ off_p, uint64_t* __restrict__ base_off,
                                                                 int32_t* __restrict__ off_e, int32_t* __restrict__ d_e,
                                                                 int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int live = eff_count(d_m, m_host);
    bool bad = false;
    auto degrees = [&](int i0, long long (&v)[LIST_SCAN_PER]) {
        list_row_degrees(rowptr, N, rows, i0, live, v, bad);
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q)                               // (the kept count, until the second prefix)
            if (i0 + q < m_host) off_e[i0 + q] = (int)(v[q] < fanout ? v[q] : fanout);
    };
    auto kept = [&](int i0, int (&v)[LIST_SCAN_PER]) {
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) v[q] = i0 + q < m_host ? off_e[i0 + q] : 0;
    };
    const unsigned long long total_d = list_scan_tiles<long long>(degrees, m_host, LIST_NO_CAP, off_p, lds);
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    const unsigned long long total_c = list_scan_tiles<int>(kept, m_host, (unsigned long long)e_cap, off_e, lds);
    list_scan_finish(total_c, e_cap, nullptr, d_e, status);
    if (threadIdx.x == 0) {
        const uint64_t base = d_philox_offset ? *d_philox_offset : philox_offset;
        *base_off = base;
        if (d_philox_offset) *d_philox_offset = base + (uint64_t)((total_d + 3ull) >> 2);
    }
}

// One kept entry, t of row i, into slot p.  A column outside [0, N) raises GRAPES_STATUS_BAD_INDEX and is dropped: its slot holds -1 in
// every array, so the list's layout does not depend on the data.
__device__ __forceinline__ void sage_store(int p, long long t, const int32_t* __restrict__ col, int64_t a, int i, int N,
                                           int32_t* __restrict__ edge_src, int32_t* __restrict__ edge_dst,
                                           int64_t* __restrict__ edge_pos, int32_t* status) {
    const int c = col[a + t];
    const bool ok = (unsigned)c < (unsigned)N;
    if (!ok && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    edge_src[p] = ok ? c : -1;
    edge_dst[p] = ok ? i : -1;
    if (edge_pos) edge_pos[p] = ok ? (int64_t)(a + t) : (int64_t)-1;
}

// The kept lanes (one entry each), compacted behind `base` in lane order (= ascending t); nothing is written at or past e_cap.
__device__ __forceinline__ void sage_emit(bool kept, long long t, int lane, const int32_t* __restrict__ col, int64_t a, int i, int N,
                                          int& base, int e_cap, int32_t* __restrict__ edge_src, int32_t* __restrict__ edge_dst,
                                          int64_t* __restrict__ edge_pos, int32_t* status) {
    const int p = wave_compact_slot(kept, lane, base);
    if (kept && p < e_cap) sage_store(p, t, col, a, i, N, edge_src, edge_dst, edge_pos, status);
}

// A lane's share of one trip over a long row: the four stream positions 4 c .. 4 c + 3 of Philox counter c = c0 + rel (one Philox
// call), t0 + j = their positions in the row, in[j] = inside the row, kw[j] = their keys (0xffffffff outside the row).
struct SageTrip { uint32_t kw[4]; bool in[4]; long long t0; };
__device__ __forceinline__ void sage_trip(SageTrip& T, const uint32_t* __restrict__ keys, long long n_keys, uint64_t seed, uint64_t off,
                                          long long P, long long deg, long long c0, long long nctr, long long rel, int32_t* status) {
    const long long c = c0 + rel;
    T.t0 = 4 * c - P;
#pragma unroll
    for (int j = 0; j < 4; ++j) T.in[j] = rel < nctr && T.t0 + j >= 0 && T.t0 + j < deg;
    if (keys) {
#pragma unroll
        for (int j = 0; j < 4; ++j) T.kw[j] = T.in[j] ? sage_key(keys, n_keys, seed, off, 4 * c + j, status) : 0xffffffffu;
    } else {
        const Philox4 w = philox4x32_10(off + (uint64_t)c, seed);
#pragma unroll
        for (int j = 0; j < 4; ++j) T.kw[j] = T.in[j] ? w.v[j] : 0xffffffffu;
    }
}

__global__ __launch_bounds__(256) void sage_write_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                    const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                    int fanout, const uint32_t* __restrict__ keys, long long n_keys, uint64_t seed,
                                                    const long long* __restrict__ off_p, const uint64_t* __restrict__ base_off,
                                                    const int32_t* __restrict__ off_e, int e_cap, int32_t* __restrict__ edge_src,
                                                    int32_t* __restrict__ edge_dst, int64_t* __restrict__ edge_pos, int32_t* status) {
    __shared__ int hist[4][256];
    const int r = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (r >= m_host) return;                                                  // (whole wavefronts leave)
    const ListRow R = list_row(rowptr, N, rows, r, eff_count(d_m, m_host), nullptr);   // (a bad id: empty, the bit raised by sage_scan_k)
    const int i = R.i;
    const int64_t a = R.a;
    const long long deg = R.deg;
    int base = off_e[r];
    if (deg <= 0 || base >= e_cap) return;
    const long long P = off_p[r];
    const uint64_t off = *base_off;

    if (deg <= fanout) {                                                      // keeps everything: no key is looked at
        for (long long t0 = 0; t0 < deg && base < e_cap; t0 += 64)
            sage_emit(t0 + lane < deg, t0 + lane, lane, col, a, i, N, base, e_cap, edge_src, edge_dst, edge_pos, status);
        return;
    }
    if (deg <= 64) {                                                          // in registers: lane t holds key t
        const int d = (int)deg;
        const uint32_t key = lane < d ? sage_key(keys, n_keys, seed, off, P + lane, status) : 0xffffffffu;
        int rank = 0;                                                         // entries with a smaller composite (key, t)
        for (int s = 0; s < d; ++s) {
            const uint32_t ks = (uint32_t)__shfl((int)key, s, 64);
            rank += (ks < key || (ks == key && s < lane)) ? 1 : 0;
        }
        sage_emit(lane < d && rank < fanout, lane, lane, col, a, i, N, base, e_cap, edge_src, edge_dst, edge_pos, status);
        return;
    }
    // Longer rows.  A lane takes one Philox counter per trip — four consecutive stream positions, 256 per trip — so a generation of
    // the row's keys costs deg / 4 Philox calls.  Radix select: after pass q the top 8 (q + 1) bits of the threshold word are known
    // (prefix), `need` = how many entries are still to be taken among those whose word matches them, and the candidates — the
    // entries at or below the prefix on those bits — number (fanout - need) + the matching bin.  As soon as they fit SAGE_CAND slots
    // (after ONE pass unless deg is beyond ~ 256 (SAGE_CAND - fanout) or the words tie) a collect pass lists them in t order in the
    // histogram's LDS and the row ends in registers like a short one: two or three generations of the keys.  Words that tie beyond
    // that take all four passes and a fifth that writes word < T and the first `need` positions with word == T.
    int* h = hist[threadIdx.x >> 6];
    const long long c0 = P >> 2, nctr = ((P + deg + 3) >> 2) - c0;           // the counters that cover the row's positions
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t prefix = 0u;
    int need = fanout;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int b = lane; b < 256; b += 64) h[b] = 0;
        __builtin_amdgcn_wave_barrier();
        for (long long cb = 0; cb < nctr; cb += 64) {
            SageTrip T;
            sage_trip(T, keys, n_keys, seed, off, P, deg, c0, nctr, cb + lane, status);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (T.in[j] && ((uint64_t)T.kw[j] >> (shift + 8)) == ((uint64_t)prefix >> (shift + 8)))
                    atomicAdd(&h[(T.kw[j] >> shift) & 255u], 1);
        }
        __builtin_amdgcn_wave_barrier();
        const int b0 = h[4 * lane], b1 = h[4 * lane + 1], b2 = h[4 * lane + 2], b3 = h[4 * lane + 3];   // lane l: bins 4 l .. 4 l + 3
        const int s4 = b0 + b1 + b2 + b3;
        const int incl = wave_incl_scan(s4), excl = incl - s4;
        const bool here = excl < need && need <= incl;                        // exactly one lane: 1 <= need <= the matching entries
        int bin = 0, below = excl, cbin = b0;
        if (need > below + b0) { below += b0; bin = 1; cbin = b1;
            if (need > below + b1) { below += b1; bin = 2; cbin = b2;
                if (need > below + b2) { below += b2; bin = 3; cbin = b3; } } }
        bin += 4 * lane;
        const unsigned long long hb = __ballot(here);
        const int from = hb ? __ffsll((long long)hb) - 1 : 0;
        bin = __shfl(bin, from, 64);
        below = __shfl(below, from, 64);
        cbin = __shfl(cbin, from, 64);
        prefix |= (uint32_t)bin << shift;
        need -= below;
        __builtin_amdgcn_wave_barrier();
        const int C = (fanout - need) + cbin;                                 // the candidates: at or below the prefix on the known bits
        if (C > SAGE_CAND || deg >= (1ll << 31)) continue;
        uint32_t* ckey = reinterpret_cast<uint32_t*>(h);                      // (the histogram is read: its LDS holds the candidates)
        int* ct = h + SAGE_CAND;
        int cn = 0;
        for (long long cb = 0; cb < nctr; cb += 64) {
            SageTrip T;
            sage_trip(T, keys, n_keys, seed, off, P, deg, c0, nctr, cb + lane, status);
            bool cand[4];
            int before = 0, total = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cand[j] = T.in[j] && ((uint64_t)T.kw[j] >> shift) <= ((uint64_t)prefix >> shift);
                const unsigned long long bj = __ballot(cand[j]);
                before += __popcll(bj & lt); total += __popcll(bj);
            }
            int slot = cn + before;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cand[j]) {
                    if (slot < SAGE_CAND) { ckey[slot] = T.kw[j]; ct[slot] = (int)(T.t0 + j); }
                    ++slot;
                }
            cn += total;
        }
        __builtin_amdgcn_wave_barrier();
        if (cn > SAGE_CAND) cn = SAGE_CAND;                                   // (cn == C)
        // candidate q < cn sits in slot q, in t order: lane l ranks the candidates l and l + 64 by (word, slot)
        const int q0 = lane, q1 = lane + 64;
        const uint32_t k0 = q0 < cn ? ckey[q0] : 0xffffffffu, k1 = q1 < cn ? ckey[q1] : 0xffffffffu;
        const int t0 = q0 < cn ? ct[q0] : 0, t1 = q1 < cn ? ct[q1] : 0;
        int r0 = 0, r1 = 0;
        for (int q = 0; q < cn; ++q) {
            const uint32_t kq = ckey[q];                                      // (one address for the wavefront: a broadcast read)
            r0 += (kq < k0 || (kq == k0 && q < q0)) ? 1 : 0;
            r1 += (kq < k1 || (kq == k1 && q < q1)) ? 1 : 0;
        }
        sage_emit(q0 < cn && r0 < fanout, t0, lane, col, a, i, N, base, e_cap, edge_src, edge_dst, edge_pos, status);
        sage_emit(q1 < cn && r1 < fanout, t1, lane, col, a, i, N, base, e_cap, edge_src, edge_dst, edge_pos, status);
        return;
    }
    // prefix = the threshold word T; every word < T is kept (fanout - need of them) and the first `need` positions with word == T
    int eq_seen = 0;
    for (long long cb = 0; cb < nctr && base < e_cap; cb += 64) {
        SageTrip T;
        sage_trip(T, keys, n_keys, seed, off, P, deg, c0, nctr, cb + lane, status);
        bool eq[4], kept[4];
        int eq_before = 0, eq_total = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            eq[j] = T.in[j] && T.kw[j] == prefix;
            const unsigned long long bj = __ballot(eq[j]);
            eq_before += __popcll(bj & lt); eq_total += __popcll(bj);
        }
        int run = eq_seen + eq_before;                                        // the equal words at lower positions
        int before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kept[j] = T.in[j] && (T.kw[j] < prefix || (eq[j] && run < need));
            run += eq[j] ? 1 : 0;
            const unsigned long long bj = __ballot(kept[j]);
            before += __popcll(bj & lt); total += __popcll(bj);
        }
        int slot = base + before;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (kept[j]) {
                if (slot < e_cap) sage_store(slot, T.t0 + j, col, a, i, N, edge_src, edge_dst, edge_pos, status);
                ++slot;
            }
        base += total;
        eq_seen += eq_total;
    }
}

// off_p int64[m] | base_off uint64[1] (+ 8 bytes of padding) | off_e int32[m]
extern "C" size_t grapes_sage_sample_layer_workspace_bytes(int32_t m) {
    return (size_t)(m > 0 ? m : 1) * 12 + 16;
}

extern "C" int grapes_sage_sample_layer(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m,
                                        const int32_t* d_m, int32_t fanout, const uint32_t* keys, int64_t n_keys,
                                        uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, int32_t e_cap,
                                        int32_t* edge_src, int32_t* edge_dst, int64_t* edge_pos, int32_t* d_e, void* workspace,
                                        int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || m <= 0 || e_cap <= 0 || fanout < 1 || fanout > SAGE_MAX_FANOUT) return GRAPES_EINVAL;
    if (!rowptr || !col || !rows || !edge_src || !edge_dst || !d_e || !workspace || (keys && n_keys < 0)) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 7) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    long long* off_p = (long long*)workspace;
    uint64_t* base_off = (uint64_t*)(off_p + m);
    int32_t* off_e = (int32_t*)(base_off + 2);
    hipLaunchKernelGGL(sage_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, rowptr, num_nodes, rows, m, d_m, fanout, e_cap,
                       philox_offset, d_philox_offset, off_p, base_off, off_e, d_e, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(sage_write_k, dim3(grapes_div_up((int64_t)m * 64, 256)), dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m,
                       fanout, keys, (long long)n_keys, philox_seed, (const long long*)off_p, (const uint64_t*)base_off,
                       (const int32_t*)off_e, e_cap, edge_src, edge_dst, edge_pos, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
