// PPRGo [Bojchevski et al., KDD 2020]: logits_b = sum_t w[b][t] MLP(x)[nbr[b][t]] over a root's k best personalised-PageRank nodes.
// The push and the selection are grapes_pprgo_topk (shadow_kernels.hip, beside the ShaDow scope that shares them); this file holds
// what follows them.  The rules written in include/grapes_hip.h are the contract; tests/pprgo_oracle.py reproduces them.
//
// grapes_pprgo_batch: the slot tables nbr / cnt [m][K] -> the batch structure.
//   pprgo_mark_k      the live slots' ids into the caller's bitmap (integer atomics; a set, so the order changes nothing).  Its own
//                     kernel and not grapes_bitmap_mark_lists: that call marks whole lists, and here slots at or past cnt[b] are
//                     not read — a table whose dead slots were never written is a legal input.
//   grapes_frontier_compact(node_map =)   the project's union past 4096 ids: node_idx ascending, node_map[id] = rank, the bitmap
//                     back to zero.  Called from inside the entry point.
//   pprgo_loc_k       loc[s] = node_map[nbr[s]] per live slot and a histogram of the sources (integer atomics on a counter per local
//                     row); a dead slot repeats its root's rank (-1 in a row without a live slot)
//   pprgo_scan_k      ONE workgroup on list_scan_tiles: tptr, *d_n, *d_e, the overflow bit, and the longest segment (*d_seg_max:
//                     a caller that reads it with n and E knows whether the backward needs its chunked form at all)
//   pprgo_scatter_k   slot s behind its source's offset; the cursor is the histogram counted back down, so the counters end at zero
//                     (the order inside a segment is whatever the atomics gave: the next kernel fixes it)
//   pprgo_order_k     every segment ascending (seg_order.h): at most 64 entries in a wavefront's registers (a bitonic network on
//                     shuffles, 21 steps), longer ones — a hub is in up to m = 4096 lists — by the workgroup in LDS on the network
//                     shadow_stage runs; nothing ranks a segment against itself entry by entry.
// Integers only; two runs give the same bits.  Scratch of the caller: bits uint64[ceil(N / 64)], zero on entry and zero again on
// return; node_map int32[N], any state on entry (it holds the ranks of this batch's ids afterwards).
//
// grapes_pprgo_aggregate_fwd / _bwd: the weighted gathers, on the row-gather scaffold.
//   forward   out[b] = sum_{t < cnt[b]} w[b][t] z[loc[b][t]]: a group of lanes owns a root, a lane reads one (loc, w) pair per batch
//             of entries, gather_batch fetches the rows, HistUnroll of them in flight (as vrgcn_kernels.hip).
//   backward  dz[u] = sum_{s in tslot[tptr[u] .. tptr[u + 1])} w[s] g[s / K], ascending s: the same walk over the inverted index.
//   A row of more than HIST_LONG_ROW entries is cut into chunks of that many: the rows kernel takes chunk 0, one group per further
//   chunk writes a partial row, and hist_combine_k (hist_rows.h) adds the partials in chunk order.  The forward's rows all hold K
//   slots, so its item list is arithmetic (item = b (nc - 1) + c - 1) and needs no preparation; the backward's segments differ, so
//   pprgo_items_k scans them first (one workgroup, list_scan_tiles).
//   Slots at or past cnt[b] are never read, neither w nor loc; a lane past the end of a batch points at the batch's first row with
//   weight 0 (gather_batch), which is a row the batch names.  No float atomics: every sum has a fixed order.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): pprgo_order_k 16 644 B LDS, 30 VGPRs, occupancy 8 waves per SIMD;
// pprgo_scan_k / pprgo_items_k 32 VGPRs, 144 / 136 B; the gather kernels use no LDS: 52 - 54 VGPRs (occupancy 8) for scalar columns
// up to 64 wide, 100 - 118 (occupancy 4) for the float4 and four-slab forms, whose HistUnroll rows in flight fill the registers.
// Measured (profiles/pprgo_bench.json, a kernel trace at k = 200 over 512 roots, about 97 k rows): the one-workgroup scans are the
// long poles — pprgo_scan_k 66.4 us of grapes_pprgo_batch's 121 us, and pprgo_items_k took 63.3 us in front of a 39 us backward —
// which is why the batch also reports its longest segment: a caller that reads it passes item_cap = 0 and the backward is its rows
// kernel alone.
#include "hist_rows.h"
#include "row_list.h"
#include "seg_order.h"

#define PPRGO_MAX_ROOTS 4096
#define PPRGO_MAX_K 1024                 // K = k + 1 slots
#define PPRGO_ITEM_CAP_MAX (1 << 22)

__device__ __forceinline__ int pprgo_live(const int32_t* __restrict__ cnt, int b, int K) {
    const int c = cnt[b];
    return c < 0 ? 0 : (c > K ? K : c);
}

__global__ __launch_bounds__(256) void pprgo_mark_k(const int32_t* __restrict__ nbr, const int32_t* __restrict__ cnt, int m, int K, int N,
                                                    unsigned long long* __restrict__ bits, int32_t* status) {
    const int total = m * K;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < total; s += gridDim.x * 256) {
        const int b = s / K, t = s - b * K;
        if (t >= pprgo_live(cnt, b, K)) continue;
        const int id = nbr[s];
        if ((unsigned)id < (unsigned)N) atomicOr(&bits[id >> 6], 1ull << (id & 63));
        else if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    }
}

// the rank of id among the n batch nodes, or -1 (an id outside [0, N), or one the compaction dropped past n_cap)
__device__ __forceinline__ int pprgo_rank(const int32_t* __restrict__ node_map, const int32_t* __restrict__ node_idx, int n, int N, int id) {
    if ((unsigned)id >= (unsigned)N) return -1;
    const int u = node_map[id];
    return ((unsigned)u < (unsigned)n && node_idx[u] == id) ? u : -1;
}

__global__ __launch_bounds__(256) void pprgo_loc_k(const int32_t* __restrict__ nbr, const int32_t* __restrict__ cnt, int m, int K, int N,
                                                   const int32_t* __restrict__ node_map, const int32_t* __restrict__ node_idx,
                                                   const int32_t* __restrict__ counts, int n_cap, int32_t* __restrict__ loc,
                                                   int32_t* __restrict__ cur) {
    const int total = m * K;
    const int n = counts[0] < n_cap ? counts[0] : n_cap;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < total; s += gridDim.x * 256) {
        const int b = s / K, t = s - b * K, c = pprgo_live(cnt, b, K);
        if (t < c) {
            const int u = pprgo_rank(node_map, node_idx, n, N, nbr[s]);
            loc[s] = u;
            if (u >= 0) atomicAdd(&cur[u], 1);
        } else {
            loc[s] = c > 0 ? pprgo_rank(node_map, node_idx, n, N, nbr[b * K]) : -1;
        }
    }
}

__global__ __launch_bounds__(LIST_SCAN_THREADS) void pprgo_scan_k(const int32_t* __restrict__ cur, const int32_t* __restrict__ counts,
                                                                  int n_cap, int e_cap, int32_t* __restrict__ tptr,
                                                                  int32_t* __restrict__ d_n, int32_t* __restrict__ d_e,
                                                                  int32_t* __restrict__ d_seg_max, int32_t* status) {
    __shared__ unsigned long long lds[17];
    __shared__ int seg_max;
    const int n = counts[0] < n_cap ? counts[0] : n_cap;
    if (threadIdx.x == 0) seg_max = 0;
    __syncthreads();
    int mine = 0;
    const unsigned long long total = list_scan_tiles<int, int32_t>(
        [&](int i0, int (&v)[LIST_SCAN_PER]) {
#pragma unroll
            for (int q = 0; q < LIST_SCAN_PER; ++q) {
                v[q] = i0 + q < n ? cur[i0 + q] : 0;
                mine = v[q] > mine ? v[q] : mine;
            }
        },
        n, (unsigned long long)e_cap, tptr, lds);
    list_scan_finish(total, e_cap, tptr + n, d_e, status);
    if (d_seg_max) {                                                            // (an integer maximum: the order changes nothing)
        if (mine > 0) atomicMax(&seg_max, mine);
        __syncthreads();
        if (threadIdx.x == 0) *d_seg_max = seg_max;
    }
    if (threadIdx.x == 0) *d_n = n;
}

__global__ __launch_bounds__(256) void pprgo_scatter_k(const int32_t* __restrict__ cnt, int m, int K, const int32_t* __restrict__ loc,
                                                       const int32_t* __restrict__ tptr, int e_cap, int32_t* __restrict__ cur,
                                                       int32_t* __restrict__ tslot) {
    const int total = m * K;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < total; s += gridDim.x * 256) {
        const int b = s / K, t = s - b * K;
        if (t >= pprgo_live(cnt, b, K)) continue;
        const int u = loc[s];
        if (u < 0) continue;
        const long long p = (long long)tptr[u] + (atomicSub(&cur[u], 1) - 1);
        if (p < e_cap) tslot[p] = s;
    }
}

// (seg_order.h: the pass itself, shared with bag_kernels.hip)
__global__ __launch_bounds__(SEG_ORDER_THREADS) void pprgo_order_k(const int32_t* __restrict__ tptr, const int32_t* __restrict__ d_n,
                                                                   int n_cap, int e_cap, int32_t* __restrict__ tslot, int32_t* status) {
    seg_order(tptr, d_n, n_cap, e_cap, tslot, status);
}

// cur int32[n_cap] | two int32[n_cap] lists the compaction wants | counts int32[4] | the compaction's workspace
extern "C" size_t grapes_pprgo_batch_workspace_bytes(int32_t n_cap, int32_t num_nodes) {
    if (n_cap < 1 || num_nodes < 1) return 0;
    return ((size_t)3 * n_cap + 4) * sizeof(int32_t) + grapes_frontier_compact_workspace_bytes(n_cap, num_nodes) + 16;
}

extern "C" int grapes_pprgo_batch(const int32_t* nbr, const int32_t* cnt, int32_t m, int32_t K, int32_t num_nodes, uint64_t* bits,
                                  int32_t* node_map, int32_t n_cap, int32_t e_cap, int32_t* node_idx, int32_t* loc, int32_t* tptr,
                                  int32_t* tslot, int32_t* d_n, int32_t* d_e, int32_t* d_seg_max, void* workspace, int32_t* status,
                                  grapes_stream_t stream) {
    if (m < 1 || m > PPRGO_MAX_ROOTS || K < 2 || K > PPRGO_MAX_K || num_nodes < 1 || n_cap < 1 || e_cap < 1) return GRAPES_EINVAL;
    if (!nbr || !cnt || !bits || !node_map || !node_idx || !loc || !tptr || !tslot || !d_n || !d_e || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* cur = (int32_t*)workspace;
    int32_t* nn = cur + n_cap;
    int32_t* nl = nn + n_cap;
    int32_t* counts = nl + n_cap;
    void* cws = counts + 4;
    const int total = m * K;
    int grid = grapes_div_up(total, 256);
    if (grid > 4096) grid = 4096;
    if (grapes_zero_async(cur, (size_t)n_cap * sizeof(int32_t), s) != hipSuccess) return GRAPES_EINVAL;
    hipLaunchKernelGGL(pprgo_mark_k, dim3(grid), dim3(256), 0, s, nbr, cnt, m, K, num_nodes, (unsigned long long*)bits, status);
    GRAPES_LAUNCH_CHECK();
    const int rc = grapes_frontier_compact(bits, nullptr, nullptr, num_nodes, n_cap, node_idx, nn, nl, node_map, counts, nullptr, 0u,
                                           nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, cws, nullptr, status, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(pprgo_loc_k, dim3(grid), dim3(256), 0, s, nbr, cnt, m, K, num_nodes, (const int32_t*)node_map,
                       (const int32_t*)node_idx, (const int32_t*)counts, n_cap, loc, cur);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(pprgo_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, (const int32_t*)cur, (const int32_t*)counts, n_cap, e_cap,
                       tptr, d_n, d_e, d_seg_max, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(pprgo_scatter_k, dim3(grid), dim3(256), 0, s, cnt, m, K, (const int32_t*)loc, (const int32_t*)tptr, e_cap, cur,
                       tslot);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(pprgo_order_k, dim3(seg_order_grid(n_cap)), dim3(SEG_ORDER_THREADS), 0, s, (const int32_t*)tptr, (const int32_t*)d_n, n_cap, e_cap,
                       tslot, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the aggregation
// what hist_combine_k asks of its arguments, answered without tables: a row's first item (arithmetic in the forward), the row's own
// id and a unit scale
struct PprgoItemOff {
    const int32_t* p; int stride;
    __device__ __forceinline__ int operator[](int r) const { return p ? p[r] : r * stride; }
};
struct PprgoSelf { __device__ __forceinline__ int operator[](int r) const { return r; } };
struct PprgoOne { __device__ __forceinline__ float operator[](int) const { return 1.f; } };

struct PprgoArgs {
    const float* x; int x_rows;          // the gathered matrix: z [n, F] (forward), g [m, F] (backward)
    const float* w;                      // [m][K]
    const int32_t* idx;                  // loc [m][K] (forward), tslot [E] (backward)
    const int32_t* cnt;                  // forward: the live slots of a root
    const int32_t* tptr; int E;          // backward: the segments
    int K, slots;                        // slots = m K
    float* out; long long ld_out;
    PprgoItemOff item_off; PprgoSelf rows_g; PprgoOne dinv;
    int m, N;                            // (hist_combine_k's names) the rows of out
    float* pacc;
    int F;
    int32_t* status;
};

// the entries [beg, end) of row r (flat positions in idx) — false: the row's bounds are not a run inside the table
template <bool BWD>
__device__ __forceinline__ bool pprgo_row(const PprgoArgs& a, int r, int& beg, int& end) {
    if (BWD) {
        beg = a.tptr[r]; end = a.tptr[r + 1];
        if (beg < 0 || end < beg || end > a.E) { beg = end = 0; return false; }
    } else {
        beg = r * a.K; end = beg + pprgo_live(a.cnt, r, a.K);
    }
    return true;
}

// acc += sum_{t in [beg, end)} w x[row]: forward (row, weight) = (loc[t], w[t]); backward s = tslot[t], (s / K, w[s])
template <int VEC, int LPR, int NS, bool BWD>
__device__ __forceinline__ void pprgo_walk(const PprgoArgs& a, int beg, int end, int l, float (&acc)[NS][VEC]) {
    for (int b = beg; b < end; b += LPR) {
        int idx = -1;
        float wv = 0.f;
        if (b + l < end) {
            const int c = a.idx[b + l];
            if (BWD) {
                if ((unsigned)c < (unsigned)a.slots) { idx = c / a.K; wv = a.w[c]; }
            } else {
                if ((unsigned)c < (unsigned)a.x_rows) { idx = c; wv = a.w[b + l]; }
            }
            if (idx < 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
        }
        const int first = __shfl(idx, 0, LPR);                  // (a lane past the end or dropped points at the batch's first row, or row 0)
        if (idx < 0) idx = first < 0 ? 0 : first;
        const int cnt = end - b < LPR ? end - b : LPR;
        gather_batch<HistUnroll<VEC, NS>::U, VEC, LPR, NS>(
            wv, cnt, [&](int j, float (&hv)[NS][VEC]) { row_load<VEC, LPR, NS>(a.x, __shfl(idx, j, LPR), a.F, l, hv); }, acc);
    }
}

// chunked: a row of more than HIST_LONG_ROW entries (the forward: slots, K of them in every row) stops behind its first chunk
template <int VEC, int LPR, int NS, bool BWD>
__device__ __forceinline__ void pprgo_rows(const PprgoArgs& a, int chunked) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int r = blockIdx.x * G + threadIdx.x / LPR; r < a.m; r += gridDim.x * G) {
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        int beg, end;
        if (!pprgo_row<BWD>(a, r, beg, end) && l == 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
        const bool is_long = BWD ? end - beg > HIST_LONG_ROW : a.K > HIST_LONG_ROW;
        if (chunked && is_long && end - beg > HIST_LONG_ROW) end = beg + HIST_LONG_ROW;
        pprgo_walk<VEC, LPR, NS, BWD>(a, beg, end, l, acc);
        row_store_ld<VEC, LPR, NS>(a.out, r, a.ld_out, a.F, l, acc);
    }
}

template <int VEC, int LPR, int NS, bool BWD>
__device__ __forceinline__ void pprgo_chunks(const PprgoArgs& a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    const int n_items = a.item_off[a.m];
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int r, c;
        if (BWD) {
            r = lower_bound<int32_t, int, int>(a.item_off.p, a.m, it + 1) - 1;      // the last row with item_off[r] <= it
            c = it - a.item_off.p[r] + 1;
        } else {
            r = it / a.item_off.stride;
            c = it - r * a.item_off.stride + 1;
        }
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        int beg, end;
        if (pprgo_row<BWD>(a, r, beg, end)) {
            const long long cb = (long long)beg + (long long)c * HIST_LONG_ROW;
            if (cb < end) {
                const int ce = (int)cb + HIST_LONG_ROW < end ? (int)cb + HIST_LONG_ROW : end;
                pprgo_walk<VEC, LPR, NS, BWD>(a, (int)cb, ce, l, acc);
            }
        }
        row_store<VEC, LPR, NS>(a.pacc, it, a.F, l, acc);
    }
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void pprgo_fwd_rows_k(PprgoArgs a, int chunked) { pprgo_rows<VEC, LPR, NS, false>(a, chunked); }
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void pprgo_fwd_chunks_k(PprgoArgs a) { pprgo_chunks<VEC, LPR, NS, false>(a); }
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void pprgo_bwd_rows_k(PprgoArgs a, int chunked) { pprgo_rows<VEC, LPR, NS, true>(a, chunked); }
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void pprgo_bwd_chunks_k(PprgoArgs a) { pprgo_chunks<VEC, LPR, NS, true>(a); }

// ONE workgroup.  item_off[u] = min(the chunks behind the first of the long segments before u, item_cap), item_off[n] the live items;
// more than item_cap raise GRAPES_STATUS_EDGE_OVERFLOW.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void pprgo_items_k(const int32_t* __restrict__ tptr, int n, int E, int item_cap,
                                                                   int32_t* __restrict__ item_off, int32_t* status) {
    __shared__ unsigned long long lds[17];
    const unsigned long long total = list_scan_tiles<int, int32_t>(
        [&](int i0, int (&v)[LIST_SCAN_PER]) {
#pragma unroll
            for (int q = 0; q < LIST_SCAN_PER; ++q) {
                v[q] = 0;
                if (i0 + q < n) {
                    const int beg = tptr[i0 + q], end = tptr[i0 + q + 1];
                    const int len = (beg < 0 || end < beg || end > E) ? 0 : end - beg;
                    v[q] = len > HIST_LONG_ROW ? (len + HIST_LONG_ROW - 1) / HIST_LONG_ROW - 1 : 0;
                }
            }
        },
        n, (unsigned long long)item_cap, item_off, lds);
    list_scan_finish(total, item_cap, item_off + n, nullptr, status);
}

// the items the forward cuts its m rows of K slots into beyond each row's first chunk (0: K is no long row)
static inline long long pprgo_fwd_items(int m, int K) {
    return K > HIST_LONG_ROW ? (long long)m * ((K + HIST_LONG_ROW - 1) / HIST_LONG_ROW - 1) : 0;
}

extern "C" size_t grapes_pprgo_aggregate_fwd_workspace_bytes(int32_t m, int32_t K, int32_t f) {
    if (m < 1 || m > PPRGO_MAX_ROOTS || K < 2 || K > PPRGO_MAX_K || f < 1) return 0;
    return hist_workspace_bytes(0, (int32_t)pprgo_fwd_items(m, K), f);
}
extern "C" size_t grapes_pprgo_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f) {
    if (n < 1 || item_cap < 0 || item_cap > PPRGO_ITEM_CAP_MAX || f < 1) return 0;
    return hist_workspace_bytes(n, item_cap, f);
}

extern "C" int grapes_pprgo_aggregate_fwd(const float* z, int32_t n, const float* w, const int32_t* loc, const int32_t* cnt, int32_t m,
                                          int32_t K, int32_t f, float* out, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!z || !w || !loc || !cnt || !out || out == z) return GRAPES_EINVAL;
    if (n < 1 || m < 1 || m > PPRGO_MAX_ROOTS || K < 2 || K > PPRGO_MAX_K || f < 1) return GRAPES_EINVAL;
    const int items = (int)pprgo_fwd_items(m, K);
    if (items > 0 && !workspace) return GRAPES_EINVAL;
    if (items > 0 && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(f, grapes_aligned16(z) && grapes_aligned16(out));
    if (shape < 0) return shape;
    hipStream_t s = (hipStream_t)stream;
    PprgoArgs a{};
    a.x = z; a.x_rows = n; a.w = w; a.idx = loc; a.cnt = cnt; a.K = K; a.slots = m * K; a.out = out; a.ld_out = f;
    a.item_off = PprgoItemOff{nullptr, items > 0 ? items / m : 0}; a.m = m; a.N = m; a.pacc = (float*)workspace; a.F = f; a.status = status;
    const bool vec = shape == 0;
    ROW_LAUNCH(pprgo_fwd_rows_k, 4, vec, f, m, s, a, items > 0 ? 1 : 0);
    if (items > 0) {
        ROW_LAUNCH(pprgo_fwd_chunks_k, 4, vec, f, items, s, a);
        ROW_LAUNCH(hist_combine_k, 4, vec, f, m, s, a);
    }
    return 0;
}

extern "C" int grapes_pprgo_aggregate_bwd(const float* g, int32_t m, const float* w, int32_t K, const int32_t* tptr, const int32_t* tslot,
                                          int32_t n, int32_t e, int32_t f, float* dz, int32_t item_cap, void* workspace,
                                          int32_t* status, grapes_stream_t stream) {
    if (!g || !w || !tptr || !tslot || !dz || dz == g) return GRAPES_EINVAL;
    if (n < 1 || e < 0 || m < 1 || m > PPRGO_MAX_ROOTS || K < 2 || K > PPRGO_MAX_K || f < 1) return GRAPES_EINVAL;
    if (item_cap < 0 || item_cap > PPRGO_ITEM_CAP_MAX || (item_cap > 0 && !workspace)) return GRAPES_EINVAL;
    if (item_cap > 0 && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(f, grapes_aligned16(g) && grapes_aligned16(dz));
    if (shape < 0) return shape;
    hipStream_t s = (hipStream_t)stream;
    PprgoArgs a{};
    a.x = g; a.x_rows = m; a.w = w; a.idx = tslot; a.tptr = tptr; a.E = e; a.K = K; a.slots = m * K; a.out = dz; a.ld_out = f;
    a.m = n; a.N = n; a.F = f; a.status = status;
    if (item_cap > 0) {
        a.item_off = PprgoItemOff{(const int32_t*)workspace, 0};
        a.pacc = (float*)((char*)workspace + grapes_round16(((size_t)n + 1) * sizeof(int32_t)));
        hipLaunchKernelGGL(pprgo_items_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, tptr, n, e, item_cap, (int32_t*)workspace, status);
        GRAPES_LAUNCH_CHECK();
    }
    const bool vec = shape == 0;
    ROW_LAUNCH(pprgo_bwd_rows_k, 4, vec, f, n, s, a, item_cap > 0 ? 1 : 0);
    if (item_cap > 0) {
        ROW_LAUNCH(pprgo_bwd_chunks_k, 4, vec, f, item_cap, s, a);
        ROW_LAUNCH(hist_combine_k, 4, vec, f, n, s, a);
    }
    return 0;
}
