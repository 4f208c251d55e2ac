// LINKX [Lim et al., NeurIPS 2021; PyG-recall: LINKX, SparseLinear]: a node's row of the adjacency matrix is a feature vector of length
// N pushed through a learned table W [N, H],   h_A[i] = b + sum_{t in row(i)} W[col[t]].   Nothing is sampled: a batch is m rows of A
// with their global column ids.  The rules written in include/grapes_hip.h are the contract; tests/linkx_oracle.py reproduces them.
//
// grapes_bag_batch: the rows' ids -> the batch tables (integers only; two runs give the same bits).
//   bag_scan_k        ONE workgroup on list_scan_tiles (one tile: the rows' degrees are loaded once and scanned twice):
//                     bptr (the TRUE total in bptr[m], whatever e_cap), the rows' 64-entry work
//                     items and their prefix, the longest row, the overflow and bad-index bits
//   bag_mark_k        a wavefront per item = 64 consecutive entries of one row, one per lane (a hub row is cut over many wavefronts,
//                     as gas_codes_k does): the column ids into the caller's bitmap (integer atomics; a set, so the order changes
//                     nothing); the lanes that set a bit first are counted, which is the TRUE number of distinct columns
//   grapes_frontier_compact(node_map =)   the ascending union: uniq, node_map[id] = rank, the bitmap back to zero
//   bag_count_k       per entry the rank of its column and a histogram of the columns (integer atomics on a counter per column)
//   bag_tscan_k       ONE workgroup: tptr, the longest segment, the three counts
//   bag_scatter_k     the entry's batch row b behind its column's offset; the cursor is the histogram counted back down
//   bag_order_k       every segment ascending in b (seg_order.h, shared with pprgo_kernels.hip)
//   bag_clear_k       node_map[uniq[s]] = 0: a map that was zero on entry is zero on return
//
// grapes_bag_fwd: out[b] = bias + sum_t W[col[t]] over the stored entries of row rows[b], on the row-gather scaffold: a group of
//   lanes owns a batch row and keeps ONE accumulator in registers, which starts at bias; a lane reads one column id per batch of
//   entries, gather_batch fetches the rows, HistUnroll of them in flight (as vrgcn_kernels.hip).  A row of more than HIST_LONG_ROW
//   entries is cut into chunks of that many: the rows kernel takes chunk 0, one group per further chunk writes a partial row, and
//   hist_combine_k (hist_rows.h) adds the partials in chunk order.  bag_fwd_items_k scans the chunk counts (one workgroup).
//
// grapes_bag_bwd / grapes_bag_bwd_adam: a group of lanes owns a touched column s, g_s = sum_{q in segment s} G[trow[q]] in segment
//   order.  The sum is COMPENSATED (Kahan: the accumulator and the rounding error of its last addition, both in registers — per entry
//   y = x - c, t = s + y, c = (t - s) - y, s = t), because the update that follows is judged by the fp32 baseline of
//   tests/test_linkx_gpu.py: the plain fixed-order sum of a 300-entry segment is a few ulps of its partial sums off, which at H = 1
//   is the whole tensor's error — measured 4.6 times (exp_avg) and 12.7 times (exp_avg_sq) the error of torch's SparseAdam on the
//   CPU, whose sum there is correctly rounded; compensated, the sum is within an ulp of the exact one.  Its cost, measured as the fused
//   call of
//   profiles/bench_linkx.py in two builds and two runs (not alternated in one process): 13.3 -> 13.8 us and 26.4 -> 28.1 us at
//   H = 64, 28.5 -> 30.0 us and 56.1 -> 58.8 us at H = 256 (without / with the hub), 4 - 6 %; the widest form drops from occupancy
//   4 to 3.  It is also a second copy of gather_batch's loop shape, kept in this file: no other gather wants it.  A segment of more than
//   HIST_LONG_ROW entries
//   is skipped by the rows kernel: one group per 64-entry chunk writes its compensated partial sum, and the combine kernel adds the
//   partials in chunk order, compensated again.  What
//   happens to g_s is the epilogue, in the rows kernel for a short segment and in the combine kernel for a long one, so exactly
//   once per column: the plain backward stores it as row s of the row-sparse gradient's values; the fused form applies
//   torch.optim.SparseAdam's rule to row uniq[s] of W, exp_avg and exp_avg_sq — each of the three rows read once and written once,
//   no gradient written at all.  This file is compiled without floating-point contraction, so every operation of the rule is rounded
//   once and the compensation is not folded away (the forward's fmaf(1, x, acc) is an exact addition either way).
// No float atomics: every sum has a fixed order.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950; no kernel spills or uses scratch): bag_order_k 16 644 B LDS, 30 VGPRs,
// occupancy 8 waves per SIMD; the one-workgroup scans 32 - 39 VGPRs, 136 - 144 B; bag_mark_k / bag_place_k / bag_clear_k 5 - 14 VGPRs.
// The gathers use no LDS.  Forward: scalar columns up to 64 wide 51 - 59 VGPRs (occupancy 8), the float4 and four-slab forms, whose
// HistUnroll rows in flight fill the registers, 97 - 122 (occupancy 4).  Backward, with the error term beside the accumulator: 53 - 59
// (occupancy 8) for scalar columns up to 64 wide, 114 - 120 (occupancy 4) for <4,32,1>, <4,64,1> and <1,64,4> — bag_adam_rows_k 120,
// four above bag_bwd_rows_k: the three table rows are loaded after the walk, when its registers are free — and 129 - 132
// (occupancy 3) for <4,64,4>, the widths 516 - 1024.  The combine kernels 34 - 42 VGPRs scalar (occupancy 8), 86 - 111 otherwise
// (occupancy 4 - 5).
#include "hist_rows.h"
#include "row_list.h"
#include "seg_order.h"

#define BAG_MAX_ROWS 4096
#define BAG_CHUNK GRAPES_LONG_ROW
#define BAG_ITEM_CAP_MAX (1 << 22)
#define BAG_HDR 4                        // hdr[0] = the 64-entry work items, hdr[1] = the distinct columns, hdr[2] = the longest row
static_assert(BAG_CHUNK == 64, "a work item of the batch kernels is one entry per lane");
static_assert(BAG_MAX_ROWS <= LIST_SCAN_THREADS * LIST_SCAN_PER, "bag_scan_k keeps a thread's degrees of the ONE scan tile in registers");

// ------------------------------------------------------------------------------------------------------------ the batch

__global__ __launch_bounds__(LIST_SCAN_THREADS) void bag_scan_k(const int64_t* __restrict__ rowptr, int N, const int32_t* __restrict__ rows,
                                                                int m, int e_cap, int32_t* __restrict__ bptr,
                                                                int32_t* __restrict__ item_off, int32_t* __restrict__ hdr,
                                                                int32_t* status) {
    __shared__ unsigned long long lds[17];
    __shared__ int row_max;
    if (threadIdx.x == 0) row_max = 0;
    __syncthreads();
    bool bad = false;
    long long mine = 0, deg[LIST_SCAN_PER];                                    // m <= 4096: one tile, so a thread's degrees are read once
    auto degs = [&](int i0, long long (&v)[LIST_SCAN_PER]) {
        list_row_degrees(rowptr, N, rows, i0, m, v, bad);
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) {
            deg[q] = v[q];
            mine = v[q] > mine ? v[q] : mine;
        }
    };
    const unsigned long long total = list_scan_tiles<long long>(degs, m, 0x7fffffffull, bptr, lds);
    __syncthreads();                                                           // (lds is reused by the second scan)
    auto items = [&](int, long long (&v)[LIST_SCAN_PER]) {                     // (the same tile: the degrees kept above)
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) v[q] = (deg[q] + BAG_CHUNK - 1) / BAG_CHUNK;
    };
    const unsigned long long n_items = list_scan_tiles<long long>(items, m, 0x7fffffffull, item_off, lds);
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    if (mine > 0) atomicMax(&row_max, (int)(mine < 0x7fffffffll ? mine : 0x7fffffffll));
    __syncthreads();
    if (threadIdx.x == 0) {
        const int it = (int)(n_items < 0x7fffffffull ? n_items : 0x7fffffffull);
        item_off[m] = it;
        hdr[0] = it; hdr[1] = 0; hdr[2] = row_max; hdr[3] = 0;
        bptr[m] = (int)(total < 0x7fffffffull ? total : 0x7fffffffull);
        if (total > (unsigned long long)e_cap && status) atomicOr(status, GRAPES_STATUS_EDGE_OVERFLOW);
    }
}

// Lane `lane` of the wavefront that owns item `it`: the batch row b, its entry's position p behind bptr[b] and the column id;
// false for a lane past the row's end.
__device__ __forceinline__ bool bag_entry(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                          const int32_t* __restrict__ rows, int m, const int32_t* __restrict__ bptr,
                                          const int32_t* __restrict__ item_off, int it, int lane, int& b, long long& p, int& v) {
    b = lower_bound<int32_t, int, int>(item_off, m, it + 1) - 1;               // rows without an entry own no item and are stepped over
    const int r = rows[b];
    if ((unsigned)r >= (unsigned)N) return false;                              // (an empty row: bag_scan_k raised the bit)
    const int64_t a = rowptr[r];
    const long long t = (long long)(it - item_off[b]) * BAG_CHUNK + lane;
    if (t >= (long long)(rowptr[r + 1] - a)) return false;
    v = col[a + t];
    p = (long long)bptr[b] + t;
    return true;
}

#define BAG_ITEM_LOOP(it, hdr) \
    for (int it = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), n_it_ = (hdr)[0]; it < n_it_; it += (int)(gridDim.x * 4))

__global__ __launch_bounds__(256) void bag_mark_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                  const int32_t* __restrict__ rows, int m, const int32_t* __restrict__ bptr,
                                                  const int32_t* __restrict__ item_off, int32_t* __restrict__ hdr,
                                                  unsigned long long* __restrict__ bits, int32_t* status) {
    const int lane = threadIdx.x & 63;
    BAG_ITEM_LOOP(it, hdr) {
        int b, v = 0; long long p;
        const bool in_row = bag_entry(rowptr, col, N, rows, m, bptr, item_off, it, lane, b, p, v);
        const bool ok = in_row && (unsigned)v < (unsigned)N;
        if (in_row && !ok && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        bool fresh = false;
        if (ok) {
            const unsigned long long bit = 1ull << (v & 63);
            fresh = (atomicOr(&bits[v >> 6], bit) & bit) == 0ull;
        }
        const unsigned long long fb = __ballot(fresh);
        if (lane == 0 && fb) atomicAdd(&hdr[1], __popcll(fb));
    }
}

// the rank of id among the n kept columns, or -1 (an id outside [0, N), or one the compaction dropped past u_cap)
__device__ __forceinline__ int bag_rank(const int32_t* __restrict__ node_map, const int32_t* __restrict__ uniq, int n, int N, int id) {
    if ((unsigned)id >= (unsigned)N) return -1;
    const int u = node_map[id];
    return ((unsigned)u < (unsigned)n && uniq[u] == id) ? u : -1;
}

template <bool SCATTER>
__global__ __launch_bounds__(256) void bag_place_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                   const int32_t* __restrict__ rows, int m, const int32_t* __restrict__ bptr,
                                                   const int32_t* __restrict__ item_off, const int32_t* __restrict__ hdr,
                                                   const int32_t* __restrict__ node_map, const int32_t* __restrict__ uniq,
                                                   const int32_t* __restrict__ counts, int u_cap, const int32_t* __restrict__ tptr,
                                                   int e_cap, int32_t* __restrict__ cur, int32_t* __restrict__ trow) {
    const int lane = threadIdx.x & 63;
    const int n = counts[0] < u_cap ? counts[0] : u_cap;
    BAG_ITEM_LOOP(it, hdr) {
        int b, v = 0; long long p;
        if (!bag_entry(rowptr, col, N, rows, m, bptr, item_off, it, lane, b, p, v)) continue;
        const int u = bag_rank(node_map, uniq, n, N, v);
        if (u < 0) continue;
        if (SCATTER) {
            const long long q = (long long)tptr[u] + (atomicSub(&cur[u], 1) - 1);
            if (q < e_cap) trow[q] = b;
        } else {
            atomicAdd(&cur[u], 1);
        }
    }
}

__global__ __launch_bounds__(LIST_SCAN_THREADS) void bag_tscan_k(const int32_t* __restrict__ cur, const int32_t* __restrict__ counts,
                                                                 int u_cap, int e_cap, const int32_t* __restrict__ hdr,
                                                                 const int32_t* __restrict__ bptr_m, int32_t* __restrict__ tptr,
                                                                 int32_t* __restrict__ d_counts, int32_t* status) {
    __shared__ unsigned long long lds[17];
    __shared__ int seg_max;
    const int n = counts[0] < u_cap ? counts[0] : u_cap;
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
    list_scan_finish(total, e_cap, tptr + n, nullptr, status);
    if (mine > 0) atomicMax(&seg_max, mine);                                    // (an integer maximum: the order changes nothing)
    __syncthreads();
    if (threadIdx.x == 0) {
        d_counts[0] = hdr[1]; d_counts[1] = *bptr_m; d_counts[2] = seg_max; d_counts[3] = hdr[2];
    }
}

__global__ __launch_bounds__(SEG_ORDER_THREADS) void bag_order_k(const int32_t* __restrict__ tptr, const int32_t* __restrict__ counts,
                                                                 int u_cap, int e_cap, int32_t* __restrict__ trow, int32_t* status) {
    seg_order(tptr, counts, u_cap, e_cap, trow, status);
}

__global__ __launch_bounds__(256) void bag_clear_k(const int32_t* __restrict__ uniq, const int32_t* __restrict__ counts, int u_cap, int N,
                                                   int32_t* __restrict__ node_map) {
    const int n = counts[0] < u_cap ? counts[0] : u_cap;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < n; s += gridDim.x * 256) {
        const int id = uniq[s];
        if ((unsigned)id < (unsigned)N) node_map[id] = 0;
    }
}

// hdr int32[BAG_HDR] | item_off int32[m + 1] | cur int32[u_cap] | two int32[u_cap] lists the compaction wants | counts int32[4] |
// the compaction's workspace
extern "C" size_t grapes_bag_batch_workspace_bytes(int32_t m, int32_t u_cap, int32_t num_nodes) {
    if (m < 1 || u_cap < 1 || num_nodes < 1) return 0;
    return ((size_t)BAG_HDR + (size_t)m + 1 + (size_t)3 * u_cap + 4) * sizeof(int32_t) +
           grapes_frontier_compact_workspace_bytes(u_cap, num_nodes) + 16;
}

extern "C" int grapes_bag_batch(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m,
                                uint64_t* bits, int32_t* node_map, int32_t u_cap, int32_t e_cap, int32_t* bptr, int32_t* uniq,
                                int32_t* tptr, int32_t* trow, int32_t* d_counts, void* workspace, int32_t* status,
                                grapes_stream_t stream) {
    if (m < 1 || m > BAG_MAX_ROWS || num_nodes < 1 || u_cap < 1 || e_cap < 1) return GRAPES_EINVAL;
    if (!rowptr || !col || !rows || !bits || !node_map || !bptr || !uniq || !tptr || !trow || !d_counts || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* hdr = (int32_t*)workspace;
    int32_t* item_off = hdr + BAG_HDR;
    int32_t* cur = item_off + m + 1;
    int32_t* nn = cur + u_cap;
    int32_t* nl = nn + u_cap;
    int32_t* counts = nl + u_cap;
    void* cws = counts + 4;
    if (grapes_zero_async(cur, (size_t)u_cap * sizeof(int32_t), s) != hipSuccess) return GRAPES_EINVAL;
    hipLaunchKernelGGL(bag_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, rowptr, num_nodes, rows, m, e_cap, bptr, item_off, hdr, status);
    GRAPES_LAUNCH_CHECK();
    int grid = grapes_div_up((int64_t)e_cap / BAG_CHUNK + m, 4);               // (a wavefront per item while the items fit; else a stride)
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(bag_mark_k, dim3(grid), dim3(256), 0, s, rowptr, col, num_nodes, rows, m, (const int32_t*)bptr,
                       (const int32_t*)item_off, hdr, (unsigned long long*)bits, status);
    GRAPES_LAUNCH_CHECK();
    const int rc = grapes_frontier_compact(bits, nullptr, nullptr, num_nodes, u_cap, uniq, nn, nl, node_map, counts, nullptr, 0u,
                                           nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, cws, nullptr, status, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(bag_place_k<false>, dim3(grid), dim3(256), 0, s, rowptr, col, num_nodes, rows, m, (const int32_t*)bptr,
                       (const int32_t*)item_off, (const int32_t*)hdr, (const int32_t*)node_map, (const int32_t*)uniq,
                       (const int32_t*)counts, u_cap, (const int32_t*)tptr, e_cap, cur, trow);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(bag_tscan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, (const int32_t*)cur, (const int32_t*)counts, u_cap, e_cap,
                       (const int32_t*)hdr, (const int32_t*)(bptr + m), tptr, d_counts, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(bag_place_k<true>, dim3(grid), dim3(256), 0, s, rowptr, col, num_nodes, rows, m, (const int32_t*)bptr,
                       (const int32_t*)item_off, (const int32_t*)hdr, (const int32_t*)node_map, (const int32_t*)uniq,
                       (const int32_t*)counts, u_cap, (const int32_t*)tptr, e_cap, cur, trow);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(bag_order_k, dim3(seg_order_grid(u_cap)), dim3(SEG_ORDER_THREADS), 0, s, (const int32_t*)tptr,
                       (const int32_t*)counts, u_cap, e_cap, trow, status);
    GRAPES_LAUNCH_CHECK();
    int cg = grapes_div_up(u_cap, 256);
    if (cg > 1024) cg = 1024;
    hipLaunchKernelGGL(bag_clear_k, dim3(cg), dim3(256), 0, s, (const int32_t*)uniq, (const int32_t*)counts, u_cap, num_nodes, node_map);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the gathers

// acc += sum_{t in [beg, end)} x[idx[t]] in that order, rows ld floats apart.  An index outside [0, x_rows) raises
// GRAPES_STATUS_BAD_INDEX and the entry is dropped: its lane, like the lanes past a batch's end, points at the batch's first row (or
// row 0) with weight 0 (gather_batch).
// acc += x with the rounding error of the addition carried in c (Kahan); every operation rounded once (no contraction in this file)
template <int VEC, int NS>
__device__ __forceinline__ void slab_add_comp(const float (&x)[NS][VEC], float (&acc)[NS][VEC], float (&c)[NS][VEC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float y = x[s][v] - c[s][v];
            const float t = acc[s][v] + y;
            c[s][v] = (t - acc[s][v]) - y;
            acc[s][v] = t;
        }
}

// COMP: the same walk with the compensated addition (the backward); cmp is the error term beside acc (not touched without COMP)
template <int VEC, int LPR, int NS, bool COMP>
__device__ __forceinline__ void bag_walk(const float* __restrict__ x, long long ld, int x_rows, const int32_t* __restrict__ idx, int beg,
                                         int end, int F, int l, float (&acc)[NS][VEC], float (&cmp)[NS][VEC], int32_t* status) {
    for (int b = beg; b < end; b += LPR) {
        int r = -1;
        if (b + l < end) {
            const int c = idx[b + l];
            if ((unsigned)c < (unsigned)x_rows) r = c;
            else if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        }
        const float wv = r < 0 ? 0.f : 1.f;
        const int first = __shfl(r, 0, LPR);
        if (r < 0) r = first < 0 ? 0 : first;
        const int cnt = end - b < LPR ? end - b : LPR;
        if constexpr (COMP) {
            constexpr int U = HistUnroll<VEC, NS>::U;
            for (int k = 0; k < cnt; k += U) {                      // gather_batch's shape: U rows requested together, added in entry order
                float hv[U][NS][VEC], wk[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    wk[u] = __shfl(wv, k + u, LPR);
                    row_load_ld<VEC, LPR, NS>(x, __shfl(r, k + u, LPR), ld, F, l, hv[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (k + u < cnt) {                              // (group-uniform: nothing is added for the lanes past the batch's end)
                        slab_scale<VEC, NS>(hv[u], wk[u]);          // (1 for an entry, 0 for a dropped one)
                        slab_add_comp<VEC, NS>(hv[u], acc, cmp);
                    }
            }
        } else {
            gather_batch<HistUnroll<VEC, NS>::U, VEC, LPR, NS>(
                wv, cnt, [&](int j, float (&hv)[NS][VEC]) { row_load_ld<VEC, LPR, NS>(x, __shfl(r, j, LPR), ld, F, l, hv); }, acc);
        }
    }
}

struct BagSelf { __device__ __forceinline__ int operator[](int r) const { return r; } };
struct BagOne { __device__ __forceinline__ float operator[](int) const { return 1.f; } };

struct BagFwdArgs {
    const int64_t* rowptr; const int32_t* col; int n_nodes;
    const int32_t* rows;
    const float* w; long long ld_w;
    const float* bias;
    float* out; long long ld_out;
    const int32_t* item_off;             // [m + 1]: the chunks behind the first of the long rows before b (NULL: no row is cut)
    BagSelf rows_g; BagOne dinv;
    int m, N;                            // (hist_combine_k's names) the rows of out
    float* pacc;
    int F;
    int32_t* status;
};

// the stored entries of batch row b: col + a, len of them (0 for a row id outside [0, n_nodes))
__device__ __forceinline__ bool bag_fwd_row(const BagFwdArgs& a, int b, const int32_t*& ent, int& len) {
    const int r = a.rows[b];
    ent = a.col; len = 0;
    if ((unsigned)r >= (unsigned)a.n_nodes) return false;
    const int64_t p = a.rowptr[r], d = a.rowptr[r + 1] - p;
    ent = a.col + p;
    len = d > 0 ? (int)(d < 0x7fffffffll ? d : 0x7fffffffll) : 0;
    return true;
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void bag_fwd_rows_k(BagFwdArgs a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int b = blockIdx.x * G + threadIdx.x / LPR; b < a.m; b += gridDim.x * G) {
        float acc[NS][VEC];
        if (a.bias) row_load<VEC, LPR, NS>(a.bias, 0, a.F, l, acc);
        else slab_zero<VEC, NS>(acc);
        const int32_t* ent; int len;
        if (!bag_fwd_row(a, b, ent, len) && l == 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
        if (a.item_off && len > HIST_LONG_ROW) len = HIST_LONG_ROW;
        bag_walk<VEC, LPR, NS, false>(a.w, a.ld_w, a.n_nodes, ent, 0, len, a.F, l, acc, acc, a.status);
        row_store_ld<VEC, LPR, NS>(a.out, b, a.ld_out, a.F, l, acc);
    }
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void bag_fwd_chunks_k(BagFwdArgs a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    const int n_items = a.item_off[a.m];
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        const int b = lower_bound<int32_t, int, int>(a.item_off, a.m, it + 1) - 1;      // the last row with item_off[b] <= it
        const int c = it - a.item_off[b] + 1;
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        const int32_t* ent; int len;
        if (bag_fwd_row(a, b, ent, len)) {
            const long long cb = (long long)c * HIST_LONG_ROW;
            if (cb < len) {
                const int ce = (int)cb + HIST_LONG_ROW < len ? (int)cb + HIST_LONG_ROW : len;
                bag_walk<VEC, LPR, NS, false>(a.w, a.ld_w, a.n_nodes, ent, (int)cb, ce, a.F, l, acc, acc, a.status);
            }
        }
        row_store<VEC, LPR, NS>(a.pacc, it, a.F, l, acc);
    }
}

// ONE workgroup.  item_off[b] = min(the chunks behind the first of the long rows before b, item_cap), item_off[m] the live items; more
// than item_cap raise GRAPES_STATUS_EDGE_OVERFLOW.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void bag_fwd_items_k(const int64_t* __restrict__ rowptr, int N,
                                                                     const int32_t* __restrict__ rows, int m, int item_cap,
                                                                     int32_t* __restrict__ item_off, int32_t* status) {
    __shared__ unsigned long long lds[17];
    bool bad = false;                                                           // (the rows kernel raises the bit)
    const unsigned long long total = list_scan_tiles<long long, int32_t>(
        [&](int i0, long long (&v)[LIST_SCAN_PER]) {
            list_row_degrees(rowptr, N, rows, i0, m, v, bad);
#pragma unroll
            for (int q = 0; q < LIST_SCAN_PER; ++q) v[q] = v[q] > HIST_LONG_ROW ? (v[q] + HIST_LONG_ROW - 1) / HIST_LONG_ROW - 1 : 0;
        },
        m, (unsigned long long)item_cap, item_off, lds);
    list_scan_finish(total, item_cap, item_off + m, nullptr, status);
}

extern "C" size_t grapes_bag_fwd_workspace_bytes(int32_t m, int32_t item_cap, int32_t h) {
    if (m < 1 || m > BAG_MAX_ROWS || item_cap < 0 || item_cap > BAG_ITEM_CAP_MAX || h < 1) return 0;
    return hist_workspace_bytes(m, item_cap, h);
}

extern "C" int grapes_bag_fwd(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m,
                              const float* w, int64_t ld_w, const float* bias, int32_t h, float* out, int64_t ld_out, int32_t item_cap,
                              void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!rowptr || !col || !rows || !w || !out || out == w) return GRAPES_EINVAL;
    if (num_nodes < 1 || m < 1 || m > BAG_MAX_ROWS || h < 1 || ld_w < h || ld_out < h) return GRAPES_EINVAL;
    if (item_cap < 0 || item_cap > BAG_ITEM_CAP_MAX || (item_cap > 0 && !workspace)) return GRAPES_EINVAL;
    if (item_cap > 0 && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(h, hist_vec_ok(w, ld_w) && hist_vec_ok(out, ld_out) && (!bias || grapes_aligned16(bias)));
    if (shape < 0) return shape;
    hipStream_t s = (hipStream_t)stream;
    BagFwdArgs a{};
    a.rowptr = rowptr; a.col = col; a.n_nodes = num_nodes; a.rows = rows; a.w = w; a.ld_w = ld_w; a.bias = bias; a.out = out;
    a.ld_out = ld_out; a.m = m; a.N = m; a.F = h; a.status = status;
    if (item_cap > 0) {
        a.item_off = (const int32_t*)workspace;
        a.pacc = (float*)((char*)workspace + grapes_round16(((size_t)m + 1) * sizeof(int32_t)));
        hipLaunchKernelGGL(bag_fwd_items_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, rowptr, num_nodes, rows, m, item_cap,
                           (int32_t*)workspace, status);
        GRAPES_LAUNCH_CHECK();
    }
    const bool vec = shape == 0;
    ROW_LAUNCH(bag_fwd_rows_k, 4, vec, h, m, s, a);
    if (item_cap > 0) {
        ROW_LAUNCH(bag_fwd_chunks_k, 4, vec, h, item_cap, s, a);
        ROW_LAUNCH(hist_combine_k, 4, vec, h, m, s, a);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the backward

struct BagBwdArgs {
    const float* g; long long ld_g; int m;               // G [m, F]
    const int32_t* tptr; const int32_t* trow; int n_u, e;
    const int32_t* uniq; int n_nodes;                    // the fused form: the table row of segment s
    float* grad; long long ld_grad;                      // the plain form: the values [n_u, F]
    float* w; long long ld_w;
    float* exp_avg; float* exp_avg_sq; long long ld_state;
    float omb1, omb2, eps, step_size;
    const int32_t* item_off;                             // [n_u + 1]: the chunks of the long segments before s (NULL: none is cut)
    float* pacc;
    int F;
    int32_t* status;
};

__device__ __forceinline__ bool bag_segment(const BagBwdArgs& a, int s, int& beg, int& end) {
    beg = a.tptr[s]; end = a.tptr[s + 1];
    if (beg < 0 || end < beg || end > a.e) { beg = end = 0; return false; }
    return true;
}

// what happens to g_s = acc, once per touched column
template <int VEC, int LPR, int NS, bool ADAM>
__device__ __forceinline__ void bag_finish(const BagBwdArgs& a, int s, int l, const float (&acc)[NS][VEC]) {
    if (!ADAM) {
        row_store_ld<VEC, LPR, NS>(a.grad, s, a.ld_grad, a.F, l, acc);
        return;
    }
    const int j = a.uniq[s];
    if ((unsigned)j >= (unsigned)a.n_nodes) {
        if (l == 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
        return;
    }
    float p[NS][VEC], m1[NS][VEC], v1[NS][VEC];
    row_load_ld<VEC, LPR, NS>(a.w, j, a.ld_w, a.F, l, p);
    row_load_ld<VEC, LPR, NS>(a.exp_avg, j, a.ld_state, a.F, l, m1);
    row_load_ld<VEC, LPR, NS>(a.exp_avg_sq, j, a.ld_state, a.F, l, v1);
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            const float gv = acc[q][c];
            const float mn = m1[q][c] + a.omb1 * (gv - m1[q][c]);
            const float vn = v1[q][c] + a.omb2 * (gv * gv - v1[q][c]);
            const float den = sqrtf(vn) + a.eps;
            p[q][c] = p[q][c] - a.step_size * (mn / den);
            m1[q][c] = mn; v1[q][c] = vn;
        }
    row_store_ld<VEC, LPR, NS>(a.w, j, a.ld_w, a.F, l, p);
    row_store_ld<VEC, LPR, NS>(a.exp_avg, j, a.ld_state, a.F, l, m1);
    row_store_ld<VEC, LPR, NS>(a.exp_avg_sq, j, a.ld_state, a.F, l, v1);
}

template <int VEC, int LPR, int NS, bool ADAM>
__device__ __forceinline__ void bag_bwd_rows(const BagBwdArgs& a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int s = blockIdx.x * G + threadIdx.x / LPR; s < a.n_u; s += gridDim.x * G) {
        int beg, end;
        if (!bag_segment(a, s, beg, end) && l == 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
        if (a.item_off && end - beg > HIST_LONG_ROW) continue;                  // (the combine kernel finishes it)
        float acc[NS][VEC], cmp[NS][VEC];
        slab_zero<VEC, NS>(acc);
        slab_zero<VEC, NS>(cmp);
        bag_walk<VEC, LPR, NS, true>(a.g, a.ld_g, a.m, a.trow, beg, end, a.F, l, acc, cmp, a.status);
        bag_finish<VEC, LPR, NS, ADAM>(a, s, l, acc);
    }
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void bag_bwd_chunks_k(BagBwdArgs a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    const int n_items = a.item_off[a.n_u];
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        const int s = lower_bound<int32_t, int, int>(a.item_off, a.n_u, it + 1) - 1;    // the last segment with item_off[s] <= it
        const int c = it - a.item_off[s];
        float acc[NS][VEC], cmp[NS][VEC];
        slab_zero<VEC, NS>(acc);
        slab_zero<VEC, NS>(cmp);
        int beg, end;
        if (bag_segment(a, s, beg, end)) {
            const long long cb = (long long)beg + (long long)c * HIST_LONG_ROW;
            if (cb < end) {
                const int ce = (int)cb + HIST_LONG_ROW < end ? (int)cb + HIST_LONG_ROW : end;
                bag_walk<VEC, LPR, NS, true>(a.g, a.ld_g, a.m, a.trow, (int)cb, ce, a.F, l, acc, cmp, a.status);
            }
        }
        row_store<VEC, LPR, NS>(a.pacc, it, a.F, l, acc);
    }
}

template <int VEC, int LPR, int NS, bool ADAM>
__device__ __forceinline__ void bag_bwd_combine(const BagBwdArgs& a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int s = blockIdx.x * G + threadIdx.x / LPR; s < a.n_u; s += gridDim.x * G) {
        const int i0 = a.item_off[s], i1 = a.item_off[s + 1];
        if (i1 <= i0) continue;
        constexpr int U = HistUnroll<VEC, NS>::U;
        float acc[NS][VEC], cmp[NS][VEC], p[U][NS][VEC];
        slab_zero<VEC, NS>(acc);
        slab_zero<VEC, NS>(cmp);
        for (int it = i0; it < i1; it += U) {                       // U partial rows requested together, added in chunk order
#pragma unroll
            for (int u = 0; u < U; ++u) row_load<VEC, LPR, NS>(a.pacc, it + u < i1 ? it + u : i0, a.F, l, p[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (it + u < i1) slab_add_comp<VEC, NS>(p[u], acc, cmp);
        }
        bag_finish<VEC, LPR, NS, ADAM>(a, s, l, acc);
    }
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void bag_bwd_rows_k(BagBwdArgs a) { bag_bwd_rows<VEC, LPR, NS, false>(a); }
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void bag_adam_rows_k(BagBwdArgs a) { bag_bwd_rows<VEC, LPR, NS, true>(a); }
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void bag_bwd_combine_k(BagBwdArgs a) { bag_bwd_combine<VEC, LPR, NS, false>(a); }
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void bag_adam_combine_k(BagBwdArgs a) { bag_bwd_combine<VEC, LPR, NS, true>(a); }

// ONE workgroup.  item_off[s] = min(the chunks of the long segments before s, item_cap) — a long segment of L entries has ceil(L / 64),
// its first included — item_off[n_u] the live items; more than item_cap raise GRAPES_STATUS_EDGE_OVERFLOW.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void bag_bwd_items_k(const int32_t* __restrict__ tptr, int n, int E, int item_cap,
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
                    v[q] = len > HIST_LONG_ROW ? (len + HIST_LONG_ROW - 1) / HIST_LONG_ROW : 0;
                }
            }
        },
        n, (unsigned long long)item_cap, item_off, lds);
    list_scan_finish(total, item_cap, item_off + n, nullptr, status);
}

extern "C" size_t grapes_bag_bwd_workspace_bytes(int32_t n_u, int32_t item_cap, int32_t h) {
    if (n_u < 1 || item_cap < 0 || item_cap > BAG_ITEM_CAP_MAX || h < 1) return 0;
    return hist_workspace_bytes(n_u, item_cap, h);
}

template <bool ADAM>
static int bag_bwd_launch(BagBwdArgs& a, int32_t item_cap, void* workspace, bool vec, hipStream_t s) {
    if (item_cap > 0) {
        a.item_off = (const int32_t*)workspace;
        a.pacc = (float*)((char*)workspace + grapes_round16(((size_t)a.n_u + 1) * sizeof(int32_t)));
        hipLaunchKernelGGL(bag_bwd_items_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, a.tptr, a.n_u, a.e, item_cap, (int32_t*)workspace,
                           a.status);
        GRAPES_LAUNCH_CHECK();
    }
    if (ADAM) ROW_LAUNCH(bag_adam_rows_k, 4, vec, a.F, a.n_u, s, a);
    else ROW_LAUNCH(bag_bwd_rows_k, 4, vec, a.F, a.n_u, s, a);
    if (item_cap > 0) {
        ROW_LAUNCH(bag_bwd_chunks_k, 4, vec, a.F, item_cap, s, a);
        if (ADAM) ROW_LAUNCH(bag_adam_combine_k, 4, vec, a.F, a.n_u, s, a);
        else ROW_LAUNCH(bag_bwd_combine_k, 4, vec, a.F, a.n_u, s, a);
    }
    return 0;
}

static int bag_bwd_check(const float* g, int64_t ld_g, int32_t m, const int32_t* tptr, const int32_t* trow, int32_t n_u, int32_t e,
                         int32_t h, int32_t item_cap, const void* workspace) {
    if (!g || !tptr || !trow) return GRAPES_EINVAL;
    if (m < 1 || m > BAG_MAX_ROWS || n_u < 1 || e < 0 || h < 1 || ld_g < h) return GRAPES_EINVAL;
    if (item_cap < 0 || item_cap > BAG_ITEM_CAP_MAX || (item_cap > 0 && !workspace)) return GRAPES_EINVAL;
    if (item_cap > 0 && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    return 0;
}

extern "C" int grapes_bag_bwd(const float* g, int64_t ld_g, int32_t m, const int32_t* tptr, const int32_t* trow, int32_t n_u, int32_t e,
                              int32_t h, float* grad, int64_t ld_grad, int32_t item_cap, void* workspace, int32_t* status,
                              grapes_stream_t stream) {
    const int rc = bag_bwd_check(g, ld_g, m, tptr, trow, n_u, e, h, item_cap, workspace);
    if (rc) return rc;
    if (!grad || grad == g || ld_grad < h) return GRAPES_EINVAL;
    const int shape = gather_shape(h, hist_vec_ok(g, ld_g) && hist_vec_ok(grad, ld_grad));
    if (shape < 0) return shape;
    BagBwdArgs a{};
    a.g = g; a.ld_g = ld_g; a.m = m; a.tptr = tptr; a.trow = trow; a.n_u = n_u; a.e = e; a.grad = grad; a.ld_grad = ld_grad; a.F = h;
    a.status = status;
    return bag_bwd_launch<false>(a, item_cap, workspace, shape == 0, (hipStream_t)stream);
}

extern "C" int grapes_bag_bwd_adam(const float* g, int64_t ld_g, int32_t m, const int32_t* tptr, const int32_t* trow,
                                   const int32_t* uniq, int32_t n_u, int32_t e, int32_t num_nodes, int32_t h, float* w, int64_t ld_w,
                                   float* exp_avg, float* exp_avg_sq, int64_t ld_state, float one_minus_beta1, float one_minus_beta2,
                                   float eps, float step_size, int32_t item_cap, void* workspace, int32_t* status,
                                   grapes_stream_t stream) {
    const int rc = bag_bwd_check(g, ld_g, m, tptr, trow, n_u, e, h, item_cap, workspace);
    if (rc) return rc;
    if (!uniq || !w || !exp_avg || !exp_avg_sq || num_nodes < 1 || ld_w < h || ld_state < h) return GRAPES_EINVAL;
    if (w == exp_avg || w == exp_avg_sq || exp_avg == exp_avg_sq || (const float*)w == g) return GRAPES_EINVAL;
    const int shape = gather_shape(h, hist_vec_ok(g, ld_g) && hist_vec_ok(w, ld_w) && hist_vec_ok(exp_avg, ld_state) &&
                                          hist_vec_ok(exp_avg_sq, ld_state));
    if (shape < 0) return shape;
    BagBwdArgs a{};
    a.g = g; a.ld_g = ld_g; a.m = m; a.tptr = tptr; a.trow = trow; a.n_u = n_u; a.e = e; a.uniq = uniq; a.n_nodes = num_nodes;
    a.w = w; a.ld_w = ld_w; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.ld_state = ld_state;
    a.omb1 = one_minus_beta1; a.omb2 = one_minus_beta2; a.eps = eps; a.step_size = step_size; a.F = h; a.status = status;
    return bag_bwd_launch<true>(a, item_cap, workspace, shape == 0, (hipStream_t)stream);
}
