// N1 above 2^31 entries: full-batch message passing (eval.py:47-70, modules/gcn.py:32,36) over a graph whose CSR needs 64-bit
// row offsets (ogbn-papers100M symmetrised: 3.2e9 entries).  The int32 path (grapes_gcn_prepare_from_csr + grapes_gcn_aggregate_fwd*)
// is unchanged; these kernels read the graph's own int64 rowptr / int32 col (or its transpose) in place, with no edge-list copy:
//   * lg_prepare_k    dinv[r] = (1 + #{entries of row r that are not r})^-1/2 — PyG's self-loop replacement without copying the
//                     edge list — and the number of hub-row work items (rows longer than `chunk` entries);
//   * lg_symmetric_k  every stored (r, c), r != c, has (c, r): binary search of r in row c (columns ascend);
//   * lg_items_k / lg_chunks_k / lg_aggregate_k   the gather-SpMM over a contiguous row range or an explicit row list: one
//                     wavefront per row, LPR lanes per 4*LPR columns, 64/LPR entry slots combined by xor-shuffles in a fixed
//                     order; a hub row is cut into `chunk`-entry items (one workgroup each) whose partials the row's wavefront
//                     adds in chunk order.  Every sum has a fixed order: two runs are bit-identical.
// All entry offsets and row addresses are 64-bit (col is 12.8 GB and X 57 GB at papers100M: no 32-bit buffer offset covers them).
#include "common.h"
#include "philox.h"

// Hub rows: rows with more than `chunk` entries (a multiple of 64; 1024 from Python by default) are split into items of `chunk`.

// ---------------------------------------------------------------------------------------------- prepare: dinv + hub item count
__global__ __launch_bounds__(256) void lg_prepare_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n,
                                                    int chunk, float* __restrict__ dinv, unsigned long long* __restrict__ d_items) {
    const int lane = lane_id();
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long row = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < n; row += nw) {
        const long long beg = rowptr[row], end = rowptr[row + 1];
        int loops = 0;
        for (long long j = beg + lane; j < end; j += 64) loops += col[j] == (int32_t)row ? 1 : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) loops += __shfl_xor(loops, d, 64);
        if (lane == 0) {
            dinv[row] = 1.0f / sqrtf((float)(end - beg - loops + 1));      // deg = in-degree (self-loops skipped) + unit loop
            if (end - beg > chunk) atomicAdd(d_items, (unsigned long long)((end - beg + chunk - 1) / chunk));
        }
    }
}

// ---------------------------------------------------------------------------------------------- symmetry check
// flag |= 1: some (r, c) has no (c, r);  flag |= 2: a column id outside [0, n)
__global__ __launch_bounds__(256) void lg_symmetric_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n,
                                                      int32_t* __restrict__ flag) {
    const int lane = lane_id();
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    int bad = 0;
    for (long long row = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < n; row += nw) {
        const long long beg = rowptr[row], end = rowptr[row + 1];
        for (long long j = beg + lane; j < end; j += 64) {
            const int c = col[j];
            if (c == (int)row) continue;
            if (c < 0 || c >= n) { bad |= 2; continue; }
            long long lo = rowptr[c], hi = rowptr[c + 1];                    // first position with col >= row
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if (col[mid] < (int32_t)row) lo = mid + 1; else hi = mid; }
            if (lo >= rowptr[c + 1] || col[lo] != (int32_t)row) bad |= 1;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad |= __shfl_xor(bad, d, 64);
    if (lane == 0 && bad) atomicOr(flag, bad);
}

// ---------------------------------------------------------------------------------------------- gather-SpMM
// Row i of a launch: rows ? rows[i] : r0 + i.  h / out rows are 16-byte aligned with pitches ldh / ldo (floats); f % 4 == 0.
struct LgArgs {
    const float* h; long long ldh;
    const int64_t* rowptr; const int32_t* col; const float* dinv;
    int r0; const int32_t* rows; int m; int f;
    const float* bias; int relu; float* out; long long ldo;
    int chunk;                                                      // hub-row item length (entries)
    const int32_t* items; const unsigned long long* d_items; int item_cap;      // items[2 * it] = launch row index i, [2 * it + 1] = chunk
    const int32_t* item_start; float* partials;                     // item_start[i]: first item of hub row i (or -1)
    const int32_t* srcs;                                            // LG_TRANSPOSED: source id of structure row i (its dinv)
};

// Forms of the gather: LG_WEIGHTED w_s = dinv[s] dinv[r] and self term dinv[r]^2 h[r]; LG_PRESCALED rows of h pre-scaled
// (w = 1, dinv[r] (sum + h[r])); LG_TRANSPOSED the row-list transpose of the backward pass (rl_t_*: rowptr = per-source
// offsets, col = positions into h = G, self entries stored): no entry skipped, no self term, out = dinv[srcs[i]] * sum.
enum { LG_WEIGHTED = 0, LG_PRESCALED = 1, LG_TRANSPOSED = 2 };

__device__ __forceinline__ int lg_row(const LgArgs& a, int i) { return a.rows ? a.rows[i] : a.r0 + i; }

// sum over entries [beg, end) of row `row` (self-loop skipped) of w_s * h[s, f .. f+4): slot `slot` of `slots` takes every
// slots-th entry, U entries in flight; MODE: see LG_WEIGHTED / LG_PRESCALED / LG_TRANSPOSED
template <int U, int MODE>
__device__ __forceinline__ float4 lg_accumulate(const LgArgs& a, int row, long long beg, long long end, float dc, int f, int slot,
                                                int slots, bool live) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long j = beg + slot; j < end; j += (long long)U * slots) {
        int s[U]; float w[U]; float4 t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const long long jj = j + (long long)u * slots; s[u] = a.col[jj < end ? jj : end - 1]; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = j + (long long)u * slots < end && (MODE == LG_TRANSPOSED || s[u] != row);
            w[u] = in ? (MODE != LG_WEIGHTED ? 1.0f : a.dinv[s[u]] * dc) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            t[u] = live ? *reinterpret_cast<const float4*>(a.h + (long long)s[u] * a.ldh + f) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            acc.x = fmaf(w[u], t[u].x, acc.x); acc.y = fmaf(w[u], t[u].y, acc.y);
            acc.z = fmaf(w[u], t[u].z, acc.z); acc.w = fmaf(w[u], t[u].w, acc.w);
        }
    }
    return acc;
}
template <int LPR>
__device__ __forceinline__ float4 lg_combine_slots(float4 acc) {
#pragma unroll
    for (int d = LPR; d < 64; d <<= 1) {
        acc.x += __shfl_xor(acc.x, d, 64); acc.y += __shfl_xor(acc.y, d, 64);
        acc.z += __shfl_xor(acc.z, d, 64); acc.w += __shfl_xor(acc.w, d, 64);
    }
    return acc;
}

// hub-row work items of this launch's rows: a row's nc items are reserved together (one atomic on a 64-bit counter, which no
// row list can wrap), so they are contiguous and in chunk order.  A row whose reservation does not end below item_cap (only a
// row list with repeats needs more items than the graph has) marks the slots it got below the cap as empty (-1: lg_chunks_k
// skips them, so no slot below the cap is left unwritten), is walked by its own wavefront and raises GRAPES_STATUS_NODE_OVERFLOW.
__global__ __launch_bounds__(256) void lg_items_k(LgArgs a, int32_t* __restrict__ items, unsigned long long* __restrict__ d_items,
                                                  int32_t* __restrict__ item_start, int32_t* status) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += gridDim.x * blockDim.x) {
        const int row = lg_row(a, i);
        const long long len = a.rowptr[row + 1] - a.rowptr[row];
        if (len <= a.chunk) continue;
        const long long nc = (len + a.chunk - 1) / a.chunk;
        const long long slot = (long long)atomicAdd(d_items, (unsigned long long)nc);
        if (slot + nc > a.item_cap) {
            for (long long c = slot; c < a.item_cap; ++c) items[2 * c] = -1;
            item_start[i] = -1;
            if (status) atomicOr(status, GRAPES_STATUS_NODE_OVERFLOW);
            continue;
        }
        for (int c = 0; c < (int)nc; ++c) { items[2 * (slot + c)] = i; items[2 * (slot + c) + 1] = c; }
        item_start[i] = (int)slot;
    }
}

// one workgroup per item: 4 wavefronts take a quarter of the chunk each, their sums are added in wavefront order
template <int LPR, int MODE>
__global__ __launch_bounds__(256) void lg_chunks_k(LgArgs a) {
    constexpr int U = LPR >= 64 ? 8 : 4;
    constexpr int SLOTS = 64 / LPR;
    __shared__ float4 part[4][64];
    const unsigned long long reserved = *a.d_items;
    const int n_items = reserved < (unsigned long long)a.item_cap ? (int)reserved : a.item_cap;
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const int slot = lane / LPR, sub = lane % LPR;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int li = a.items[2 * it];
        if (li < 0) continue;                                            // (a slot of a row that did not fit)
        const int row = lg_row(a, li), chunk = a.items[2 * it + 1];
        const long long rbeg = a.rowptr[row], rend = a.rowptr[row + 1];
        const long long beg = rbeg + (long long)chunk * a.chunk;
        const long long end = beg + a.chunk < rend ? beg + a.chunk : rend;
        const long long wb = beg + (long long)wid * (a.chunk / 4);
        const long long we = wb + a.chunk / 4 < end ? wb + a.chunk / 4 : end;
        const float dc = MODE == LG_WEIGHTED ? a.dinv[row] : 0.f;
        for (int fb = 0; fb < a.f; fb += 4 * LPR) {
            const int f = fb + 4 * sub;
            const bool live = f < a.f;
            const float4 acc = lg_combine_slots<LPR>(lg_accumulate<U, MODE>(a, row, wb, we, dc, f, slot, SLOTS, live));
            if (slot == 0) part[wid][sub] = acc;
            __syncthreads();
            if (wid == 0 && slot == 0 && live) {
                const float4 p = part[0][sub], q = part[1][sub], r = part[2][sub], s = part[3][sub];
                *reinterpret_cast<float4*>(a.partials + (long long)it * a.f + f) =
                    make_float4(((p.x + q.x) + r.x) + s.x, ((p.y + q.y) + r.y) + s.y, ((p.z + q.z) + r.z) + s.z, ((p.w + q.w) + r.w) + s.w);
            }
            __syncthreads();
        }
    }
}

template <int LPR, int MODE>
__global__ __launch_bounds__(256) void lg_aggregate_k(LgArgs a) {
    constexpr int U = LPR >= 64 ? 8 : 4;
    constexpr int SLOTS = 64 / LPR;
    const int lane = lane_id();
    const int slot = lane / LPR, sub = lane % LPR;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int i = wave; i < a.m; i += nwaves) {
        const int row = lg_row(a, i);
        const long long beg = a.rowptr[row], end = a.rowptr[row + 1];
        const float dc = MODE == LG_TRANSPOSED ? a.dinv[a.srcs[i]] : a.dinv[row];
        const int it0 = (end - beg > a.chunk && a.item_start) ? a.item_start[i] : -1;
        for (int fb = 0; fb < a.f; fb += 4 * LPR) {
            const int f = fb + 4 * sub;
            const bool live = f < a.f;
            float4 acc;
            if (it0 < 0) {
                acc = lg_combine_slots<LPR>(lg_accumulate<U, MODE>(a, row, beg, end, dc, f, slot, SLOTS, live));
            } else {                                                         // the row's item partials, in chunk order
                acc = make_float4(0.f, 0.f, 0.f, 0.f);
                const int nc = (int)((end - beg + a.chunk - 1) / a.chunk);
                if (slot == 0 && live)
                    for (int c = 0; c < nc; ++c) {
                        const float4 p = *reinterpret_cast<const float4*>(a.partials + (long long)(it0 + c) * a.f + f);
                        acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
                    }
            }
            if (MODE == LG_TRANSPOSED) {
                if (slot == 0 && live)
                    *reinterpret_cast<float4*>(a.out + (long long)i * a.ldo + f) = make_float4(dc * acc.x, dc * acc.y, dc * acc.z, dc * acc.w);
            } else if (slot == 0 && live) {
                const float4 sv = *reinterpret_cast<const float4*>(a.h + (long long)row * a.ldh + f);
                const float w = dc * dc;
                float4 r = MODE == LG_PRESCALED ? make_float4(dc * (acc.x + sv.x), dc * (acc.y + sv.y), dc * (acc.z + sv.z), dc * (acc.w + sv.w))
                               : make_float4(fmaf(w, sv.x, acc.x), fmaf(w, sv.y, acc.y), fmaf(w, sv.z, acc.z), fmaf(w, sv.w, acc.w));
                if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + f); r.x += b.x; r.y += b.y; r.z += b.z; r.w += b.w; }
                if (a.relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
                *reinterpret_cast<float4*>(a.out + (long long)i * a.ldo + f) = r;
            }
        }
    }
}

template <int LPR, int MODE>
static int lg_launch_mode(const LgArgs& a, bool with_items, hipStream_t s) {
    if (with_items) {
        int cgrid = a.item_cap < 8192 ? a.item_cap : 8192;
        hipLaunchKernelGGL((lg_chunks_k<LPR, MODE>), dim3(cgrid), dim3(256), 0, s, a);
        GRAPES_LAUNCH_CHECK();
    }
    int grid = grapes_div_up(a.m, 4); if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL((lg_aggregate_k<LPR, MODE>), dim3(grid), dim3(256), 0, s, a);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
template <int LPR>
static int lg_launch(const LgArgs& a, int mode, bool with_items, hipStream_t s) {
    if (mode == LG_TRANSPOSED) return lg_launch_mode<LPR, LG_TRANSPOSED>(a, with_items, s);
    if (mode == LG_PRESCALED) return lg_launch_mode<LPR, LG_PRESCALED>(a, with_items, s);
    return lg_launch_mode<LPR, LG_WEIGHTED>(a, with_items, s);
}

static inline size_t lg_al256(size_t x) { return (x + 255) & ~(size_t)255; }
static int lg_run(LgArgs a, int mode, void* workspace, int32_t* status, hipStream_t s);

// ---------------------------------------------------------------------------------------------- C-ABI
extern "C" int grapes_gcn_large_prepare(const int64_t* rowptr_t, const int32_t* col_t, int32_t n, int32_t chunk, float* dinv,
                                        int64_t* d_items, grapes_stream_t stream) {
    if (n <= 0 || chunk < 64 || (chunk & 63) || !rowptr_t || !col_t || !dinv || !d_items) return GRAPES_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = grapes_zero_async(d_items, 8, s);
    if (e != hipSuccess) return (int)e;
    int grid = grapes_div_up(n, 4); if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(lg_prepare_k, dim3(grid), dim3(256), 0, s, rowptr_t, col_t, n, chunk, dinv, (unsigned long long*)d_items);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_csr_symmetric_check(const int64_t* rowptr, const int32_t* col, int32_t n, int32_t* d_flag,
                                          grapes_stream_t stream) {
    if (n <= 0 || !rowptr || !col || !d_flag) return GRAPES_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = grapes_zero_async(d_flag, 4, s);
    if (e != hipSuccess) return (int)e;
    int grid = grapes_div_up(n, 4); if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(lg_symmetric_k, dim3(grid), dim3(256), 0, s, rowptr, col, n, d_flag);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t grapes_gcn_large_aggregate_workspace_bytes(int32_t m, int32_t item_cap, int32_t f) {
    const size_t M = (size_t)(m > 0 ? m : 1), C = (size_t)(item_cap > 0 ? item_cap : 0), F = (size_t)(f > 0 ? f : 1);
    return 256 + lg_al256(C * 2 * 4) + lg_al256(M * 4) + lg_al256(C * F * 4) + 256;
}

extern "C" int grapes_gcn_large_aggregate(const float* h, int64_t ldh, const int64_t* rowptr_t, const int32_t* col_t,
                                          const float* dinv, int32_t prescaled, int32_t r0, const int32_t* rows, int32_t m,
                                          int32_t f, const float* bias, int32_t relu, float* out, int64_t ldo, int32_t chunk,
                                          int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (m < 0 || f <= 0 || (f & 3) || f > 4096 || ldh < f || ldo < f || (ldh & 3) || (ldo & 3) || item_cap < 0 || r0 < 0 ||
        chunk < 64 || (chunk & 63))
        return GRAPES_EINVAL;
    if (m == 0) return 0;
    if (!h || !rowptr_t || !col_t || !dinv || !out || (item_cap > 0 && !workspace)) return GRAPES_EINVAL;
    if (((uintptr_t)h & 15) || ((uintptr_t)out & 15) || (bias && ((uintptr_t)bias & 15)) || ((uintptr_t)workspace & 255))
        return GRAPES_EALIGN;
    LgArgs a{h, (long long)ldh, rowptr_t, col_t, dinv, r0, rows, m, f, bias, relu, out, (long long)ldo, chunk,
             nullptr, nullptr, item_cap, nullptr, nullptr, nullptr};
    return lg_run(a, prescaled ? LG_PRESCALED : LG_WEIGHTED, workspace, status, (hipStream_t)stream);
}

static int lg_run(LgArgs a, int mode, void* workspace, int32_t* status, hipStream_t s) {
    const int m = a.m, f = a.f, item_cap = a.item_cap;
    const bool with_items = item_cap > 0;
    if (with_items) {
        char* w = (char*)workspace;
        unsigned long long* d_items = (unsigned long long*)w; w += 256;
        int32_t* items = (int32_t*)w; w += lg_al256((size_t)item_cap * 2 * 4);
        int32_t* item_start = (int32_t*)w; w += lg_al256((size_t)m * 4);
        a.items = items; a.d_items = d_items; a.item_start = item_start; a.partials = (float*)w;
        hipError_t e = grapes_zero_async(d_items, 8, s);
        if (e != hipSuccess) return (int)e;
        int igrid = grapes_div_up(m, 256); if (igrid > 4096) igrid = 4096;
        hipLaunchKernelGGL(lg_items_k, dim3(igrid), dim3(256), 0, s, a, items, d_items, item_start, status);
        GRAPES_LAUNCH_CHECK();
    }
    const int f4 = f >> 2;                                   // lanes per row: the smallest power of two >= f / 4, at most 64
    if (f4 <= 1) return lg_launch<1>(a, mode, with_items, s);
    if (f4 <= 2) return lg_launch<2>(a, mode, with_items, s);
    if (f4 <= 4) return lg_launch<4>(a, mode, with_items, s);
    if (f4 <= 8) return lg_launch<8>(a, mode, with_items, s);
    if (f4 <= 16) return lg_launch<16>(a, mode, with_items, s);
    if (f4 <= 32) return lg_launch<32>(a, mode, with_items, s);
    return lg_launch<64>(a, mode, with_items, s);
}

// ---------------------------------------------------------------------------------------------- full-batch training (full-batch.py:100-105)
// Transposed gather over the row-list transpose (grapes_rowlist_transpose): out[j] = dinv[srcs[j]] * sum of g[pos[k]] over
// k in [src_off[j], src_off[j+1]) — the gradient of dinv ⊙ (Â T) restricted to the loss rows, taken back to dU = dinv ⊙ dT on the
// sources.  Positions ascend within a source; a source with more than `chunk` entries is cut into items whose partials are
// added in chunk order (lg_chunks_k), so two runs are bit-identical.  item_cap bounds the items: 2 * entries / chunk + 1.
extern "C" size_t grapes_rowlist_gather_t_workspace_bytes(int32_t n_src, int32_t item_cap, int32_t f) {
    return grapes_gcn_large_aggregate_workspace_bytes(n_src, item_cap, f);
}
extern "C" int grapes_rowlist_gather_t(const float* g, int64_t ldg, const int32_t* srcs, const int64_t* src_off, const int32_t* pos,
                                       const float* dinv, int32_t n_src, int32_t f, float* out, int64_t ldo, int32_t chunk,
                                       int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (n_src < 0 || f <= 0 || (f & 3) || f > 4096 || ldg < f || ldo < f || (ldg & 3) || (ldo & 3) || item_cap < 0 ||
        chunk < 64 || (chunk & 63))
        return GRAPES_EINVAL;
    if (n_src == 0) return 0;
    if (!g || !srcs || !src_off || !pos || !dinv || !out || (item_cap > 0 && !workspace)) return GRAPES_EINVAL;
    if (((uintptr_t)g & 15) || ((uintptr_t)out & 15) || ((uintptr_t)workspace & 255)) return GRAPES_EALIGN;
    LgArgs a{g, (long long)ldg, src_off, pos, dinv, 0, nullptr, n_src, f, nullptr, 0, out, (long long)ldo, chunk,
             nullptr, nullptr, item_cap, nullptr, nullptr, srcs};
    return lg_run(a, LG_TRANSPOSED, workspace, status, (hipStream_t)stream);
}

// Dropout of a row list of an N x width matrix (modules/gcn.py:33,37 inside full-batch.py:101): element (i, c), c < f, of the
// m x f block belongs to row r = rows ? rows[i] : r0 + i and is kept iff philox_uniform(seed, offset, r * width + c) >= p — the
// mask grapes_dropout_fwd draws on the whole contiguous N x width matrix — then scaled by 1 / (1 - p); dropped elements are 0.
// y may be x (in place).  Columns f .. of the block are not touched.
__global__ __launch_bounds__(256) void lg_dropout_rows_k(const float* x, long long ldx, float* y, long long ldy, int r0,
                                                         const int32_t* __restrict__ rows, int m, int f, long long width, float p,
                                                         uint64_t seed, uint64_t offset) {
    const float scale = p < 1.0f ? 1.0f / (1.0f - p) : 0.f;
    const long long total = (long long)m * f;
    for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
        const long long i = it / f;
        const int c = (int)(it - i * f);
        const long long r = rows ? (long long)rows[i] : (long long)r0 + i;
        const bool keep = philox_uniform_at(seed, offset, r * width + c) >= p;
        const float v = x[i * ldx + c];
        y[i * ldy + c] = keep ? v * scale : 0.f;
    }
}
extern "C" int grapes_dropout_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int32_t r0, const int32_t* rows, int32_t m,
                                   int32_t f, int64_t width, float p, uint64_t philox_seed, uint64_t philox_offset,
                                   grapes_stream_t stream) {
    if (m < 0 || f <= 0 || (int64_t)f > width || ldx < f || ldy < f || r0 < 0 || !(p >= 0.f && p <= 1.f)) return GRAPES_EINVAL;
    if (m == 0) return 0;
    if (!x || !y) return GRAPES_EINVAL;
    long long grid = ((long long)m * f + 255) / 256; if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(lg_dropout_rows_k, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (long long)ldx, y,
                       (long long)ldy, r0, rows, m, f, (long long)width, p, philox_seed, philox_offset);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
