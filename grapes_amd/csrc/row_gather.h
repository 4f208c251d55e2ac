// The scaffold the row-gather aggregations share (gat_, gatv2_, gcn2_, pna_, sage_ and wgcn_kernels.hip): a new aggregation starts
// here and adds only its own arithmetic; one that is a plain row sum with a row-local epilogue starts at row_sum.h.  Every one of
// them walks the CSRs grapes_gcn_prepare builds with the same three kernels:
//
//   *_rows_k      a group of LPR lanes (half a wavefront or a whole one) owns a row; per batch of LPR entries every lane reads ONE
//                 column index (batch_entry), then the batch's rows are gathered with the indices broadcast from their lanes
//   *_chunks_k    rows longer than GRAPES_LONG_ROW: one group per work item (row, chunk) of the prepared item list (item_range)
//   *_combine_k   one workgroup per long row, led by its chunk-0 item (item_leads), merges the row's items in chunk order
//
// Device side: the slab layout of a row over a group's lanes and its arithmetic (slab_zero, _scale, _fma, _dot), the group
// butterflies, the item-list readers, the batch-entry reader and gather_batch, the weighted gather of one batch of entries: a walk
// says which rows a batch names and with which weights, and how a row is fetched.  Host side: the grids and the launch-by-width
// dispatch.  What a kernel weighs its entries with, and its epilogue, stay in its file; so does the gather loop of a walk that
// reduces a per-entry dot product over the group inside it (wg_range, GAT's backward ranges, GATv2's three).
#pragma once
#include "common.h"

template <int LPR>
__device__ __forceinline__ float grp_sum(float v) {
#pragma unroll
    for (int d = LPR / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, LPR);
    return v;
}
template <int LPR>
__device__ __forceinline__ float grp_max(float v) {
#pragma unroll
    for (int d = LPR / 2; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, LPR));
    return v;
}

// VEC consecutive floats, VEC 4 (one 16-byte access, p aligned) or 1
template <int VEC>
__device__ __forceinline__ void vec_load(const float* __restrict__ p, float (&r)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
        r[0] = *p;
    }
}
template <int VEC>
__device__ __forceinline__ void vec_store(float* __restrict__ p, const float (&r)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else *p = r[0];
}

// lane l of a group holds columns (s LPR + l) VEC ... + VEC of a row, s < NS; columns at or beyond F read as zero
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void row_load(const float* __restrict__ base, long long row, int F, int l, float (&r)[NS][VEC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int f = (s * LPR + l) * VEC;
        if (f < F) {
            if (VEC == 4) {
                const float4 t = *reinterpret_cast<const float4*>(base + row * F + f);
                r[s][0] = t.x; r[s][VEC > 1 ? 1 : 0] = t.y; r[s][VEC > 2 ? 2 : 0] = t.z; r[s][VEC > 3 ? 3 : 0] = t.w;
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) r[s][v] = base[row * F + f + v];
            }
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) r[s][v] = 0.f;
        }
    }
}
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void row_store(float* __restrict__ base, long long row, int F, int l, const float (&r)[NS][VEC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int f = (s * LPR + l) * VEC;
        if (f < F) {
            if (VEC == 4) *reinterpret_cast<float4*>(base + row * F + f) = make_float4(r[s][0], r[s][VEC > 1 ? 1 : 0], r[s][VEC > 2 ? 2 : 0], r[s][VEC > 3 ? 3 : 0]);
            else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) base[row * F + f + v] = r[s][v];
            }
        }
    }
}

// the same slabs of a matrix whose rows are ld >= F floats apart (a column block of a wider matrix: sage_kernels.hip); with
// VEC == 4 the base is 16-byte aligned and ld % 4 == 0
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void row_load_ld(const float* __restrict__ base, long long row, long long ld, int F, int l,
                                            float (&r)[NS][VEC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int f = (s * LPR + l) * VEC;
        if (f < F) vec_load<VEC>(base + row * ld + f, r[s]);
        else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) r[s][v] = 0.f;
        }
    }
}
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void row_store_ld(float* __restrict__ base, long long row, long long ld, int F, int l,
                                             const float (&r)[NS][VEC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int f = (s * LPR + l) * VEC;
        if (f < F) vec_store<VEC>(base + row * ld + f, r[s]);
    }
}

// the live length of a long-row item list: the device count, at most the list's capacity
__device__ __forceinline__ int item_count(const int32_t* __restrict__ d_n_items, int item_cap) {
    const int n_items = *d_n_items;
    return n_items > item_cap ? item_cap : n_items;
}

// Work item `it` = (row, chunk): entries [beg, end) of the row, GRAPES_LONG_ROW of them at most.  False for an item that names no
// row below n or a negative chunk; a chunk that starts at or past the row's end (formed in 64 bits) is an empty range.
__device__ __forceinline__ bool item_range(const int32_t* __restrict__ items, int it, const int32_t* __restrict__ rowptr, int n,
                                           int& row, int& beg, int& end) {
    row = items[2 * it];
    const int chunk = items[2 * it + 1];
    beg = 0; end = 0;
    if (!((unsigned)row < (unsigned)n && chunk >= 0)) return false;
    const int rbeg = rowptr[row], rend = rowptr[row + 1];
    const long long cb = (long long)rbeg + (long long)chunk * GRAPES_LONG_ROW;
    if (cb < rend) {
        beg = (int)cb;
        end = beg + GRAPES_LONG_ROW < rend ? beg + GRAPES_LONG_ROW : rend;
    }
    return true;
}

// The item with chunk 0 leads its row: its nc items are contiguous and in chunk order (nc stays inside the list).  True for such
// an item of a row below n.
__device__ __forceinline__ bool item_leads(const int32_t* __restrict__ items, int it, int n_items, const int32_t* __restrict__ rowptr,
                                           int n, int& row, int& nc) {
    if (items[2 * it + 1] != 0) return false;
    row = items[2 * it];
    if ((unsigned)row >= (unsigned)n) return false;
    nc = (rowptr[row + 1] - rowptr[row] + GRAPES_LONG_ROW - 1) / GRAPES_LONG_ROW;
    if (it + nc > n_items) nc = n_items - it;
    return true;
}

// Entry t of a walk that ends at `end`: its column index, or -1 past the end and for an index outside [0, n), which raises
// GRAPES_STATUS_BAD_INDEX (the entry is dropped).  Lane l of a group calls it with t = b + l for the batch at b.
__device__ __forceinline__ int batch_entry(const int32_t* __restrict__ csr, int t, int end, int n, int32_t* status) {
    int idx = -1;
    if (t < end) {
        const int c = csr[t];
        if ((unsigned)c < (unsigned)n) idx = c;
        else if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    }
    return idx;
}

// entry t of a walk over [beg - with_self, end): the row itself for t < beg (the implied unit self-loop), else csr[t].
// An index outside [0, n) raises GRAPES_STATUS_BAD_INDEX and the entry is dropped.
__device__ __forceinline__ bool gat_entry(const int32_t* __restrict__ csr, int t, int beg, int end, int row, int n, int& idx,
                                          int32_t* status) {
    idx = row;
    if (t >= end) return false;
    if (t < beg) return true;
    const int c = batch_entry(csr, t, end, n, status);
    if (c < 0) return false;
    idx = c;
    return true;
}

// gathered rows a group keeps in flight per step of a gather loop: independent row loads, as many as the registers of NS slabs allow
template <int NS> struct RowUnroll { static constexpr int U = NS == 1 ? 4 : (NS <= 4 ? 2 : 1); };

// a lane's slabs of a row, a[NS][VEC]: zero, scale, acc += w x, and the dot product as one fmaf chain in (s, v) order
template <int VEC, int NS>
__device__ __forceinline__ void slab_zero(float (&a)[NS][VEC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v) a[s][v] = 0.f;
}
template <int VEC, int NS>
__device__ __forceinline__ void slab_scale(float (&a)[NS][VEC], float c) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v) a[s][v] *= c;
}
template <int VEC, int NS>
__device__ __forceinline__ void slab_fma(float w, const float (&x)[NS][VEC], float (&acc)[NS][VEC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[s][v] = fmaf(w, x[s][v], acc[s][v]);
}
template <int VEC, int NS>
__device__ __forceinline__ float slab_dot(const float (&a)[NS][VEC], const float (&b)[NS][VEC]) {
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v) d = fmaf(a[s][v], b[s][v], d);
    return d;
}

// One batch of a weighted gather: lane j < cnt of the group holds the weight w of entry j; load(j, hv) fetches entry j's row
// (it broadcasts whatever index it needs from lane j).  U rows are requested together, then added in entry order.
// No load is predicated: a lane past cnt and a lane whose entry was dropped hold weight 0 and the index of a row that is always
// there (the caller says which), so they add 0 * that row.  Finite operands are unaffected; a non-finite value in that row would
// put NaN into the sum.  The select form, acc += live ? h : 0, has no such case but costs the small-graph rows kernel of GCN2
// 3 - 4 %: profiles/row_sum_ab.txt.
template <int U, int VEC, int LPR, int NS, class LOAD>
__device__ __forceinline__ void gather_batch(float w, int cnt, LOAD load, float (&acc)[NS][VEC]) {
    for (int k = 0; k < cnt; k += U) {
        float hv[U][NS][VEC], wk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wk[u] = __shfl(w, k + u, LPR);
            load(k + u, hv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) slab_fma<VEC, NS>(wk[u], hv[u], acc);
    }
}

// ------------------------------------------------------------------------------------------------------------ host side

static inline int row_grid(int rows, int lanes) {
    int g = grapes_div_up(rows > 0 ? rows : 1, 256 / lanes);
    return g > 16384 ? 16384 : g;
}
static inline int flat_grid(int64_t n, int64_t f, int vec) {
    int64_t g = (n * f / vec + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// The column shape of a width-f gather whose wide scalar form is not built (ROW_LAUNCH with NS_WIDE = 4) — 0: float4 columns,
// 1: scalar columns, negative: not covered (GRAPES_EALIGN where alignment alone stands in the way)
static inline int gather_shape(int f, bool aligned) {
    if (f < 1) return GRAPES_EINVAL;
    if (f % 4 == 0 && aligned) return f <= 1024 ? 0 : GRAPES_EINVAL;
    if (f <= 256) return 1;
    return f % 4 == 0 && f <= 1024 ? GRAPES_EALIGN : GRAPES_EINVAL;
}

// KERNEL<VEC, LPR, NS> over `rows` rows or work items, a group of LPR lanes each: lanes per row and slabs per lane by width —
// float4 columns (vec: f % 4 == 0, 16-byte aligned rows) up to 1024, scalar ones up to 256 and, with NS_WIDE slabs, beyond
// (NS_WIDE = 4: the caller refuses those widths, and nothing wider than <1, 64, 4> is instantiated).
#define ROW_LAUNCH(KERNEL, NS_WIDE, vec, f, rows, s, ...)                                                                   \
    do {                                                                                                                    \
        const dim3 g32_(row_grid(rows, 32)), g64_(row_grid(rows, 64));                                                      \
        if (vec) {                                                                                                          \
            if ((f) <= 128) hipLaunchKernelGGL((KERNEL<4, 32, 1>), g32_, dim3(256), 0, s, __VA_ARGS__);                      \
            else if ((f) <= 256) hipLaunchKernelGGL((KERNEL<4, 64, 1>), g64_, dim3(256), 0, s, __VA_ARGS__);                 \
            else hipLaunchKernelGGL((KERNEL<4, 64, 4>), g64_, dim3(256), 0, s, __VA_ARGS__);                                 \
        } else {                                                                                                            \
            if ((f) <= 32) hipLaunchKernelGGL((KERNEL<1, 32, 1>), g32_, dim3(256), 0, s, __VA_ARGS__);                       \
            else if ((f) <= 64) hipLaunchKernelGGL((KERNEL<1, 64, 1>), g64_, dim3(256), 0, s, __VA_ARGS__);                  \
            else if ((f) <= 256) hipLaunchKernelGGL((KERNEL<1, 64, 4>), g64_, dim3(256), 0, s, __VA_ARGS__);                 \
            else hipLaunchKernelGGL((KERNEL<1, 64, NS_WIDE>), g64_, dim3(256), 0, s, __VA_ARGS__);                           \
        }                                                                                                                   \
        GRAPES_LAUNCH_CHECK();                                                                                              \
    } while (0)

// KERNEL<VEC, LPR> for kernels that walk a row once per column tile of LPR * VEC features: any f >= 1
#define ROW_LAUNCH_TILED(KERNEL, vec, f, rows, s, ...)                                                                      \
    do {                                                                                                                    \
        const dim3 g32_(row_grid(rows, 32)), g64_(row_grid(rows, 64));                                                      \
        if (vec) {                                                                                                          \
            if ((f) <= 128) hipLaunchKernelGGL((KERNEL<4, 32>), g32_, dim3(256), 0, s, __VA_ARGS__);                         \
            else hipLaunchKernelGGL((KERNEL<4, 64>), g64_, dim3(256), 0, s, __VA_ARGS__);                                    \
        } else {                                                                                                            \
            if ((f) <= 32) hipLaunchKernelGGL((KERNEL<1, 32>), g32_, dim3(256), 0, s, __VA_ARGS__);                          \
            else hipLaunchKernelGGL((KERNEL<1, 64>), g64_, dim3(256), 0, s, __VA_ARGS__);                                    \
        }                                                                                                                   \
        GRAPES_LAUNCH_CHECK();                                                                                              \
    } while (0)
