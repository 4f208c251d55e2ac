// What the aggregations over historical activations share (vrgcn_kernels.hip, gas_kernels.hip), on the row-gather scaffold: a
// batch of n_local rows, node_idx[local id] = global id, dinv a table on GLOBAL ids; a row longer than HIST_LONG_ROW entries is cut
// into chunks of that many entries, one group of lanes each, whose partial sums pacc[item] are added in chunk order.
//   HistUnroll        the source rows a group keeps in flight in a walk over a whole neighbourhood
//   hist_combine_k    a group per listed row: the long row's items added in chunk order to what the rows kernel left, then dinv_u
//   hist_bwd_k        a group per local row over the by-source CSR of a preparation, entries in the CSR's order; WHAT a target
//                     contributes (which row of dA, which factor) is the caller's policy
//   hist_workspace_bytes, hist_carve   the forward's workspace [item_off | pacc] and its two pointers.  (The launches after it —
//                     items, rows, chunks, hist_combine_k — stay written out in the two files: their kernels differ by name, and
//                     one body for both would be a macro that takes kernel names.)
// No float atomics: every sum has a fixed order.
#pragma once
#include "row_gather.h"

// The long-row threshold (= the chunk length) and the history rows in flight were chosen by measurement on the products-shaped
// synthetic graph (batch 512, width 256; DESIGN.md has the table): chunks of 512 entries walked four rows at a time leave one group
// with 128 dependent trips, 114 - 132 us per call; chunks of 64 with 16 rows in flight take 27 - 28 us.
#ifndef VRGCN_LONG_MULT
#define VRGCN_LONG_MULT 1
#endif
#define HIST_LONG_ROW (VRGCN_LONG_MULT * GRAPES_LONG_ROW)
#ifndef VRGCN_FULL_BUDGET
#define VRGCN_FULL_BUDGET 64
#endif

// history rows a group keeps in flight in the full walk: VRGCN_FULL_BUDGET floats per lane (at most that many / 4 rows), and never
// fewer than the scaffold's RowUnroll
template <int VEC, int NS> struct HistUnroll {
    static constexpr int B = VRGCN_FULL_BUDGET / (NS * VEC), M = VRGCN_FULL_BUDGET / 4;
    static constexpr int U = B > M ? M : (B > RowUnroll<NS>::U ? B : RowUnroll<NS>::U);
};

// A: the forward's arguments — item_off int32[m + 1] (a row's first item), m listed rows with global ids rows_g, N, out / ld_out,
// pacc [items, F], dinv, F.
template <int VEC, int LPR, int NS, class A>
__global__ __launch_bounds__(256) void hist_combine_k(A a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int r = blockIdx.x * G + threadIdx.x / LPR; r < a.m; r += gridDim.x * G) {
        const int i0 = a.item_off[r], i1 = a.item_off[r + 1];
        if (i1 <= i0) continue;
        const int u = a.rows_g[r];
        if ((unsigned)u >= (unsigned)a.N) continue;
        constexpr int U = HistUnroll<VEC, NS>::U;
        float acc[NS][VEC], p[U][NS][VEC];
        row_load_ld<VEC, LPR, NS>(a.out, r, a.ld_out, a.F, l, acc);
        int it = i0;
        for (; it + U <= i1; it += U) {                                       // U partial rows requested together, added in chunk order
#pragma unroll
            for (int u = 0; u < U; ++u) row_load<VEC, LPR, NS>(a.pacc, it + u, a.F, l, p[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[s][v] += p[u][s][v];
        }
        for (; it < i1; ++it) {
            row_load<VEC, LPR, NS>(a.pacc, it, a.F, l, p[0]);
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[s][v] += p[0][s][v];
        }
        slab_scale<VEC, NS>(acc, a.dinv[u]);
        row_store_ld<VEC, LPR, NS>(a.out, r, a.ld_out, a.F, l, acc);
    }
}

struct HistBwdArgs {
    const float* da; long long ld_da;
    const int32_t* node_idx;
    const float* dinv; int N;
    const int32_t* rowptr_s; const int32_t* csr_dst;
    float* dh; long long ld_dh;
    int n_local, F;
    int32_t* status;
};

// dh[lv] = dinv_v (sum_{c in by-source row lv} w(c) da[row(c)] + dinv_v da[self(lv)]), the self term only where self(lv) >= 0.
// T: row(c, status) = the row of da a target c reads or -1 (dropped), weight(r) = its factor, self(lv) = lv's own row of da or -1.
template <int VEC, int LPR, int NS, class T>
__global__ __launch_bounds__(256) void hist_bwd_k(HistBwdArgs a, T tgt) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int lv = blockIdx.x * G + threadIdx.x / LPR; lv < a.n_local; lv += gridDim.x * G) {
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        const int gv = a.node_idx[lv];
        if ((unsigned)gv >= (unsigned)a.N) {
            if (l == 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
            row_store_ld<VEC, LPR, NS>(a.dh, lv, a.ld_dh, a.F, l, acc);
            continue;
        }
        const int beg = a.rowptr_s[lv], end = a.rowptr_s[lv + 1];
        for (int b = beg; b < end; b += LPR) {
            const int c = batch_entry(a.csr_dst, b + l, end, a.n_local, a.status);
            const int r = c >= 0 ? tgt.row(c, a.status) : -1;
            const int idx = r < 0 ? 0 : r;                      // (a dropped lane points at row 0 of da)
            const int cnt = end - b < LPR ? end - b : LPR;
            gather_batch<RowUnroll<NS>::U, VEC, LPR, NS>(
                r < 0 ? 0.f : tgt.weight(r), cnt,
                [&](int j, float (&g)[NS][VEC]) { row_load_ld<VEC, LPR, NS>(a.da, __shfl(idx, j, LPR), a.ld_da, a.F, l, g); }, acc);
        }
        const float dv = a.dinv[gv];
        const int rs = tgt.self(lv);
        if (rs >= 0) {
            float g[NS][VEC];
            row_load_ld<VEC, LPR, NS>(a.da, rs, a.ld_da, a.F, l, g);
            slab_fma<VEC, NS>(dv, g, acc);
        }
        slab_scale<VEC, NS>(acc, dv);
        row_store_ld<VEC, LPR, NS>(a.dh, lv, a.ld_dh, a.F, l, acc);
    }
}

// ------------------------------------------------------------------------------------------------------------ host side

static inline bool hist_vec_ok(const void* p, int64_t ld) { return grapes_aligned16(p) && ld % 4 == 0; }

// the forward's workspace: [item_off int32 (m + 1)] [pacc item_cap f]
static inline size_t hist_workspace_bytes(int32_t m, int32_t item_cap, int32_t f) {
    const size_t M = m > 0 ? (size_t)m : 0, I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    return grapes_round16((M + 1) * sizeof(int32_t)) + grapes_round16(I * F * sizeof(float)) + 16;
}
// ... carved into A's item_off and pacc (both NULL without long-row items); A::m is set
template <class A>
static inline void hist_carve(A& a, void* workspace, int32_t item_cap) {
    a.item_cap = item_cap;
    a.item_off = item_cap > 0 ? (const int32_t*)workspace : nullptr;
    a.pacc = item_cap > 0 ? (float*)((char*)workspace + grapes_round16(((size_t)a.m + 1) * sizeof(int32_t))) : nullptr;
}
