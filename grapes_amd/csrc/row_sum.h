// The plain-sum gather GCN2Conv and the aggregation of SAGEConv and ClusterGCNConv share (gcn2_kernels.hip, rootsum_kernels.hip), on
// the row-gather scaffold:
//
//   p[row] = sum_{t in row} src[csr[t]] + loops[row] src[row]          then a row-local epilogue, the one thing the layers differ in
//
// An epilogue type EPI (G2Epi, RootSumEpi: each in its file) carries
//   src, ld_src, loops                          the gathered matrix, rows ld_src floats apart, and the optional stored-loop counts
//                                               (ld_src: 32 bits in G2Epi, where it is the width; 64 in RootSumEpi, a caller's stride;
//                                               ClusterGCNConv's CSRs are loop-free and its loops stays NULL)
//   pre<VEC, LPR, NS>(row, F, l)                the row-local step of EVERY row, long or not (GCN2's aux, RootSumEpi's copy)
//   finish<VEC, LPR, NS>(p, row, deg, F, l)     a lane's slabs of p -> the outputs; deg = the row's entries + loops[row]
//   finish_col(p, row, deg, F, f)               the same arithmetic for column f alone (row_sum_combine_k)
// The kernels deduce EPI from their first argument, so ROW_LAUNCH dispatches them by width like any other kernel.  Every sum has
// a fixed order: entry order inside a row, chunk order across work items.
#pragma once
#include "row_gather.h"

// acc += sum of the rows m[csr[t]], t in [beg, end), rows ld floats apart.  An index outside [0, n) raises
// GRAPES_STATUS_BAD_INDEX and the entry is dropped: its lane, like the lanes past a batch's end, points at `row` with weight 0.
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void row_sum_gather(const float* __restrict__ m, long long ld, const int32_t* __restrict__ csr, int row,
                                               int n, int beg, int end, int F, int l, float (&acc)[NS][VEC], int32_t* status) {
    for (int b = beg; b < end; b += LPR) {
        const int c = batch_entry(csr, b + l, end, n, status);
        const int idx = c < 0 ? row : c;
        const int cnt = end - b < LPR ? end - b : LPR;
        gather_batch<RowUnroll<NS>::U, VEC, LPR, NS>(
            c < 0 ? 0.f : 1.f, cnt, [&](int j, float (&hv)[NS][VEC]) { row_load_ld<VEC, LPR, NS>(m, __shfl(idx, j, LPR), ld, F, l, hv); }, acc);
    }
}

// rows longer than GRAPES_LONG_ROW (skip_long): only the row-local pre-step here, the sum by row_sum_chunks_k / row_sum_combine_k
template <int VEC, int LPR, int NS, class EPI>
__global__ __launch_bounds__(256) void row_sum_rows_k(EPI e, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                      int n_host, const int32_t* d_n, int F, int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        e.template pre<VEC, LPR, NS>(row, F, l);
        if (skip_long && end - beg > GRAPES_LONG_ROW) continue;
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        row_sum_gather<VEC, LPR, NS>(e.src, e.ld_src, csr, row, n, beg, end, F, l, acc, status);
        const int lp = e.loops ? e.loops[row] : 0;
        if (lp != 0) {
            float xr[NS][VEC];
            row_load_ld<VEC, LPR, NS>(e.src, row, e.ld_src, F, l, xr);
            slab_fma<VEC, NS>((float)lp, xr, acc);
        }
        e.template finish<VEC, LPR, NS>(acc, row, (end - beg) + lp, F, l);
    }
}

// one group per work item (row, chunk): the chunk's sum -> pacc[it F]
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void row_sum_chunks_k(const float* __restrict__ m, long long ld, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ csr, int n_host, const int32_t* d_n, int F,
                                                        const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                        int item_cap, float* __restrict__ pacc, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) row_sum_gather<VEC, LPR, NS>(m, ld, csr, row, n, beg, end, F, l, acc, status);
        row_store<VEC, LPR, NS>(pacc, it, F, l, acc);
    }
}

// one workgroup per long row (led by its chunk-0 item), a thread per column: the items added in chunk order, then the epilogue
template <class EPI>
__global__ __launch_bounds__(256) void row_sum_combine_k(EPI e, const int32_t* __restrict__ rowptr, int n_host, const int32_t* d_n,
                                                         int F, const int32_t* __restrict__ items,
                                                         const int32_t* __restrict__ d_n_items, int item_cap,
                                                         const float* __restrict__ pacc) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        const int lp = e.loops ? e.loops[row] : 0;
        const int deg = (rowptr[row + 1] - rowptr[row]) + lp;
        for (int f = threadIdx.x; f < F; f += 256) {
            float a = 0.f;
            int c = 0;
            for (; c + 4 <= nc; c += 4) {
                const float p0 = pacc[(long long)(it + c) * F + f], p1 = pacc[(long long)(it + c + 1) * F + f];
                const float p2 = pacc[(long long)(it + c + 2) * F + f], p3 = pacc[(long long)(it + c + 3) * F + f];
                a += p0; a += p1; a += p2; a += p3;
            }
            for (; c < nc; ++c) a += pacc[(long long)(it + c) * F + f];
            if (lp != 0) a = fmaf((float)lp, e.src[(long long)row * e.ld_src + f], a);
            e.finish_col(a, row, deg, F, f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host side

// the launches of a gather over (rowptr, csr): rows, and for long rows chunks + combine.  NS_WIDE: ROW_LAUNCH's, of the caller
template <int NS_WIDE, class EPI>
static int row_sum_propagate(const EPI& epi, const int32_t* rowptr, const int32_t* csr, int32_t n, const int32_t* d_n, int32_t f,
                             bool vec, const int32_t* items, const int32_t* d_n_items, int32_t item_cap, float* pacc, int32_t* status,
                             hipStream_t s) {
    const int skip = (items && d_n_items && pacc && item_cap > 0) ? 1 : 0;
    ROW_LAUNCH(row_sum_rows_k, NS_WIDE, vec, f, n, s, epi, rowptr, csr, n, d_n, f, skip, status);
    if (skip) {
        ROW_LAUNCH(row_sum_chunks_k, NS_WIDE, vec, f, item_cap, s, epi.src, epi.ld_src, rowptr, csr, n, d_n, f, items, d_n_items,
                   item_cap, pacc, status);
        const int g2 = item_cap < 2048 ? item_cap : 2048;
        hipLaunchKernelGGL(row_sum_combine_k<EPI>, dim3(g2), dim3(256), 0, s, epi, rowptr, n, d_n, f, items, d_n_items, item_cap,
                           (const float*)pacc);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}
