// The row-local pass that opens the backward of a plain-sum aggregation (rootsum_kernels.hip):
//   g = dout gated by relu_out > 0;  dadd = g;  gs = s_row g (rows F floats apart);  dbias = the column sums of g.
// SCALE is a small functor, scale(row) -> float (RootSumScale: none, mean or mean-plus-one).  No float atomics: the column
// sums are per-slab partials (ROW_GATE_SLAB rows each) added in a fixed order.
#pragma once
#include "common.h"

#define ROW_GATE_SLAB 128             // rows per column-sum partial

// part[slab] = the column sums of g over the slab's ROW_GATE_SLAB rows: thread (rg, column) adds the rows rg, rg + 4, ... of the slab,
// the four sums meet in rg order.  gs, dadd and part are optional.  Workgroup (x, y): 64 columns at 64 x, the slabs y, y + gridDim.y, ...
template <class SCALE>
__global__ __launch_bounds__(256) void row_gate_k(const float* __restrict__ dout, long long ld_dout, const float* __restrict__ relu_out,
                                                  long long ld_relu, SCALE scale, float* __restrict__ gs, float* __restrict__ dadd,
                                                  long long ld_dadd, float* __restrict__ part, int n_host, const int32_t* d_n, int F) {
    __shared__ float red[4][64];
    const int n = eff_count(d_n, n_host);
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, f = blockIdx.x * 64 + cl;
    const int slabs = (n_host + ROW_GATE_SLAB - 1) / ROW_GATE_SLAB;
    for (int slab = blockIdx.y; slab < slabs; slab += gridDim.y) {
        const int r0 = slab * ROW_GATE_SLAB, r1 = min(r0 + ROW_GATE_SLAB, n);
        float acc = 0.f;
        for (int row = r0 + rg; row < r1; row += 4) {
            const float sc = scale(row);
            if (f < F) {
                float g = dout[(long long)row * ld_dout + f];
                if (relu_out && !(relu_out[(long long)row * ld_relu + f] > 0.f)) g = 0.f;
                if (dadd) dadd[(long long)row * ld_dadd + f] = g;
                if (gs) gs[(long long)row * F + f] = sc * g;
                acc += g;
            }
        }
        if (part) {                                                           // (workgroup-uniform)
            red[rg][cl] = acc;
            __syncthreads();
            if (rg == 0 && f < F) part[(long long)slab * F + f] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
            __syncthreads();
        }
    }
}

// one wavefront per column: lane l adds the partials l, l + 64, ... in that order, then a butterfly over the lanes
template <int LANES = 64>
__global__ __launch_bounds__(256) void row_colsum_k(const float* __restrict__ part, int slabs, int F, float* __restrict__ dbias) {
    static_assert(LANES == 64, "one wavefront per column");
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (f >= F) return;
    float a = 0.f;
    for (int b = l; b < slabs; b += LANES) a += part[(long long)b * F + f];
    a = wave_sum(a);
    if (l == 0) dbias[f] = a;
}

// ------------------------------------------------------------------------------------------------------------ host side

static inline size_t row_gate_slabs(int32_t n) { return n > 0 ? ((size_t)n + ROW_GATE_SLAB - 1) / ROW_GATE_SLAB : 0; }

// the gate pass and, for dbias, the column sums: gs [n, f] and part [slabs, f] are the caller's workspace
template <class SCALE>
static int row_gate_launch(const float* dout, long long ld_dout, const float* relu_out, long long ld_relu, const SCALE& scale, float* gs,
                           float* dadd, long long ld_dadd, float* part, float* dbias, int32_t n, const int32_t* d_n, int32_t f,
                           hipStream_t s) {
    const int slabs = (int)row_gate_slabs(n);
    const dim3 grid(grapes_div_up(f, 64), slabs < 4096 ? slabs : 4096);
    hipLaunchKernelGGL(row_gate_k<SCALE>, grid, dim3(256), 0, s, dout, ld_dout, relu_out, ld_relu, scale, gs, dadd, ld_dadd,
                       dbias ? part : (float*)nullptr, n, d_n, f);
    GRAPES_LAUNCH_CHECK();
    if (dbias) {
        hipLaunchKernelGGL(row_colsum_k<64>, dim3(grapes_div_up(f, 4)), dim3(256), 0, s, (const float*)part, slabs, f, dbias);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}
