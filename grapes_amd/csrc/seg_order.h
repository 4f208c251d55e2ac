// The in-segment ordering pass of an inverted index (pprgo_kernels.hip: tslot; bag_kernels.hip: trow): the scatter that fills a
// by-source segment runs on integer atomics, so the order inside a segment is whatever they gave; this pass makes every segment
// ascending.  At most 64 entries sit in a wavefront's registers (a bitonic network on shuffles, 21 steps); longer ones — a hub is in
// up to 4096 lists — are sorted by the workgroup in LDS on the network shadow_stage runs.  Nothing ranks a segment against itself
// entry by entry.  Equal values are allowed (they end up adjacent).  Integers only: two runs give the same bits.
// A kernel of SEG_ORDER_THREADS threads calls seg_order from every thread; it uses 16 644 B of LDS.
#pragma once
#include "common.h"

#define SEG_ORDER_THREADS 1024
#define SEG_ORDER_ROWS 64                // segments one workgroup looks at per trip: four per wavefront
#define SEG_ORDER_MAX 4096               // the longest segment the LDS sort holds

static inline int seg_order_grid(int n_cap) {
    const int g = grapes_div_up(n_cap > 0 ? n_cap : 1, SEG_ORDER_ROWS);
    return g > 1024 ? 1024 : g;
}

// Segment r < min(*d_n, n_cap) is val[ptr[r] .. min(ptr[r + 1], e_cap)).  A segment of more than SEG_ORDER_MAX entries raises
// GRAPES_STATUS_BAD_INDEX and stays unordered.
__device__ __forceinline__ void seg_order(const int32_t* __restrict__ ptr, const int32_t* __restrict__ d_n, int n_cap, int e_cap,
                                          int32_t* __restrict__ val, int32_t* status) {
    __shared__ int keys[SEG_ORDER_MAX];
    __shared__ int longs[SEG_ORDER_ROWS];
    __shared__ int n_long;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = *d_n < n_cap ? *d_n : n_cap;
    for (int r0 = blockIdx.x * SEG_ORDER_ROWS; r0 < n; r0 += gridDim.x * SEG_ORDER_ROWS) {   // (workgroup-uniform)
        if (tid == 0) n_long = 0;
        __syncthreads();
        for (int r = r0 + wid; r < n && r < r0 + SEG_ORDER_ROWS; r += SEG_ORDER_THREADS / 64) {
            const int beg = ptr[r], end = ptr[r + 1] < e_cap ? ptr[r + 1] : e_cap, len = end - beg;
            if (beg < 0 || len <= 1) continue;
            if (len > 64) {
                if (lane == 0) longs[atomicAdd(&n_long, 1)] = r;
                continue;
            }
            int v = lane < len ? val[beg + lane] : 0x7fffffff;
#pragma unroll
            for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
                for (int j = k >> 1; j > 0; j >>= 1) {
                    const int p = __shfl_xor(v, j, 64);
                    const bool lower = (lane & j) == 0, asc = (lane & k) == 0;
                    v = lower == asc ? (v < p ? v : p) : (v > p ? v : p);
                }
            }
            if (lane < len) val[beg + lane] = v;
        }
        __syncthreads();
        const int nl = n_long;
        for (int q = 0; q < nl; ++q) {                                          // the long segments, each by the whole workgroup
            const int r = longs[q];
            const int beg = ptr[r], end = ptr[r + 1] < e_cap ? ptr[r + 1] : e_cap, len = end - beg;
            if (len > SEG_ORDER_MAX) {                                          // (workgroup-uniform)
                if (tid == 0 && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
                continue;
            }
            int P = 1;
            while (P < len) P <<= 1;
            for (int i = tid; i < P; i += SEG_ORDER_THREADS) keys[i] = i < len ? val[beg + i] : 0x7fffffff;
            __syncthreads();
            for (int kk = 2; kk <= P; kk <<= 1) {
                for (int j = kk >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < P; i += SEG_ORDER_THREADS) {
                        const int x = i ^ j;
                        if (x > i) {
                            const int u = keys[i], w = keys[x];
                            if ((u > w) == ((i & kk) == 0)) { keys[i] = w; keys[x] = u; }
                        }
                    }
                    __syncthreads();
                }
            }
            for (int i = tid; i < len; i += SEG_ORDER_THREADS) val[beg + i] = keys[i];
            __syncthreads();                                                    // (keys is refilled by the next segment)
        }
        __syncthreads();                                                        // (n_long is reset by the next trip)
    }
}
