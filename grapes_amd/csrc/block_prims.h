// Wavefront and workgroup scans, the sum of per-workgroup totals and the searches every kernel file needs (included from common.h,
// after lane_id and lds_barrier).  One copy of each; a new kernel includes this instead of writing its own.
//
// Which scan when:
//   block_scan_1b<NW>     in a kernel on the captured step's path that scans several times between global stores: ONE LDS-only
//                         barrier per scan, but every scan in flight needs its own NW-int buffer and NW is a compile-time constant
//   block_excl_scan       anywhere else: any blockDim.x (a multiple of 64, <= 1024), one 17-int buffer that back-to-back calls share
//   block_excl_scan3      three counts per thread on block_excl_scan's three barriers (51 ints)
//   block_excl_scan_u64   two 32-bit counts packed in one 64-bit value, or a 64-bit sum (17 64-bit words)
// The inclusive value is the exclusive one plus the thread's own v.  Everything here is integer arithmetic: results do not depend
// on the order of the additions.
#pragma once

// Inclusive scan over the wavefront on the DPP network (no LDS crossbar round trips: the ds_bpermute form of the same scan
// cost six dependent ~100-cycle hops).  Rows of 16 lanes scan with row_shr 1/2/4/8 (lanes without a source add 0), then
// lane 15 of row 0 / 2 is added to row 1 / 3 (row_bcast:15) and lane 31 to rows 2 and 3 (row_bcast:31).  No LDS, no barrier.
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}
// The same over 64-bit values, of the first W lanes (W = 16: the wavefront totals of a workgroup).  No LDS, no barrier.
template <int W = 64>
__device__ __forceinline__ unsigned long long wave_incl_scan64(unsigned long long v) {
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
        const unsigned long long t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive scan over the block (blockDim.x a multiple of 64, <= 1024).  `lds` needs 17 ints.
// Returns the exclusive prefix of v for this thread; *total = block sum.  Contains THREE __syncthreads — the first in front of
// the first LDS write, so it may be called back to back on the same buffer; every thread of the block must call it.
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int* total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    int incl = wave_incl_scan(v);
    __syncthreads();  // protect lds reuse across consecutive calls
    if (lane == 63) lds[wid] = incl;
    __syncthreads();
    if (wid == 0) {
        int x = (lane < nw) ? lds[lane] : 0;
        int xs = wave_incl_scan(x);
        if (lane < nw) lds[lane] = xs - x;
        if (lane == nw - 1) lds[16] = xs;
    }
    __syncthreads();
    int base = lds[wid];
    *total = lds[16];
    return base + incl - v;
}

// Three exclusive scans at once (the same three barriers as one): a, b, c -> their exclusive prefixes; *ta / *tb / *tc the block sums.
// `lds` needs 51 ints; back-to-back calls on it are fine, as for block_excl_scan.
__device__ __forceinline__ void block_excl_scan3(int& a, int& b, int& c, int* lds, int* ta, int* tb, int* tc) {
    const int lane = lane_id(), wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const int ia = wave_incl_scan(a), ib = wave_incl_scan(b), ic = wave_incl_scan(c);
    __syncthreads();  // protect lds reuse across consecutive calls
    if (lane == 63) { lds[wid] = ia; lds[17 + wid] = ib; lds[34 + wid] = ic; }
    __syncthreads();
    if (wid == 0) {
        const int xa = (lane < nw) ? lds[lane] : 0, xb = (lane < nw) ? lds[17 + lane] : 0, xc = (lane < nw) ? lds[34 + lane] : 0;
        const int sa = wave_incl_scan(xa), sb = wave_incl_scan(xb), sc = wave_incl_scan(xc);
        if (lane < nw) { lds[lane] = sa - xa; lds[17 + lane] = sb - xb; lds[34 + lane] = sc - xc; }
        if (lane == nw - 1) { lds[16] = sa; lds[33] = sb; lds[50] = sc; }
    }
    __syncthreads();
    *ta = lds[16]; *tb = lds[33]; *tc = lds[50];
    a = lds[wid] + ia - a; b = lds[17 + wid] + ib - b; c = lds[34 + wid] + ic - c;
}

// Exclusive scan over a workgroup of NW wavefronts on ONE barrier, and that one LDS-only (lds_barrier: __syncthreads would wait
// for every store / atomic in flight).  `buf` needs NW ints and must NOT be in use by a scan that some wavefront may still be
// reading: no barrier protects it, so two scans without another barrier between them take two buffers.
template <int NW>
__device__ __forceinline__ int block_scan_1b(int v, int* buf, int* total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) buf[wid] = incl;
    lds_barrier();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const int x = buf[w]; tot += x; base += w < wid ? x : 0; }
    *total = tot;
    return base + incl - v;
}

// block_excl_scan for a 64-bit value (two counts packed 32 + 32 whose sums stay inside their fields, or one 64-bit sum).  `lds`
// needs 17 64-bit words; three __syncthreads, the first in front of the first LDS write: back-to-back calls may share the buffer.
__device__ __forceinline__ unsigned long long block_excl_scan_u64(unsigned long long v, unsigned long long* lds,
                                                                  unsigned long long* total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const unsigned long long incl = wave_incl_scan64(v);
    __syncthreads();
    if (lane == 63) lds[wid] = incl;
    __syncthreads();
    if (wid == 0) {
        const unsigned long long x = lane < nw ? lds[lane] : 0ull, xs = wave_incl_scan64<16>(x);
        if (lane < nw) lds[lane] = xs - x;
        if (lane == nw - 1) lds[16] = xs;
    }
    __syncthreads();
    *total = lds[16];
    return lds[wid] + incl - v;
}

// Sum of bsum[0 .. b) — the totals of the workgroups in front of workgroup b — by the whole workgroup, returned to every thread.
// `lds`: block_excl_scan's 17 ints, and its three barriers.
__device__ __forceinline__ int block_sum_of(const int32_t* __restrict__ bsum, int b, int* lds) {
    int acc = 0;
    for (int i = threadIdx.x; i < b; i += blockDim.x) acc += bsum[i];
    int tot;
    block_excl_scan(acc, lds, &tot);
    return tot;
}

// First index i in [0, n) with a[i] >= key, or n (a ascending).  One thread, log2 n dependent loads; I = the index type.  The
// key is compared in its own integer type, which must have the elements' signedness.
template <class T, class I, class K>
__device__ __forceinline__ I lower_bound(const T* __restrict__ a, I n, K key) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The largest i in [0, n) with cdf(i) <= t, where cdf(0) = 0 (never read), cdf(i) = arr[i + shift] for i >= 1, non-decreasing, and
// 0 <= t < cdf(n).  64-ary: every lane probes one position per round, so a search of n entries is ceil(log64 n) dependent loads.
// All 64 lanes of the wavefront call it with the same arguments; no LDS, no barrier.
__device__ __forceinline__ int64_t wave_search64(const int64_t* __restrict__ arr, int shift, int64_t n, int64_t t) {
    const int lane = lane_id();
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) >> 6;
        const int64_t p = lo + (int64_t)(lane + 1) * step;
        const bool le = p < hi && arr[p + shift] <= t;
        lo += (int64_t)__popcll(__ballot(le)) * step;         // cdf is monotone: the lanes with cdf(p) <= t are the first ones
        hi = min(hi, lo + step);
    }
    return lo;
}
