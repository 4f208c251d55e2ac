// The row-list pattern of the samplers: a kernel is handed a list of rows (rows[0 .. m), live count *d_m) and turns it into a layer's
// edge list — a count per row (or per work item), ONE workgroup that turns the counts into offsets, and a wavefront per row (or item)
// that writes its kept entries behind its offset.  One copy of each piece; a new sampler includes this instead of writing its own.
//   list_row          the row of list position r: id, start, degree; an id outside [0, N) is an empty row and sets the caller's flag,
//                     so the caller decides which lane raises GRAPES_STATUS_BAD_INDEX (or passes no flag where another kernel did)
//   list_row_degrees  the same lookup for the consecutive positions of one scanning thread, its loads requested together
//   list_scan_tiles   the one-workgroup exclusive prefix, clamped to a capacity, 32- or 64-bit offsets
//   list_scan_finish  its tail: the total into its slot, *d_e, and GRAPES_STATUS_EDGE_OVERFLOW
//   wave_compact_slot the slot of a kept lane behind `base` in lane order, and base's advance
// The item of a chunked row is found with lower_bound(item_off, m, it + 1) - 1 (block_prims.h): the last row with item_off[r] <= it.
//
// Which scan when: list_scan_tiles wherever ONE workgroup of LIST_SCAN_THREADS turns a list's counts into offsets and the counts sit
// behind loads (a table, or rows -> rowptr): a thread's LIST_SCAN_PER values are requested together, so a tile costs one memory
// round trip per level of indirection: measured on layers of thousands of rows (sage_scan_k, labor_items_k, labor_scan_k; the three
// one-workgroup kernels of cluster_kernels.hip follow them).  A list
// of a few hundred values whose counts another kernel left in one table gains nothing from the tiles and measured 1 - 2 % slower on
// them: ladies_scan_k, saint_edge_scan_k and vrgcn_items_k keep a thread walking its own span, on block_excl_scan(_u64), and share
// list_scan_finish alone (profiles/row_list_ab.json).
// Integer code only: nothing here depends on the floating-point flags of the file that includes it.
#pragma once
#include "common.h"

#define LIST_SCAN_THREADS 1024
#define LIST_SCAN_PER 4               // consecutive values a thread takes from one tile
#define LIST_NO_CAP (~0ull)           // the capacity of offsets that must not be clamped

// The row of list position r: its id, the start of its entries and their number (0 for a row at or past the live count or outside [0, N)).
struct ListRow { int i; int64_t a; long long deg; };
__device__ __forceinline__ ListRow list_row(const int64_t* __restrict__ rowptr, int N, const int32_t* __restrict__ rows, int r, int live,
                                            bool* bad) {
    ListRow R; R.i = -1; R.a = 0; R.deg = 0;
    if (r >= live) return R;
    const int i = rows[r];
    if ((unsigned)i >= (unsigned)N) { if (bad) *bad = true; return R; }
    R.i = i; R.a = rowptr[i];
    const long long deg = (long long)(rowptr[i + 1] - R.a);
    R.deg = deg > 0 ? deg : 0;
    return R;
}

// list_row for the LIST_SCAN_PER consecutive positions i0 .. of one thread of list_scan_tiles: ids, then row pointers, each level
// requested together.  deg[q] = the degree (0 for none); a live id outside [0, N) sets bad.
__device__ __forceinline__ void list_row_degrees(const int64_t* __restrict__ rowptr, int N, const int32_t* __restrict__ rows, int i0,
                                                 int live, long long (&deg)[LIST_SCAN_PER], bool& bad) {
    int id[LIST_SCAN_PER];
    int64_t a[LIST_SCAN_PER], b[LIST_SCAN_PER];
#pragma unroll
    for (int q = 0; q < LIST_SCAN_PER; ++q) id[q] = i0 + q < live ? rows[i0 + q] : 0;
#pragma unroll
    for (int q = 0; q < LIST_SCAN_PER; ++q) {
        const bool ok = i0 + q < live && (unsigned)id[q] < (unsigned)N;
        bad = bad || (i0 + q < live && !ok);
        a[q] = b[q] = 0;
        if (ok) { a[q] = rowptr[id[q]]; b[q] = rowptr[id[q] + 1]; }         // (one 16-byte request: a scanning CU is bound by its requests)
    }
#pragma unroll
    for (int q = 0; q < LIST_SCAN_PER; ++q) deg[q] = b[q] > a[q] ? (long long)(b[q] - a[q]) : 0ll;
}

// The exclusive prefix of n values by ONE workgroup of LIST_SCAN_THREADS, in tiles of LIST_SCAN_THREADS * LIST_SCAN_PER values: a
// thread takes LIST_SCAN_PER consecutive values per tile — value(i0, v) fills v[q] with the value of index i0 + q (0 at or past n) and
// requests its loads together, so a wavefront's loads cover whole cache lines — then one block_excl_scan_u64 per tile with the carry of
// the tiles before.  out[i] = min(prefix, cap) for i < n (int32 or 64-bit; LIST_NO_CAP: never clamped); returns the total.  value may
// read out[i0 + q] of its own indices (an in-place scan: out is not __restrict__).  V = the values' type.  n is workgroup-uniform;
// every thread must call it.
template <class V, class T, class F>
__device__ __forceinline__ unsigned long long list_scan_tiles(F value, int n, unsigned long long cap, T* out,
                                                              unsigned long long* lds) {
    unsigned long long carry = 0ull;
    for (int tile = 0; tile < n; tile += LIST_SCAN_THREADS * LIST_SCAN_PER) {
        const int i0 = tile + (int)threadIdx.x * LIST_SCAN_PER;
        V v[LIST_SCAN_PER];
        value(i0, v);
        unsigned long long s = 0ull;
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) s += (unsigned long long)v[q];
        unsigned long long tot;
        unsigned long long run = carry + block_excl_scan_u64(s, lds, &tot);
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) {
            if (i0 + q < n) out[i0 + q] = (T)(run < cap ? run : cap);
            run += (unsigned long long)v[q];
        }
        carry += tot;
    }
    return carry;
}

// The tail of a list's scan, by thread 0: *slot (the offset behind the last value) and *d_e = min(total, cap), each when given; a
// total above cap raises GRAPES_STATUS_EDGE_OVERFLOW.
__device__ __forceinline__ void list_scan_finish(unsigned long long total, int cap, int32_t* __restrict__ slot, int32_t* __restrict__ d_e,
                                                 int32_t* status) {
    if (threadIdx.x != 0) return;
    const int t = total < (unsigned long long)cap ? (int)total : cap;
    if (slot) *slot = t;
    if (d_e) *d_e = t;
    if (total > (unsigned long long)cap && status) atomicOr(status, GRAPES_STATUS_EDGE_OVERFLOW);
}

// The kept lanes of a wavefront compacted behind `base` in lane order: returns this lane's slot (meaningful when kept) and advances
// base by the number kept.  All 64 lanes call it; the caller stores only while its slot is below its capacity.
__device__ __forceinline__ int wave_compact_slot(bool kept, int lane, int& base) {
    const unsigned long long bal = __ballot(kept);
    const int p = base + __popcll(bal & ((1ull << lane) - 1ull));
    base += __popcll(bal);
    return p;
}
