// GNNAutoScale, "GAS" [Fey, Lenssen, Weichert and Leskovec, ICML 2021; pyg_autoscale-recall: ScalableGNN, History, SubgraphLoader]:
// a cluster batch whose rows aggregate their WHOLE global neighbourhood — an in-batch neighbour by its current activation, an
// out-of-batch one by the last activation pushed into a per-level history table.  Nothing is sampled, no edge is dropped, no halo is
// materialised.  The paper and the library are recalled, not read: the rule written in include/grapes_hip.h is the contract;
// tests/gas_oracle.py reproduces every integer.
//
// The graph is the loop-free global CSR (rowptr int64[N + 1], col int32), d_u = row u's stored entries, dinv_u = (d_u + 1)^-1/2 (a
// table), P = D^-1/2 (A + I) D^-1/2.  The batch is grapes_cluster_batch's: n rows, node_idx[i] = the global id of row i.
//
// ---- the resolve (grapes_gas_resolve), once per batch, after grapes_cluster_batch with the same stamp table and serial: entry t of
// batch row i names v = col[rowptr[node_idx[i]] + t];  code = the local row of v when v is in the batch (stamp[where[v].cluster].serial
// == serial: base + where[v].position), else -1 - v.  The row-list pattern of row_list.h, two launches:
//   gas_scan_k        ONE workgroup: the batch rows' global degrees and their exclusive prefix -> rowptr_h (rowptr_h[n] = the TRUE
//                     total, whatever e_cap), the rows' 64-entry work items and their prefix -> item_off, the overflow bit, counts = 0
//   gas_codes_k       a wavefront per item = 64 consecutive entries of one row, one per lane (a hub row is cut over many
//                     wavefronts): col -> where -> stamp, the code behind rowptr_h[i] + t; nothing is written at or past e_cap
// Integer code only; the two counts are integer atomics, so two runs give the same values.
//
// ---- the aggregation (grapes_gas_aggregate_fwd), on the row-gather scaffold (row_gather.h) with the long-row pieces VR-GCN uses
// (hist_rows.h):
//
//   A[i] = dinv_u ( dinv_u H[i] + sum_{t in row i of rowptr_h} dinv_{v_t} (code_t >= 0 ? H[code_t] : Hbar[-1 - code_t]) ),  u = node_idx[i]
//
//   gas_rows_k        a group of LPR lanes owns a row and keeps ONE accumulator in registers over one walk of its codes: a batch of
//                     LPR codes is read one per lane (coalesced) with the factor dinv_v beside it; per source row the table (H or
//                     Hbar), its leading dimension and the row index are SELECTED from the code, never branched on, so the row
//                     loads of HistUnroll source rows are requested together; dinv_u once at the end
//   gas_items_k       ONE workgroup: rows with more than HIST_LONG_ROW codes are cut into chunks of that many
//   gas_chunks_k      a group per work item: the chunk's part of the walk -> pacc[item]
//   hist_combine_k    (hist_rows.h) the long row's items added in chunk order, then dinv_u
// Backward (Hbar is a constant), hist_bwd_k over the by-source CSR of the batch's INDUCED entries (grapes_gcn_prepare over the
// batch's edge list), exact for any stored multiset — the code list is not assumed to be its own transpose:
//
//   dH[j] = dinv_{v_j} ( dinv_{v_j} dA[j] + sum_{i in by-source row j} dinv_{u_i} dA[i] )
//
// No float atomics: every sum has a fixed order (code order inside a row or chunk, chunk order across items), two runs give the
// same bits.  No kernel waits on another workgroup.  A code outside [-N, n) raises GRAPES_STATUS_BAD_INDEX and is dropped; it then
// contributes 0 times row 0 of H (gather_batch, row_gather.h).
#include "hist_rows.h"
#include "row_list.h"

#define GAS_CHUNK GRAPES_LONG_ROW
#define GAS_ITEM_CAP_MAX (1 << 24)                                             // (64 item_cap threads in one grid)
#define GAS_AGG_ITEM_CAP_MAX (1 << 20)
#define GAS_BAD_CODE 0x7fffffff                                                // the code of an entry the resolve had to drop
static_assert(GAS_CHUNK == 64, "a work item of the resolve is one entry per lane");

// hdr[0] = the live work items
#define GAS_HDR 4

// ------------------------------------------------------------------------------------------------------------ the resolve

// ONE workgroup.  rowptr_h[i] = the entries of the batch rows before i (32-bit: the graph holds fewer than 2^31), rowptr_h[n] their
// total; item_off[i] = min(the items of the rows before i, item_cap), item_off[n] = hdr[0] = min(their total, item_cap).  A total
// above e_cap, or more items than item_cap, raise GRAPES_STATUS_EDGE_OVERFLOW.  A row id outside [0, N) is an empty row and raises
// GRAPES_STATUS_BAD_INDEX.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void gas_scan_k(const int64_t* __restrict__ rowptr, int N,
                                                                const int32_t* __restrict__ node_idx, int n, int e_cap, int item_cap,
                                                                int32_t* __restrict__ rowptr_h, int32_t* __restrict__ item_off,
                                                                int32_t* __restrict__ hdr, unsigned long long* __restrict__ counts,
                                                                int32_t* status) {
    __shared__ unsigned long long lds[17];
    bool bad = false;
    auto degs = [&](int i0, long long (&v)[LIST_SCAN_PER]) { list_row_degrees(rowptr, N, node_idx, i0, n, v, bad); };
    const unsigned long long total = list_scan_tiles<long long>(degs, n, 0x7fffffffull, rowptr_h, lds);
    __syncthreads();                                                           // (lds is reused by the second scan)
    bool bad2 = false;
    auto items = [&](int i0, long long (&v)[LIST_SCAN_PER]) {
        list_row_degrees(rowptr, N, node_idx, i0, n, v, bad2);
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) v[q] = (v[q] + GAS_CHUNK - 1) / GAS_CHUNK;
    };
    const unsigned long long n_items = list_scan_tiles<long long>(items, n, (unsigned long long)item_cap, item_off, lds);
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    list_scan_finish(n_items, item_cap, item_off + n, hdr, status);
    if (threadIdx.x == 0) {
        rowptr_h[n] = (int)(total < 0x7fffffffull ? total : 0x7fffffffull);
        if (total > (unsigned long long)e_cap && status) atomicOr(status, GRAPES_STATUS_EDGE_OVERFLOW);
        counts[0] = 0ull; counts[1] = 0ull;
    }
}

// A wavefront per item.  A column outside [0, N), a `where` entry outside its table (a cluster outside [0, P), a local row outside
// [0, n)) raise GRAPES_STATUS_BAD_INDEX; the entry's code is GAS_BAD_CODE, which the aggregation drops, and it is counted on neither
// side.  counts[0] += the in-batch entries, counts[1] += the out-of-batch ones (of every entry, also those past e_cap).
__global__ __launch_bounds__(256) void gas_codes_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                   const int32_t* __restrict__ node_idx, int n, const int2* __restrict__ where,
                                                   const int2* __restrict__ stamp, int P, int serial,
                                                   const int32_t* __restrict__ rowptr_h, const int32_t* __restrict__ item_off,
                                                   const int32_t* __restrict__ hdr, int e_cap, int32_t* __restrict__ code,
                                                   unsigned long long* __restrict__ counts, int32_t* status) {
    const int it = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (it >= hdr[0]) return;                                                  // (whole wavefronts leave)
    const int r = lower_bound<int32_t, int, int>(item_off, n, it + 1) - 1;     // rows without an entry own no item and are stepped over
    const int u = node_idx[r];
    if ((unsigned)u >= (unsigned)N) return;                                    // (an empty row: gas_scan_k raised the bit)
    const int64_t a = rowptr[u];
    const long long t = (long long)(it - item_off[r]) * GAS_CHUNK + lane;
    const bool in_row = t < (long long)(rowptr[u + 1] - a);
    const int v = in_row ? col[a + t] : 0;
    bool ok = in_row && (unsigned)v < (unsigned)N;
    int c = GAS_BAD_CODE;
    if (ok) {
        const int2 w = where[v];
        ok = (unsigned)w.x < (unsigned)P;
        if (ok) {
            const int2 st = stamp[w.x];
            if (st.x == serial) {
                const long long loc = (long long)st.y + w.y;
                ok = loc >= 0 && loc < n;
                if (ok) c = (int)loc;
            } else {
                c = -1 - v;
            }
        }
    }
    if (in_row && !ok && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    const long long p = (long long)rowptr_h[r] + t;
    if (in_row && p < e_cap) code[p] = c;
    const unsigned long long in_b = __ballot(ok && c >= 0), out_b = __ballot(ok && c < 0);
    if (lane == 0) {
        if (in_b) atomicAdd(&counts[0], (unsigned long long)__popcll(in_b));
        if (out_b) atomicAdd(&counts[1], (unsigned long long)__popcll(out_b));
    }
}

// hdr int32[GAS_HDR] | item_off int32[n + 1]
extern "C" size_t grapes_gas_resolve_workspace_bytes(int32_t n) {
    const size_t M = n > 0 ? (size_t)n : 1;
    return GAS_HDR * 4 + (M + 1) * 4 + 16;
}

extern "C" int grapes_gas_resolve(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* node_idx, int32_t n,
                                  const int32_t* where, const int32_t* stamp, int32_t num_parts, int32_t serial, int32_t e_cap,
                                  int32_t item_cap, int32_t* rowptr_h, int32_t* code, int64_t* counts, void* workspace, int32_t* status,
                                  grapes_stream_t stream) {
    if (num_nodes <= 0 || num_parts <= 0 || n <= 0 || serial <= 0 || e_cap <= 0 || item_cap <= 0 || item_cap > GAS_ITEM_CAP_MAX)
        return GRAPES_EINVAL;
    if (!rowptr || !col || !node_idx || !where || !stamp || !rowptr_h || !code || !counts || !workspace) return GRAPES_EINVAL;
    if (((uintptr_t)where & 7) || ((uintptr_t)stamp & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)workspace & 3)) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* hdr = (int32_t*)workspace;
    int32_t* item_off = hdr + GAS_HDR;
    unsigned long long* cnt = (unsigned long long*)counts;
    hipLaunchKernelGGL(gas_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, rowptr, num_nodes, node_idx, n, e_cap, item_cap, rowptr_h,
                       item_off, hdr, cnt, status);
    GRAPES_LAUNCH_CHECK();
    const int64_t item_threads = (int64_t)item_cap * 64;
    hipLaunchKernelGGL(gas_codes_k, dim3(grapes_div_up(item_threads, 256)), dim3(256), 0, s, rowptr, col, num_nodes, node_idx, n,
                       (const int2*)where, (const int2*)stamp, num_parts, serial, (const int32_t*)rowptr_h, (const int32_t*)item_off,
                       (const int32_t*)hdr, e_cap, code, cnt, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the aggregation

// (m = the batch's rows and rows_g = node_idx: the names hist_combine_k reads)
struct GasArgs {
    const float* h; long long ld_h;
    const float* hbar; long long ld_hbar;
    const float* dinv; int N;
    const int32_t* rows_g; int m;
    const int32_t* rowptr_h; const int32_t* code; int e;
    float* out; long long ld_out;
    const int32_t* item_off; int item_cap;
    float* pacc;
    int F;
    int32_t* status;
};

// the codes of row r: [beg, end) inside the list's e entries
__device__ __forceinline__ void gas_row_range(const GasArgs& a, int r, int& beg, int& end) {
    beg = a.rowptr_h[r]; end = a.rowptr_h[r + 1];
    end = end < a.e ? end : a.e;
    beg = beg < 0 ? 0 : (beg < end ? beg : end);
}

// acc += sum_{t in [beg, end)} dinv[v_t] (code_t >= 0 ? H[code_t] : Hbar[-1 - code_t])
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gas_walk(const GasArgs& a, int beg, int end, int l, float (&acc)[NS][VEC]) {
    for (int b = beg; b < end; b += LPR) {
        const bool live = b + l < end;
        const int c = live ? a.code[b + l] : 0;
        bool ok = live && c >= -a.N && c < a.m;
        // v: node_idx of an in-batch source (read for every lane, of row 0 where there is none), -1 - code of a halo one
        const int gl = a.rows_g[ok && c >= 0 ? c : 0];
        int gv = ok && c < 0 ? -1 - c : gl;
        ok = ok && (unsigned)gv < (unsigned)a.N;
        if (live && !ok && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
        gv = ok ? gv : 0;
        const float dv = a.dinv[gv];
        const int cc = ok ? c : 0;                              // (a dropped lane points at row 0 of H)
        const int cnt = end - b < LPR ? end - b : LPR;
        gather_batch<HistUnroll<VEC, NS>::U, VEC, LPR, NS>(
            ok ? dv : 0.f, cnt,
            [&](int j, float (&hv)[NS][VEC]) {
                const int ck = __shfl(cc, j, LPR);
                const bool in = ck >= 0;                        // selects, not branches: the U row loads leave together
                const float* base = in ? a.h : a.hbar;
                const long long ld = in ? a.ld_h : a.ld_hbar;
                const long long row = in ? ck : -1 - ck;
                row_load_ld<VEC, LPR, NS>(base, row, ld, a.F, l, hv);
            },
            acc);
    }
}

// skip_long: rows longer than HIST_LONG_ROW leave their walk to gas_chunks_k / hist_combine_k and store the self term alone
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gas_rows_k(GasArgs a, int skip_long) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int r = blockIdx.x * G + threadIdx.x / LPR; r < a.m; r += gridDim.x * G) {
        const int u = a.rows_g[r];
        float acc[NS][VEC];
        if ((unsigned)u >= (unsigned)a.N) {                                    // a row that names no node: zeros
            if (l == 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
            slab_zero<VEC, NS>(acc);
            row_store_ld<VEC, LPR, NS>(a.out, r, a.ld_out, a.F, l, acc);
            continue;
        }
        int beg, end;
        gas_row_range(a, r, beg, end);
        const float du = a.dinv[u];
        row_load_ld<VEC, LPR, NS>(a.h, r, a.ld_h, a.F, l, acc);
        slab_scale<VEC, NS>(acc, du);
        if (!(skip_long && end - beg > HIST_LONG_ROW)) {
            gas_walk<VEC, LPR, NS>(a, beg, end, l, acc);
            slab_scale<VEC, NS>(acc, du);
        }
        row_store_ld<VEC, LPR, NS>(a.out, r, a.ld_out, a.F, l, acc);
    }
}

// ONE workgroup.  item_off[r] = min(the chunks of the long rows before r, item_cap), item_off[m] = the live items; more than item_cap
// raise GRAPES_STATUS_EDGE_OVERFLOW (the rows past the capacity then lack chunks: the result is invalid).
__global__ __launch_bounds__(LIST_SCAN_THREADS) void gas_items_k(GasArgs a, int32_t* __restrict__ item_off) {
    __shared__ unsigned long long lds[17];
    auto chunks = [&](int i0, int (&v)[LIST_SCAN_PER]) {
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) {
            v[q] = 0;
            if (i0 + q < a.m) {
                int beg, end;
                gas_row_range(a, i0 + q, beg, end);
                const int d = end - beg;
                v[q] = d > HIST_LONG_ROW ? (d + HIST_LONG_ROW - 1) / HIST_LONG_ROW : 0;
            }
        }
    };
    const unsigned long long total = list_scan_tiles<int>(chunks, a.m, (unsigned long long)a.item_cap, item_off, lds);
    list_scan_finish(total, a.item_cap, item_off + a.m, nullptr, a.status);
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gas_chunks_k(GasArgs a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    const int n_items = a.item_off[a.m];
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        // the last row with item_off[r] <= it: rows without items share their successor's offset and are stepped over
        const int r = lower_bound<int32_t, int, int>(a.item_off, a.m, it + 1) - 1;
        int rb, re;
        gas_row_range(a, r, rb, re);
        const long long cb = (long long)rb + (long long)(it - a.item_off[r]) * HIST_LONG_ROW;
        const int beg = cb < re ? (int)cb : re;
        const int end = re - beg > HIST_LONG_ROW ? beg + HIST_LONG_ROW : re;
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        gas_walk<VEC, LPR, NS>(a, beg, end, l, acc);
        row_store<VEC, LPR, NS>(a.pacc, it, a.F, l, acc);
    }
}

// The backward's policy (hist_bwd_k): target i reads its own row of dA with the factor dinv of its node; every row has a self term.
struct GasBwdTarget {
    const int32_t* node_idx;
    const float* dinv;
    int N;
    __device__ __forceinline__ int row(int c, int32_t* status) const {
        if ((unsigned)node_idx[c] < (unsigned)N) return c;
        if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        return -1;
    }
    __device__ __forceinline__ float weight(int r) const { return dinv[node_idx[r]]; }
    __device__ __forceinline__ int self(int lv) const { return lv; }
};

extern "C" size_t grapes_gas_aggregate_workspace_bytes(int32_t n, int32_t item_cap, int32_t f) {
    return hist_workspace_bytes(n, item_cap, f);
}

extern "C" int grapes_gas_aggregate_fwd(const float* h, int64_t ld_h, const float* hbar, int64_t ld_hbar, const float* dinv,
                                        int32_t num_nodes, const int32_t* node_idx, int32_t n, const int32_t* rowptr_h,
                                        const int32_t* code, int32_t e, float* out, int64_t ld_out, int32_t f, int32_t item_cap,
                                        void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!h || !hbar || !dinv || !node_idx || !rowptr_h || !code || !out) return GRAPES_EINVAL;
    if (n < 1 || num_nodes < 1 || e < 0 || f < 1 || ld_h < f || ld_hbar < f || ld_out < f) return GRAPES_EINVAL;
    if (item_cap < 0 || item_cap > GAS_AGG_ITEM_CAP_MAX || (item_cap > 0 && !workspace)) return GRAPES_EINVAL;
    if (out == h || out == hbar) return GRAPES_EINVAL;
    if (item_cap > 0 && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(f, hist_vec_ok(h, ld_h) && hist_vec_ok(hbar, ld_hbar) && hist_vec_ok(out, ld_out));
    if (shape < 0) return shape;
    hipStream_t s = (hipStream_t)stream;
    GasArgs a;
    a.h = h; a.ld_h = ld_h; a.hbar = hbar; a.ld_hbar = ld_hbar; a.dinv = dinv; a.N = num_nodes; a.rows_g = node_idx; a.m = n;
    a.rowptr_h = rowptr_h; a.code = code; a.e = e; a.out = out; a.ld_out = ld_out; a.F = f; a.status = status;
    hist_carve(a, workspace, item_cap);
    const bool vec = shape == 0;
    if (item_cap > 0) {
        hipLaunchKernelGGL(gas_items_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, a, (int32_t*)workspace);
        GRAPES_LAUNCH_CHECK();
    }
    ROW_LAUNCH(gas_rows_k, 4, vec, f, n, s, a, item_cap > 0 ? 1 : 0);
    if (item_cap > 0) {
        ROW_LAUNCH(gas_chunks_k, 4, vec, f, item_cap, s, a);
        ROW_LAUNCH(hist_combine_k, 4, vec, f, n, s, a);
    }
    return 0;
}

extern "C" int grapes_gas_aggregate_bwd(const float* da, int64_t ld_da, const int32_t* node_idx, const float* dinv, int32_t num_nodes,
                                        const int32_t* rowptr_s, const int32_t* csr_dst, float* dh, int64_t ld_dh, int32_t n, int32_t f,
                                        int32_t* status, grapes_stream_t stream) {
    if (!da || !node_idx || !dinv || !rowptr_s || !csr_dst || !dh) return GRAPES_EINVAL;
    if (n < 1 || num_nodes < 1 || f < 1 || ld_da < f || ld_dh < f || dh == da) return GRAPES_EINVAL;
    const int shape = gather_shape(f, hist_vec_ok(da, ld_da) && hist_vec_ok(dh, ld_dh));
    if (shape < 0) return shape;
    HistBwdArgs a;
    a.da = da; a.ld_da = ld_da; a.node_idx = node_idx; a.dinv = dinv; a.N = num_nodes; a.rowptr_s = rowptr_s; a.csr_dst = csr_dst;
    a.dh = dh; a.ld_dh = ld_dh; a.n_local = n; a.F = f; a.status = status;
    const GasBwdTarget tgt{node_idx, dinv, num_nodes};
    ROW_LAUNCH(hist_bwd_k, 4, shape == 0, f, n, (hipStream_t)stream, a, tgt);
    return 0;
}
