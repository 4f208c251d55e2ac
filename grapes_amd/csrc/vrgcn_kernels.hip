// VR-GCN [Chen, Zhu and Song, "Stochastic Training of Graph Convolutional Networks with Variance Reduction", ICML 2018]: the
// control-variate aggregation over historical activations, forward and backward, on the row-gather scaffold (row_gather.h).
//
// The graph is the loop-free global CSR (rowptr int64[N + 1], col int32), d_u = row u's stored entries, dinv_u = (d_u + 1)^-1/2 (given
// as a table), P = D^-1/2 (A + I) D^-1/2.  A batch has n_local nodes, node_idx[local id] = global id; H [n_local, f] holds the
// layer's input on local rows, Hbar [N, f] its history on GLOBAL rows.  For the m listed rows (u = rows_g[r], loc u = rows_l[r]) and
// the layer's kept entries, given as the by-target CSR grapes_gcn_prepare builds over the batch's local ids (rowptr_k, csr_k: row
// loc u holds the local ids of its k_u kept sources):
//
//   A[r] = dinv_u ( dinv_u H[loc u] + (d_u / k_u) sum_{kept v} dinv_v (H[loc v] - Hbar[v]) + sum_{every entry v of row u} dinv_v Hbar[v] )
//
//   vrgcn_rows_k      a group of LPR lanes owns a listed row and keeps ONE accumulator in registers across both walks: the kept
//                     entries (two independent row loads per entry: H by local id, Hbar by node_idx of it), the scale d_u / k_u and
//                     the exact self term, then the row's entries in the global CSR with Hbar read in place; dinv_u once at the end
//   vrgcn_items_k     ONE workgroup: rows with more than VRGCN_LONG_ROW entries are cut into chunks of VRGCN_LONG_ROW entries, the
//                     exclusive prefix of the chunk counts in list order is the row's first work item
//   vrgcn_chunks_k    a group per work item: the chunk's part of the full walk -> pacc[item]
//   hist_combine_k    (hist_rows.h) a group per listed row: a long row's items are added in chunk order to what vrgcn_rows_k left, then dinv_u
// Rows up to VRGCN_LONG_ROW entries never leave vrgcn_rows_k; without long rows (item_cap = 0) it is the only launch.
//
// Backward (Hbar is a constant), over the by-source CSR of the same preparation (rowptr_s, csr_dst: row loc v holds the local ids
// of the rows that kept v), coef[r] = (d_u / k_u) dinv_u as the forward wrote it, pos[local id] = r or -1:
//
//   dH[loc v] = dinv_v sum_{kept (u, v)} coef[pos[loc u]] dA[pos[loc u]] + dinv_v^2 dA[pos[loc v]]       (the self term for listed v)
//
//   hist_bwd_k        (hist_rows.h, VrBwdTarget) a group per local row, entries in the CSR's order
// No float atomics anywhere: every sum has a fixed order (entry order inside a row or chunk, chunk order across items), two runs
// give the same bits.  No kernel waits on another workgroup.  An index outside its table raises GRAPES_STATUS_BAD_INDEX and the
// entry is dropped; it then contributes 0 times row 0 of the table (gather_batch, row_gather.h).
#include "hist_rows.h"
#include "row_list.h"

// (the long-row threshold, the history rows in flight, the combine pass and the backward's body are hist_rows.h's: GNNAutoScale's
// aggregation shares them)
#define VRGCN_LONG_ROW HIST_LONG_ROW
#define VRGCN_SCAN_THREADS 1024
template <int VEC, int NS> using VrUnroll = HistUnroll<VEC, NS>;

struct VrArgs {
    const float* h; long long ld_h; int n_local;
    const int32_t* node_idx;
    const float* hbar; long long ld_hbar;
    const float* dinv;
    const int64_t* rowptr; const int32_t* col; int N;
    const int32_t* rows_g; const int32_t* rows_l; int m;
    const int32_t* rowptr_k; const int32_t* csr_k;
    float* out; long long ld_out;
    float* coef;
    const int32_t* item_off; int item_cap;
    float* pacc;
    int F;
    int32_t* status;
};

// acc += sum_{t in [beg, end)} dinv[v] Hbar[v], v = col[t]: the rows of the history read in place by global id
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void vr_full_walk(const VrArgs& a, long long beg, long long end, int l, float (&acc)[NS][VEC]) {
    for (long long b = beg; b < end; b += LPR) {
        int c = -1;
        if (b + l < end) {
            c = a.col[b + l];
            if ((unsigned)c >= (unsigned)a.N) {
                c = -1;
                if (a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
            }
        }
        const int idx = c < 0 ? 0 : c;                          // (a dropped lane points at row 0 of Hbar)
        const int cnt = end - b < LPR ? (int)(end - b) : LPR;
        gather_batch<VrUnroll<VEC, NS>::U, VEC, LPR, NS>(
            c < 0 ? 0.f : a.dinv[c], cnt,
            [&](int j, float (&hv)[NS][VEC]) { row_load_ld<VEC, LPR, NS>(a.hbar, __shfl(idx, j, LPR), a.ld_hbar, a.F, l, hv); }, acc);
    }
}

// acc += sum_{t in [kb, ke)} dinv[v] (H[lv] - Hbar[v]), lv = csr_k[t], v = node_idx[lv]
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void vr_kept_walk(const VrArgs& a, int kb, int ke, int l, float (&acc)[NS][VEC]) {
    for (int b = kb; b < ke; b += LPR) {
        int lv = batch_entry(a.csr_k, b + l, ke, a.n_local, a.status);
        int gv = 0;
        if (lv >= 0) {
            gv = a.node_idx[lv];
            if ((unsigned)gv >= (unsigned)a.N) {
                lv = -1;
                if (a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
            }
        }
        const int il = lv < 0 ? 0 : lv, ig = lv < 0 ? 0 : gv;   // (a dropped lane points at row 0 of H and of Hbar)
        const int cnt = ke - b < LPR ? ke - b : LPR;
        gather_batch<RowUnroll<NS>::U, VEC, LPR, NS>(
            lv < 0 ? 0.f : a.dinv[ig], cnt,
            [&](int j, float (&hv)[NS][VEC]) {
                float bv[NS][VEC];
                row_load_ld<VEC, LPR, NS>(a.h, __shfl(il, j, LPR), a.ld_h, a.F, l, hv);
                row_load_ld<VEC, LPR, NS>(a.hbar, __shfl(ig, j, LPR), a.ld_hbar, a.F, l, bv);
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) hv[s][v] -= bv[s][v];
            },
            acc);
    }
}

// skip_long: rows longer than VRGCN_LONG_ROW leave their full walk to vrgcn_chunks_k / hist_combine_k and store the sum so far
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void vrgcn_rows_k(VrArgs a, int skip_long) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int r = blockIdx.x * G + threadIdx.x / LPR; r < a.m; r += gridDim.x * G) {
        const int u = a.rows_g[r], lu = a.rows_l[r];
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        if ((unsigned)u >= (unsigned)a.N || (unsigned)lu >= (unsigned)a.n_local) {      // a row that names no node: zeros
            if (l == 0 && a.status) atomicOr(a.status, GRAPES_STATUS_BAD_INDEX);
            if (l == 0 && a.coef) a.coef[r] = 0.f;
            row_store_ld<VEC, LPR, NS>(a.out, r, a.ld_out, a.F, l, acc);
            continue;
        }
        const long long rb = a.rowptr[u], re = a.rowptr[u + 1];
        const int kb = a.rowptr_k[lu], ke = a.rowptr_k[lu + 1];
        const float du = a.dinv[u];
        vr_kept_walk<VEC, LPR, NS>(a, kb, ke, l, acc);
        const float sc = ke > kb ? (float)(re - rb) / (float)(ke - kb) : 0.f;
        if (l == 0 && a.coef) a.coef[r] = sc * du;
        float xr[NS][VEC];
        row_load_ld<VEC, LPR, NS>(a.h, lu, a.ld_h, a.F, l, xr);
        slab_scale<VEC, NS>(acc, sc);
        slab_fma<VEC, NS>(du, xr, acc);
        if (!(skip_long && re - rb > VRGCN_LONG_ROW)) {
            vr_full_walk<VEC, LPR, NS>(a, rb, re, l, acc);
            slab_scale<VEC, NS>(acc, du);
        }
        row_store_ld<VEC, LPR, NS>(a.out, r, a.ld_out, a.F, l, acc);
    }
}

// ONE workgroup.  item_off[r] = min(the chunks of the long rows listed before r, item_cap), item_off[m] = the live items; more
// than item_cap raise GRAPES_STATUS_EDGE_OVERFLOW (the rows past the capacity then lack chunks: the result is invalid).  A row that
// names no node has no chunks; vrgcn_rows_k raises its bit.
// (Its own 32-bit prefix, not row_list.h's tiled 64-bit one: on that the call measured 5 % slower at 512 rows, above the spread
// between two runs of the parent — profiles/row_list_ab.json.)
__global__ __launch_bounds__(VRGCN_SCAN_THREADS) void vrgcn_items_k(const int64_t* __restrict__ rowptr, int N,
                                                                    const int32_t* __restrict__ rows_g, int m, int item_cap,
                                                                    int32_t* __restrict__ item_off, int32_t* status) {
    __shared__ int lds[17];
    const int per = (m + VRGCN_SCAN_THREADS - 1) / VRGCN_SCAN_THREADS;
    const int lo = min((int)threadIdx.x * per, m), hi = min(lo + per, m);
    int mine = 0;
    for (int r = lo; r < hi; ++r) {
        const long long d = list_row(rowptr, N, rows_g, r, m, nullptr).deg;
        const long long nc = d > VRGCN_LONG_ROW ? (d + VRGCN_LONG_ROW - 1) / VRGCN_LONG_ROW : 0;
        const int c = nc > item_cap ? item_cap + 1 : (int)nc;                // (clamped: the prefix stays inside 32 bits)
        item_off[r + 1] = c;                                                  // (the count, until the second loop)
        mine = mine + c > item_cap + 1 ? item_cap + 1 : mine + c;
    }
    int total;
    long long run = block_excl_scan(mine, lds, &total);                       // (at most 1024 (item_cap + 1): item_cap <= 2^20 on the host)
    for (int r = lo; r < hi; ++r) {
        run += item_off[r + 1];
        item_off[r + 1] = run < item_cap ? (int)run : item_cap;
    }
    if (threadIdx.x == 0) item_off[0] = 0;
    list_scan_finish((unsigned long long)total, item_cap, nullptr, nullptr, status);
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void vrgcn_chunks_k(VrArgs a) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    const int n_items = a.item_off[a.m];
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        // the last row with item_off[r] <= it: rows without items share their successor's offset and are stepped over
        const int r = lower_bound<int32_t, int, int>(a.item_off, a.m, it + 1) - 1;
        const ListRow R = list_row(a.rowptr, a.N, a.rows_g, r, a.m, nullptr);
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        if (R.i >= 0) {
            const long long beg = R.a + (long long)(it - a.item_off[r]) * VRGCN_LONG_ROW, re = R.a + R.deg;
            const long long end = beg + VRGCN_LONG_ROW < re ? beg + VRGCN_LONG_ROW : re;
            vr_full_walk<VEC, LPR, NS>(a, beg, end, l, acc);
        }
        row_store<VEC, LPR, NS>(a.pacc, it, a.F, l, acc);
    }
}

// The backward's policy (hist_bwd_k): a target c reads row pos[c] of dA with the factor coef the forward wrote for it; a target that
// is none of the listed rows raises GRAPES_STATUS_BAD_INDEX and is dropped.
struct VrBwdTarget {
    const float* coef;
    const int32_t* pos;
    int m;
    __device__ __forceinline__ int row(int c, int32_t* status) const {
        const int r = pos[c];
        if ((unsigned)r < (unsigned)m) return r;
        if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        return -1;
    }
    __device__ __forceinline__ float weight(int r) const { return coef[r]; }
    __device__ __forceinline__ int self(int lv) const {
        const int rs = pos[lv];
        return (unsigned)rs < (unsigned)m ? rs : -1;
    }
};

// ------------------------------------------------------------------------------------------------------------ host side

#define VRGCN_ITEM_CAP_MAX (1 << 20)

extern "C" int32_t grapes_vrgcn_long_row(void) { return VRGCN_LONG_ROW; }

extern "C" size_t grapes_vrgcn_aggregate_workspace_bytes(int32_t m, int32_t item_cap, int32_t f) {
    return hist_workspace_bytes(m, item_cap, f);
}

extern "C" int grapes_vrgcn_aggregate_fwd(const float* h, int64_t ld_h, const int32_t* node_idx, int32_t n_local, const float* hbar,
                                          int64_t ld_hbar, const float* dinv, const int64_t* rowptr, const int32_t* col,
                                          int32_t num_nodes, const int32_t* rows_g, const int32_t* rows_l, int32_t m,
                                          const int32_t* rowptr_k, const int32_t* csr_k, float* out, int64_t ld_out, float* coef,
                                          int32_t f, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!h || !node_idx || !hbar || !dinv || !rowptr || !col || !rows_g || !rows_l || !rowptr_k || !csr_k || !out) return GRAPES_EINVAL;
    if (n_local < 1 || num_nodes < 1 || m < 0 || f < 1 || ld_h < f || ld_hbar < f || ld_out < f) return GRAPES_EINVAL;
    if (item_cap < 0 || item_cap > VRGCN_ITEM_CAP_MAX || (item_cap > 0 && !workspace)) return GRAPES_EINVAL;
    if (out == h || out == hbar) return GRAPES_EINVAL;
    if (item_cap > 0 && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(f, hist_vec_ok(h, ld_h) && hist_vec_ok(hbar, ld_hbar) && hist_vec_ok(out, ld_out));
    if (shape < 0) return shape;
    if (m == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    VrArgs a;
    a.h = h; a.ld_h = ld_h; a.n_local = n_local; a.node_idx = node_idx; a.hbar = hbar; a.ld_hbar = ld_hbar; a.dinv = dinv;
    a.rowptr = rowptr; a.col = col; a.N = num_nodes; a.rows_g = rows_g; a.rows_l = rows_l; a.m = m; a.rowptr_k = rowptr_k;
    a.csr_k = csr_k; a.out = out; a.ld_out = ld_out; a.coef = coef; a.F = f; a.status = status;
    hist_carve(a, workspace, item_cap);
    const bool vec = shape == 0;
    if (item_cap > 0) {
        hipLaunchKernelGGL(vrgcn_items_k, dim3(1), dim3(VRGCN_SCAN_THREADS), 0, s, rowptr, num_nodes, rows_g, m, item_cap,
                           (int32_t*)workspace, status);
        GRAPES_LAUNCH_CHECK();
    }
    ROW_LAUNCH(vrgcn_rows_k, 4, vec, f, m, s, a, item_cap > 0 ? 1 : 0);
    if (item_cap > 0) {
        ROW_LAUNCH(vrgcn_chunks_k, 4, vec, f, item_cap, s, a);
        ROW_LAUNCH(hist_combine_k, 4, vec, f, m, s, a);
    }
    return 0;
}

extern "C" int grapes_vrgcn_aggregate_bwd(const float* da, int64_t ld_da, const float* coef, const int32_t* pos,
                                          const int32_t* node_idx, const float* dinv, int32_t num_nodes, const int32_t* rowptr_s,
                                          const int32_t* csr_dst, float* dh, int64_t ld_dh, int32_t n_local, int32_t m, int32_t f,
                                          int32_t* status, grapes_stream_t stream) {
    if (!da || !coef || !pos || !node_idx || !dinv || !rowptr_s || !csr_dst || !dh) return GRAPES_EINVAL;
    if (n_local < 1 || num_nodes < 1 || m < 1 || f < 1 || ld_da < f || ld_dh < f || dh == da) return GRAPES_EINVAL;
    const int shape = gather_shape(f, hist_vec_ok(da, ld_da) && hist_vec_ok(dh, ld_dh));
    if (shape < 0) return shape;
    HistBwdArgs a;
    a.da = da; a.ld_da = ld_da; a.node_idx = node_idx; a.dinv = dinv; a.N = num_nodes; a.rowptr_s = rowptr_s; a.csr_dst = csr_dst;
    a.dh = dh; a.ld_dh = ld_dh; a.n_local = n_local; a.F = f; a.status = status;
    const VrBwdTarget tgt{coef, pos, m};
    ROW_LAUNCH(hist_bwd_k, 4, shape == 0, f, n_local, (hipStream_t)stream, a, tgt);
    return 0;
}
