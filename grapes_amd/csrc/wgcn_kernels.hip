// GCNConv with edge weights (PyG 2.5 gcn_norm(edge_index, edge_weight, add_self_loops=True, improved=False,
// flow='source_to_target') + GCNConv.propagate [PyG-recall: torch_geometric 2.5.2]), forward and backward, over the CSRs
// grapes_gcn_prepare builds.  With w the weights of the input entries (r -> c), lw[i] the weight of node i's self-loop (1, or the
// weight of the LAST stored entry (i, i)), deg[c] = lw[c] + sum_{e -> c} w_e and s = deg^-1/2 (inf -> 0):
//
//   out[c] = s_c sum_{e: r -> c} w_e s_r H[r] + s_c^2 lw_c H[c] + b                                  (ReLU where the layer fuses it)
//   dH[r]  = s_r sum_{e: r -> c} w_e s_c G[c] + s_r^2 lw_r G[r]                                      G = dout gated by the ReLU
//   dw_e   = s_r s_c p_e + q_c,   p_e = G[c] . H[r],   q_i = -1/2 s_i^3 t_i,
//   t_i    = sum_{e -> i} w_e s_r p_e + sum_{e: i -> c} w_e s_c p_e + 2 s_i lw_i (G[i] . H[i])
//
//   wgcn_claim_k / _rank_k / _invert_k   the structure pass, once per edge list: slot of every input entry in both CSRs (pos_t,
//                         pos_s), their inverses (inv_t, inv_s) and loop_src.  A binary search finds the run of equal neighbour ids
//                         an entry belongs to, an integer atomic claims a place in it, and the entry's final slot is the run's
//                         start plus the number of claimed input indices below its own: duplicates sit in input order whatever
//                         order the claims arrived in.
//   wgcn_weights_k        per call: val_t / val_s (the weights in both CSR orders, read through inv_*), lw, deg in slot order, dinv
//   wgcn_rows_k           a group of LPR lanes owns a row: per batch of LPR entries every lane reads ONE column index and ONE val,
//                         the batch's rows are gathered with val * dinv[col] broadcast from the owning lane; the epilogue applies
//                         dinv[row], the self-loop term, bias and ReLU.  The backward's by-source pass is the same kernel over G.
//   wgcn_rows_dot_k       ... and, when the weight gradient is wanted, p_e = G[c] . H[r] per entry on the way: sum_src, G[i] . H[i]
//   wgcn_dst_k            by target: p_e at its slot, sum_dst
//   *_chunks_k / *_combine_k   rows longer than GRAPES_LONG_ROW: one group per work item, merged per row in chunk order
//   (grapes_colsum_launch of spmm_kernels.hip)   G and its column sums (dbias): the pass the unweighted backward uses
//   wgcn_dw_k             q and dw in input order through pos_t and loop_src
//
// The other modes of GCNConv change the rule for lw and, for one of them, drop the normalisation (the CSRs never hold a loop):
//   GRAPES_WGCN_LOOP_FILL     (add_self_loops) lw[i] = the weight of the last stored (i, i), or fill (1; improved: 2)
//   GRAPES_WGCN_LOOP_SUM      (add_self_loops=False) lw[i] = the weights of all stored (i, i) added in input order, 0 without one: the
//                             formulas above then ARE s_c sum_{e -> c} w_e s_r H[r] with loops as ordinary entries, and every stored
//                             loop of i gets s_i^2 (G[i] . H[i]) + q_i
//   GRAPES_WGCN_UNNORMALIZED  (normalize=False) lw as LOOP_SUM, no deg, no dinv: out[c] = sum_e w_e H[r] + lw_c H[c] + b,
//                             dH[r] = sum_e w_e G[c] + lw_r G[r], dw_e = p_e (a loop: G[i] . H[i]).  The *_un_k kernels: the same
//                             gathers without the dinv[col] read per entry, without the sums and without q.
//   wgcn_loop_*_k         the structure pass of the last two: every node's stored loops as a list in input order
//
// A negative degree gives NaN (as in PyG); it is not checked.  No floating-point atomics: every sum has a fixed order (slot order
// inside a row, chunk order across work items, a fixed tree across partials), so results are bit-identical from run to run.  No
// kernel waits on another workgroup.
#include "row_gather.h"

// the project's gated column sum (spmm_kernels.hip): out[c] = sum_r [gate > 0] src[r][c] in a fixed order, the gated rows -> dst
int grapes_colsum_launch(const float* src, const float* gate, const float* wrow, float* dst, float* out, int n, const int32_t* d_n,
                         int F, int accumulate, float* workspace, hipStream_t s, unsigned* ticket);
size_t grapes_colsum_workspace_bytes(int F);

enum { WG_ACC = 0, WG_ACC_DOT = 1, WG_DOT = 2 };
// the rule for lw and the normalisation: GRAPES_WGCN_LOOP_FILL / _LOOP_SUM / _UNNORMALIZED of the header
enum { WG_LOOP_FILL = GRAPES_WGCN_LOOP_FILL, WG_LOOP_SUM = GRAPES_WGCN_LOOP_SUM, WG_UNNORM = GRAPES_WGCN_UNNORMALIZED };

// Entries [beg, end) of row `row`: acc += sum_e val_e dinv[col_e] m[col_e] (MODE != WG_DOT) and, MODE != WG_ACC, the dot product
// p_e = m[col_e] . oth of every entry (stored at its slot when pslot != NULL); returns this lane's share of sum_e val_e dinv[col_e] p_e.
// An index outside [0, n) raises GRAPES_STATUS_BAD_INDEX and the entry is dropped: its lane, like the lanes past a batch's end, points
// at `row` with weight 0 (as in gather_batch, row_gather.h; the loop stays here for the group reduction inside it).
// NORM false (GRAPES_WGCN_UNNORMALIZED): the weight of an entry is val_e alone; dinv is never read and the returned share is unused.
template <int MODE, int VEC, int LPR, int NS, bool NORM = true>
__device__ __forceinline__ float wg_range(const float* __restrict__ m, const int32_t* __restrict__ csr, const float* __restrict__ val,
                                          const float* __restrict__ dinv, int row, int n, int beg, int end, int F, int l,
                                          float (&acc)[NS][VEC], const float (&oth)[NS][VEC], float* __restrict__ pslot,
                                          int32_t* status) {
    constexpr int U = RowUnroll<NS>::U;
    float part = 0.f;
    for (int b = beg; b < end; b += LPR) {
        const int c = batch_entry(csr, b + l, end, n, status);
        const int idx = c < 0 ? row : c;
        const float w = c < 0 ? 0.f : (NORM ? val[b + l] * dinv[c] : val[b + l]);
        float dot_mine = 0.f;
        const int cnt = end - b < LPR ? end - b : LPR;
        for (int k = 0; k < cnt; k += U) {                      // (lanes past cnt hold idx = row, w = 0: no predicates)
            float hv[U][NS][VEC], wk[U], d[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ik = __shfl(idx, k + u, LPR);
                wk[u] = __shfl(w, k + u, LPR);
                row_load<VEC, LPR, NS>(m, ik, F, l, hv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (MODE != WG_ACC) d[u] = slab_dot<VEC, NS>(hv[u], oth);
                if (MODE != WG_DOT) {                           // (bare, not slab_fma: see gat_bwd_src_range, gat_kernels.hip)
#pragma unroll
                    for (int s = 0; s < NS; ++s)
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[s][v] = fmaf(wk[u], hv[u][s][v], acc[s][v]);
                }
            }
            if (MODE != WG_ACC) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    d[u] = grp_sum<LPR>(d[u]);
                    if (l == k + u) dot_mine = d[u];
                }
            }
        }
        if (MODE != WG_ACC) {
            part = fmaf(w, dot_mine, part);
            if (pslot && b + l < end) pslot[b + l] = dot_mine;
        }
    }
    return part;
}

// What a row's sum becomes:  out[row] = act(dinv[row] sum + dinv[row]^2 lw[row] m[row] + bias), unnormalised act(sum + lw[row] m[row] +
// bias) with dinv NULL.  bias and out are optional.
struct WgEpi {
    const float* m;
    const float* dinv;
    const float* lw;
    const float* bias;
    float* out;
    int relu;
};

template <int VEC, int LPR, int NS, bool NORM = true>
__device__ __forceinline__ void wg_finish(const WgEpi& e, float (&acc)[NS][VEC], const float (&self)[NS][VEC], int row, int F, int l) {
    if (!e.out) return;
    const float d = NORM ? e.dinv[row] : 1.f, cs = NORM ? d * d * e.lw[row] : e.lw[row];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int f = (s * LPR + l) * VEC + v;
            float r = fmaf(cs, self[s][v], NORM ? d * acc[s][v] : acc[s][v]);
            if (e.bias && f < F) r += e.bias[f];
            acc[s][v] = e.relu ? fmaxf(r, 0.f) : r;
        }
    row_store<VEC, LPR, NS>(e.out, row, F, l, acc);
}

// MODE WG_ACC: the aggregation alone.  WG_ACC_DOT: oth_m is the other factor of the weight gradient (H when e.m is G):
// sum_out[row] = sum_e val_e dinv[col_e] (m[col_e] . oth_m[row]), gh[row] = m[row] . oth_m[row].
// Rows longer than GRAPES_LONG_ROW (skip_long): only gh here, the rest by the chunk and combine kernels.
// NORM false: WG_ACC_DOT forms gh alone (dw_e = p_e needs no sums: the entries' dots come from the by-target pass).
template <int MODE, int VEC, int LPR, int NS, bool NORM = true>
__device__ __forceinline__ void wg_rows_body(const WgEpi& e, const float* __restrict__ oth_m, const int32_t* __restrict__ rowptr,
                                             const int32_t* __restrict__ csr, const float* __restrict__ val,
                                             float* __restrict__ sum_out, float* __restrict__ gh, int n_host, const int32_t* d_n,
                                             int F, int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        const bool is_long = skip_long && end - beg > GRAPES_LONG_ROW;
        if (MODE == WG_ACC && is_long) continue;
        float self[NS][VEC], oth[NS][VEC], acc[NS][VEC];
        row_load<VEC, LPR, NS>(e.m, row, F, l, self);
        slab_zero<VEC, NS>(acc);
        slab_zero<VEC, NS>(oth);
        if (MODE == WG_ACC_DOT) {
            row_load<VEC, LPR, NS>(oth_m, row, F, l, oth);
            const float g = grp_sum<LPR>(slab_dot<VEC, NS>(self, oth));
            if (l == 0) gh[row] = g;
            if (is_long) continue;
        }
        float part = wg_range<NORM ? MODE : WG_ACC, VEC, LPR, NS, NORM>(e.m, csr, val, e.dinv, row, n, beg, end, F, l, acc, oth, nullptr,
                                                                      status);
        if (NORM && MODE == WG_ACC_DOT) {
            part = grp_sum<LPR>(part);
            if (l == 0) sum_out[row] = part;
        }
        wg_finish<VEC, LPR, NS, NORM>(e, acc, self, row, F, l);
    }
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_rows_k(WgEpi e, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                   const float* __restrict__ val, int n_host, const int32_t* d_n, int F,
                                                   int skip_long, int32_t* status) {
    wg_rows_body<WG_ACC, VEC, LPR, NS>(e, nullptr, rowptr, csr, val, nullptr, nullptr, n_host, d_n, F, skip_long, status);
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_rows_dot_k(WgEpi e, const float* __restrict__ oth_m, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ csr, const float* __restrict__ val,
                                                       float* __restrict__ sum_out, float* __restrict__ gh, int n_host,
                                                       const int32_t* d_n, int F, int skip_long, int32_t* status) {
    wg_rows_body<WG_ACC_DOT, VEC, LPR, NS>(e, oth_m, rowptr, csr, val, sum_out, gh, n_host, d_n, F, skip_long, status);
}
// the unnormalised specialisations: no dinv anywhere
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_rows_un_k(WgEpi e, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                      const float* __restrict__ val, int n_host, const int32_t* d_n, int F,
                                                      int skip_long, int32_t* status) {
    wg_rows_body<WG_ACC, VEC, LPR, NS, false>(e, nullptr, rowptr, csr, val, nullptr, nullptr, n_host, d_n, F, skip_long, status);
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_rows_gh_un_k(WgEpi e, const float* __restrict__ oth_m, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ csr, const float* __restrict__ val,
                                                         float* __restrict__ gh, int n_host, const int32_t* d_n, int F,
                                                         int skip_long, int32_t* status) {
    wg_rows_body<WG_ACC_DOT, VEC, LPR, NS, false>(e, oth_m, rowptr, csr, val, nullptr, gh, n_host, d_n, F, skip_long, status);
}

// one group per work item (row, chunk): the chunk's sum -> pacc[it F] and (WG_ACC_DOT) its share of sum_out -> psum[it]
template <int MODE, int VEC, int LPR, int NS, bool NORM = true>
__device__ __forceinline__ void wg_chunks_body(const float* __restrict__ m, const float* __restrict__ oth_m,
                                               const float* __restrict__ dinv, const int32_t* __restrict__ rowptr,
                                               const int32_t* __restrict__ csr, const float* __restrict__ val, int n_host,
                                               const int32_t* d_n, int F, const int32_t* __restrict__ items,
                                               const int32_t* __restrict__ d_n_items, int item_cap, float* __restrict__ pacc,
                                               float* __restrict__ psum, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float acc[NS][VEC], oth[NS][VEC], part = 0.f;
        slab_zero<VEC, NS>(acc);
        slab_zero<VEC, NS>(oth);
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            if (MODE == WG_ACC_DOT) row_load<VEC, LPR, NS>(oth_m, row, F, l, oth);
            part = wg_range<MODE, VEC, LPR, NS, NORM>(m, csr, val, dinv, row, n, beg, end, F, l, acc, oth, nullptr, status);
        }
        row_store<VEC, LPR, NS>(pacc, it, F, l, acc);
        if (MODE == WG_ACC_DOT) {
            part = grp_sum<LPR>(part);
            if (l == 0) psum[it] = part;
        }
    }
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_chunks_k(const float* __restrict__ m, const float* __restrict__ dinv,
                                                     const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                     const float* __restrict__ val, int n_host, const int32_t* d_n, int F,
                                                     const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                     int item_cap, float* __restrict__ pacc, int32_t* status) {
    wg_chunks_body<WG_ACC, VEC, LPR, NS>(m, nullptr, dinv, rowptr, csr, val, n_host, d_n, F, items, d_n_items, item_cap, pacc, nullptr,
                                         status);
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_chunks_dot_k(const float* __restrict__ m, const float* __restrict__ oth_m,
                                                         const float* __restrict__ dinv, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ csr, const float* __restrict__ val, int n_host,
                                                         const int32_t* d_n, int F, const int32_t* __restrict__ items,
                                                         const int32_t* __restrict__ d_n_items, int item_cap,
                                                         float* __restrict__ pacc, float* __restrict__ psum, int32_t* status) {
    wg_chunks_body<WG_ACC_DOT, VEC, LPR, NS>(m, oth_m, dinv, rowptr, csr, val, n_host, d_n, F, items, d_n_items, item_cap, pacc, psum,
                                             status);
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_chunks_un_k(const float* __restrict__ m, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ csr, const float* __restrict__ val, int n_host,
                                                        const int32_t* d_n, int F, const int32_t* __restrict__ items,
                                                        const int32_t* __restrict__ d_n_items, int item_cap, float* __restrict__ pacc,
                                                        int32_t* status) {
    wg_chunks_body<WG_ACC, VEC, LPR, NS, false>(m, nullptr, nullptr, rowptr, csr, val, n_host, d_n, F, items, d_n_items, item_cap, pacc,
                                                nullptr, status);
}

// The item with chunk 0 leads its row: its nc items are contiguous and in chunk order.  One workgroup per long row, a thread per
// column: the items added in chunk order, then the epilogue of wg_finish; psum (optional) -> sum_out[row] in the same order.
template <bool NORM>
__global__ __launch_bounds__(256) void wgcn_combine_k(WgEpi e, const int32_t* __restrict__ rowptr, int n_host, const int32_t* d_n, int F,
                                                      const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                      int item_cap, const float* __restrict__ pacc, const float* __restrict__ psum,
                                                      float* __restrict__ sum_out) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        if (psum && threadIdx.x == 0) {
            float t = 0.f;
            for (int c = 0; c < nc; ++c) t += psum[it + c];
            sum_out[row] = t;
        }
        if (!e.out) continue;
        const float d = NORM ? e.dinv[row] : 1.f, cs = NORM ? d * d * e.lw[row] : e.lw[row];
        for (int f = threadIdx.x; f < F; f += 256) {
            float a = 0.f;
            int c = 0;
            for (; c + 4 <= nc; c += 4) {
                const float p0 = pacc[(long long)(it + c) * F + f], p1 = pacc[(long long)(it + c + 1) * F + f];
                const float p2 = pacc[(long long)(it + c + 2) * F + f], p3 = pacc[(long long)(it + c + 3) * F + f];
                a += p0; a += p1; a += p2; a += p3;
            }
            for (; c < nc; ++c) a += pacc[(long long)(it + c) * F + f];
            const long long o = (long long)row * F + f;
            float r = fmaf(cs, e.m[o], NORM ? d * a : a);
            if (e.bias) r += e.bias[f];
            e.out[o] = e.relu ? fmaxf(r, 0.f) : r;
        }
    }
}

// by target: p_e = G[row] . H[col_e] at its slot, sum_dst[row] = sum_e val_e dinv[col_e] p_e (long rows: chunks + combine)
// NORM false: p_e alone (no sums: dw_e = p_e)
template <int VEC, int LPR, int NS, bool NORM>
__device__ __forceinline__ void wg_dst_body(const float* __restrict__ h, const float* __restrict__ gmat, const float* __restrict__ dinv,
                                            const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                            const float* __restrict__ val, float* __restrict__ p_slot, float* __restrict__ sum_dst,
                                            int n_host, const int32_t* d_n, int F, int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        if (skip_long && end - beg > GRAPES_LONG_ROW) continue;
        float g[NS][VEC], none[NS][VEC];
        row_load<VEC, LPR, NS>(gmat, row, F, l, g);
        slab_zero<VEC, NS>(none);
        const float mine = wg_range<WG_DOT, VEC, LPR, NS, NORM>(h, csr, val, dinv, row, n, beg, end, F, l, none, g, p_slot, status);
        if (NORM) {
            const float part = grp_sum<LPR>(mine);
            if (l == 0) sum_dst[row] = part;
        }
    }
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_dst_k(const float* __restrict__ h, const float* __restrict__ gmat,
                                                  const float* __restrict__ dinv, const int32_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ csr, const float* __restrict__ val,
                                                  float* __restrict__ p_slot, float* __restrict__ sum_dst, int n_host,
                                                  const int32_t* d_n, int F, int skip_long, int32_t* status) {
    wg_dst_body<VEC, LPR, NS, true>(h, gmat, dinv, rowptr, csr, val, p_slot, sum_dst, n_host, d_n, F, skip_long, status);
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_dst_un_k(const float* __restrict__ h, const float* __restrict__ gmat,
                                                     const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                     const float* __restrict__ val, float* __restrict__ p_slot, int n_host,
                                                     const int32_t* d_n, int F, int skip_long, int32_t* status) {
    wg_dst_body<VEC, LPR, NS, false>(h, gmat, nullptr, rowptr, csr, val, p_slot, nullptr, n_host, d_n, F, skip_long, status);
}
template <int VEC, int LPR, int NS, bool NORM>
__device__ __forceinline__ void wg_dst_chunks_body(const float* __restrict__ h, const float* __restrict__ gmat,
                                                   const float* __restrict__ dinv, const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ csr, const float* __restrict__ val,
                                                   float* __restrict__ p_slot, int n_host, const int32_t* d_n, int F,
                                                   const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                   int item_cap, float* __restrict__ psum, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float part = 0.f;
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            float g[NS][VEC], none[NS][VEC];
            row_load<VEC, LPR, NS>(gmat, row, F, l, g);
            slab_zero<VEC, NS>(none);
            part = wg_range<WG_DOT, VEC, LPR, NS, NORM>(h, csr, val, dinv, row, n, beg, end, F, l, none, g, p_slot, status);
            if (NORM) part = grp_sum<LPR>(part);
        }
        if (NORM && l == 0) psum[it] = part;
    }
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_dst_chunks_k(const float* __restrict__ h, const float* __restrict__ gmat,
                                                         const float* __restrict__ dinv, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ csr, const float* __restrict__ val,
                                                         float* __restrict__ p_slot, int n_host, const int32_t* d_n, int F,
                                                         const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                         int item_cap, float* __restrict__ psum, int32_t* status) {
    wg_dst_chunks_body<VEC, LPR, NS, true>(h, gmat, dinv, rowptr, csr, val, p_slot, n_host, d_n, F, items, d_n_items, item_cap, psum,
                                           status);
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void wgcn_dst_chunks_un_k(const float* __restrict__ h, const float* __restrict__ gmat,
                                                            const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                            const float* __restrict__ val, float* __restrict__ p_slot, int n_host,
                                                            const int32_t* d_n, int F, const int32_t* __restrict__ items,
                                                            const int32_t* __restrict__ d_n_items, int item_cap, int32_t* status) {
    wg_dst_chunks_body<VEC, LPR, NS, false>(h, gmat, nullptr, rowptr, csr, val, p_slot, n_host, d_n, F, items, d_n_items, item_cap,
                                            nullptr, status);
}
// one thread per long row: the row's chunk sums in chunk order
__global__ __launch_bounds__(256) void wgcn_dst_combine_k(const int32_t* __restrict__ rowptr, float* __restrict__ sum_dst, int n_host,
                                                          const int32_t* d_n, const int32_t* __restrict__ items,
                                                          const int32_t* __restrict__ d_n_items, int item_cap,
                                                          const float* __restrict__ psum) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x * 256 + threadIdx.x; it < n_items; it += gridDim.x * 256) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        float t = 0.f;
        for (int c = 0; c < nc; ++c) t += psum[it + c];
        sum_dst[row] = t;
    }
}

// q_i = -1/2 s_i^3 t_i (0 where s_i = 0)
__device__ __forceinline__ float wg_q(int i, const float* __restrict__ dinv, const float* __restrict__ lw,
                                      const float* __restrict__ sum_dst, const float* __restrict__ sum_src,
                                      const float* __restrict__ gh) {
    const float s = dinv[i];
    if (s == 0.f) return 0.f;
    const float t = fmaf(2.f * s * lw[i], gh[i], sum_dst[i] + sum_src[i]);
    return -0.5f * s * s * s * t;
}
// dw in input order: a stored entry s_r s_c p_e + q_c, the loop that set lw[i] s_i^2 (G[i] . H[i]) + q_i, everything else 0.
// WG_LOOP_SUM: every stored loop of i entered lw[i], so every one gets the loop term.  WG_UNNORM: dw_e = p_e, a loop G[i] . H[i]; dinv,
// lw and the sums are not read.
template <int LOOPS>
__global__ __launch_bounds__(256) void wgcn_dw_k(const int32_t* __restrict__ es, const int32_t* __restrict__ ed, int e_host,
                                                 const int32_t* d_e, const int32_t* __restrict__ pos_t,
                                                 const int32_t* __restrict__ loop_src, const float* __restrict__ p_slot,
                                                 const float* __restrict__ dinv, const float* __restrict__ lw,
                                                 const float* __restrict__ sum_dst, const float* __restrict__ sum_src,
                                                 const float* __restrict__ gh, int n_host, const int32_t* d_n,
                                                 float* __restrict__ dw) {
    const int e = eff_count(d_e, e_host), n = eff_count(d_n, n_host);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e_host; i += gridDim.x * 256) {
        float g = 0.f;
        if (i < e) {
            const int r = es[i], c = ed[i];
            if ((unsigned)r < (unsigned)n && (unsigned)c < (unsigned)n) {
                const int pt = pos_t[i];
                if (LOOPS == WG_UNNORM) {
                    if (pt >= 0) g = p_slot[pt];
                    else if (r == c) g = gh[r];
                } else if (pt >= 0) g = fmaf(dinv[r] * dinv[c], p_slot[pt], wg_q(c, dinv, lw, sum_dst, sum_src, gh));
                else if (r == c && (LOOPS == WG_LOOP_SUM || loop_src[r] == i))
                    g = fmaf(dinv[r] * dinv[r], gh[r], wg_q(r, dinv, lw, sum_dst, sum_src, gh));
            }
        }
        dw[i] = g;
    }
}

// ------------------------------------------------------------------------------------------------------------ structure pass

// The run of `key` in the ascending row [beg, end) of csr: its first slot, or -1 when the row does not hold the key.
__device__ __forceinline__ int wg_run_start(const int32_t* __restrict__ csr, int beg, int end, int key) {
    const int lo = beg + lower_bound(csr + beg, end - beg, key);
    return (lo < end && csr[lo] == key) ? lo : -1;
}
// Input entry i claims the k-th place of its run (k: the order the claims arrive in, an integer atomic).  pos[i] = the run's
// start for now; claim[start + k] = i.  A claim past the run's end (an edge list the CSR was not built from) is dropped.
__device__ __forceinline__ int wg_claim(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr, int row, int key, int i,
                                        int32_t* __restrict__ cnt, int32_t* __restrict__ claim, int32_t* status) {
    const int beg = rowptr[row], end = rowptr[row + 1];
    const int lo = wg_run_start(csr, beg, end, key);
    if (lo >= 0) {
        const int k = atomicAdd(&cnt[lo], 1);
        if (lo + k < end && csr[lo + k] == key) {
            claim[lo + k] = i;
            return lo;
        }
    }
    if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    return -1;
}
// loop_src[] is -1 and cnt_t / cnt_s are zero on entry
__global__ __launch_bounds__(256) void wgcn_claim_k(const int32_t* __restrict__ es, const int32_t* __restrict__ ed, int e_host,
                                                    const int32_t* d_e, int n_host, const int32_t* d_n,
                                                    const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ csr_src,
                                                    const int32_t* __restrict__ rowptr_s, const int32_t* __restrict__ csr_dst,
                                                    int32_t* __restrict__ pos_t, int32_t* __restrict__ pos_s,
                                                    int32_t* __restrict__ claim_t, int32_t* __restrict__ claim_s,
                                                    int32_t* __restrict__ cnt_t, int32_t* __restrict__ cnt_s,
                                                    int32_t* __restrict__ loop_src, int32_t* status) {
    const int e = eff_count(d_e, e_host), n = eff_count(d_n, n_host);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e_host; i += gridDim.x * 256) {
        int pt = -1, ps = -1;
        if (i < e) {
            const int r = es[i], c = ed[i];
            if ((unsigned)r < (unsigned)n && (unsigned)c < (unsigned)n) {
                if (r == c) atomicMax(&loop_src[r], i);            // the last stored loop in input order sets lw
                else {
                    pt = wg_claim(rowptr_t, csr_src, c, r, i, cnt_t, claim_t, status);
                    ps = wg_claim(rowptr_s, csr_dst, r, c, i, cnt_s, claim_s, status);
                }
            }
        }
        pos_t[i] = pt; pos_s[i] = ps;
    }
}
// pos[i] = its run's start + the number of the run's claimed input indices below i: duplicates in input order
__device__ __forceinline__ int wg_rank(int lo, int i, int row_end, const int32_t* __restrict__ cnt, const int32_t* __restrict__ claim) {
    if (lo < 0) return -1;
    int len = cnt[lo];
    if (len > row_end - lo) len = row_end - lo;
    int rank = 0;
    for (int k = 0; k < len; ++k) rank += claim[lo + k] < i ? 1 : 0;
    return lo + rank;
}
__global__ __launch_bounds__(256) void wgcn_rank_k(const int32_t* __restrict__ es, const int32_t* __restrict__ ed, int e_host,
                                                   const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ rowptr_s,
                                                   int32_t* __restrict__ pos_t, int32_t* __restrict__ pos_s,
                                                   const int32_t* __restrict__ claim_t, const int32_t* __restrict__ claim_s,
                                                   const int32_t* __restrict__ cnt_t, const int32_t* __restrict__ cnt_s) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e_host; i += gridDim.x * 256) {
        const int pt = pos_t[i], ps = pos_s[i];
        if (pt >= 0) pos_t[i] = wg_rank(pt, i, rowptr_t[ed[i] + 1], cnt_t, claim_t);
        if (ps >= 0) pos_s[i] = wg_rank(ps, i, rowptr_s[es[i] + 1], cnt_s, claim_s);
    }
}
__global__ __launch_bounds__(256) void wgcn_invert_k(int e_host, const int32_t* __restrict__ pos_t, const int32_t* __restrict__ pos_s,
                                                     int32_t* __restrict__ inv_t, int32_t* __restrict__ inv_s) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e_host; i += gridDim.x * 256) {
        const int pt = pos_t[i], ps = pos_s[i];
        if (pt >= 0) inv_t[pt] = i;
        if (ps >= 0) inv_s[ps] = i;
    }
}
__global__ __launch_bounds__(256) void wgcn_fill_k(int32_t* __restrict__ p, int count, int value) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) p[i] = value;
}

// The stored loops of every node as a list in input order: loop_ptr [n + 1], loop_idx [loop_ptr[n]].  Count (integer atomics: per
// node, and per block of WG_SCAN nodes), scan, claim and rank as wgcn_claim_k / _rank_k: a loop claims a place among its node's in
// the order the claims arrive, and its final place is the number of the node's claimed input indices below its own.
#define WG_SCAN 1024
// cnt[] and bsum[] are zero on entry
__global__ __launch_bounds__(256) void wgcn_loop_count_k(const int32_t* __restrict__ es, const int32_t* __restrict__ ed, int e_host,
                                                         const int32_t* d_e, int n_host, const int32_t* d_n, int32_t* __restrict__ cnt,
                                                         int32_t* __restrict__ bsum) {
    const int e = eff_count(d_e, e_host), n = eff_count(d_n, n_host);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e; i += gridDim.x * 256) {
        const int r = es[i];
        if (r == ed[i] && (unsigned)r < (unsigned)n) {
            atomicAdd(&cnt[r], 1);
            atomicAdd(&bsum[r / WG_SCAN], 1);
        }
    }
}
// workgroup b: loop_ptr of nodes [b WG_SCAN, (b + 1) WG_SCAN) = the totals of the blocks in front + the scan of its own counts;
// the last workgroup also writes loop_ptr[n_host]
__global__ __launch_bounds__(WG_SCAN) void wgcn_loop_scan_k(const int32_t* __restrict__ cnt, const int32_t* __restrict__ bsum, int n_host,
                                                            int32_t* __restrict__ loop_ptr) {
    __shared__ int lds[17];
    const int b = blockIdx.x, i = b * WG_SCAN + threadIdx.x;
    const int base = block_sum_of(bsum, b, lds);
    const int v = i < n_host ? cnt[i] : 0;
    int total;
    const int ex = block_excl_scan(v, lds, &total);
    if (i < n_host) loop_ptr[i] = base + ex;
    if (b == gridDim.x - 1 && threadIdx.x == 0) loop_ptr[n_host] = base + total;
}
// fill[] is zero on entry
__global__ __launch_bounds__(256) void wgcn_loop_claim_k(const int32_t* __restrict__ es, const int32_t* __restrict__ ed, int e_host,
                                                         const int32_t* d_e, int n_host, const int32_t* d_n,
                                                         const int32_t* __restrict__ loop_ptr, int32_t* __restrict__ fill,
                                                         int32_t* __restrict__ claim) {
    const int e = eff_count(d_e, e_host), n = eff_count(d_n, n_host);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e; i += gridDim.x * 256) {
        const int r = es[i];
        if (r == ed[i] && (unsigned)r < (unsigned)n) {
            const int lo = loop_ptr[r], k = atomicAdd(&fill[r], 1);
            if (lo + k < loop_ptr[r + 1]) claim[lo + k] = i;
        }
    }
}
__global__ __launch_bounds__(256) void wgcn_loop_rank_k(const int32_t* __restrict__ es, const int32_t* __restrict__ ed, int e_host,
                                                        const int32_t* d_e, int n_host, const int32_t* d_n,
                                                        const int32_t* __restrict__ loop_ptr, const int32_t* __restrict__ claim,
                                                        int32_t* __restrict__ loop_idx) {
    const int e = eff_count(d_e, e_host), n = eff_count(d_n, n_host);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < e; i += gridDim.x * 256) {
        const int r = es[i];
        if (r == ed[i] && (unsigned)r < (unsigned)n) {
            const int lo = loop_ptr[r], hi = loop_ptr[r + 1];
            int rank = 0;
            for (int k = lo; k < hi; ++k) rank += claim[k] < i ? 1 : 0;
            if (lo + rank < hi) loop_idx[lo + rank] = i;
        }
    }
}

// 16 lanes per node: val_t / val_s of its two rows through inv_*, lw, deg (lane j adds slots j, j + 16, ... in that order, then a
// butterfly over the lanes), dinv.  w NULL: every weight is 1.  MODE WG_LOOP_FILL: lw = the weight of the last stored loop, or fill;
// WG_LOOP_SUM: the weights of the node's stored loops added in input order (0 without one); WG_UNNORM: that, and no deg, no dinv.
template <int MODE>
__global__ __launch_bounds__(256) void wgcn_weights_k(const float* __restrict__ w, int e_host, const int32_t* __restrict__ inv_t,
                                                      const int32_t* __restrict__ inv_s, const int32_t* __restrict__ loop_src,
                                                      const int32_t* __restrict__ loop_ptr, const int32_t* __restrict__ loop_idx,
                                                      const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ rowptr_s,
                                                      int n_host, const int32_t* d_n, float fill, float* __restrict__ val_t,
                                                      float* __restrict__ val_s, float* __restrict__ lw, float* __restrict__ dinv) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x & 15;
    for (int row = blockIdx.x * 16 + (threadIdx.x >> 4); row < n; row += gridDim.x * 16) {
        float acc = 0.f;
        for (int t = rowptr_t[row] + l, end = rowptr_t[row + 1]; t < end; t += 16) {
            const int i = inv_t[t];
            const float v = (unsigned)i < (unsigned)e_host ? (w ? w[i] : 1.f) : 0.f;
            val_t[t] = v;
            acc += v;
        }
        for (int t = rowptr_s[row] + l, end = rowptr_s[row + 1]; t < end; t += 16) {
            const int i = inv_s[t];
            val_s[t] = (unsigned)i < (unsigned)e_host ? (w ? w[i] : 1.f) : 0.f;
        }
        if (MODE != WG_UNNORM) acc = grp_sum<16>(acc);
        if (l == 0) {
            float lwv;
            if (MODE == WG_LOOP_FILL) {
                const int ls = loop_src[row];
                lwv = (unsigned)ls < (unsigned)e_host ? (w ? w[ls] : 1.f) : fill;
            } else {
                lwv = 0.f;
                for (int k = loop_ptr[row], end = loop_ptr[row + 1]; k < end; ++k) {
                    const int i = loop_idx[k];
                    if ((unsigned)i < (unsigned)e_host) lwv += w ? w[i] : 1.f;
                }
            }
            lw[row] = lwv;
            if (MODE != WG_UNNORM) {
                const float d = 1.f / sqrtf(lwv + acc);
                dinv[row] = isinf(d) ? 0.f : d;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host side

static inline int wg_flat_grid(int count) {
    int g = grapes_div_up(count > 0 ? count : 1, 256);
    return g > 4096 ? 4096 : g;
}

// workspace: [cnt_t e] [cnt_s e]
extern "C" size_t grapes_wgcn_structure_workspace_bytes(int32_t e) {
    return 2 * grapes_round16((size_t)(e > 0 ? e : 0) * sizeof(int32_t)) + 16;
}

extern "C" int grapes_wgcn_structure(const int32_t* edge_src, const int32_t* edge_dst, int32_t e, const int32_t* d_e, int32_t n,
                                     const int32_t* d_n, const int32_t* rowptr_t, const int32_t* csr_src, const int32_t* rowptr_s,
                                     const int32_t* csr_dst, int32_t* pos_t, int32_t* pos_s, int32_t* inv_t, int32_t* inv_s,
                                     int32_t* loop_src, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (n < 0 || e < 0 || !rowptr_t || !rowptr_s || !loop_src) return GRAPES_EINVAL;
    if (e > 0 && (!edge_src || !edge_dst || !csr_src || !csr_dst || !pos_t || !pos_s || !inv_t || !inv_s || !workspace)) return GRAPES_EINVAL;
    if (e > 0 && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        hipLaunchKernelGGL(wgcn_fill_k, dim3(wg_flat_grid(n)), dim3(256), 0, s, loop_src, n, -1);
        GRAPES_LAUNCH_CHECK();
    }
    if (e == 0 || n == 0) return 0;
    const size_t half = grapes_round16((size_t)e * sizeof(int32_t));
    int32_t* cnt_t = (int32_t*)workspace;
    int32_t* cnt_s = (int32_t*)((char*)workspace + half);
    hipError_t err = grapes_zero_async(workspace, 2 * half, s);
    if (err != hipSuccess) return (int)err;
    const int grid = wg_flat_grid(e);
    // (inv_* hold the claims until wgcn_invert_k overwrites them; a slot no entry claims keeps -1)
    hipLaunchKernelGGL(wgcn_fill_k, dim3(grid), dim3(256), 0, s, inv_t, e, -1);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgcn_fill_k, dim3(grid), dim3(256), 0, s, inv_s, e, -1);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgcn_claim_k, dim3(grid), dim3(256), 0, s, edge_src, edge_dst, e, d_e, n, d_n, rowptr_t, csr_src, rowptr_s,
                       csr_dst, pos_t, pos_s, inv_t, inv_s, cnt_t, cnt_s, loop_src, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgcn_rank_k, dim3(grid), dim3(256), 0, s, edge_src, edge_dst, e, rowptr_t, rowptr_s, pos_t, pos_s,
                       (const int32_t*)inv_t, (const int32_t*)inv_s, (const int32_t*)cnt_t, (const int32_t*)cnt_s);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgcn_invert_k, dim3(grid), dim3(256), 0, s, e, (const int32_t*)pos_t, (const int32_t*)pos_s, inv_t, inv_s);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// workspace: [cnt n] [fill n] [bsum ceil(n / WG_SCAN)] [claim e]
struct WgLoopWs { size_t cnt, fill, bsum, claim, zero, total; };
static inline WgLoopWs wg_loop_ws(int32_t n, int32_t e) {
    const size_t N = n > 0 ? (size_t)n : 1, E = e > 0 ? (size_t)e : 1;
    WgLoopWs w;
    w.cnt = 0;
    w.fill = w.cnt + grapes_round16(N * sizeof(int32_t));
    w.bsum = w.fill + grapes_round16(N * sizeof(int32_t));
    w.claim = w.bsum + grapes_round16((size_t)grapes_div_up((int)N, WG_SCAN) * sizeof(int32_t));
    w.zero = w.claim;                                   // (the claims need no clearing: only claimed places are read)
    w.total = w.claim + grapes_round16(E * sizeof(int32_t)) + 16;
    return w;
}
extern "C" size_t grapes_wgcn_loops_workspace_bytes(int32_t n, int32_t e) { return wg_loop_ws(n, e).total; }

extern "C" int grapes_wgcn_loops(const int32_t* edge_src, const int32_t* edge_dst, int32_t e, const int32_t* d_e, int32_t n,
                                 const int32_t* d_n, int32_t* loop_ptr, int32_t* loop_idx, void* workspace, grapes_stream_t stream) {
    if (n < 0 || e < 0 || !loop_ptr || !workspace) return GRAPES_EINVAL;
    if (e > 0 && (!edge_src || !edge_dst || !loop_idx)) return GRAPES_EINVAL;
    if (!grapes_aligned16(workspace)) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const WgLoopWs w = wg_loop_ws(n, e);
    char* base = (char*)workspace;
    int32_t* cnt = (int32_t*)(base + w.cnt);
    int32_t* fill = (int32_t*)(base + w.fill);
    int32_t* bsum = (int32_t*)(base + w.bsum);
    int32_t* claim = (int32_t*)(base + w.claim);
    hipError_t err = grapes_zero_async(workspace, w.zero, s);
    if (err != hipSuccess) return (int)err;
    const int grid = wg_flat_grid(e);
    if (e > 0 && n > 0) {
        hipLaunchKernelGGL(wgcn_loop_count_k, dim3(grid), dim3(256), 0, s, edge_src, edge_dst, e, d_e, n, d_n, cnt, bsum);
        GRAPES_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(wgcn_loop_scan_k, dim3(grapes_div_up(n > 0 ? n : 1, WG_SCAN)), dim3(WG_SCAN), 0, s, (const int32_t*)cnt,
                       (const int32_t*)bsum, n, loop_ptr);
    GRAPES_LAUNCH_CHECK();
    if (e == 0 || n == 0) return 0;
    hipLaunchKernelGGL(wgcn_loop_claim_k, dim3(grid), dim3(256), 0, s, edge_src, edge_dst, e, d_e, n, d_n, (const int32_t*)loop_ptr,
                       fill, claim);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgcn_loop_rank_k, dim3(grid), dim3(256), 0, s, edge_src, edge_dst, e, d_e, n, d_n, (const int32_t*)loop_ptr,
                       (const int32_t*)claim, loop_idx);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

static int wg_weights(const float* edge_weight, int32_t e, const int32_t* inv_t, const int32_t* inv_s, const int32_t* loop_src,
                      const int32_t* loop_ptr, const int32_t* loop_idx, const int32_t* rowptr_t, const int32_t* rowptr_s, int32_t n,
                      const int32_t* d_n, int mode, float fill, float* val_t, float* val_s, float* lw, float* dinv, hipStream_t s) {
    if (n == 0) return 0;
    int grid = grapes_div_up(n, 16); if (grid > 16384) grid = 16384;
#define WG_WEIGHTS(M)                                                                                                         \
    hipLaunchKernelGGL(wgcn_weights_k<M>, dim3(grid), dim3(256), 0, s, edge_weight, e, inv_t, inv_s, loop_src, loop_ptr, loop_idx,  \
                       rowptr_t, rowptr_s, n, d_n, fill, val_t, val_s, lw, dinv)
    if (mode == WG_LOOP_FILL) WG_WEIGHTS(WG_LOOP_FILL);
    else if (mode == WG_LOOP_SUM) WG_WEIGHTS(WG_LOOP_SUM);
    else WG_WEIGHTS(WG_UNNORM);
#undef WG_WEIGHTS
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_wgcn_weights(const float* edge_weight, int32_t e, const int32_t* inv_t, const int32_t* inv_s,
                                   const int32_t* loop_src, const int32_t* loop_ptr, const int32_t* loop_idx, const int32_t* rowptr_t,
                                   const int32_t* rowptr_s, int32_t n, const int32_t* d_n, int32_t mode, float fill, float* val_t,
                                   float* val_s, float* lw, float* dinv, grapes_stream_t stream) {
    if (n < 0 || e < 0 || !rowptr_t || !rowptr_s || !lw || mode < WG_LOOP_FILL || mode > WG_UNNORM) return GRAPES_EINVAL;
    if (mode == WG_LOOP_FILL ? !loop_src : (!loop_ptr || (e > 0 && !loop_idx))) return GRAPES_EINVAL;
    if (mode != WG_UNNORM && !dinv) return GRAPES_EINVAL;
    if (e > 0 && (!inv_t || !inv_s || !val_t || !val_s)) return GRAPES_EINVAL;
    return wg_weights(edge_weight, e, inv_t, inv_s, loop_src, loop_ptr, loop_idx, rowptr_t, rowptr_s, n, d_n, mode, fill, val_t, val_s, lw,
                      dinv, (hipStream_t)stream);
}

// the launches of an aggregation over (rowptr, csr, val): rows, and for long rows chunks + combine; oth_m != NULL: with the dots
// (norm false: with gh alone)
static int wg_propagate(const WgEpi& epi, const float* oth_m, float* sum_out, float* gh, const int32_t* rowptr, const int32_t* csr,
                        const float* val, int32_t n, const int32_t* d_n, int32_t f, bool vec, const int32_t* items,
                        const int32_t* d_n_items, int32_t item_cap, float* pacc, float* psum, int32_t* status, hipStream_t s,
                        bool norm = true) {
    const int skip = (items && d_n_items && pacc && item_cap > 0) ? 1 : 0;
    const int g2 = item_cap < 2048 ? item_cap : 2048;
    if (!norm) {
        if (oth_m) ROW_LAUNCH(wgcn_rows_gh_un_k, 4, vec, f, n, s, epi, oth_m, rowptr, csr, val, gh, n, d_n, f, skip, status);
        else ROW_LAUNCH(wgcn_rows_un_k, 4, vec, f, n, s, epi, rowptr, csr, val, n, d_n, f, skip, status);
        if (skip) {
            ROW_LAUNCH(wgcn_chunks_un_k, 4, vec, f, item_cap, s, epi.m, rowptr, csr, val, n, d_n, f, items, d_n_items, item_cap, pacc,
                       status);
            hipLaunchKernelGGL(wgcn_combine_k<false>, dim3(g2), dim3(256), 0, s, epi, rowptr, n, d_n, f, items, d_n_items, item_cap,
                               (const float*)pacc, (const float*)nullptr, (float*)nullptr);
            GRAPES_LAUNCH_CHECK();
        }
        return 0;
    }
    if (oth_m) ROW_LAUNCH(wgcn_rows_dot_k, 4, vec, f, n, s, epi, oth_m, rowptr, csr, val, sum_out, gh, n, d_n, f, skip, status);
    else ROW_LAUNCH(wgcn_rows_k, 4, vec, f, n, s, epi, rowptr, csr, val, n, d_n, f, skip, status);
    if (skip) {
        if (oth_m) ROW_LAUNCH(wgcn_chunks_dot_k, 4, vec, f, item_cap, s, epi.m, oth_m, epi.dinv, rowptr, csr, val, n, d_n, f, items,
                              d_n_items, item_cap, pacc, psum, status);
        else ROW_LAUNCH(wgcn_chunks_k, 4, vec, f, item_cap, s, epi.m, epi.dinv, rowptr, csr, val, n, d_n, f, items, d_n_items, item_cap,
                        pacc, status);
        hipLaunchKernelGGL(wgcn_combine_k<true>, dim3(g2), dim3(256), 0, s, epi, rowptr, n, d_n, f, items, d_n_items, item_cap,
                           (const float*)pacc, (const float*)(oth_m ? psum : nullptr), sum_out);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}

// workspace of the forward: [pacc item_cap f]
extern "C" size_t grapes_wgcn_aggregate_workspace_bytes(int32_t item_cap, int32_t f) {
    return grapes_round16((size_t)(item_cap > 0 ? item_cap : 0) * (size_t)(f > 0 ? f : 1) * sizeof(float)) + 16;
}

static int wg_forward(const float* h, const int32_t* rowptr_t, const int32_t* csr_src, const float* val_t, const float* dinv,
                      const float* lw, const float* bias, float* out, int32_t n, const int32_t* d_n, int32_t f, int32_t relu,
                      bool norm, const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap, void* workspace,
                      int32_t* status, grapes_stream_t stream) {
    if (!h || !rowptr_t || !csr_src || !val_t || (norm && !dinv) || !lw || !out || out == h || n < 0) return GRAPES_EINVAL;
    const bool use_items = long_items && d_n_items && workspace && item_cap > 0;
    if (use_items && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(f, grapes_aligned16(h) && grapes_aligned16(out) && (!bias || grapes_aligned16(bias)));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    WgEpi epi;
    epi.m = h; epi.dinv = norm ? dinv : nullptr; epi.lw = lw; epi.bias = bias; epi.out = out; epi.relu = relu ? 1 : 0;
    return wg_propagate(epi, nullptr, nullptr, nullptr, rowptr_t, csr_src, val_t, n, d_n, f, shape == 0,
                        use_items ? long_items : nullptr, d_n_items, item_cap, (float*)workspace, nullptr, status, (hipStream_t)stream,
                        norm);
}
extern "C" int grapes_wgcn_aggregate_fwd(const float* h, const int32_t* rowptr_t, const int32_t* csr_src, const float* val_t,
                                         const float* dinv, const float* lw, const float* bias, float* out, int32_t n,
                                         const int32_t* d_n, int32_t f, int32_t relu, int32_t mode, const int32_t* long_items,
                                         const int32_t* d_n_items, int32_t item_cap, void* workspace, int32_t* status,
                                         grapes_stream_t stream) {
    if (mode < WG_LOOP_FILL || mode > WG_UNNORM) return GRAPES_EINVAL;
    return wg_forward(h, rowptr_t, csr_src, val_t, dinv, lw, bias, out, n, d_n, f, relu, mode != WG_UNNORM, long_items, d_n_items, item_cap,
                      workspace, status, stream);
}

// workspace layout of the backward: [G n f] [pacc item_cap f] [psum item_cap] [partials] [p e] [sum_src n] [sum_dst n] [gh n]
struct WgBwdWs { size_t g, pacc, psum, part, p, ssrc, sdst, gh, total; };
static inline WgBwdWs wg_bwd_ws(int32_t n, int32_t e, int32_t item_cap, int32_t f) {
    const size_t N = n > 0 ? (size_t)n : 1, E = e > 0 ? (size_t)e : 1, I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    WgBwdWs w;
    w.g = 0;
    w.pacc = w.g + grapes_round16(N * F * sizeof(float));
    w.psum = w.pacc + grapes_round16(I * F * sizeof(float));
    w.part = w.psum + grapes_round16(I * sizeof(float));
    w.p = w.part + grapes_round16(grapes_colsum_workspace_bytes(f));
    w.ssrc = w.p + grapes_round16(E * sizeof(float));
    w.sdst = w.ssrc + grapes_round16(N * sizeof(float));
    w.gh = w.sdst + grapes_round16(N * sizeof(float));
    w.total = w.gh + grapes_round16(N * sizeof(float)) + 16;
    return w;
}
extern "C" size_t grapes_wgcn_aggregate_bwd_workspace_bytes(int32_t n, int32_t e, int32_t item_cap, int32_t f) {
    return wg_bwd_ws(n, e, item_cap, f).total;
}

static int wg_backward(const float* dout, const float* relu_out, const float* h, const int32_t* edge_src, const int32_t* edge_dst,
                       int32_t e, const int32_t* d_e, const int32_t* pos_t, const int32_t* loop_src, const int32_t* rowptr_t,
                       const int32_t* csr_src, const float* val_t, const int32_t* rowptr_s, const int32_t* csr_dst, const float* val_s,
                       const float* dinv, const float* lw, float* dh, float* dbias, float* dw, int32_t n, const int32_t* d_n, int32_t f,
                       int mode, const int32_t* items_t, const int32_t* d_n_items_t, const int32_t* items_s,
                       const int32_t* d_n_items_s, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    const bool norm = mode != WG_UNNORM;
    if (!dout || !rowptr_s || !csr_dst || !val_s || (norm && !dinv) || !lw || !workspace || n < 0 || e < 0) return GRAPES_EINVAL;
    if (!dh && !dw && !dbias) return GRAPES_EINVAL;
    if (dw && (!h || !rowptr_t || !csr_src || !val_t || (mode == WG_LOOP_FILL && !loop_src) || (e > 0 && (!edge_src || !edge_dst || !pos_t))))
        return GRAPES_EINVAL;
    if (dh && (dh == dout || dh == h)) return GRAPES_EINVAL;
    if (!grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(f, grapes_aligned16(dout) && (!dh || grapes_aligned16(dh)) && (!relu_out || grapes_aligned16(relu_out)) &&
                                      (!dw || grapes_aligned16(h)));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = shape == 0;
    const WgBwdWs w = wg_bwd_ws(n, e, item_cap, f);
    char* base = (char*)workspace;
    float* gbuf = (float*)(base + w.g);
    float* pacc = (float*)(base + w.pacc);
    float* psum = (float*)(base + w.psum);
    float* part = (float*)(base + w.part);
    float* p_slot = (float*)(base + w.p);
    float* sum_src = (float*)(base + w.ssrc);
    float* sum_dst = (float*)(base + w.sdst);
    float* gh = (float*)(base + w.gh);
    const float* gmat = relu_out ? gbuf : dout;

    if (relu_out || dbias) {                 // G (written only when gated) and dbias: the unweighted backward's own pass
        const int rc = grapes_colsum_launch(dout, relu_out, nullptr, relu_out ? gbuf : nullptr, dbias, n, d_n, f, 0, part, s, nullptr);
        if (rc) return rc;
    }
    if (dh || dw) {
        // wgcn_bwd_src: the by-source pass (dH; with dw the by-source sums and G[i] . H[i])
        const bool use_s = items_s && d_n_items_s && item_cap > 0;
        WgEpi epi;
        epi.m = gmat; epi.dinv = norm ? dinv : nullptr; epi.lw = lw; epi.bias = nullptr; epi.out = dh; epi.relu = 0;
        const int rc = wg_propagate(epi, dw ? h : nullptr, sum_src, gh, rowptr_s, csr_dst, val_s, n, d_n, f, vec,
                                    use_s ? items_s : nullptr, d_n_items_s, item_cap, pacc, psum, status, s, norm);
        if (rc) return rc;
    }
    if (dw) {
        // wgcn_bwd_dst: the by-target pass (p_e at its slot, the by-target sums), then dw in input order
        const int skip_t = (items_t && d_n_items_t && item_cap > 0) ? 1 : 0;
        if (!norm) {
            ROW_LAUNCH(wgcn_dst_un_k, 4, vec, f, n, s, h, gmat, rowptr_t, csr_src, val_t, p_slot, n, d_n, f, skip_t, status);
            if (skip_t) ROW_LAUNCH(wgcn_dst_chunks_un_k, 4, vec, f, item_cap, s, h, gmat, rowptr_t, csr_src, val_t, p_slot, n, d_n, f,
                                   items_t, d_n_items_t, item_cap, status);
        } else {
            ROW_LAUNCH(wgcn_dst_k, 4, vec, f, n, s, h, gmat, dinv, rowptr_t, csr_src, val_t, p_slot, sum_dst, n, d_n, f, skip_t, status);
            if (skip_t) {
                ROW_LAUNCH(wgcn_dst_chunks_k, 4, vec, f, item_cap, s, h, gmat, dinv, rowptr_t, csr_src, val_t, p_slot, n, d_n, f, items_t,
                           d_n_items_t, item_cap, psum, status);
                int g2 = grapes_div_up(item_cap, 256); if (g2 > 2048) g2 = 2048;
                hipLaunchKernelGGL(wgcn_dst_combine_k, dim3(g2), dim3(256), 0, s, rowptr_t, sum_dst, n, d_n, items_t, d_n_items_t,
                                   item_cap, (const float*)psum);
                GRAPES_LAUNCH_CHECK();
            }
        }
        if (e > 0) {
#define WG_DW(M)                                                                                                              \
    hipLaunchKernelGGL(wgcn_dw_k<M>, dim3(wg_flat_grid(e)), dim3(256), 0, s, edge_src, edge_dst, e, d_e, pos_t, loop_src,           \
                       (const float*)p_slot, dinv, lw, (const float*)sum_dst, (const float*)sum_src, (const float*)gh, n, d_n, dw)
            if (mode == WG_LOOP_FILL) WG_DW(WG_LOOP_FILL);
            else if (mode == WG_LOOP_SUM) WG_DW(WG_LOOP_SUM);
            else WG_DW(WG_UNNORM);
#undef WG_DW
            GRAPES_LAUNCH_CHECK();
        }
    }
    return 0;
}
extern "C" int grapes_wgcn_aggregate_bwd(const float* dout, const float* relu_out, const float* h, const int32_t* edge_src,
                                         const int32_t* edge_dst, int32_t e, const int32_t* d_e, const int32_t* pos_t,
                                         const int32_t* loop_src, const int32_t* rowptr_t, const int32_t* csr_src, const float* val_t,
                                         const int32_t* rowptr_s, const int32_t* csr_dst, const float* val_s, const float* dinv,
                                         const float* lw, float* dh, float* dbias, float* dw, int32_t n, const int32_t* d_n,
                                         int32_t f, int32_t mode, const int32_t* items_t, const int32_t* d_n_items_t,
                                         const int32_t* items_s, const int32_t* d_n_items_s, int32_t item_cap, void* workspace,
                                         int32_t* status, grapes_stream_t stream) {
    if (mode < WG_LOOP_FILL || mode > WG_UNNORM) return GRAPES_EINVAL;
    return wg_backward(dout, relu_out, h, edge_src, edge_dst, e, d_e, pos_t, loop_src, rowptr_t, csr_src, val_t, rowptr_s, csr_dst, val_s,
                       dinv, lw, dh, dbias, dw, n, d_n, f, mode, items_t, d_n_items_t, items_s, d_n_items_s, item_cap, workspace, status,
                       stream);
}
