// GATConv aggregation (reference modules/gcn.py:45-72: GATConv(in, out) with PyG's defaults — one head, LeakyReLU slope 0.2,
// self-loops re-added, no attention dropout), forward and backward, over the CSRs grapes_gcn_prepare builds.
//
//   e_ij = LeakyReLU(s_src[j] + s_dst[i])    alpha_ij = softmax_j e_ij over {j -> i} + the unit self-loop (i, i)
//   out_i = sum_j alpha_ij H_j + b
//
//   gat_scores_k          s_src = H a_src, s_dst = H a_dst: a group of lanes per row, both dot products from one read of the row
//   gat_fwd_k             a group of LPR lanes (half a wavefront or a whole one) owns a destination row; ONE pass with an online
//                         softmax: per batch of LPR edges every lane scores ONE edge (one exp per edge, not per lane), the batch
//                         maximum and sum are butterfly reductions, then the batch's rows of H are gathered with the weights
//                         broadcast from the lanes that own them.  Epilogue: 1 / sum, bias, ReLU; row_ms[i] = (max, log sum).
//   gat_fwd_chunks_k      rows longer than GRAPES_LONG_ROW: one group per work item (64 consecutive entries) -> (max, sum, acc)
//   gat_fwd_combine_k     ... merged per row in chunk order against the row's global maximum, with the self-loop
//   gat_bwd_rows_k        G = dout (ReLU-gated), c_i = G_i . (out_i - b), row_q[i] = (s_dst, max, log sum, c)
//   gat_bwd_dst_k         by target: ds_dst[i] = sum_j g_ij        (+ _chunks_k / _combine_k for long rows)
//   gat_bwd_src_k         by source: dH_j = sum_i alpha_ij G_i + ds_src[j] a_src + ds_dst[j] a_dst, ds_src[j] = sum_i g_ij
//   gat_bwd_params_k      per-workgroup partial column sums of G, ds_src H, ds_dst H; gat_bwd_params_final_k adds them in a fixed tree
//
// with g_ij = alpha_ij (G_i . H_j - c_i) slope_ij.  alpha is never stored per edge: both backward passes recompute it from the
// two scores and row_ms, which is what lets each of them walk its own CSR without an edge permutation between the two orders.
// No floating-point atomics: every sum has a fixed order (butterflies inside a group, chunk order across work items, a fixed
// tree across partials), so results are bit-identical from run to run.  No kernel waits on another workgroup.
#include "row_gather.h"

#define GAT_SLOPE 0.2f
#define GAT_PARAM_BLOCKS 512

__device__ __forceinline__ float gat_leaky(float x) { return x > 0.f ? x : GAT_SLOPE * x; }

// online softmax + weighted gather over entries [beg - with_self, end) of row `row`: (m, sum, acc) are updated in place
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gat_fwd_range(const float* __restrict__ h, const float* __restrict__ s_src,
                                              const int32_t* __restrict__ csr, int row, int n, float sd, int beg, int end,
                                              bool with_self, int F, int l, float& m, float& sum, float (&acc)[NS][VEC],
                                              int32_t* status) {
    for (int b = with_self ? beg - 1 : beg; b < end; b += LPR) {
        int idx;                                               // (a dropped lane points at `row`)
        const bool ok = gat_entry(csr, b + l, beg, end, row, n, idx, status);
        const float e = ok ? gat_leaky(s_src[idx] + sd) : -INFINITY;
        const float mn = fmaxf(m, grp_max<LPR>(e));
        if (mn == -INFINITY) continue;                         // (every entry of the batch was dropped; uniform over the group)
        const float sc = m == -INFINITY ? 0.f : expf(m - mn);
        const float p = ok ? expf(e - mn) : 0.f;
        sum = fmaf(sum, sc, grp_sum<LPR>(p));
        m = mn;
        slab_scale<VEC, NS>(acc, sc);
        const int cnt = end - b < LPR ? end - b : LPR;
        gather_batch<RowUnroll<NS>::U, VEC, LPR, NS>(
            p, cnt, [&](int j, float (&hv)[NS][VEC]) { row_load<VEC, LPR, NS>(h, __shfl(idx, j, LPR), F, l, hv); }, acc);
    }
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_fwd_k(const float* __restrict__ h, const float* __restrict__ s_src,
                                                 const float* __restrict__ s_dst, const int32_t* __restrict__ rowptr,
                                                 const int32_t* __restrict__ csr, const float* __restrict__ bias,
                                                 float* __restrict__ out, float* __restrict__ row_ms, int n_host,
                                                 const int32_t* d_n, int F, int relu, int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        if (skip_long && end - beg > GRAPES_LONG_ROW) continue;          // gat_fwd_chunks_k + gat_fwd_combine_k
        float m = -INFINITY, sum = 0.f, acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        gat_fwd_range<VEC, LPR, NS>(h, s_src, csr, row, n, s_dst[row], beg, end, true, F, l, m, sum, acc, status);
        const float inv = 1.f / sum;                                      // (sum >= 1: the entry at the maximum contributes 1)
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const int f = (s * LPR + l) * VEC + v;
                float r = acc[s][v] * inv;
                if (bias && f < F) r += bias[f];
                acc[s][v] = relu ? fmaxf(r, 0.f) : r;
            }
        row_store<VEC, LPR, NS>(out, row, F, l, acc);
        if (l == 0) { row_ms[2 * (long long)row] = m; row_ms[2 * (long long)row + 1] = logf(sum); }
    }
}

// one group per work item (row, chunk): the chunk's (max, sum) -> pms[2 it], its unnormalised accumulator -> pacc[it F]
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_fwd_chunks_k(const float* __restrict__ h, const float* __restrict__ s_src,
                                                        const float* __restrict__ s_dst, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ csr, int n_host, const int32_t* d_n, int F,
                                                        const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                        int item_cap, float* __restrict__ pacc, float* __restrict__ pms,
                                                        int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float m = -INFINITY, sum = 0.f, acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            gat_fwd_range<VEC, LPR, NS>(h, s_src, csr, row, n, s_dst[row], beg, end, false, F, l, m, sum, acc, status);
        }
        row_store<VEC, LPR, NS>(pacc, it, F, l, acc);
        if (l == 0) { pms[2 * (long long)it] = m; pms[2 * (long long)it + 1] = sum; }
    }
}

// The item with chunk 0 leads its row: its nc items are contiguous and in chunk order.  One workgroup per row: the row's maximum
// over the chunks and the self-loop, then column f (column F = the softmax sum) = self term + sum_c exp(m_c - M) part_c[f], four
// wavefronts each over a contiguous quarter of the chunks, the quarters added in a fixed order.
__global__ __launch_bounds__(256) void gat_fwd_combine_k(const float* __restrict__ h, const float* __restrict__ s_src,
                                                         const float* __restrict__ s_dst, const int32_t* __restrict__ rowptr,
                                                         const float* __restrict__ bias, float* __restrict__ out,
                                                         float* __restrict__ row_ms, int n_host, const int32_t* d_n, int F, int relu,
                                                         const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                         int item_cap, const float* __restrict__ pacc,
                                                         const float* __restrict__ pms) {
    __shared__ float red[4], part[4][64], total;
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        const float e_self = gat_leaky(s_src[row] + s_dst[row]);
        float mx = e_self;
        for (int c = threadIdx.x; c < nc; c += 256) mx = fmaxf(mx, pms[2 * (long long)(it + c)]);
        mx = wave_max(mx);
        if (l == 0) red[g] = mx;
        __syncthreads();
        const float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const float w_self = expf(e_self - M);
        const int per = (nc + 3) >> 2;
        const int c0 = g * per < nc ? g * per : nc;
        const int c1 = c0 + per < nc ? c0 + per : nc;
        // the sum column first (its value divides every other column)
        for (int fbase = -64; fbase < F; fbase += 64) {
            const int f = fbase < 0 ? (l == 0 ? F : F + 1) : fbase + l;      // pass 0: lane 0 carries column F, the others idle
            float a = 0.f;
            if (f <= F)
                for (int c = c0; c < c1; ++c) {
                    const float mc = pms[2 * (long long)(it + c)];
                    const float w = mc == -INFINITY ? 0.f : expf(mc - M);
                    a = fmaf(w, f < F ? pacc[(long long)(it + c) * F + f] : pms[2 * (long long)(it + c) + 1], a);
                }
            part[g][l] = a;
            __syncthreads();
            if (g == 0 && f <= F) {
                const float r = fmaf(w_self, f < F ? h[(long long)row * F + f] : 1.f, ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l]);
                if (f == F) total = r;
                else {
                    float o = r / total;
                    if (bias) o += bias[f];
                    out[(long long)row * F + f] = relu ? fmaxf(o, 0.f) : o;
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) { row_ms[2 * (long long)row] = M; row_ms[2 * (long long)row + 1] = logf(total); }
        __syncthreads();
    }
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_scores_k(const float* __restrict__ h, const float* __restrict__ a_src,
                                                    const float* __restrict__ a_dst, float* __restrict__ s_src,
                                                    float* __restrict__ s_dst, int n_host, const int32_t* d_n, int F) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    float as[NS][VEC], ad[NS][VEC];
    row_load<VEC, LPR, NS>(a_src, 0, F, l, as);
    row_load<VEC, LPR, NS>(a_dst, 0, F, l, ad);
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        float hv[NS][VEC];
        row_load<VEC, LPR, NS>(h, row, F, l, hv);
        const float ss = grp_sum<LPR>(slab_dot<VEC, NS>(hv, as)), sd = grp_sum<LPR>(slab_dot<VEC, NS>(hv, ad));
        if (l == 0) { s_src[row] = ss; s_dst[row] = sd; }
    }
}

// ------------------------------------------------------------------------------------------------------------ backward

// G_i = dout_i gated by the layer's ReLU (written to gbuf only then), c_i = G_i . (out_i - b), row_q[i] = (s_dst, max, log sum, c)
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_bwd_rows_k(const float* __restrict__ dout, const float* __restrict__ out,
                                                      const float* __restrict__ bias, int relu, const float* __restrict__ s_dst,
                                                      const float* __restrict__ row_ms, float* __restrict__ gbuf,
                                                      float4* __restrict__ row_q, int n_host, const int32_t* d_n, int F) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    float bv[NS][VEC];
    if (bias) row_load<VEC, LPR, NS>(bias, 0, F, l, bv);
    else slab_zero<VEC, NS>(bv);
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        float g[NS][VEC], o[NS][VEC];
        row_load<VEC, LPR, NS>(dout, row, F, l, g);
        row_load<VEC, LPR, NS>(out, row, F, l, o);
        float c = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (relu && !(o[s][v] > 0.f)) g[s][v] = 0.f;
                c = fmaf(g[s][v], o[s][v] - bv[s][v], c);
            }
        c = grp_sum<LPR>(c);
        if (relu) row_store<VEC, LPR, NS>(gbuf, row, F, l, g);
        if (l == 0) row_q[row] = make_float4(s_dst[row], row_ms[2 * (long long)row], row_ms[2 * (long long)row + 1], c);
    }
}

// by target: this lane's share of sum_j g_ij over entries [beg - with_self, end) of row i (the caller adds the lanes up)
template <int VEC, int LPR, int NS>
__device__ __forceinline__ float gat_bwd_dst_range(const float* __restrict__ h, const float* __restrict__ s_src,
                                                   const int32_t* __restrict__ csr, int row, int n, float4 q,
                                                   const float (&g)[NS][VEC], int beg, int end, bool with_self, int F, int l,
                                                   int32_t* status) {
    constexpr int U = RowUnroll<NS>::U;
    float part = 0.f;
    for (int b = with_self ? beg - 1 : beg; b < end; b += LPR) {
        int idx;
        const bool ok = gat_entry(csr, b + l, beg, end, row, n, idx, status);
        const float raw = s_src[idx] + q.x;
        float dot_mine = 0.f;
        const int cnt = end - b < LPR ? end - b : LPR;
        for (int k = 0; k < cnt; k += U) {
            float hv[U][NS][VEC], d[U];
#pragma unroll
            for (int u = 0; u < U; ++u) row_load<VEC, LPR, NS>(h, __shfl(idx, k + u, LPR), F, l, hv[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) d[u] = slab_dot<VEC, NS>(g, hv[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = grp_sum<LPR>(d[u]);
                if (l == k + u) dot_mine = d[u];
            }
        }
        if (ok) part += expf(gat_leaky(raw) - q.y - q.z) * (dot_mine - q.w) * (raw > 0.f ? 1.f : GAT_SLOPE);
    }
    return part;
}

// rows longer than GRAPES_LONG_ROW (skip_long): only the self-loop here, the entries by gat_bwd_dst_chunks_k / _combine_k
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_bwd_dst_k(const float* __restrict__ h, const float* __restrict__ s_src,
                                                     const float* __restrict__ gmat, const float4* __restrict__ row_q,
                                                     const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                     float* __restrict__ ds_dst, int n_host, const int32_t* d_n, int F,
                                                     int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row];
        int end = rowptr[row + 1];
        if (skip_long && end - beg > GRAPES_LONG_ROW) end = beg;
        float g[NS][VEC];
        row_load<VEC, LPR, NS>(gmat, row, F, l, g);
        const float ds = grp_sum<LPR>(gat_bwd_dst_range<VEC, LPR, NS>(h, s_src, csr, row, n, row_q[row], g, beg, end, true, F, l, status));
        if (l == 0) ds_dst[row] = ds;
    }
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_bwd_dst_chunks_k(const float* __restrict__ h, const float* __restrict__ s_src,
                                                            const float* __restrict__ gmat, const float4* __restrict__ row_q,
                                                            const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                            int n_host, const int32_t* d_n, int F,
                                                            const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                            int item_cap, float* __restrict__ pds, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float ds = 0.f;
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            float g[NS][VEC];
            row_load<VEC, LPR, NS>(gmat, row, F, l, g);
            ds = grp_sum<LPR>(gat_bwd_dst_range<VEC, LPR, NS>(h, s_src, csr, row, n, row_q[row], g, beg, end, false, F, l, status));
        }
        if (l == 0) pds[it] = ds;
    }
}
// one thread per long row: ds_dst[row] (the self-loop's term) + the row's chunk sums in chunk order
__global__ __launch_bounds__(256) void gat_bwd_dst_combine_k(const int32_t* __restrict__ rowptr, float* __restrict__ ds_dst,
                                                             int n_host, const int32_t* d_n, const int32_t* __restrict__ items,
                                                             const int32_t* __restrict__ d_n_items, int item_cap,
                                                             const float* __restrict__ pds) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x * 256 + threadIdx.x; it < n_items; it += gridDim.x * 256) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        float ds = ds_dst[row];
        for (int c = 0; c < nc; ++c) ds += pds[it + c];
        ds_dst[row] = ds;
    }
}

// by source: acc += sum_i alpha_ij G_i over entries [beg - with_self, end) of row j of the by-source CSR; returns this lane's
// share of sum_i g_ij
template <int VEC, int LPR, int NS>
__device__ __forceinline__ float gat_bwd_src_range(const float* __restrict__ gmat, const float4* __restrict__ row_q,
                                                   const int32_t* __restrict__ csr, int row, int n, float ss,
                                                   const float (&hreg)[NS][VEC], int beg, int end, bool with_self, int F, int l,
                                                   float (&acc)[NS][VEC], int32_t* status) {
    constexpr int U = RowUnroll<NS>::U;
    float part = 0.f;
    for (int b = with_self ? beg - 1 : beg; b < end; b += LPR) {
        int idx;
        const bool ok = gat_entry(csr, b + l, beg, end, row, n, idx, status);
        const float4 q = row_q[idx];
        const float raw = ss + q.x;
        const float alpha = ok ? expf(gat_leaky(raw) - q.y - q.z) : 0.f;
        float dot_mine = 0.f;
        const int cnt = end - b < LPR ? end - b : LPR;
        for (int k = 0; k < cnt; k += U) {
            float gv[U][NS][VEC], d[U], ak[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ak[u] = __shfl(alpha, k + u, LPR);
                row_load<VEC, LPR, NS>(gmat, __shfl(idx, k + u, LPR), F, l, gv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = slab_dot<VEC, NS>(gv[u], hreg);
                // (bare, not slab_fma: beside the dot product the helper costs the <4, *, 1> kernels 11 - 19 VGPRs and a wave of
                // occupancy, here and in wg_range: profiles/gather_batch_resources.txt)
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[s][v] = fmaf(ak[u], gv[u][s][v], acc[s][v]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = grp_sum<LPR>(d[u]);
                if (l == k + u) dot_mine = d[u];
            }
        }
        part += alpha * (dot_mine - q.w) * (raw > 0.f ? 1.f : GAT_SLOPE);
    }
    return part;
}

// dH_j = acc + ds_src[j] a_src + ds_dst[j] a_dst
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gat_bwd_src_epilogue(float (&acc)[NS][VEC], float dss, float dsd, const float* __restrict__ a_src,
                                                     const float* __restrict__ a_dst, int F, int l) {
    float as[NS][VEC], ad[NS][VEC];
    row_load<VEC, LPR, NS>(a_src, 0, F, l, as);
    row_load<VEC, LPR, NS>(a_dst, 0, F, l, ad);
    slab_fma<VEC, NS>(dss, as, acc);
    slab_fma<VEC, NS>(dsd, ad, acc);
}

// long rows (skip_long): only the self-loop's terms, without the epilogue (gat_bwd_src_combine_k finishes them)
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_bwd_src_k(const float* __restrict__ h, const float* __restrict__ s_src,
                                                     const float* __restrict__ gmat, const float4* __restrict__ row_q,
                                                     const float* __restrict__ ds_dst, const float* __restrict__ a_src,
                                                     const float* __restrict__ a_dst, const int32_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ csr, float* __restrict__ dh,
                                                     float* __restrict__ ds_src, int n_host, const int32_t* d_n, int F,
                                                     int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row];
        int end = rowptr[row + 1];
        const bool is_long = skip_long && end - beg > GRAPES_LONG_ROW;
        if (is_long) end = beg;
        float hreg[NS][VEC], acc[NS][VEC];
        row_load<VEC, LPR, NS>(h, row, F, l, hreg);
        slab_zero<VEC, NS>(acc);
        const float ds = grp_sum<LPR>(gat_bwd_src_range<VEC, LPR, NS>(gmat, row_q, csr, row, n, s_src[row], hreg, beg, end, true, F, l, acc, status));
        if (!is_long) gat_bwd_src_epilogue<VEC, LPR, NS>(acc, ds, ds_dst[row], a_src, a_dst, F, l);
        row_store<VEC, LPR, NS>(dh, row, F, l, acc);
        if (l == 0) ds_src[row] = ds;
    }
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gat_bwd_src_chunks_k(const float* __restrict__ h, const float* __restrict__ s_src,
                                                            const float* __restrict__ gmat, const float4* __restrict__ row_q,
                                                            const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                            int n_host, const int32_t* d_n, int F,
                                                            const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                            int item_cap, float* __restrict__ pacc, float* __restrict__ pds,
                                                            int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float ds = 0.f, acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            float hreg[NS][VEC];
            row_load<VEC, LPR, NS>(h, row, F, l, hreg);
            ds = grp_sum<LPR>(gat_bwd_src_range<VEC, LPR, NS>(gmat, row_q, csr, row, n, s_src[row], hreg, beg, end, false, F, l, acc, status));
        }
        row_store<VEC, LPR, NS>(pacc, it, F, l, acc);
        if (l == 0) pds[it] = ds;
    }
}
// one workgroup per long row, a thread per column: the self-loop's terms (already in dh / ds_src) + the chunks in chunk order,
// then the epilogue
__global__ __launch_bounds__(256) void gat_bwd_src_combine_k(const int32_t* __restrict__ rowptr, const float* __restrict__ ds_dst,
                                                             const float* __restrict__ a_src, const float* __restrict__ a_dst,
                                                             float* __restrict__ dh, float* __restrict__ ds_src, int n_host,
                                                             const int32_t* d_n, int F, const int32_t* __restrict__ items,
                                                             const int32_t* __restrict__ d_n_items, int item_cap,
                                                             const float* __restrict__ pacc, const float* __restrict__ pds) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        float ds = ds_src[row];                                   // (every thread: the same sum in the same order)
        for (int c = 0; c < nc; ++c) ds += pds[it + c];
        const float dsd = ds_dst[row];
        for (int f = threadIdx.x; f < F; f += 256) {
            float a = dh[(long long)row * F + f];
            int c = 0;
            for (; c + 4 <= nc; c += 4) {
                const float p0 = pacc[(long long)(it + c) * F + f], p1 = pacc[(long long)(it + c + 1) * F + f];
                const float p2 = pacc[(long long)(it + c + 2) * F + f], p3 = pacc[(long long)(it + c + 3) * F + f];
                a += p0; a += p1; a += p2; a += p3;
            }
            for (; c < nc; ++c) a += pacc[(long long)(it + c) * F + f];
            dh[(long long)row * F + f] = fmaf(dsd, a_dst[f], fmaf(ds, a_src[f], a));
        }
        __syncthreads();                                          // (ds_src[row] is read by every thread above)
        if (threadIdx.x == 0) ds_src[row] = ds;
    }
}

// Partial column sums over a contiguous slab of rows per workgroup: part[b][0][f] = sum G[r][f], [1] = sum ds_src[r] H[r][f],
// [2] = sum ds_dst[r] H[r][f].  CW columns x 256 / CW row lanes; the row lanes are added in lane order.
__global__ __launch_bounds__(256) void gat_bwd_params_k(const float* __restrict__ gmat, const float* __restrict__ h,
                                                        const float* __restrict__ ds_src, const float* __restrict__ ds_dst,
                                                        int n_host, const int32_t* d_n, int F, int CW, float* __restrict__ part) {
    __shared__ float red[3][256];
    const int n = eff_count(d_n, n_host);
    const int per = (n + (int)gridDim.x - 1) / (int)gridDim.x;
    const long long r0 = (long long)blockIdx.x * per;
    const long long r1 = r0 + per < n ? r0 + per : n;
    const int cl = threadIdx.x % CW, rg = threadIdx.x / CW, RG = 256 / CW;
    for (int fbase = 0; fbase < F; fbase += CW) {
        const int f = fbase + cl;
        float a = 0.f, b = 0.f, c = 0.f;
        if (f < F)
            for (long long r = r0 + rg; r < r1; r += RG) {
                const float hv = h[r * F + f];
                a += gmat[r * F + f];
                b = fmaf(ds_src[r], hv, b);
                c = fmaf(ds_dst[r], hv, c);
            }
        red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
        __syncthreads();
        if (rg == 0 && f < F) {
            for (int q = 1; q < RG; ++q) { a += red[0][q * CW + cl]; b += red[1][q * CW + cl]; c += red[2][q * CW + cl]; }
            float* o = part + (long long)blockIdx.x * 3 * F;
            o[f] = a; o[F + f] = b; o[2 * F + f] = c;
        }
        __syncthreads();
    }
}
// one wavefront per output value: lane l adds partials l, l + 64, ... in that order, then a butterfly over the lanes
__global__ __launch_bounds__(256) void gat_bwd_params_final_k(const float* __restrict__ part, int blocks, int F,
                                                              float* __restrict__ dbias, float* __restrict__ da_src,
                                                              float* __restrict__ da_dst) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (t >= 3 * F) return;
    float a = 0.f;
    for (int b = l; b < blocks; b += 64) a += part[(long long)b * 3 * F + t];
    a = wave_sum(a);
    const int which = t / F, f = t - which * F;
    float* dst = which == 0 ? dbias : (which == 1 ? da_src : da_dst);
    if (dst && l == 0) dst[f] = a;
}

// ------------------------------------------------------------------------------------------------------------ host side

// 0: float4 columns, 1: scalar columns, negative: not covered
static inline int gat_shape(int f, bool aligned) {
    if (f < 1) return GRAPES_EINVAL;
    if (f % 4 == 0 && aligned) return f <= 1024 ? 0 : GRAPES_EINVAL;
    if (f <= 256) return 1;
    return f % 4 == 0 && f <= 1024 ? GRAPES_EALIGN : GRAPES_EINVAL;
}

extern "C" int grapes_gat_scores(const float* h, const float* a_src, const float* a_dst, float* s_src, float* s_dst, int32_t n,
                                 const int32_t* d_n, int32_t f, grapes_stream_t stream) {
    if (!h || !a_src || !a_dst || !s_src || !s_dst || n < 0) return GRAPES_EINVAL;
    const int shape = gat_shape(f, grapes_aligned16(h) && grapes_aligned16(a_src) && grapes_aligned16(a_dst));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = shape == 0;
    ROW_LAUNCH(gat_scores_k, 4, vec, f, n, s, h, a_src, a_dst, s_src, s_dst, n, d_n, f);
    return 0;
}

extern "C" size_t grapes_gat_aggregate_workspace_bytes(int32_t item_cap, int32_t f) {
    const size_t items = item_cap > 0 ? (size_t)item_cap : 0;
    return grapes_round16(items * (size_t)(f > 0 ? f : 1) * sizeof(float)) + grapes_round16(items * 2 * sizeof(float)) + 16;
}

extern "C" int grapes_gat_aggregate_fwd(const float* h, const float* s_src, const float* s_dst, const int32_t* rowptr_t,
                                        const int32_t* csr_src, const float* bias, float* out, float* row_ms, int32_t n,
                                        const int32_t* d_n, int32_t f, int32_t relu, const int32_t* long_items,
                                        const int32_t* d_n_items, int32_t item_cap, void* workspace, int32_t* status,
                                        grapes_stream_t stream) {
    if (!h || !s_src || !s_dst || !rowptr_t || !csr_src || !out || !row_ms || n < 0) return GRAPES_EINVAL;
    const int skip = (long_items && d_n_items && workspace && item_cap > 0) ? 1 : 0;
    if (skip && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gat_shape(f, grapes_aligned16(h) && grapes_aligned16(out) && (!bias || grapes_aligned16(bias)));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = shape == 0;
    ROW_LAUNCH(gat_fwd_k, 4, vec, f, n, s, h, s_src, s_dst, rowptr_t, csr_src, bias, out, row_ms, n,
               d_n, f, relu, skip, status);
    if (skip) {
        float* pacc = (float*)workspace;
        float* pms = (float*)((char*)workspace + grapes_round16((size_t)item_cap * f * sizeof(float)));
        ROW_LAUNCH(gat_fwd_chunks_k, 4, vec, f, item_cap, s, h, s_src, s_dst, rowptr_t, csr_src,
                   n, d_n, f, long_items, d_n_items, item_cap, pacc, pms, status);
        const int g2 = item_cap < 2048 ? item_cap : 2048;
        hipLaunchKernelGGL(gat_fwd_combine_k, dim3(g2), dim3(256), 0, s, h, s_src, s_dst, rowptr_t, bias, out, row_ms, n, d_n, f,
                           relu, long_items, d_n_items, item_cap, (const float*)pacc, (const float*)pms);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}

// workspace layout of the backward: [G n f] [row_q 4 n] [ds_src n] [ds_dst n] [pacc item_cap f] [pds item_cap] [partials]
struct GatBwdWs { size_t g, q, dss, dsd, pacc, pds, part, total; };
static inline GatBwdWs gat_bwd_ws(int32_t n, int32_t item_cap, int32_t f) {
    const size_t N = n > 0 ? (size_t)n : 1, I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    GatBwdWs w;
    w.g = 0;
    w.q = w.g + grapes_round16(N * F * sizeof(float));
    w.dss = w.q + grapes_round16(N * 4 * sizeof(float));
    w.dsd = w.dss + grapes_round16(N * sizeof(float));
    w.pacc = w.dsd + grapes_round16(N * sizeof(float));
    w.pds = w.pacc + grapes_round16(I * F * sizeof(float));
    w.part = w.pds + grapes_round16(I * sizeof(float));
    w.total = w.part + grapes_round16((size_t)GAT_PARAM_BLOCKS * 3 * F * sizeof(float));
    return w;
}
extern "C" size_t grapes_gat_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f) {
    return gat_bwd_ws(n, item_cap, f).total;
}

extern "C" int grapes_gat_aggregate_bwd(const float* dout, const float* out, const float* bias, int32_t relu, const float* h,
                                        const float* s_src, const float* s_dst, const float* row_ms, const float* a_src,
                                        const float* a_dst, const int32_t* rowptr_t, const int32_t* csr_src,
                                        const int32_t* rowptr_s, const int32_t* csr_dst, float* dh, float* da_src, float* da_dst,
                                        float* dbias, int32_t n, const int32_t* d_n, int32_t f, const int32_t* items_t,
                                        const int32_t* d_n_items_t, const int32_t* items_s, const int32_t* d_n_items_s,
                                        int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!dout || !out || !h || !s_src || !s_dst || !row_ms || !a_src || !a_dst || !rowptr_t || !csr_src || !rowptr_s || !csr_dst ||
        !dh || !workspace || n < 0)
        return GRAPES_EINVAL;
    if (!grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gat_shape(f, grapes_aligned16(dout) && grapes_aligned16(out) && grapes_aligned16(h) && grapes_aligned16(dh) &&
                                       grapes_aligned16(a_src) && grapes_aligned16(a_dst) && (!bias || grapes_aligned16(bias)));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = shape == 0;
    const int skip_t = (items_t && d_n_items_t && item_cap > 0) ? 1 : 0, skip_s = (items_s && d_n_items_s && item_cap > 0) ? 1 : 0;
    const GatBwdWs w = gat_bwd_ws(n, item_cap, f);
    char* base = (char*)workspace;
    float* gbuf = (float*)(base + w.g);
    float4* row_q = (float4*)(base + w.q);
    float* ds_src = (float*)(base + w.dss);
    float* ds_dst = (float*)(base + w.dsd);
    float* pacc = (float*)(base + w.pacc);
    float* pds = (float*)(base + w.pds);
    float* part = (float*)(base + w.part);
    const float* gmat = relu ? gbuf : dout;

    ROW_LAUNCH(gat_bwd_rows_k, 4, vec, f, n, s, dout, out, bias, relu, s_dst, row_ms, gbuf, row_q, n, d_n, f);
    ROW_LAUNCH(gat_bwd_dst_k, 4, vec, f, n, s, h, s_src, gmat, (const float4*)row_q, rowptr_t, csr_src, ds_dst, n, d_n, f, skip_t,
               status);
    if (skip_t) {
        ROW_LAUNCH(gat_bwd_dst_chunks_k, 4, vec, f, item_cap, s, h, s_src, gmat, (const float4*)row_q, rowptr_t, csr_src, n, d_n, f,
                   items_t, d_n_items_t, item_cap, pds, status);
        int g2 = grapes_div_up(item_cap, 256); if (g2 > 2048) g2 = 2048;
        hipLaunchKernelGGL(gat_bwd_dst_combine_k, dim3(g2), dim3(256), 0, s, rowptr_t, ds_dst, n, d_n, items_t, d_n_items_t, item_cap,
                           (const float*)pds);
        GRAPES_LAUNCH_CHECK();
    }
    ROW_LAUNCH(gat_bwd_src_k, 4, vec, f, n, s, h, s_src, gmat, (const float4*)row_q, (const float*)ds_dst, a_src, a_dst, rowptr_s,
               csr_dst, dh, ds_src, n, d_n, f, skip_s, status);
    if (skip_s) {
        ROW_LAUNCH(gat_bwd_src_chunks_k, 4, vec, f, item_cap, s, h, s_src, gmat, (const float4*)row_q, rowptr_s, csr_dst, n, d_n, f,
                   items_s, d_n_items_s, item_cap, pacc, pds, status);
        const int g2 = item_cap < 2048 ? item_cap : 2048;
        hipLaunchKernelGGL(gat_bwd_src_combine_k, dim3(g2), dim3(256), 0, s, rowptr_s, (const float*)ds_dst, a_src, a_dst, dh, ds_src,
                           n, d_n, f, items_s, d_n_items_s, item_cap, (const float*)pacc, (const float*)pds);
        GRAPES_LAUNCH_CHECK();
    }
    if (da_src || da_dst || dbias) {
        int blocks = grapes_div_up(n, 64); if (blocks > GAT_PARAM_BLOCKS) blocks = GAT_PARAM_BLOCKS;
        const int CW = f <= 64 ? 64 : (f <= 128 ? 128 : 256);
        hipLaunchKernelGGL(gat_bwd_params_k, dim3(blocks), dim3(256), 0, s, gmat, h, (const float*)ds_src, (const float*)ds_dst, n, d_n,
                           f, CW, part);
        GRAPES_LAUNCH_CHECK();
        hipLaunchKernelGGL(gat_bwd_params_final_k, dim3(grapes_div_up(3 * f, 4)), dim3(256), 0, s, (const float*)part, blocks, f,
                           dbias, da_src, da_dst);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}
