// GATv2Conv aggregation ([PyG-recall: torch_geometric 2.5.2 GATv2Conv], H heads of C channels, F = H C), forward and backward,
// over the CSRs grapes_gcn_prepare builds.  With x_l = lin_l(x), x_r = lin_r(x) viewed as [n, H, C]:
//
//   z_ij = x_l[j] + x_r[i]    e_ij[h] = sum_c att[h, c] LeakyReLU(z_ij[h, c])    alpha_ij[h] = softmax_j e_ij[h] over {j -> i} + (i, i)
//   agg_i[h] = sum_j alpha_ij[h] x_l[j, h]    out_i = concat_h agg_i[h] + b   or   mean_h agg_i[h] + b
//
//   gatv2_fwd_k           a group of LPR lanes owns a destination row and holds x_r[i] and att in registers; every gathered row
//                         x_l[j] is loaded ONCE and feeds both the score (the lane's partial of att . LeakyReLU(x_l + x_r), reduced
//                         PER HEAD: head_sum) and the weighted sum, U rows in flight; one online softmax per head, whose state
//                         (max, sum) a lane keeps for the head of each of its column slabs.  Epilogue: 1 / sum, then bias and
//                         ReLU (concat) or the per-head aggregate (mean; gatv2_head_mean_k finishes).  row_ms[i, h] = (max, log sum).
//   gatv2_fwd_chunks_k    rows longer than GRAPES_LONG_ROW: one group per work item -> per-head (max, sum), accumulator
//   gatv2_fwd_combine_k   ... merged per row in chunk order against each head's global maximum, with the self-loop
//   gatv2_bwd_rows_k      G = dout (ReLU-gated, / H per head for the mean), c[i, h] = G[i, h] . agg[i, h], row_q[i, h] = (max, log sum, c)
//   gatv2_bwd_dst_k       by target: dx_r[i] = sum_j dz_ij, this group's share of datt (F wide, in registers) and of sum_i G[i];
//                         per workgroup partials, added in a fixed tree by gatv2_bwd_params_final_k   (+ _chunks_k, combine)
//   gatv2_bwd_src_k       by source: dx_l[j] = sum_i alpha_ij G[i] + dz_ij, gathering x_r[i], G[i] and row_q[i, h]  (+ _chunks_k, combine)
//
// with de_ij[h] = alpha_ij[h] (G[i, h] . x_l[j, h] - c[i, h]) and dz_ij[h, c] = de_ij[h] att[h, c] (z > 0 ? 1 : slope).  Nothing of size
// e H or e F is stored: both backward passes recompute z, e and alpha from x_l, x_r and row_q, so each walks its own CSR.
// No floating-point atomics: every sum has a fixed order (butterflies inside a group, chunk order across work items, a fixed
// tree across partials), so results are bit-identical from run to run.  No kernel waits on another workgroup.
#include "row_gather.h"

#define GATV2_PART_BLOCKS 1024          // at most this many workgroups write parameter partials per launch
#define GATV2_MAX_HEADS 16

__device__ __forceinline__ float gv2_leaky(float x, float slope) { return x > 0.f ? x : slope * x; }

// Slab s of lane l holds VEC columns of ONE head (C % VEC == 0): hd[s], or -1 at or beyond F.  lh > 0: the lanes of a head are a
// contiguous, aligned power-of-two sub-group of lh lanes (segmented butterfly); 0: one masked group reduction per head.
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gv2_heads(int F, int C, int l, int (&hd)[NS], int& lh) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int f = (s * LPR + l) * VEC;
        hd[s] = f < F ? f / C : -1;
    }
    const int q = C / VEC;
    lh = (q * VEC == C && (q & (q - 1)) == 0 && q <= LPR) ? q : 0;
}
// true for the lane that holds the first column of its slab's head (it writes the head's scalars)
template <int VEC, int LPR>
__device__ __forceinline__ bool gv2_leads(int s, int l, int F, int C) {
    const int f = (s * LPR + l) * VEC;
    return f < F && f % C == 0;
}

// p[q][s] <- the sum of p[q][.] over every lane and slab of the head of slab s, for NV values at once
template <int LPR, int NS, int NV>
__device__ __forceinline__ void head_sum(float (&p)[NV][NS], const int (&hd)[NS], int H, int lh) {
    if (lh > 0) {
        for (int d = lh >> 1; d > 0; d >>= 1)
#pragma unroll
            for (int q = 0; q < NV; ++q)
#pragma unroll
                for (int s = 0; s < NS; ++s) p[q][s] += __shfl_xor(p[q][s], d, LPR);
        return;
    }
    float r[NV][NS];
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int s = 0; s < NS; ++s) r[q][s] = 0.f;
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            float v = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) v += hd[s] == h ? p[q][s] : 0.f;
            v = grp_sum<LPR>(v);
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (hd[s] == h) r[q][s] = v;
        }
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int s = 0; s < NS; ++s) p[q][s] = r[q][s];
}

// this lane's partial of att . LeakyReLU(x_l + x_r) per slab
template <int VEC, int NS>
__device__ __forceinline__ void gv2_score(const float (&hv)[NS][VEC], const float (&xr)[NS][VEC], const float (&at)[NS][VEC],
                                          float slope, float (&p)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float d = 0.f;
#pragma unroll
        for (int v = 0; v < VEC; ++v) d = fmaf(at[s][v], gv2_leaky(hv[s][v] + xr[s][v], slope), d);
        p[s] = d;
    }
}

// ------------------------------------------------------------------------------------------------------------ forward

// per-head online softmax + weighted gather over entries [beg - with_self, end) of row `row`: (m, sum, acc) are updated in place
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gv2_fwd_range(const float* __restrict__ xl, const int32_t* __restrict__ csr, int row, int n,
                                              const float (&xr)[NS][VEC], const float (&at)[NS][VEC], const int (&hd)[NS], int H,
                                              int lh, float slope, int beg, int end, bool with_self, int F, int l, float (&m)[NS],
                                              float (&sum)[NS], float (&acc)[NS][VEC], int32_t* status) {
    constexpr int U = RowUnroll<NS>::U;
    for (int b = with_self ? beg - 1 : beg; b < end; b += LPR) {
        int idx;
        const int ok = gat_entry(csr, b + l, beg, end, row, n, idx, status) ? 1 : 0;
        const int cnt = end - b < LPR ? end - b : LPR;
        for (int k = 0; k < cnt; k += U) {                     // (lanes past cnt hold idx = row, ok = 0: loads stay in range)
            float hv[U][NS][VEC], e[U][NS];
            int okk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ik = __shfl(idx, k + u, LPR);
                okk[u] = __shfl(ok, k + u, LPR);
                row_load<VEC, LPR, NS>(xl, ik, F, l, hv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) gv2_score<VEC, NS>(hv[u], xr, at, slope, e[u]);
            head_sum<LPR, NS, U>(e, hd, H, lh);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float mn = m[s];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (okk[u]) mn = fmaxf(mn, e[u][s]);
                if (mn == -INFINITY) continue;                 // (no entry kept so far)
                const float sc = m[s] == -INFINITY ? 0.f : expf(m[s] - mn);
                float t = sum[s] * sc;
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[s][v] *= sc;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float w = okk[u] ? expf(e[u][s] - mn) : 0.f;
                    t += w;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[s][v] = fmaf(w, hv[u][s][v], acc[s][v]);
                }
                sum[s] = t;
                m[s] = mn;
            }
        }
    }
}

// rows longer than GRAPES_LONG_ROW (skip_long): only the self-loop's score here (row_ms[., 0]), the rest by gatv2_fwd_chunks_k
// and gatv2_fwd_combine_k.  concat: out [n, F] = agg + bias (ReLU); else agg [n, F] receives the per-head aggregate.
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gatv2_fwd_k(const float* __restrict__ xl, const float* __restrict__ xrm,
                                                   const float* __restrict__ att, const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ csr, const float* __restrict__ bias,
                                                   float* __restrict__ out, float* __restrict__ agg, float* __restrict__ row_ms,
                                                   int n_host, const int32_t* d_n, int F, int C, int H, int concat, float slope,
                                                   int relu, int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    int hd[NS], lh;
    gv2_heads<VEC, LPR, NS>(F, C, l, hd, lh);
    float at[NS][VEC], bv[NS][VEC];
    row_load<VEC, LPR, NS>(att, 0, F, l, at);
    if (concat && bias) row_load<VEC, LPR, NS>(bias, 0, F, l, bv);
    else slab_zero<VEC, NS>(bv);
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row];
        int end = rowptr[row + 1];
        const bool is_long = skip_long && end - beg > GRAPES_LONG_ROW;
        if (is_long) end = beg;
        float xr[NS][VEC], acc[NS][VEC], m[NS], sum[NS];
        row_load<VEC, LPR, NS>(xrm, row, F, l, xr);
        slab_zero<VEC, NS>(acc);
#pragma unroll
        for (int s = 0; s < NS; ++s) { m[s] = -INFINITY; sum[s] = 0.f; }
        gv2_fwd_range<VEC, LPR, NS>(xl, csr, row, n, xr, at, hd, H, lh, slope, beg, end, true, F, l, m, sum, acc, status);
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (gv2_leads<VEC, LPR>(s, l, F, C)) {
                float* ms = row_ms + 2 * ((long long)row * H + hd[s]);
                ms[0] = m[s]; ms[1] = logf(sum[s]);
            }
        if (is_long) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float inv = 1.f / sum[s];                               // (sum >= 1: the entry at the maximum contributes 1)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float r = acc[s][v] * inv;
                if (concat) { r += bv[s][v]; if (relu) r = fmaxf(r, 0.f); }
                acc[s][v] = r;
            }
        }
        row_store<VEC, LPR, NS>(concat ? out : agg, row, F, l, acc);
    }
}

// one group per work item (row, chunk): per head the chunk's (max, sum) -> pms[it, h], its unnormalised accumulator -> pacc[it F]
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gatv2_fwd_chunks_k(const float* __restrict__ xl, const float* __restrict__ xrm,
                                                          const float* __restrict__ att, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ csr, int n_host, const int32_t* d_n, int F, int C,
                                                          int H, float slope, const int32_t* __restrict__ items,
                                                          const int32_t* __restrict__ d_n_items, int item_cap,
                                                          float* __restrict__ pacc, float* __restrict__ pms, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    int hd[NS], lh;
    gv2_heads<VEC, LPR, NS>(F, C, l, hd, lh);
    float at[NS][VEC];
    row_load<VEC, LPR, NS>(att, 0, F, l, at);
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float acc[NS][VEC], m[NS], sum[NS];
        slab_zero<VEC, NS>(acc);
#pragma unroll
        for (int s = 0; s < NS; ++s) { m[s] = -INFINITY; sum[s] = 0.f; }
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            float xr[NS][VEC];
            row_load<VEC, LPR, NS>(xrm, row, F, l, xr);
            gv2_fwd_range<VEC, LPR, NS>(xl, csr, row, n, xr, at, hd, H, lh, slope, beg, end, false, F, l, m, sum, acc, status);
        }
        row_store<VEC, LPR, NS>(pacc, it, F, l, acc);
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (gv2_leads<VEC, LPR>(s, l, F, C)) {
                float* ms = pms + 2 * ((long long)it * H + hd[s]);
                ms[0] = m[s]; ms[1] = sum[s];
            }
    }
}

// The item with chunk 0 leads its row: its nc items are contiguous and in chunk order.  One workgroup per row, a thread per
// column (F <= 1024: four columns a thread at most): the head's maximum over the chunks and the self-loop (its score is what
// gatv2_fwd_k left in row_ms[row, h, 0]), then self term + sum_c exp(m_c - M) part_c in chunk order, for the column and for the
// head's softmax sum.  Every thread of a head forms the same sum in the same order.
__global__ __launch_bounds__(256) void gatv2_fwd_combine_k(const float* __restrict__ xl, const int32_t* __restrict__ rowptr,
                                                           const float* __restrict__ bias, float* __restrict__ out,
                                                           float* __restrict__ agg, float* __restrict__ row_ms, int n_host,
                                                           const int32_t* d_n, int F, int C, int H, int concat, int relu,
                                                           const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                           int item_cap, const float* __restrict__ pacc,
                                                           const float* __restrict__ pms) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;          // (uniform over the workgroup)
        float e_self[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = threadIdx.x + 256 * q;
            e_self[q] = f < F ? row_ms[2 * ((long long)row * H + f / C)] : 0.f;
        }
        __syncthreads();                                                           // (row_ms[row] is rewritten below)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = threadIdx.x + 256 * q;
            if (f >= F) continue;
            const int h = f / C;
            float M = e_self[q];
            for (int c = 0; c < nc; ++c) M = fmaxf(M, pms[2 * ((long long)(it + c) * H + h)]);
            const float w_self = expf(e_self[q] - M);
            float tot = w_self, a = w_self * xl[(long long)row * F + f];
            for (int c = 0; c < nc; ++c) {
                const float* ms = pms + 2 * ((long long)(it + c) * H + h);
                const float w = ms[0] == -INFINITY ? 0.f : expf(ms[0] - M);
                tot = fmaf(w, ms[1], tot);
                a = fmaf(w, pacc[(long long)(it + c) * F + f], a);
            }
            float r = a / tot;
            if (concat) {
                if (bias) r += bias[f];
                out[(long long)row * F + f] = relu ? fmaxf(r, 0.f) : r;
            } else {
                agg[(long long)row * F + f] = r;
            }
            if (f % C == 0) {
                float* ms = row_ms + 2 * ((long long)row * H + h);
                ms[0] = M; ms[1] = logf(tot);
            }
        }
        __syncthreads();
    }
}

// concat = 0: out[i, c] = mean_h agg[i, h, c] + bias[c] (ReLU), the heads added in head order
__global__ __launch_bounds__(256) void gatv2_head_mean_k(const float* __restrict__ agg, const float* __restrict__ bias,
                                                         float* __restrict__ out, int n_host, const int32_t* d_n, int C, int H,
                                                         int relu) {
    const int n = eff_count(d_n, n_host);
    const long long total = (long long)n * C;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long row = t / C;
        const int c = (int)(t - row * C);
        float a = 0.f;
        for (int h = 0; h < H; ++h) a += agg[(row * H + h) * C + c];
        a = a / (float)H + (bias ? bias[c] : 0.f);
        out[t] = relu ? fmaxf(a, 0.f) : a;
    }
}

// ------------------------------------------------------------------------------------------------------------ backward

// G_i = dout_i gated by the layer's ReLU, per head (the head mean hands every head dout / H); c[i, h] = G[i, h] . agg[i, h] with
// agg = out - bias (concat) or the saved per-head aggregate; row_q[i, h] = (max, log sum, c, 0).  gbuf is written when G is not
// dout itself (ReLU or head mean).
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gatv2_bwd_rows_k(const float* __restrict__ dout, const float* __restrict__ out,
                                                        const float* __restrict__ agg, const float* __restrict__ bias, int relu,
                                                        const float* __restrict__ row_ms, float* __restrict__ gbuf,
                                                        float4* __restrict__ row_q, int n_host, const int32_t* d_n, int F, int C,
                                                        int H, int concat) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    int hd[NS], lh;
    gv2_heads<VEC, LPR, NS>(F, C, l, hd, lh);
    const int W = concat ? F : C;
    const float inv_h = concat ? 1.f : 1.f / (float)H;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        float g[NS][VEC], p[1][NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int f = (s * LPR + l) * VEC;
            p[0][s] = 0.f;
            if (f < F) {
                const int col = concat ? f : f % C;
                float o[VEC], a[VEC];
                vec_load<VEC>(dout + (long long)row * W + col, g[s]);
                vec_load<VEC>(out + (long long)row * W + col, o);
                if (concat) {
                    if (bias) vec_load<VEC>(bias + col, a);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) a[v] = o[v] - (bias ? a[v] : 0.f);
                } else {
                    vec_load<VEC>(agg + (long long)row * F + f, a);
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if (relu && !(o[v] > 0.f)) g[s][v] = 0.f;
                    g[s][v] *= inv_h;
                    p[0][s] = fmaf(g[s][v], a[v], p[0][s]);
                }
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) g[s][v] = 0.f;
            }
        }
        head_sum<LPR, NS, 1>(p, hd, H, lh);
        if (relu || !concat) row_store<VEC, LPR, NS>(gbuf, row, F, l, g);
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (gv2_leads<VEC, LPR>(s, l, F, C)) {
                const long long k = (long long)row * H + hd[s];
                row_q[k] = make_float4(row_ms[2 * k], row_ms[2 * k + 1], p[0][s], 0.f);
            }
    }
}

// an F-wide register row per group (VEC columns per lane and slab), added over the workgroup's groups in group order -> dst[F]
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gv2_block_columns(float* red, const float (&a)[NS][VEC], float* __restrict__ dst, int F, int l) {
    constexpr int G = 256 / LPR, WID = NS * LPR * VEC;
    const int grp = threadIdx.x / LPR;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v) red[grp * WID + (s * LPR + l) * VEC + v] = a[s][v];
    __syncthreads();
    if (grp == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const int f = (s * LPR + l) * VEC + v;
                float t = red[f];
                for (int g = 1; g < G; ++g) t += red[g * WID + f];
                if (f < F) dst[f] = t;
            }
    }
}

// the (max, log sum, c) of row i's heads for this lane's slabs
template <int NS>
__device__ __forceinline__ void gv2_row_q(const float4* __restrict__ row_q, long long row, int H, const int (&hd)[NS], float4 (&q)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) q[s] = hd[s] >= 0 ? row_q[row * H + hd[s]] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// by target: dxr += sum_j dz_ij and datt += sum_j de_ij LeakyReLU(z_ij) over entries [beg - with_self, end) of row i
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gv2_bwd_dst_range(const float* __restrict__ xl, const int32_t* __restrict__ csr, int row, int n,
                                                  const float (&xr)[NS][VEC], const float (&at)[NS][VEC], const float (&g)[NS][VEC],
                                                  const float4 (&q)[NS], const int (&hd)[NS], int H, int lh, float slope, int beg,
                                                  int end, bool with_self, int F, int l, float (&dxr)[NS][VEC],
                                                  float (&datt)[NS][VEC], int32_t* status) {
    constexpr int U = RowUnroll<NS>::U;
    for (int b = with_self ? beg - 1 : beg; b < end; b += LPR) {
        int idx;
        const int ok = gat_entry(csr, b + l, beg, end, row, n, idx, status) ? 1 : 0;
        const int cnt = end - b < LPR ? end - b : LPR;
        for (int k = 0; k < cnt; k += U) {
            float hv[U][NS][VEC], ed[2 * U][NS];                 // [u]: the score's partial, [U + u]: G_i . x_l[j]'s
            int okk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                okk[u] = __shfl(ok, k + u, LPR);
                row_load<VEC, LPR, NS>(xl, __shfl(idx, k + u, LPR), F, l, hv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                gv2_score<VEC, NS>(hv[u], xr, at, slope, ed[u]);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    float d = 0.f;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) d = fmaf(g[s][v], hv[u][s][v], d);
                    ed[U + u][s] = d;
                }
            }
            head_sum<LPR, NS, 2 * U>(ed, hd, H, lh);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float de = okk[u] ? expf(ed[u][s] - q[s].x - q[s].y) * (ed[U + u][s] - q[s].z) : 0.f;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float z = hv[u][s][v] + xr[s][v];
                        dxr[s][v] = fmaf(de * at[s][v], z > 0.f ? 1.f : slope, dxr[s][v]);
                        datt[s][v] = fmaf(de, gv2_leaky(z, slope), datt[s][v]);
                    }
                }
        }
    }
}

// rows longer than GRAPES_LONG_ROW (skip_long): only the self-loop here, the entries by gatv2_bwd_dst_chunks_k + the combine.
// part[blockIdx.x][0][F] = this workgroup's share of datt, [1][F] = of the column sums of G.
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gatv2_bwd_dst_k(const float* __restrict__ xl, const float* __restrict__ xrm,
                                                       const float* __restrict__ att, const float* __restrict__ gmat,
                                                       const float4* __restrict__ row_q, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ csr, float* __restrict__ dxrm,
                                                       float* __restrict__ part, int n_host, const int32_t* d_n, int F, int C, int H,
                                                       float slope, int skip_long, int32_t* status) {
    __shared__ float red[256 * NS * VEC];
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    int hd[NS], lh;
    gv2_heads<VEC, LPR, NS>(F, C, l, hd, lh);
    float at[NS][VEC], datt[NS][VEC], gsum[NS][VEC];
    row_load<VEC, LPR, NS>(att, 0, F, l, at);
    slab_zero<VEC, NS>(datt);
    slab_zero<VEC, NS>(gsum);
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row];
        int end = rowptr[row + 1];
        if (skip_long && end - beg > GRAPES_LONG_ROW) end = beg;
        float xr[NS][VEC], g[NS][VEC], dxr[NS][VEC];
        float4 q[NS];
        row_load<VEC, LPR, NS>(xrm, row, F, l, xr);
        row_load<VEC, LPR, NS>(gmat, row, F, l, g);
        gv2_row_q<NS>(row_q, row, H, hd, q);
        slab_zero<VEC, NS>(dxr);
        gv2_bwd_dst_range<VEC, LPR, NS>(xl, csr, row, n, xr, at, g, q, hd, H, lh, slope, beg, end, true, F, l, dxr, datt, status);
        row_store<VEC, LPR, NS>(dxrm, row, F, l, dxr);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) gsum[s][v] += g[s][v];
    }
    float* o = part + (long long)blockIdx.x * 2 * F;
    gv2_block_columns<VEC, LPR, NS>(red, datt, o, F, l);
    gv2_block_columns<VEC, LPR, NS>(red, gsum, o + F, F, l);
}
// per work item: its share of dx_r[row] -> pacc[it F]; part[blockIdx.x][0][F] = this workgroup's share of datt ([1] is not used)
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gatv2_bwd_dst_chunks_k(const float* __restrict__ xl, const float* __restrict__ xrm,
                                                              const float* __restrict__ att, const float* __restrict__ gmat,
                                                              const float4* __restrict__ row_q, const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ csr, int n_host, const int32_t* d_n, int F,
                                                              int C, int H, float slope, const int32_t* __restrict__ items,
                                                              const int32_t* __restrict__ d_n_items, int item_cap,
                                                              float* __restrict__ pacc, float* __restrict__ part, int32_t* status) {
    __shared__ float red[256 * NS * VEC];
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    int hd[NS], lh;
    gv2_heads<VEC, LPR, NS>(F, C, l, hd, lh);
    float at[NS][VEC], datt[NS][VEC];
    row_load<VEC, LPR, NS>(att, 0, F, l, at);
    slab_zero<VEC, NS>(datt);
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float dxr[NS][VEC];
        slab_zero<VEC, NS>(dxr);
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            float xr[NS][VEC], g[NS][VEC];
            float4 q[NS];
            row_load<VEC, LPR, NS>(xrm, row, F, l, xr);
            row_load<VEC, LPR, NS>(gmat, row, F, l, g);
            gv2_row_q<NS>(row_q, row, H, hd, q);
            gv2_bwd_dst_range<VEC, LPR, NS>(xl, csr, row, n, xr, at, g, q, hd, H, lh, slope, beg, end, false, F, l, dxr, datt, status);
        }
        row_store<VEC, LPR, NS>(pacc, it, F, l, dxr);
    }
    gv2_block_columns<VEC, LPR, NS>(red, datt, part + (long long)blockIdx.x * 2 * F, F, l);
}

// one workgroup per long row, a thread per column: dst[row] (the self-loop's term, from the rows kernel) + the row's work items in
// chunk order.  Both backward passes finish their long rows with it.
__global__ __launch_bounds__(256) void gatv2_bwd_combine_k(const int32_t* __restrict__ rowptr, float* __restrict__ dst, int n_host,
                                                           const int32_t* d_n, int F, const int32_t* __restrict__ items,
                                                           const int32_t* __restrict__ d_n_items, int item_cap,
                                                           const float* __restrict__ pacc) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        for (int f = threadIdx.x; f < F; f += 256) {
            float a = dst[(long long)row * F + f];
            for (int c = 0; c < nc; ++c) a += pacc[(long long)(it + c) * F + f];
            dst[(long long)row * F + f] = a;
        }
    }
}

// by source: acc += sum_i alpha_ij G_i + dz_ij over entries [beg - with_self, end) of row j of the by-source CSR
template <int VEC, int LPR, int NS>
__device__ __forceinline__ void gv2_bwd_src_range(const float* __restrict__ xrm, const float* __restrict__ gmat,
                                                  const float4* __restrict__ row_q, const int32_t* __restrict__ csr, int row, int n,
                                                  const float (&xlr)[NS][VEC], const float (&at)[NS][VEC], const int (&hd)[NS], int H,
                                                  int lh, float slope, int beg, int end, bool with_self, int F, int l,
                                                  float (&acc)[NS][VEC], int32_t* status) {
    constexpr int U = RowUnroll<NS>::U;
    for (int b = with_self ? beg - 1 : beg; b < end; b += LPR) {
        int idx;
        const int ok = gat_entry(csr, b + l, beg, end, row, n, idx, status) ? 1 : 0;
        const int cnt = end - b < LPR ? end - b : LPR;
        for (int k = 0; k < cnt; k += U) {
            float rv[U][NS][VEC], gv[U][NS][VEC], ed[2 * U][NS];
            float4 q[U][NS];
            int okk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ik = __shfl(idx, k + u, LPR);
                okk[u] = __shfl(ok, k + u, LPR);
                row_load<VEC, LPR, NS>(xrm, ik, F, l, rv[u]);
                row_load<VEC, LPR, NS>(gmat, ik, F, l, gv[u]);
                gv2_row_q<NS>(row_q, ik, H, hd, q[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                gv2_score<VEC, NS>(xlr, rv[u], at, slope, ed[u]);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    float d = 0.f;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) d = fmaf(gv[u][s][v], xlr[s][v], d);
                    ed[U + u][s] = d;
                }
            }
            head_sum<LPR, NS, 2 * U>(ed, hd, H, lh);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float alpha = okk[u] ? expf(ed[u][s] - q[u][s].x - q[u][s].y) : 0.f;
                    const float de = alpha * (ed[U + u][s] - q[u][s].z);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float z = xlr[s][v] + rv[u][s][v];
                        acc[s][v] = fmaf(alpha, gv[u][s][v], fmaf(de * at[s][v], z > 0.f ? 1.f : slope, acc[s][v]));
                    }
                }
        }
    }
}

// long rows (skip_long): only the self-loop's terms, the entries by gatv2_bwd_src_chunks_k + the combine
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gatv2_bwd_src_k(const float* __restrict__ xl, const float* __restrict__ xrm,
                                                       const float* __restrict__ att, const float* __restrict__ gmat,
                                                       const float4* __restrict__ row_q, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ csr, float* __restrict__ dxl, int n_host,
                                                       const int32_t* d_n, int F, int C, int H, float slope, int skip_long,
                                                       int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    int hd[NS], lh;
    gv2_heads<VEC, LPR, NS>(F, C, l, hd, lh);
    float at[NS][VEC];
    row_load<VEC, LPR, NS>(att, 0, F, l, at);
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row];
        int end = rowptr[row + 1];
        if (skip_long && end - beg > GRAPES_LONG_ROW) end = beg;
        float xlr[NS][VEC], acc[NS][VEC];
        row_load<VEC, LPR, NS>(xl, row, F, l, xlr);
        slab_zero<VEC, NS>(acc);
        gv2_bwd_src_range<VEC, LPR, NS>(xrm, gmat, row_q, csr, row, n, xlr, at, hd, H, lh, slope, beg, end, true, F, l, acc, status);
        row_store<VEC, LPR, NS>(dxl, row, F, l, acc);
    }
}
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void gatv2_bwd_src_chunks_k(const float* __restrict__ xl, const float* __restrict__ xrm,
                                                              const float* __restrict__ att, const float* __restrict__ gmat,
                                                              const float4* __restrict__ row_q, const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ csr, int n_host, const int32_t* d_n, int F,
                                                              int C, int H, float slope, const int32_t* __restrict__ items,
                                                              const int32_t* __restrict__ d_n_items, int item_cap,
                                                              float* __restrict__ pacc, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    int hd[NS], lh;
    gv2_heads<VEC, LPR, NS>(F, C, l, hd, lh);
    float at[NS][VEC];
    row_load<VEC, LPR, NS>(att, 0, F, l, at);
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        float acc[NS][VEC];
        slab_zero<VEC, NS>(acc);
        item_range(items, it, rowptr, n, row, beg, end);
        if (beg < end) {
            float xlr[NS][VEC];
            row_load<VEC, LPR, NS>(xl, row, F, l, xlr);
            gv2_bwd_src_range<VEC, LPR, NS>(xrm, gmat, row_q, csr, row, n, xlr, at, hd, H, lh, slope, beg, end, false, F, l, acc, status);
        }
        row_store<VEC, LPR, NS>(pacc, it, F, l, acc);
    }
}

// One wavefront per output value: lane l adds partials l, l + 64, ... in that order, then a butterfly over the lanes.  Values
// [0, F): datt over all `blocks` partials; [F, F + W): dbias over the first blocks_g of them, W = F (concat) or C, where the
// column sums of the H heads' G are added in head order (G = dout / H per head: their sum is dout's).
__global__ __launch_bounds__(256) void gatv2_bwd_params_final_k(const float* __restrict__ part, int blocks, int blocks_g, int F, int C,
                                                                int H, int concat, float* __restrict__ datt,
                                                                float* __restrict__ dbias) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    const int W = concat ? F : C;
    if (t >= F + W) return;
    float a = 0.f;
    if (t < F) {
        for (int b = l; b < blocks; b += 64) a += part[(long long)b * 2 * F + t];
        a = wave_sum(a);
        if (datt && l == 0) datt[t] = a;
    } else {
        const int c = t - F, hm = concat ? 1 : H;
        for (int b = l; b < blocks_g; b += 64)
            for (int h = 0; h < hm; ++h) a += part[((long long)b * 2 + 1) * F + h * C + c];
        a = wave_sum(a);
        if (dbias && l == 0) dbias[c] = a;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side

// 0: float4 columns (every head a whole number of them), 1: scalar columns, negative: not covered
static inline int gatv2_shape(int heads, int c, bool aligned) {
    if (heads < 1 || heads > GATV2_MAX_HEADS || c < 1 || c > 1024) return GRAPES_EINVAL;
    const int f = heads * c;
    if (c % 4 == 0 && aligned) return f <= 1024 ? 0 : GRAPES_EINVAL;
    if (f <= 256) return 1;
    return c % 4 == 0 && f <= 1024 ? GRAPES_EALIGN : GRAPES_EINVAL;
}
// the lanes per row ROW_LAUNCH picks (the partial buffers are sized by the grid it forms)
static inline int gatv2_lanes(bool vec, int f) { return (vec ? f <= 128 : f <= 32) ? 32 : 64; }
static inline int gatv2_part_rows(int rows) { return rows < GATV2_PART_BLOCKS * 4 ? rows : GATV2_PART_BLOCKS * 4; }

extern "C" size_t grapes_gatv2_aggregate_workspace_bytes(int32_t item_cap, int32_t f, int32_t heads) {
    const size_t items = item_cap > 0 ? (size_t)item_cap : 0;
    return grapes_round16(items * (size_t)(f > 0 ? f : 1) * sizeof(float)) +
           grapes_round16(items * (size_t)(heads > 0 ? heads : 1) * 2 * sizeof(float)) + 16;
}

extern "C" int grapes_gatv2_aggregate_fwd(const float* x_l, const float* x_r, const float* att, const int32_t* rowptr_t,
                                          const int32_t* csr_src, const float* bias, float* out, float* agg, float* row_ms,
                                          int32_t n, const int32_t* d_n, int32_t heads, int32_t c, int32_t concat,
                                          float negative_slope, int32_t relu, const int32_t* long_items, const int32_t* d_n_items,
                                          int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!x_l || !x_r || !att || !rowptr_t || !csr_src || !out || !row_ms || n < 0 || (!concat && !agg)) return GRAPES_EINVAL;
    if (!(negative_slope >= 0.f && negative_slope < 1.f)) return GRAPES_EINVAL;
    const int skip = (long_items && d_n_items && workspace && item_cap > 0) ? 1 : 0;
    if (skip && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gatv2_shape(heads, c, grapes_aligned16(x_l) && grapes_aligned16(x_r) && grapes_aligned16(att) &&
                                                grapes_aligned16(out) && (concat || grapes_aligned16(agg)) &&
                                                (!bias || grapes_aligned16(bias)));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = shape == 0;
    const int f = heads * c;
    ROW_LAUNCH(gatv2_fwd_k, 4, vec, f, n, s, x_l, x_r, att, rowptr_t, csr_src, bias, out, agg, row_ms, n, d_n, f, c, heads, concat,
               negative_slope, relu, skip, status);
    if (skip) {
        float* pacc = (float*)workspace;
        float* pms = (float*)((char*)workspace + grapes_round16((size_t)item_cap * f * sizeof(float)));
        ROW_LAUNCH(gatv2_fwd_chunks_k, 4, vec, f, item_cap, s, x_l, x_r, att, rowptr_t, csr_src, n, d_n, f, c, heads, negative_slope,
                   long_items, d_n_items, item_cap, pacc, pms, status);
        const int g2 = item_cap < 2048 ? item_cap : 2048;
        hipLaunchKernelGGL(gatv2_fwd_combine_k, dim3(g2), dim3(256), 0, s, x_l, rowptr_t, bias, out, agg, row_ms, n, d_n, f, c, heads,
                           concat, relu, long_items, d_n_items, item_cap, (const float*)pacc, (const float*)pms);
        GRAPES_LAUNCH_CHECK();
    }
    if (!concat) {
        hipLaunchKernelGGL(gatv2_head_mean_k, dim3(flat_grid(n, c, 1)), dim3(256), 0, s, (const float*)agg, bias, out, n, d_n, c, heads,
                           relu);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}

// workspace layout of the backward: [G n f] [row_q 4 n heads] [pacc item_cap f] [partials 2 GATV2_PART_BLOCKS x 2 f]
struct Gatv2BwdWs { size_t g, q, pacc, part, total; };
static inline Gatv2BwdWs gatv2_bwd_ws(int32_t n, int32_t item_cap, int32_t f, int32_t heads) {
    const size_t N = n > 0 ? (size_t)n : 1, I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    const size_t H = heads > 0 ? (size_t)heads : 1;
    Gatv2BwdWs w;
    w.g = 0;
    w.q = w.g + grapes_round16(N * F * sizeof(float));
    w.pacc = w.q + grapes_round16(N * H * 4 * sizeof(float));
    w.part = w.pacc + grapes_round16(I * F * sizeof(float));
    w.total = w.part + grapes_round16((size_t)2 * GATV2_PART_BLOCKS * 2 * F * sizeof(float));
    return w;
}
extern "C" size_t grapes_gatv2_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f, int32_t heads) {
    return gatv2_bwd_ws(n, item_cap, f, heads).total;
}

extern "C" int grapes_gatv2_aggregate_bwd(const float* dout, const float* out, const float* agg, const float* bias, int32_t relu,
                                          const float* x_l, const float* x_r, const float* att, const float* row_ms,
                                          const int32_t* rowptr_t, const int32_t* csr_src, const int32_t* rowptr_s,
                                          const int32_t* csr_dst, float* dx_l, float* dx_r, float* datt, float* dbias, int32_t n,
                                          const int32_t* d_n, int32_t heads, int32_t c, int32_t concat, float negative_slope,
                                          const int32_t* items_t, const int32_t* d_n_items_t, const int32_t* items_s,
                                          const int32_t* d_n_items_s, int32_t item_cap, void* workspace, int32_t* status,
                                          grapes_stream_t stream) {
    if (!dout || !out || !x_l || !x_r || !att || !row_ms || !rowptr_t || !csr_src || !rowptr_s || !csr_dst || !dx_l || !dx_r ||
        !workspace || n < 0 || (!concat && !agg))
        return GRAPES_EINVAL;
    if (!(negative_slope >= 0.f && negative_slope < 1.f)) return GRAPES_EINVAL;
    if (!grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gatv2_shape(heads, c, grapes_aligned16(dout) && grapes_aligned16(out) && grapes_aligned16(x_l) &&
                                                grapes_aligned16(x_r) && grapes_aligned16(att) && grapes_aligned16(dx_l) &&
                                                grapes_aligned16(dx_r) && (concat || grapes_aligned16(agg)) &&
                                                (!bias || grapes_aligned16(bias)));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = shape == 0;
    const int f = heads * c;
    const int skip_t = (items_t && d_n_items_t && item_cap > 0) ? 1 : 0, skip_s = (items_s && d_n_items_s && item_cap > 0) ? 1 : 0;
    const Gatv2BwdWs w = gatv2_bwd_ws(n, item_cap, f, heads);
    char* base = (char*)workspace;
    float* gbuf = (float*)(base + w.g);
    float4* row_q = (float4*)(base + w.q);
    float* pacc = (float*)(base + w.pacc);
    float* part = (float*)(base + w.part);
    const float* gmat = (relu || !concat) ? gbuf : dout;
    const int lanes = gatv2_lanes(vec, f);
    const int g2 = item_cap < 2048 ? item_cap : 2048;

    ROW_LAUNCH(gatv2_bwd_rows_k, 4, vec, f, n, s, dout, out, agg, bias, relu, row_ms, gbuf, row_q, n, d_n, f, c, heads, concat);
    const int rows_a = gatv2_part_rows(n);
    const int blocks_g = row_grid(rows_a, lanes);
    int blocks = blocks_g;
    ROW_LAUNCH(gatv2_bwd_dst_k, 4, vec, f, rows_a, s, x_l, x_r, att, gmat, (const float4*)row_q, rowptr_t, csr_src, dx_r, part, n,
               d_n, f, c, heads, negative_slope, skip_t, status);
    if (skip_t) {
        const int rows_b = gatv2_part_rows(item_cap);
        ROW_LAUNCH(gatv2_bwd_dst_chunks_k, 4, vec, f, rows_b, s, x_l, x_r, att, gmat, (const float4*)row_q, rowptr_t, csr_src, n, d_n,
                   f, c, heads, negative_slope, items_t, d_n_items_t, item_cap, pacc, part + (size_t)blocks_g * 2 * f, status);
        blocks += row_grid(rows_b, lanes);
        hipLaunchKernelGGL(gatv2_bwd_combine_k, dim3(g2), dim3(256), 0, s, rowptr_t, dx_r, n, d_n, f, items_t, d_n_items_t, item_cap,
                           (const float*)pacc);
        GRAPES_LAUNCH_CHECK();
    }
    ROW_LAUNCH(gatv2_bwd_src_k, 4, vec, f, n, s, x_l, x_r, att, gmat, (const float4*)row_q, rowptr_s, csr_dst, dx_l, n, d_n, f, c,
               heads, negative_slope, skip_s, status);
    if (skip_s) {
        ROW_LAUNCH(gatv2_bwd_src_chunks_k, 4, vec, f, item_cap, s, x_l, x_r, att, gmat, (const float4*)row_q, rowptr_s, csr_dst, n,
                   d_n, f, c, heads, negative_slope, items_s, d_n_items_s, item_cap, pacc, status);
        hipLaunchKernelGGL(gatv2_bwd_combine_k, dim3(g2), dim3(256), 0, s, rowptr_s, dx_l, n, d_n, f, items_s, d_n_items_s, item_cap,
                           (const float*)pacc);
        GRAPES_LAUNCH_CHECK();
    }
    if (datt || dbias) {
        const int outs = f + (concat ? f : c);
        hipLaunchKernelGGL(gatv2_bwd_params_final_k, dim3(grapes_div_up(outs, 4)), dim3(256), 0, s, (const float*)part, blocks,
                           blocks_g, f, c, heads, concat, datt, dbias);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}
