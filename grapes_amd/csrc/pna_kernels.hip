// PNAConv (reference modules/gcn.py:120-149: PNAConv(in_channels, out_channels, aggregators, scalers, deg), every other argument
// at its default [PyG-recall: torch_geometric 2.5.2]) — the multi-aggregator gather and its backward over the CSRs
// grapes_gcn_prepare builds.  No per-edge tensor exists: pre_nn is linear, so the message of a stored edge (j -> i) is
//
//   m_ij = a_i + b_j        a = x W_i^T + bias_pre,  b = x W_j^T        (W_pre = [W_i | W_j]; two GEMM outputs with one pitch)
//
// and mean / min / max over j are a_i + the statistic of b_j, while var / std do not see a_i at all.  Every occurrence of a stored
// edge counts, the stored self-loops the build drops come back through loops[i] (grapes_gcn2_loop_counts), no loop is added.
//
//   pna_rows_k        a group of LPR lanes (half a wavefront or a whole one) owns a row of the by-target CSR and walks it once per
//                     column tile of LPR * VEC features: each b_j row is read once, and per feature the lane keeps the running
//                     (count, mean, M2) of Welford's update, min, max and the number of entries equal to each in registers.  The
//                     epilogue writes row i of post_nn's operand directly — [x_i | scaler_1(aggs) | scaler_2(aggs) | ...], the
//                     scalers from d_i = row length + loops[i] — and beside it the statistics of b the backward needs.
//   pna_chunks_k      rows longer than GRAPES_LONG_ROW: one group per work item (row, chunk) -> the chunk's six statistics
//   pna_combine_k     ... one workgroup per long row merges its chunks IN CHUNK ORDER (Chan's update for (count, mean, M2); min,
//                     max and their tie counts), then the same epilogue
//   pna_fold_k        backward, row-local: the scalers folded into the gradient of each aggregate, then into four per-row
//                     coefficients  Gm = gmean / d, Gv = 2 gvar / d, Gmin = gmin / ties_min, Gmax = gmax / ties_max  and
//                     da_i = gmean + gmin + gmax
//   pna_bwd_rows_k    the gather over the by-source CSR:  db_j = sum_{i <- j} Gm_i + Gv_i (b_j - mean_i) + Gmax_i [b_j == max_i]
//                     + Gmin_i [b_j == min_i]  (+ loops[j] times the same with i = j); pna_bwd_chunks_k / pna_bwd_combine_k for
//                     long rows, partial sums added in chunk order
//   pna_add_k         dx += dZ[:, :F]  (the copy of x_i in post_nn's operand)
//
// Variance: centred (Welford per entry, Chan across chunks and for a loop of multiplicity c), never E[b^2] - E[b]^2.  Ties: an
// entry bit-equal to the row's max (min) gets 1 / (number of such entries) of its gradient, so the weights of a row sum to one.
// No floating-point atomics, every reduction has a fixed order: two runs are bit-identical.  No kernel waits on another workgroup.
#include "row_gather.h"

#include <math.h>

enum { PNA_MEAN = 0, PNA_MIN = 1, PNA_MAX = 2, PNA_STD = 3, PNA_VAR = 4, PNA_SUM = 5 };
enum { PNA_IDENTITY = 0, PNA_AMPLIFICATION = 1, PNA_ATTENUATION = 2, PNA_LINEAR = 3, PNA_INVERSE_LINEAR = 4 };
#define PNA_STD_EPS 1e-5f
#define PNA_NSTAT 6        // mean, min, max, var, ties_min, ties_max of b per (row, feature)

struct PnaCfg {
    int n_agg, n_scal, agg_code, scal_code;      // codes: 3 bits per entry, first entry in the low bits
    float avg_log, avg_lin;
};
__device__ __forceinline__ int pna_code(int code, int k) { return (code >> (3 * k)) & 7; }

__device__ __forceinline__ float pna_scaler(int kind, int d, float avg_log, float avg_lin) {
    const float df = (float)d, d1 = (float)(d > 1 ? d : 1);
    switch (kind) {
        case PNA_AMPLIFICATION: return logf(df + 1.f) / avg_log;
        case PNA_ATTENUATION: return avg_log / logf(d1 + 1.f);
        case PNA_LINEAR: return df / avg_lin;
        case PNA_INVERSE_LINEAR: return avg_lin / d1;
        default: return 1.f;
    }
}

// the running statistics of one lane's VEC features
template <int VEC>
struct PnaAcc {
    float mean[VEC], m2[VEC], mn[VEC], mx[VEC], tn[VEC], tx[VEC];
    int cnt;
    __device__ __forceinline__ void init() {
        cnt = 0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) { mean[v] = 0.f; m2[v] = 0.f; mn[v] = INFINITY; mx[v] = -INFINITY; tn[v] = 0.f; tx[v] = 0.f; }
    }
    __device__ __forceinline__ void extremes(int v, float lo, float tlo, float hi, float thi) {
        if (lo < mn[v]) { mn[v] = lo; tn[v] = tlo; } else if (lo == mn[v]) tn[v] += tlo;
        if (hi > mx[v]) { mx[v] = hi; tx[v] = thi; } else if (hi == mx[v]) tx[v] += thi;
    }
    // one more entry (Welford)
    __device__ __forceinline__ void push(const float (&x)[VEC]) {
        cnt += 1;
        const float inv = 1.f / (float)cnt;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float d = x[v] - mean[v];
            mean[v] = fmaf(d, inv, mean[v]);
            m2[v] = fmaf(d, x[v] - mean[v], m2[v]);
            extremes(v, x[v], 1.f, x[v], 1.f);
        }
    }
    // another set of nb entries with its own (mean, M2, min, max, ties): Chan's update
    __device__ __forceinline__ void merge(int nb, int v, float bmean, float bm2, float bmn, float btn, float bmx, float btx, float wb,
                                          float wab) {
        const float d = bmean - mean[v];
        mean[v] = fmaf(d, wb, mean[v]);
        m2[v] = (m2[v] + bm2) + d * d * wab;
        extremes(v, bmn, btn, bmx, btx);
    }
    // c copies of the value x (a stored self-loop of multiplicity c)
    __device__ __forceinline__ void push_copies(const float (&x)[VEC], int c) {
        const float na = (float)cnt, nb = (float)c, nn = na + nb;
        const float wb = nb / nn, wab = na * nb / nn;
#pragma unroll
        for (int v = 0; v < VEC; ++v) merge(c, v, x[v], 0.f, x[v], nb, x[v], nb, wb, wab);
        cnt += c;
    }
};

struct PnaFwd {
    const float* x;          // [n, F]
    const float* a;          // [n, ld]  a_i (pre_nn's bias inside)
    const float* b;          // [n, ld]  b_j
    const int32_t* loops;    // [n] or NULL
    float* z;                // [n, (1 + n_agg n_scal) F]
    float* stats;            // [n, PNA_NSTAT, F]
    int ld, F;
    PnaCfg c;
};

// row i of post_nn's operand and of the saved statistics from the finished accumulators; d = the row's in-degree (loops included)
template <int VEC>
__device__ __forceinline__ void pna_emit(const PnaFwd& p, int row, int f0, int d, const PnaAcc<VEC>& acc) {
    const int F = p.F;
    const long long ldz = (long long)(1 + p.c.n_agg * p.c.n_scal) * F;
    float* __restrict__ zr = p.z + (long long)row * ldz + f0;
    float* __restrict__ sr = p.stats + (long long)row * PNA_NSTAT * F + f0;
    float xr[VEC], ar[VEC], val[6][VEC], st[PNA_NSTAT][VEC];
    vec_load<VEC>(p.x + (long long)row * F + f0, xr);
    vec_store<VEC>(zr, xr);
    vec_load<VEC>(p.a + (long long)row * p.ld + f0, ar);
    const float df = (float)d;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        if (d > 0) {
            const float var = fmaxf(acc.m2[v] / df, 0.f);
            st[0][v] = acc.mean[v]; st[1][v] = acc.mn[v]; st[2][v] = acc.mx[v]; st[3][v] = var; st[4][v] = acc.tn[v]; st[5][v] = acc.tx[v];
            const float mean_m = ar[v] + acc.mean[v];
            val[PNA_MEAN][v] = mean_m; val[PNA_MIN][v] = ar[v] + acc.mn[v]; val[PNA_MAX][v] = ar[v] + acc.mx[v];
            val[PNA_STD][v] = sqrtf(var + PNA_STD_EPS); val[PNA_VAR][v] = var; val[PNA_SUM][v] = df * mean_m;
        } else {                                       // no incoming message: 0, 0, 0, sqrt(eps)
#pragma unroll
            for (int q = 0; q < PNA_NSTAT; ++q) st[q][v] = 0.f;
            val[PNA_MEAN][v] = 0.f; val[PNA_MIN][v] = 0.f; val[PNA_MAX][v] = 0.f;
            val[PNA_STD][v] = sqrtf(PNA_STD_EPS); val[PNA_VAR][v] = 0.f; val[PNA_SUM][v] = 0.f;
        }
    }
#pragma unroll
    for (int q = 0; q < PNA_NSTAT; ++q) vec_store<VEC>(sr + (long long)q * F, st[q]);
    for (int s = 0; s < p.c.n_scal; ++s) {
        const float sc = pna_scaler(pna_code(p.c.scal_code, s), d, p.c.avg_log, p.c.avg_lin);
        for (int k = 0; k < p.c.n_agg; ++k) {
            const int kind = pna_code(p.c.agg_code, k);
            float o[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float t = val[0][v];
#pragma unroll
                for (int q = 1; q < 6; ++q) t = kind == q ? val[q][v] : t;       // (a select chain: no dynamically indexed registers)
                o[v] = sc * t;
            }
            vec_store<VEC>(zr + (long long)(1 + s * p.c.n_agg + k) * F, o);
        }
    }
}

// acc takes the rows b[csr[t]], t in [beg, end), of this lane's columns f0 .. f0 + VEC (active: f0 < F).  An index outside [0, n)
// raises GRAPES_STATUS_BAD_INDEX and the entry is dropped.
template <int VEC, int LPR>
__device__ __forceinline__ void pna_gather(const float* __restrict__ b, int ld, const int32_t* __restrict__ csr, int n, int beg, int end,
                                           int f0, bool active, int l, PnaAcc<VEC>& acc, int32_t* status) {
    constexpr int U = 4;
    for (int t0 = beg; t0 < end; t0 += LPR) {
        const int idx = batch_entry(csr, t0 + l, end, n, status);
        const int cnt = end - t0 < LPR ? end - t0 : LPR;
        for (int k = 0; k < cnt; k += U) {
            float hv[U][VEC];
            int ik[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int src = __shfl(idx, k + u, LPR);
                ik[u] = k + u < cnt ? src : -1;
#pragma unroll
                for (int v = 0; v < VEC; ++v) hv[u][v] = 0.f;
                if (ik[u] >= 0 && active) vec_load<VEC>(b + (long long)ik[u] * ld + f0, hv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ik[u] >= 0) acc.push(hv[u]);
        }
    }
}

template <int VEC, int LPR>
__global__ __launch_bounds__(256) void pna_rows_k(PnaFwd p, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                  int n_host, const int32_t* d_n, int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        if (skip_long && end - beg > GRAPES_LONG_ROW) continue;
        const int lp = p.loops ? p.loops[row] : 0;
        for (int c0 = 0; c0 < p.F; c0 += LPR * VEC) {
            const int f0 = c0 + l * VEC;
            const bool active = f0 < p.F;
            PnaAcc<VEC> acc;
            acc.init();
            pna_gather<VEC, LPR>(p.b, p.ld, csr, n, beg, end, f0, active, l, acc, status);
            if (active) {
                if (lp > 0) {
                    float br[VEC];
                    vec_load<VEC>(p.b + (long long)row * p.ld + f0, br);
                    acc.push_copies(br, lp);
                }
                pna_emit<VEC>(p, row, f0, end - beg + (lp > 0 ? lp : 0), acc);
            }
        }
    }
}

// one group per work item (row, chunk): the chunk's statistics -> pacc[it][PNA_NSTAT][F] (var's slot holds M2), pcnt[it]
template <int VEC, int LPR>
__global__ __launch_bounds__(256) void pna_chunks_k(const float* __restrict__ b, int ld, int F, const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ csr, int n_host, const int32_t* d_n,
                                                    const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                    int item_cap, float* __restrict__ pacc, int32_t* __restrict__ pcnt, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        item_range(items, it, rowptr, n, row, beg, end);
        for (int c0 = 0; c0 < F; c0 += LPR * VEC) {
            const int f0 = c0 + l * VEC;
            const bool active = f0 < F;
            PnaAcc<VEC> acc;
            acc.init();
            pna_gather<VEC, LPR>(b, ld, csr, n, beg, end, f0, active, l, acc, status);
            if (active) {
                float* __restrict__ pr = pacc + (long long)it * PNA_NSTAT * F + f0;
                vec_store<VEC>(pr, acc.mean); vec_store<VEC>(pr + F, acc.mn); vec_store<VEC>(pr + 2LL * F, acc.mx);
                vec_store<VEC>(pr + 3LL * F, acc.m2); vec_store<VEC>(pr + 4LL * F, acc.tn); vec_store<VEC>(pr + 5LL * F, acc.tx);
            }
            if (c0 == 0 && l == 0) pcnt[it] = acc.cnt;
        }
    }
}

// The item with chunk 0 leads its row: its nc items are contiguous and in chunk order.  One workgroup per long row, a thread per
// column: the chunks merged in chunk order, then the stored loops and the epilogue of pna_rows_k.
__global__ __launch_bounds__(256) void pna_combine_k(PnaFwd p, const int32_t* __restrict__ rowptr, int n_host, const int32_t* d_n,
                                                     const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                     int item_cap, const float* __restrict__ pacc, const int32_t* __restrict__ pcnt) {
    const int n = eff_count(d_n, n_host);
    const int F = p.F;
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        const int len = rowptr[row + 1] - rowptr[row];
        const int lp = p.loops ? p.loops[row] : 0;
        for (int f = threadIdx.x; f < F; f += 256) {
            PnaAcc<1> acc;
            acc.init();
            for (int c = 0; c < nc; ++c) {
                const int nb = pcnt[it + c];
                if (nb <= 0) continue;
                const float* __restrict__ pr = pacc + (long long)(it + c) * PNA_NSTAT * F + f;
                const float na = (float)acc.cnt, fb = (float)nb, nn = na + fb;
                acc.merge(nb, 0, pr[0], pr[3LL * F], pr[F], pr[4LL * F], pr[2LL * F], pr[5LL * F], fb / nn, na * fb / nn);
                acc.cnt += nb;
            }
            if (lp > 0) {
                const float br[1] = {p.b[(long long)row * p.ld + f]};
                acc.push_copies(br, lp);
            }
            pna_emit<1>(p, row, f, len + (lp > 0 ? lp : 0), acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ backward
// Row-local, a thread per (row, feature): coef[row] = [Gm | Gv | Gmin | Gmax] and da[row] (see the head of the file).
__global__ __launch_bounds__(256) void pna_fold_k(const float* __restrict__ dz, const float* __restrict__ stats,
                                                  const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ loops, PnaCfg c,
                                                  float* __restrict__ coef, float* __restrict__ da, int ld_d, int n_host,
                                                  const int32_t* d_n, int F) {
    const long long total = (long long)eff_count(d_n, n_host) * F;
    const long long ldz = (long long)(1 + c.n_agg * c.n_scal) * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / F), f = (int)(i - (long long)row * F);
        const int lp = loops ? loops[row] : 0;
        const int d = rowptr_t[row + 1] - rowptr_t[row] + (lp > 0 ? lp : 0);
        float gmean = 0.f, gmin = 0.f, gmax = 0.f, gvar = 0.f;
        float* __restrict__ cr = coef + (long long)row * 4 * F + f;
        if (d > 0) {
            const float* __restrict__ sr = stats + (long long)row * PNA_NSTAT * F + f;
            const float var = sr[3LL * F], df = (float)d;
            const float* __restrict__ zr = dz + (long long)row * ldz + f;
            for (int s = 0; s < c.n_scal; ++s) {
                const float sc = pna_scaler(pna_code(c.scal_code, s), d, c.avg_log, c.avg_lin);
                for (int k = 0; k < c.n_agg; ++k) {
                    const float g = sc * zr[(long long)(1 + s * c.n_agg + k) * F];
                    switch (pna_code(c.agg_code, k)) {
                        case PNA_MEAN: gmean += g; break;
                        case PNA_SUM: gmean = fmaf(df, g, gmean); break;
                        case PNA_MIN: gmin += g; break;
                        case PNA_MAX: gmax += g; break;
                        case PNA_VAR: gvar += g; break;
                        default: gvar = fmaf(g, 0.5f / sqrtf(var + PNA_STD_EPS), gvar); break;       // std
                    }
                }
            }
            if (!(var > 0.f)) gvar = 0.f;                     // the relu under the variance
            cr[0] = gmean / df;
            cr[F] = 2.f * gvar / df;
            const float tn = sr[4LL * F], tx = sr[5LL * F];
            cr[2LL * F] = tn > 0.f ? gmin / tn : 0.f;
            cr[3LL * F] = tx > 0.f ? gmax / tx : 0.f;
        } else {
            cr[0] = 0.f; cr[F] = 0.f; cr[2LL * F] = 0.f; cr[3LL * F] = 0.f;
        }
        da[(long long)row * ld_d + f] = gmean + gmin + gmax;
    }
}

struct PnaBwd {
    const float* b;          // [n, ld]
    const float* stats;      // [n, PNA_NSTAT, F]
    const float* coef;       // [n, 4, F]
    const int32_t* loops;
    float* db;               // [n, ld_d]
    int ld, ld_d, F;
};

// this lane's share of d b_j from the target row i
template <int VEC>
__device__ __forceinline__ void pna_bwd_term(const PnaBwd& p, int i, int f0, const float (&bj)[VEC], float w, float (&acc)[VEC]) {
    const float* __restrict__ cr = p.coef + (long long)i * 4 * p.F + f0;
    const float* __restrict__ sr = p.stats + (long long)i * PNA_NSTAT * p.F + f0;
    float gm[VEC], gv[VEC], gn[VEC], gx[VEC], mean[VEC], mn[VEC], mx[VEC];
    vec_load<VEC>(cr, gm); vec_load<VEC>(cr + p.F, gv); vec_load<VEC>(cr + 2LL * p.F, gn); vec_load<VEC>(cr + 3LL * p.F, gx);
    vec_load<VEC>(sr, mean); vec_load<VEC>(sr + p.F, mn); vec_load<VEC>(sr + 2LL * p.F, mx);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        float t = fmaf(gv[v], bj[v] - mean[v], gm[v]);
        t += bj[v] == mx[v] ? gx[v] : 0.f;
        t += bj[v] == mn[v] ? gn[v] : 0.f;
        acc[v] = fmaf(w, t, acc[v]);
    }
}

template <int VEC, int LPR>
__device__ __forceinline__ void pna_bwd_gather(const PnaBwd& p, const int32_t* __restrict__ csr, int n, int beg, int end, int f0,
                                               bool active, int l, const float (&bj)[VEC], float (&acc)[VEC], int32_t* status) {
    for (int t0 = beg; t0 < end; t0 += LPR) {
        const int idx = batch_entry(csr, t0 + l, end, n, status);
        const int cnt = end - t0 < LPR ? end - t0 : LPR;
        for (int k = 0; k < cnt; ++k) {
            const int i = __shfl(idx, k, LPR);
            if (i >= 0 && active) pna_bwd_term<VEC>(p, i, f0, bj, 1.f, acc);
        }
    }
}

template <int VEC, int LPR>
__global__ __launch_bounds__(256) void pna_bwd_rows_k(PnaBwd p, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                      int n_host, const int32_t* d_n, int skip_long, int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int row = blockIdx.x * G + threadIdx.x / LPR; row < n; row += gridDim.x * G) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        if (skip_long && end - beg > GRAPES_LONG_ROW) continue;
        const int lp = p.loops ? p.loops[row] : 0;
        for (int c0 = 0; c0 < p.F; c0 += LPR * VEC) {
            const int f0 = c0 + l * VEC;
            const bool active = f0 < p.F;
            float bj[VEC], acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) { bj[v] = 0.f; acc[v] = 0.f; }
            if (active) vec_load<VEC>(p.b + (long long)row * p.ld + f0, bj);
            pna_bwd_gather<VEC, LPR>(p, csr, n, beg, end, f0, active, l, bj, acc, status);
            if (active) {
                if (lp > 0) pna_bwd_term<VEC>(p, row, f0, bj, (float)lp, acc);
                vec_store<VEC>(p.db + (long long)row * p.ld_d + f0, acc);
            }
        }
    }
}

template <int VEC, int LPR>
__global__ __launch_bounds__(256) void pna_bwd_chunks_k(PnaBwd p, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr,
                                                        int n_host, const int32_t* d_n, const int32_t* __restrict__ items,
                                                        const int32_t* __restrict__ d_n_items, int item_cap, float* __restrict__ pacc,
                                                        int32_t* status) {
    const int n = eff_count(d_n, n_host);
    const int n_items = item_count(d_n_items, item_cap);
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int it = blockIdx.x * G + threadIdx.x / LPR; it < n_items; it += gridDim.x * G) {
        int row, beg, end;
        const bool ok = item_range(items, it, rowptr, n, row, beg, end);
        for (int c0 = 0; c0 < p.F; c0 += LPR * VEC) {
            const int f0 = c0 + l * VEC;
            const bool active = f0 < p.F;
            float bj[VEC], acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) { bj[v] = 0.f; acc[v] = 0.f; }
            if (active && ok) vec_load<VEC>(p.b + (long long)row * p.ld + f0, bj);
            pna_bwd_gather<VEC, LPR>(p, csr, n, beg, end, f0, active, l, bj, acc, status);
            if (active) vec_store<VEC>(pacc + (long long)it * p.F + f0, acc);
        }
    }
}

__global__ __launch_bounds__(256) void pna_bwd_combine_k(PnaBwd p, const int32_t* __restrict__ rowptr, int n_host, const int32_t* d_n,
                                                         const int32_t* __restrict__ items, const int32_t* __restrict__ d_n_items,
                                                         int item_cap, const float* __restrict__ pacc) {
    const int n = eff_count(d_n, n_host);
    const int F = p.F;
    const int n_items = item_count(d_n_items, item_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        int row, nc;
        if (!item_leads(items, it, n_items, rowptr, n, row, nc)) continue;
        const int lp = p.loops ? p.loops[row] : 0;
        for (int f = threadIdx.x; f < F; f += 256) {
            float acc[1] = {0.f};
            for (int c = 0; c < nc; ++c) acc[0] += pacc[(long long)(it + c) * F + f];
            if (lp > 0) {
                const float bj[1] = {p.b[(long long)row * p.ld + f]};
                pna_bwd_term<1>(p, row, f, bj, (float)lp, acc);
            }
            p.db[(long long)row * p.ld_d + f] = acc[0];
        }
    }
}

// dst[i, :F] += src[i, :F] over the first n rows (src with its own pitch)
__global__ __launch_bounds__(256) void pna_add_k(float* __restrict__ dst, const float* __restrict__ src, long long ld_src, int n_host,
                                                 const int32_t* d_n, int F) {
    const long long total = (long long)eff_count(d_n, n_host) * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long row = i / F, f = i - row * F;
        dst[i] += src[row * ld_src + f];
    }
}

// ------------------------------------------------------------------------------------------------------------ host side

static bool pna_cfg(int32_t n_agg, int32_t agg_code, int32_t n_scal, int32_t scal_code, float avg_log, float avg_lin, PnaCfg* c) {
    if (n_agg < 1 || n_agg > 6 || n_scal < 1 || n_scal > 5) return false;
    for (int k = 0; k < n_agg; ++k)
        if (((agg_code >> (3 * k)) & 7) > PNA_SUM) return false;
    for (int k = 0; k < n_scal; ++k) {
        const int s = (scal_code >> (3 * k)) & 7;
        if (s > PNA_INVERSE_LINEAR) return false;
        if ((s == PNA_AMPLIFICATION || s == PNA_ATTENUATION) && !(avg_log > 0.f)) return false;
        if ((s == PNA_LINEAR || s == PNA_INVERSE_LINEAR) && !(avg_lin > 0.f)) return false;
    }
    c->n_agg = n_agg; c->n_scal = n_scal; c->agg_code = agg_code; c->scal_code = scal_code; c->avg_log = avg_log; c->avg_lin = avg_lin;
    return true;
}

// workspace: [pacc item_cap PNA_NSTAT f] [pcnt item_cap]
extern "C" size_t grapes_pna_aggregate_fwd_workspace_bytes(int32_t item_cap, int32_t f) {
    const size_t I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    return grapes_round16(I * PNA_NSTAT * F * sizeof(float)) + grapes_round16(I * sizeof(int32_t)) + 16;
}

extern "C" int grapes_pna_aggregate_fwd(const float* x, const float* a, const float* b, int32_t ld, const int32_t* loops,
                                        const int32_t* rowptr_t, const int32_t* csr_src, int32_t n_agg, int32_t agg_code,
                                        int32_t n_scal, int32_t scal_code, float avg_log, float avg_lin, float* z, float* stats,
                                        int32_t n, const int32_t* d_n, int32_t f, const int32_t* long_items,
                                        const int32_t* d_n_items, int32_t item_cap, void* workspace, int32_t* status,
                                        grapes_stream_t stream) {
    PnaFwd p;
    if (!x || !a || !b || !rowptr_t || !csr_src || !z || !stats || n < 0 || f < 1 || ld < f) return GRAPES_EINVAL;
    if (!pna_cfg(n_agg, agg_code, n_scal, scal_code, avg_log, avg_lin, &p.c)) return GRAPES_EINVAL;
    if ((int64_t)(1 + n_agg * n_scal) * f > INT32_MAX) return GRAPES_EINVAL;
    if (z == x || z == a || z == b || stats == z) return GRAPES_EINVAL;
    const bool use_items = long_items && d_n_items && workspace && item_cap > 0;
    if (use_items && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = f % 4 == 0 && ld % 4 == 0 && grapes_aligned16(x) && grapes_aligned16(a) && grapes_aligned16(b) && grapes_aligned16(z) &&
                     grapes_aligned16(stats);
    p.x = x; p.a = a; p.b = b; p.loops = loops; p.z = z; p.stats = stats; p.ld = ld; p.F = f;
    ROW_LAUNCH_TILED(pna_rows_k, vec, f, n, s, p, rowptr_t, csr_src, n, d_n, use_items ? 1 : 0, status);
    if (use_items) {
        float* pacc = (float*)workspace;
        int32_t* pcnt = (int32_t*)((char*)workspace + grapes_round16((size_t)item_cap * PNA_NSTAT * f * sizeof(float)));
        ROW_LAUNCH_TILED(pna_chunks_k, vec, f, item_cap, s, b, ld, f, rowptr_t, csr_src, n, d_n, long_items, d_n_items, item_cap, pacc, pcnt,
                   status);
        const int g2 = item_cap < 2048 ? item_cap : 2048;
        hipLaunchKernelGGL(pna_combine_k, dim3(g2), dim3(256), 0, s, p, rowptr_t, n, d_n, long_items, d_n_items, item_cap,
                           (const float*)pacc, (const int32_t*)pcnt);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}

// workspace: [coef n 4 f] [pacc item_cap f]
extern "C" size_t grapes_pna_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f) {
    const size_t N = n > 0 ? (size_t)n : 0, I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    return grapes_round16(N * 4 * F * sizeof(float)) + grapes_round16(I * F * sizeof(float)) + 16;
}

extern "C" int grapes_pna_aggregate_bwd(const float* dz, const float* b, int32_t ld, const float* stats, const int32_t* loops,
                                        const int32_t* rowptr_t, const int32_t* rowptr_s, const int32_t* csr_dst, int32_t n_agg,
                                        int32_t agg_code, int32_t n_scal, int32_t scal_code, float avg_log, float avg_lin, float* da,
                                        float* db, int32_t ld_d, int32_t n, const int32_t* d_n, int32_t f, const int32_t* items_s,
                                        const int32_t* d_n_items_s, int32_t item_cap, void* workspace, int32_t* status,
                                        grapes_stream_t stream) {
    PnaCfg c;
    if (!dz || !b || !stats || !rowptr_t || !rowptr_s || !csr_dst || !da || !db || !workspace || n < 0 || f < 1 || ld < f || ld_d < f)
        return GRAPES_EINVAL;
    if (!pna_cfg(n_agg, agg_code, n_scal, scal_code, avg_log, avg_lin, &c)) return GRAPES_EINVAL;
    if ((int64_t)(1 + n_agg * n_scal) * f > INT32_MAX) return GRAPES_EINVAL;
    if (!grapes_aligned16(workspace)) return GRAPES_EALIGN;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool use_items = items_s && d_n_items_s && item_cap > 0;
    float* coef = (float*)workspace;
    float* pacc = (float*)((char*)workspace + grapes_round16((size_t)n * 4 * f * sizeof(float)));
    hipLaunchKernelGGL(pna_fold_k, dim3(flat_grid(n, f, 1)), dim3(256), 0, s, dz, stats, rowptr_t, loops, c, coef, da, ld_d, n, d_n, f);
    GRAPES_LAUNCH_CHECK();
    const bool vec = f % 4 == 0 && ld % 4 == 0 && ld_d % 4 == 0 && grapes_aligned16(b) && grapes_aligned16(stats) && grapes_aligned16(db);
    PnaBwd p;
    p.b = b; p.stats = stats; p.coef = coef; p.loops = loops; p.db = db; p.ld = ld; p.ld_d = ld_d; p.F = f;
    ROW_LAUNCH_TILED(pna_bwd_rows_k, vec, f, n, s, p, rowptr_s, csr_dst, n, d_n, use_items ? 1 : 0, status);
    if (use_items) {
        ROW_LAUNCH_TILED(pna_bwd_chunks_k, vec, f, item_cap, s, p, rowptr_s, csr_dst, n, d_n, items_s, d_n_items_s, item_cap, pacc, status);
        const int g2 = item_cap < 2048 ? item_cap : 2048;
        hipLaunchKernelGGL(pna_bwd_combine_k, dim3(g2), dim3(256), 0, s, p, rowptr_s, n, d_n, items_s, d_n_items_s, item_cap,
                           (const float*)pacc);
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int grapes_pna_add_input_grad(float* dx, const float* dz, int32_t ld_z, int32_t n, const int32_t* d_n, int32_t f,
                                         grapes_stream_t stream) {
    if (!dx || !dz || n < 0 || f < 1 || ld_z < f) return GRAPES_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(pna_add_k, dim3(flat_grid(n, f, 1)), dim3(256), 0, (hipStream_t)stream, dx, dz, (long long)ld_z, n, d_n, f);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
