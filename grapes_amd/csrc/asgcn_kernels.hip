// AS-GCN: the adaptive layer-wise sampler (Huang et al., "Adaptive Sampling Towards Fast Graph Representation Learning", NeurIPS
// 2018) on the LADIES conventions of ladies_kernels.hip: V = A + I over the DeviceGraph CSR (a stored (i, i) makes v_ii = 2),
// P = D^-1 V with D_i = (rowptr[i + 1] - rowptr[i]) + 1.  The sampler's parameters are w_g fp32[F] and b_g fp32[1].
//
//   asgcn_importance_k<VEC>  one wavefront per candidate j: c_j = sum over the rows i of a set of P_ij by a walk of row j of A^T (the
//                            walk of ladies_importance_k, P_ij instead of P_ij^2), and in the same wavefront the lane-strided dot
//                            product a_j = <x_j, w_g> + b_g over the candidate's feature row (VEC: 16-byte loads); g = max(a, 0) + 1,
//                            q = c g, logq = logf(q)
//   asgcn_shift_k            ONE workgroup: M = max logq, logit = (logq - M) - 20, those two roundings
//   asgcn_rows_init_k        row r of a layer's entry list: its offsets to 0, pos[rows[r]] = r
//   asgcn_row_runs_k         one thread per entry: the runs of edge_dst give each row its [start, end) (the list is row-contiguous)
//   asgcn_variance_k<K>      one wavefront per row: mu = sum_j w_j H_j in a first sweep, then per entry |H_j|^2 and <mu, H_j>:
//                            V = s sum w^2 |H|^2 - |mu|^2 and dw = (2 / m)(s w |H|^2 - <mu, H>)
//   asgcn_sum_k              ONE workgroup: L_var = (sum_r V_r) / m
//   asgcn_gbar_k             one wavefront per row: Gbar = sum_j G_j w_j
//   asgcn_colsum_k           one wavefront per batch node j: T_j += sum over the rows, in row order, of w_ij (G_ij - Gbar_i); lane l
//                            takes the rows l, l + 64, ... and finds j in each by a binary search (a row's sources ascend)
//
// Sum order: as in ladies_kernels.hip — lane-strided partial sums in walk order, then the xor butterfly of wave_sum; every output is
// a function of the input (no float atomics), so two calls give the same bits.  No kernel waits on another workgroup.
#include "common.h"

#define ASGCN_SHIFT_THREADS 1024
#define ASGCN_SUM_THREADS 256

__device__ __forceinline__ bool asgcn_bit(const unsigned long long* __restrict__ bits, int v) {
    return (bits[v >> 6] >> (v & 63)) & 1ull;
}

// 1 / D_i in fp32 (D_i below 2^31 + 1: the wrappers refuse larger graphs)
__device__ __forceinline__ float asgcn_inv_deg(const int64_t* __restrict__ rowptr, int i) {
    return 1.0f / (float)(rowptr[i + 1] - rowptr[i] + 1);
}

template <bool VEC>
__global__ __launch_bounds__(256) void asgcn_importance_k(
        const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t, int N,
        const int32_t* __restrict__ ids, int n_host, const int32_t* __restrict__ d_n, const unsigned long long* __restrict__ prev_bits,
        const float* __restrict__ x, int64_t ldx, int F, const float* __restrict__ w_g, const float* __restrict__ b_g,
        float* __restrict__ c_out, float* __restrict__ a_out, float* __restrict__ q_out, float* __restrict__ logq,
        float* __restrict__ q_table, float* __restrict__ a_table, int32_t* status) {
    const int k = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (k >= n_host) return;                                             // (whole wavefronts leave)
    if (k >= eff_count(d_n, n_host)) return;                             // entries past the live count stay untouched
    const int j = ids ? ids[k] : k;
    if ((unsigned)j >= (unsigned)N) {
        if (lane == 0) {
            if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
            c_out[k] = 0.f; a_out[k] = 0.f; q_out[k] = 0.f; logq[k] = -INFINITY;
        }
        return;
    }
    // the feature row first: its loads are in flight while the transpose row is walked
    const float* __restrict__ xr = x + (int64_t)j * ldx;
    float dot = 0.f;
    if (VEC) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(xr);
        const float4* __restrict__ w4 = reinterpret_cast<const float4*>(w_g);
        for (int ch = lane; ch < (F >> 2); ch += 64) {
            const float4 xv = x4[ch], wv = w4[ch];
            dot = fmaf(xv.x, wv.x, dot); dot = fmaf(xv.y, wv.y, dot); dot = fmaf(xv.z, wv.z, dot); dot = fmaf(xv.w, wv.w, dot);
        }
    } else {
        for (int f = lane; f < F; f += 64) dot = fmaf(xr[f], w_g[f], dot);
    }
    const int64_t t0 = rowptr_t[j], t1 = rowptr_t[j + 1];
    float acc = 0.f;
    bool loop = false;
    for (int64_t t = t0 + lane; t < t1; t += 64) {
        const int i = col_t[t];
        if ((unsigned)i >= (unsigned)N) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); continue; }
        if (i == j) { loop = true; continue; }                           // the stored (j, j): part of the diagonal term
        if (prev_bits && !asgcn_bit(prev_bits, i)) continue;
        acc += asgcn_inv_deg(rowptr, i);
    }
    acc = wave_sum(acc);
    dot = wave_sum(dot);
    if (!prev_bits || asgcn_bit(prev_bits, j)) acc += (__any(loop) ? 2.0f : 1.0f) * asgcn_inv_deg(rowptr, j);
    if (lane == 0) {
        const float a = dot + b_g[0];
        const float g = fmaxf(a, 0.f) + 1.0f;
        const float q = acc * g;
        c_out[k] = acc; a_out[k] = a; q_out[k] = q; logq[k] = logf(q);
        if (q_table) q_table[j] = q;
        if (a_table) a_table[j] = a;
    }
}

// ONE workgroup: logit[k] = (logq[k] - M) - 20 with M = max over the live entries (a bad id's -inf stays -inf); 16-byte loads and
// stores over the part of the arrays that allows them
__device__ __forceinline__ float asgcn_shifted(float l, float M) {
    return l == -INFINITY ? -INFINITY : __fsub_rn(__fsub_rn(l, M), 20.0f);
}

__global__ __launch_bounds__(ASGCN_SHIFT_THREADS) void asgcn_shift_k(const float* __restrict__ logq, int n_host,
                                                                     const int32_t* __restrict__ d_n, float* __restrict__ logit) {
    __shared__ float lds[ASGCN_SHIFT_THREADS / 64];
    const int n = eff_count(d_n, n_host), tid = threadIdx.x;
    const int n4 = ((((uintptr_t)logq | (uintptr_t)logit) & 15) == 0) ? n >> 2 : 0;      // (chunks of four; the rest one by one)
    const float4* __restrict__ q4 = reinterpret_cast<const float4*>(logq);
    float mx = -INFINITY;
    for (int k = tid; k < n4; k += ASGCN_SHIFT_THREADS) {
        const float4 v = q4[k];
        mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
    for (int k = 4 * n4 + tid; k < n; k += ASGCN_SHIFT_THREADS) mx = fmaxf(mx, logq[k]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) lds[tid >> 6] = mx;
    __syncthreads();
    float M = lds[0];
#pragma unroll
    for (int w = 1; w < ASGCN_SHIFT_THREADS / 64; ++w) M = fmaxf(M, lds[w]);
    float4* __restrict__ l4 = reinterpret_cast<float4*>(logit);
    for (int k = tid; k < n4; k += ASGCN_SHIFT_THREADS) {
        const float4 v = q4[k];
        l4[k] = make_float4(asgcn_shifted(v.x, M), asgcn_shifted(v.y, M), asgcn_shifted(v.z, M), asgcn_shifted(v.w, M));
    }
    for (int k = 4 * n4 + tid; k < n; k += ASGCN_SHIFT_THREADS) logit[k] = asgcn_shifted(logq[k], M);
}

// ---------------------------------------------------------------------------------------------- a layer's entry list by rows
// workspace: pos int32[n_local] | start int32[m] | end int32[m] | gbar fp32[m]
__global__ __launch_bounds__(256) void asgcn_rows_init_k(const int32_t* __restrict__ rows, int m, int n_local, int32_t* __restrict__ pos,
                                                         int32_t* __restrict__ start, int32_t* __restrict__ end, int32_t* status) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    start[r] = 0; end[r] = 0;
    const int i = rows[r];
    if ((unsigned)i >= (unsigned)n_local) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); return; }
    pos[i] = r;
}

// pos holds a rank only at the ids of `rows` (the rest of it is whatever the workspace held): an entry whose target is not one of
// the rows reads a word that fails one of the two tests below, belongs to no row and raises the status bit
__global__ __launch_bounds__(256) void asgcn_row_runs_k(const int32_t* __restrict__ edge_dst, int e, int n_local,
                                                        const int32_t* __restrict__ rows, int m, const int32_t* __restrict__ pos,
                                                        int32_t* __restrict__ start, int32_t* __restrict__ end, int32_t* status) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= e) return;
    const int i = edge_dst[t];
    const bool head = t == 0 || edge_dst[t - 1] != i, tail = t == e - 1 || edge_dst[t + 1] != i;
    if (!head && !tail) return;
    int r = -1;
    if ((unsigned)i < (unsigned)n_local) r = pos[i];
    if ((unsigned)r >= (unsigned)m || rows[r] != i) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); return; }
    if (head) start[r] = t;
    if (tail) end[r] = t + 1;
}

// ---------------------------------------------------------------------------------------------- the variance term
// One wavefront per row.  The lanes are (entry slot g, channel cl): cw = min(64, the power of two >= C) channels wide, 64 / cw
// entries side by side, so a narrow H (C = a few classes) still fills the wavefront; above 64 channels lane l holds the channels
// l, l + 64, ... (K of them).  Sweep 1: slot g adds the entries g, g + 64 / cw, ... of the row into its mu, the slots' sums meet in a
// butterfly over the slot bits.  Sweep 2: per entry |H_j|^2 and <mu, H_j> by a butterfly over the channel bits.
template <int K>
__global__ __launch_bounds__(256) void asgcn_variance_k(const int32_t* __restrict__ edge_src, const float* __restrict__ weight,
                                                        const float* __restrict__ H, int C, int n_local, int cw,
                                                        const int32_t* __restrict__ start, const int32_t* __restrict__ end, int m,
                                                        float* __restrict__ V, float* __restrict__ dw, int32_t* status) {
    const int r = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (r >= m) return;
    const int a = start[r], b = end[r], s = b - a;
    if (s <= 0) { if (lane == 0) V[r] = 0.f; return; }
    const int G = 64 / cw, g = lane / cw, cl = lane & (cw - 1);
    float mu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = 0.f;
    for (int t = a + g; t < b; t += G) {
        const int j = edge_src[t];
        if ((unsigned)j >= (unsigned)n_local) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); continue; }
        const float wt = weight[t];
        const float* __restrict__ h = H + (int64_t)j * C;
#pragma unroll
        for (int k = 0; k < K; ++k) { const int c = cl + 64 * k; if (c < C) mu[k] = fmaf(wt, h[c], mu[k]); }
    }
    for (int d = cw; d < 64; d <<= 1) {                                   // (wavefront-uniform: the slots' partial sums)
#pragma unroll
        for (int k = 0; k < K; ++k) mu[k] += __shfl_xor(mu[k], d, 64);
    }
    float mm = 0.f;
    if (g == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) mm = fmaf(mu[k], mu[k], mm);          // (channels at or past C hold 0)
    }
    mm = wave_sum(mm);
    const float sf = (float)s, two_over_m = 2.0f / (float)m;
    float acc = 0.f;
    for (int t0 = a; t0 < b; t0 += G) {                                   // (wavefront-uniform trips)
        const int t = t0 + g;
        const int j = t < b ? edge_src[t] : -1;
        const bool ok = (unsigned)j < (unsigned)n_local;
        float hh = 0.f, mh = 0.f;
        if (ok) {
            const float* __restrict__ h = H + (int64_t)j * C;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int c = cl + 64 * k;
                if (c < C) { const float v = h[c]; hh = fmaf(v, v, hh); mh = fmaf(mu[k], v, mh); }
            }
        }
        for (int d = cw >> 1; d > 0; d >>= 1) { hh += __shfl_xor(hh, d, 64); mh += __shfl_xor(mh, d, 64); }
        if (cl == 0 && t < b) {
            const float wt = ok ? weight[t] : 0.f;
            acc = fmaf(wt * wt, hh, acc);
            dw[t] = ok ? two_over_m * (sf * wt * hh - mh) : 0.f;
        }
    }
    acc = wave_sum(cl == 0 ? acc : 0.f);
    if (lane == 0) V[r] = sf * acc - mm;
}

// ONE workgroup: out[0] = (sum of v[0 .. n)) * scale, thread-strided partial sums, a butterfly, the wavefronts in index order
__global__ __launch_bounds__(ASGCN_SUM_THREADS) void asgcn_sum_k(const float* __restrict__ v, int n, float scale, float* __restrict__ out) {
    __shared__ float lds[ASGCN_SUM_THREADS / 64];
    float acc = 0.f;
    for (int k = threadIdx.x; k < n; k += ASGCN_SUM_THREADS) acc += v[k];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < ASGCN_SUM_THREADS / 64; ++w) t += lds[w];
        out[0] = t * scale;
    }
}

// ---------------------------------------------------------------------------------------------- d L / d logq
__global__ __launch_bounds__(256) void asgcn_gbar_k(const int32_t* __restrict__ edge_src, const float* __restrict__ weight,
                                                    const float* __restrict__ G, const int32_t* __restrict__ start,
                                                    const int32_t* __restrict__ end, int m, int n_local, float* __restrict__ gbar,
                                                    int32_t* status) {
    const int r = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (r >= m) return;
    const int a = start[r], b = end[r];
    float acc = 0.f;
    for (int t = a + lane; t < b; t += 64) {
        if ((unsigned)edge_src[t] >= (unsigned)n_local) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); continue; }
        acc = fmaf(G[t], weight[t], acc);                                 // (a bad source is left out of the mean, as of the column sums)
    }
    acc = wave_sum(acc);
    if (lane == 0) gbar[r] = acc;
}

__global__ __launch_bounds__(256) void asgcn_colsum_k(const int32_t* __restrict__ edge_src, const float* __restrict__ weight,
                                                      const float* __restrict__ G, const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ end, const float* __restrict__ gbar, int m,
                                                      int n_local, float* __restrict__ T) {
    const int j = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (j >= n_local) return;
    float acc = 0.f;
    for (int r = lane; r < m; r += 64) {
        const int a = start[r], len = end[r] - a;
        if (len <= 0) continue;
        const int p = lower_bound(edge_src + a, len, j);
        if (p < len && edge_src[a + p] == j) acc += weight[a + p] * (G[a + p] - gbar[r]);
    }
    acc = wave_sum(acc);
    if (lane == 0) T[j] += acc;
}

// ---------------------------------------------------------------------------------------------- entry points
extern "C" int grapes_asgcn_importance(const int64_t* rowptr, const int64_t* rowptr_t, const int32_t* col_t, int32_t num_nodes,
                                       const int32_t* ids, int32_t n, const int32_t* d_n, const uint64_t* prev_bits, int32_t m,
                                       const int32_t* d_m, const float* x, int64_t ldx, int32_t f, const float* w_g, const float* b_g,
                                       float* c, float* a, float* q, float* logq, float* logit, float* q_table, float* a_table,
                                       int32_t* status, grapes_stream_t stream) {
    (void)d_m;                                                           // (the shift is the layer's maximum: the set's size is not read)
    if (num_nodes <= 0 || n <= 0 || m <= 0 || (!ids && n > num_nodes) || f < 1 || ldx < f) return GRAPES_EINVAL;
    if (!rowptr || !rowptr_t || !col_t || !x || !w_g || !b_g || !c || !a || !q || !logq || !logit) return GRAPES_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long* bits = (const unsigned long long*)prev_bits;
    const dim3 grid(grapes_div_up((int64_t)n * 64, 256));
    if ((f & 3) == 0 && (ldx & 3) == 0 && grapes_aligned16(x) && grapes_aligned16(w_g))
        hipLaunchKernelGGL(asgcn_importance_k<true>, grid, dim3(256), 0, s, rowptr, rowptr_t, col_t, num_nodes, ids, n, d_n, bits, x,
                           ldx, f, w_g, b_g, c, a, q, logq, q_table, a_table, status);
    else
        hipLaunchKernelGGL(asgcn_importance_k<false>, grid, dim3(256), 0, s, rowptr, rowptr_t, col_t, num_nodes, ids, n, d_n, bits, x,
                           ldx, f, w_g, b_g, c, a, q, logq, q_table, a_table, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(asgcn_shift_k, dim3(1), dim3(ASGCN_SHIFT_THREADS), 0, s, (const float*)logq, n, d_n, logit);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t grapes_asgcn_rows_workspace_bytes(int32_t m, int32_t n_local) {
    return ((size_t)(n_local > 0 ? n_local : 1) + 3 * (size_t)(m > 0 ? m : 1)) * 4;
}

struct AsgcnRows { int32_t* pos; int32_t* start; int32_t* end; float* gbar; };

static int asgcn_rows(const int32_t* edge_dst, int e, const int32_t* rows, int m, int n_local, void* workspace, int32_t* status,
                      hipStream_t s, AsgcnRows& R) {
    R.pos = (int32_t*)workspace;
    R.start = R.pos + n_local;
    R.end = R.start + m;
    R.gbar = (float*)(R.end + m);
    hipLaunchKernelGGL(asgcn_rows_init_k, dim3(grapes_div_up(m, 256)), dim3(256), 0, s, rows, m, n_local, R.pos, R.start, R.end, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(asgcn_row_runs_k, dim3(grapes_div_up(e, 256)), dim3(256), 0, s, edge_dst, e, n_local, rows, m,
                       (const int32_t*)R.pos, R.start, R.end, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_asgcn_variance(const int32_t* edge_src, const int32_t* edge_dst, const float* weight, int32_t e,
                                     const int32_t* rows, int32_t m, const float* h, int32_t n_local, int32_t c, float* v,
                                     float* l_var, float* dw, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (e <= 0 || m <= 0 || n_local <= 0 || c < 1 || c > 1024 || (c > 256 && (c & 3))) return GRAPES_EINVAL;
    if (!edge_src || !edge_dst || !weight || !rows || !h || !v || !l_var || !dw || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    AsgcnRows R;
    const int rc = asgcn_rows(edge_dst, e, rows, m, n_local, workspace, status, s, R);
    if (rc) return rc;
    int cw = 1;
    while (cw < c && cw < 64) cw <<= 1;
    const dim3 grid(grapes_div_up((int64_t)m * 64, 256));
#define ASGCN_VARIANCE(K_)                                                                                                   \
    hipLaunchKernelGGL(asgcn_variance_k<K_>, grid, dim3(256), 0, s, edge_src, weight, h, c, n_local, cw, (const int32_t*)R.start, \
                       (const int32_t*)R.end, m, v, dw, status)
    if (c <= 64) ASGCN_VARIANCE(1);
    else if (c <= 128) ASGCN_VARIANCE(2);
    else if (c <= 256) ASGCN_VARIANCE(4);
    else if (c <= 512) ASGCN_VARIANCE(8);
    else ASGCN_VARIANCE(16);
#undef ASGCN_VARIANCE
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(asgcn_sum_k, dim3(1), dim3(ASGCN_SUM_THREADS), 0, s, (const float*)v, m, 1.0f / (float)m, l_var);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_asgcn_logq_bwd(const int32_t* edge_src, const int32_t* edge_dst, const float* weight, const float* g, int32_t e,
                                     const int32_t* rows, int32_t m, int32_t n_local, float* t, void* workspace, int32_t* status,
                                     grapes_stream_t stream) {
    if (e <= 0 || m <= 0 || n_local <= 0) return GRAPES_EINVAL;
    if (!edge_src || !edge_dst || !weight || !g || !rows || !t || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    AsgcnRows R;
    const int rc = asgcn_rows(edge_dst, e, rows, m, n_local, workspace, status, s, R);
    if (rc) return rc;
    hipLaunchKernelGGL(asgcn_gbar_k, dim3(grapes_div_up((int64_t)m * 64, 256)), dim3(256), 0, s, edge_src, weight, g,
                       (const int32_t*)R.start, (const int32_t*)R.end, m, n_local, R.gbar, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(asgcn_colsum_k, dim3(grapes_div_up((int64_t)n_local * 64, 256)), dim3(256), 0, s, edge_src, weight, g,
                       (const int32_t*)R.start, (const int32_t*)R.end, (const float*)R.gbar, m, n_local, t);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
