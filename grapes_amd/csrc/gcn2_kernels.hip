// GCN2Conv (GCNII, reference modules/gcn.py:76-117: GCN2Conv(channels, alpha, theta, layer, shared_weights, normalize=False)
// [PyG-recall: torch_geometric 2.5.2]) — the initial-residual propagation and the identity-mapping blend, forward and backward,
// over the CSRs grapes_gcn_prepare builds.  normalize=False: no gcn_norm, no dinv, no implied unit loop; every stored edge counts
// once per occurrence, and the stored self-loops the build drops come back through loops[i] (grapes_gcn2_loop_counts).
//
//   S_i  = (1 - alpha) (sum_{j -> i} x_j + loops[i] x_i) + alpha x0_i                 P'_i = (1 - alpha) (sum ... ) (optional)
//   out  = act(c0 S + c1 T1 [+ c2 T2])          T1 = S W1 (shared) or P' W1, T2 = x0 W2: the project's GEMM entry points
//
//   row_sum_rows_k / row_sum_chunks_k / row_sum_combine_k   the plain-sum gather shared with SAGEConv (row_sum.h): the sum stays
//                     in registers and the epilogue below (G2Epi: scale, x0 blend, the optional second output) writes each output
//                     row once; rows longer than GRAPES_LONG_ROW go through work items added in chunk order
//   gcn2_bwd_sum_k    backward only, when the gradient of S arrives in two pieces: D = ds + ds_add and the x0 gradient, one pass
//   gcn2_mix_fwd_k / gcn2_mix_bwd_k   the blend and its gated backward, one read of every operand
//   gcn2_loops_k / gcn2_loops_csr_k   loops[i] = number of stored edges (i, i)
//
// The backward propagation is the SAME gather over the by-source CSR (dx_j = (1 - alpha) (sum_{j -> i} D_i + loops[j] D_j)):
// no floating-point atomics anywhere, every sum has a fixed order (entry order inside a row, chunk order across work items), so
// two runs are bit-identical.  No kernel waits on another workgroup.
#include "row_sum.h"

// The epilogue of the shared row sum (row_sum.h), p = the row's sum + loops[row] src[row]:
//   q = c_acc p;  out1[row] = q + c_self self_mat[row];  out2[row] = q;  aux[row] (+)= c_aux src[row] (every row, long or not).
// self_mat, loops, out2 and aux are optional.  Every matrix has rows F = ld_src floats apart.
struct G2Epi {
    const float* src; int ld_src;
    const int32_t* loops;
    const float* self_mat;
    float* out1;
    float* out2;
    float* aux;
    float c_acc, c_self, c_aux;
    int aux_accumulate;

    template <int VEC, int LPR, int NS>
    __device__ __forceinline__ void pre(int row, int F, int l) const {
        if (!aux) return;
        float d[NS][VEC], a[NS][VEC];
        row_load<VEC, LPR, NS>(src, row, F, l, d);
        if (aux_accumulate) row_load<VEC, LPR, NS>(aux, row, F, l, a);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) d[s][v] = aux_accumulate ? fmaf(c_aux, d[s][v], a[s][v]) : c_aux * d[s][v];
        row_store<VEC, LPR, NS>(aux, row, F, l, d);
    }
    template <int VEC, int LPR, int NS>
    __device__ __forceinline__ void finish(float (&acc)[NS][VEC], int row, int, int F, int l) const {
        slab_scale<VEC, NS>(acc, c_acc);
        if (out2) row_store<VEC, LPR, NS>(out2, row, F, l, acc);
        if (self_mat) {
            float x0[NS][VEC];
            row_load<VEC, LPR, NS>(self_mat, row, F, l, x0);
            slab_fma<VEC, NS>(c_self, x0, acc);
        }
        row_store<VEC, LPR, NS>(out1, row, F, l, acc);
    }
    __device__ __forceinline__ void finish_col(float a, int row, int, int F, int f) const {
        const long long o = (long long)row * F + f;
        a *= c_acc;
        if (out2) out2[o] = a;
        out1[o] = self_mat ? fmaf(c_self, self_mat[o], a) : a;
    }
};

// D = ds + ds_add;  dx0 (+)= alpha (add_is_p ? ds : D) + dx0_add   over the first n rows, flat (VEC elements per thread)
template <int VEC>
__global__ __launch_bounds__(256) void gcn2_bwd_sum_k(const float* __restrict__ ds, const float* __restrict__ ds_add, int add_is_p,
                                                      const float* dx0_add, float alpha, float* __restrict__ dsum,
                                                      float* dx0, int accumulate, int n_host, const int32_t* d_n, int F) {
    const long long total = (long long)eff_count(d_n, n_host) * F / VEC;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float a[VEC], b[VEC], c[VEC], o[VEC], d[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const long long j = i * VEC + v;
            a[v] = ds[j];
            b[v] = ds_add ? ds_add[j] : 0.f;
            c[v] = (dx0 && dx0_add) ? dx0_add[j] : 0.f;
            o[v] = (dx0 && accumulate) ? dx0[j] : 0.f;
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            d[v] = a[v] + b[v];
            o[v] = (o[v] + c[v]) + alpha * (add_is_p ? a[v] : d[v]);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const long long j = i * VEC + v;
            dsum[j] = d[v];
            if (dx0) dx0[j] = o[v];
        }
    }
}

// out = act(c0 s + c1 t1 + c2 t2)   (t2 optional)
template <int VEC>
__global__ __launch_bounds__(256) void gcn2_mix_fwd_k(const float* __restrict__ s, const float* __restrict__ t1,
                                                      const float* __restrict__ t2, float c0, float c1, float c2, int relu,
                                                      float* __restrict__ out, int n_host, const int32_t* d_n, int F) {
    const long long total = (long long)eff_count(d_n, n_host) * F / VEC;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (VEC == 4) {
            const float4 a = reinterpret_cast<const float4*>(s)[i], b = reinterpret_cast<const float4*>(t1)[i];
            float4 r = make_float4(fmaf(c1, b.x, c0 * a.x), fmaf(c1, b.y, c0 * a.y), fmaf(c1, b.z, c0 * a.z), fmaf(c1, b.w, c0 * a.w));
            if (t2) {
                const float4 c = reinterpret_cast<const float4*>(t2)[i];
                r.x = fmaf(c2, c.x, r.x); r.y = fmaf(c2, c.y, r.y); r.z = fmaf(c2, c.z, r.z); r.w = fmaf(c2, c.w, r.w);
            }
            if (relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
            reinterpret_cast<float4*>(out)[i] = r;
        } else {
            float r = fmaf(c1, t1[i], c0 * s[i]);
            if (t2) r = fmaf(c2, t2[i], r);
            out[i] = relu ? fmaxf(r, 0.f) : r;
        }
    }
}

// g = dout gated by out > 0 (relu);  g0 = c0 g, g1 = c1 g, g2 = c2 g (g1, g2 optional): one read of dout and out
template <int VEC>
__global__ __launch_bounds__(256) void gcn2_mix_bwd_k(const float* __restrict__ dout, const float* __restrict__ out, int relu, float c0,
                                                      float c1, float c2, float* __restrict__ g0, float* __restrict__ g1,
                                                      float* __restrict__ g2, int n_host, const int32_t* d_n, int F) {
    const long long total = (long long)eff_count(d_n, n_host) * F / VEC;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (VEC == 4) {
            float4 g = reinterpret_cast<const float4*>(dout)[i];
            if (relu) {
                const float4 o = reinterpret_cast<const float4*>(out)[i];
                if (!(o.x > 0.f)) g.x = 0.f;
                if (!(o.y > 0.f)) g.y = 0.f;
                if (!(o.z > 0.f)) g.z = 0.f;
                if (!(o.w > 0.f)) g.w = 0.f;
            }
            reinterpret_cast<float4*>(g0)[i] = make_float4(c0 * g.x, c0 * g.y, c0 * g.z, c0 * g.w);
            if (g1) reinterpret_cast<float4*>(g1)[i] = make_float4(c1 * g.x, c1 * g.y, c1 * g.z, c1 * g.w);
            if (g2) reinterpret_cast<float4*>(g2)[i] = make_float4(c2 * g.x, c2 * g.y, c2 * g.z, c2 * g.w);
        } else {
            float g = dout[i];
            if (relu && !(out[i] > 0.f)) g = 0.f;
            g0[i] = c0 * g;
            if (g1) g1[i] = c1 * g;
            if (g2) g2[i] = c2 * g;
        }
    }
}

// loops[] is zero on entry; integer atomics (the counts do not depend on their order)
__global__ __launch_bounds__(256) void gcn2_loops_k(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int e_host,
                                                    const int32_t* d_e, const int32_t* __restrict__ node_map, int n_host,
                                                    const int32_t* d_n, int32_t* __restrict__ loops) {
    const int e = eff_count(d_e, e_host), n = eff_count(d_n, n_host);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < e; i += (long long)gridDim.x * 256) {
        int a = src[i];
        if (a != dst[i] || a < 0) continue;                      // (node_map is a function: equal global ids are equal local ids)
        if (node_map) a = node_map[a];
        if ((unsigned)a < (unsigned)n) atomicAdd(&loops[a], 1);
    }
}
// one wavefront per row of a 64-bit CSR: the number of entries equal to the row's own id
__global__ __launch_bounds__(256) void gcn2_loops_csr_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n,
                                                        int32_t* __restrict__ loops) {
    const int l = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += gridDim.x * 4) {
        const int64_t beg = rowptr[row], end = rowptr[row + 1];
        int c = 0;
        for (int64_t t = beg + l; t < end; t += 64) c += col[t] == row ? 1 : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
        if (l == 0) loops[row] = c;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side

extern "C" int grapes_gcn2_loop_counts(const int32_t* edge_src, const int32_t* edge_dst, int32_t e, const int32_t* d_e,
                                       const int32_t* node_map, int32_t n, const int32_t* d_n, int32_t* loops,
                                       grapes_stream_t stream) {
    if (!loops || n < 0 || e < 0 || (e > 0 && (!edge_src || !edge_dst))) return GRAPES_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = grapes_zero_async(loops, (size_t)n * sizeof(int32_t), s);
    if (err != hipSuccess) return (int)err;
    if (e == 0) return 0;
    int grid = grapes_div_up(e, 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(gcn2_loops_k, dim3(grid), dim3(256), 0, s, edge_src, edge_dst, e, d_e, node_map, n, d_n, loops);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_gcn2_loop_counts_csr(const int64_t* rowptr, const int32_t* col, int32_t n, int32_t* loops,
                                           grapes_stream_t stream) {
    if (!rowptr || !col || !loops || n < 0) return GRAPES_EINVAL;
    if (n == 0) return 0;
    int grid = grapes_div_up(n, 4); if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(gcn2_loops_csr_k, dim3(grid), dim3(256), 0, (hipStream_t)stream, rowptr, col, n, loops);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// workspace: [pacc item_cap f] [D n f]
extern "C" size_t grapes_gcn2_propagate_workspace_bytes(int32_t n, int32_t item_cap, int32_t f) {
    const size_t N = n > 0 ? (size_t)n : 0, I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    return grapes_round16(I * F * sizeof(float)) + grapes_round16(N * F * sizeof(float)) + 16;
}

extern "C" int grapes_gcn2_propagate_fwd(const float* x, const float* x0, const int32_t* loops, const int32_t* rowptr_t,
                                         const int32_t* csr_src, float alpha, float* s_out, float* p_out, int32_t n,
                                         const int32_t* d_n, int32_t f, const int32_t* long_items, const int32_t* d_n_items,
                                         int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!x || !x0 || !rowptr_t || !csr_src || !s_out || n < 0 || f < 1 || f > 1024) return GRAPES_EINVAL;
    if (s_out == x || s_out == x0 || (p_out && (p_out == x || p_out == x0 || p_out == s_out))) return GRAPES_EINVAL;
    const bool use_items = long_items && d_n_items && workspace && item_cap > 0;
    if (use_items && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    if (n == 0) return 0;
    const bool vec = f % 4 == 0 && grapes_aligned16(x) && grapes_aligned16(x0) && grapes_aligned16(s_out) && (!p_out || grapes_aligned16(p_out));
    G2Epi epi;
    epi.src = x; epi.ld_src = f; epi.self_mat = x0; epi.loops = loops; epi.out1 = s_out; epi.out2 = p_out; epi.aux = nullptr;
    epi.c_acc = 1.f - alpha; epi.c_self = alpha; epi.c_aux = 0.f; epi.aux_accumulate = 0;
    return row_sum_propagate<16>(epi, rowptr_t, csr_src, n, d_n, f, vec, use_items ? long_items : nullptr, d_n_items, item_cap,
                        (float*)workspace, status, (hipStream_t)stream);
}

extern "C" int grapes_gcn2_propagate_bwd(const float* ds, const float* ds_add, int32_t add_is_p, const float* dx0_add,
                                         const int32_t* loops, const int32_t* rowptr_s, const int32_t* csr_dst, float alpha,
                                         float* dx, float* dx0, int32_t accumulate_x0, int32_t n, const int32_t* d_n, int32_t f,
                                         const int32_t* items_s, const int32_t* d_n_items_s, int32_t item_cap, void* workspace,
                                         int32_t* status, grapes_stream_t stream) {
    if (!ds || !rowptr_s || !csr_dst || !dx || n < 0 || f < 1 || f > 1024) return GRAPES_EINVAL;
    if (dx == ds || dx == ds_add || dx == dx0 || (dx0 && (dx0 == ds || dx0 == ds_add))) return GRAPES_EINVAL;
    const bool two = ds_add || dx0_add;
    const bool use_items = items_s && d_n_items_s && workspace && item_cap > 0;
    if (two && !workspace) return GRAPES_EINVAL;
    if ((two || use_items) && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = f % 4 == 0 && grapes_aligned16(ds) && grapes_aligned16(dx) && (!ds_add || grapes_aligned16(ds_add)) &&
                     (!dx0_add || grapes_aligned16(dx0_add)) && (!dx0 || grapes_aligned16(dx0));
    float* pacc = (float*)workspace;
    float* dsum = (float*)((char*)workspace + grapes_round16((size_t)(item_cap > 0 ? item_cap : 0) * f * sizeof(float)));
    G2Epi epi;
    epi.src = ds; epi.ld_src = f; epi.self_mat = nullptr; epi.loops = loops; epi.out1 = dx; epi.out2 = nullptr;
    epi.aux = dx0; epi.c_acc = 1.f - alpha; epi.c_self = 0.f; epi.c_aux = alpha; epi.aux_accumulate = accumulate_x0 ? 1 : 0;
    if (two) {
        if (vec) hipLaunchKernelGGL(gcn2_bwd_sum_k<4>, dim3(flat_grid(n, f, 4)), dim3(256), 0, s, ds, ds_add, add_is_p ? 1 : 0,
                                    dx0_add, alpha, dsum, dx0, accumulate_x0 ? 1 : 0, n, d_n, f);
        else hipLaunchKernelGGL(gcn2_bwd_sum_k<1>, dim3(flat_grid(n, f, 1)), dim3(256), 0, s, ds, ds_add, add_is_p ? 1 : 0,
                                dx0_add, alpha, dsum, dx0, accumulate_x0 ? 1 : 0, n, d_n, f);
        GRAPES_LAUNCH_CHECK();
        epi.src = dsum; epi.aux = nullptr;
    }
    return row_sum_propagate<16>(epi, rowptr_s, csr_dst, n, d_n, f, vec, use_items ? items_s : nullptr, d_n_items_s, item_cap, pacc, status, s);
}

extern "C" int grapes_gcn2_mix_fwd(const float* s_in, const float* t1, const float* t2, float c0, float c1, float c2, int32_t relu,
                                   float* out, int32_t n, const int32_t* d_n, int32_t f, grapes_stream_t stream) {
    if (!s_in || !t1 || !out || n < 0 || f < 1) return GRAPES_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = f % 4 == 0 && grapes_aligned16(s_in) && grapes_aligned16(t1) && grapes_aligned16(out) && (!t2 || grapes_aligned16(t2));
    if (vec) hipLaunchKernelGGL(gcn2_mix_fwd_k<4>, dim3(flat_grid(n, f, 4)), dim3(256), 0, s, s_in, t1, t2, c0, c1, c2, relu, out, n, d_n, f);
    else hipLaunchKernelGGL(gcn2_mix_fwd_k<1>, dim3(flat_grid(n, f, 1)), dim3(256), 0, s, s_in, t1, t2, c0, c1, c2, relu, out, n, d_n, f);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_gcn2_mix_bwd(const float* dout, const float* out, int32_t relu, float c0, float c1, float c2, float* g0,
                                   float* g1, float* g2, int32_t n, const int32_t* d_n, int32_t f, grapes_stream_t stream) {
    if (!dout || !g0 || (relu && !out) || n < 0 || f < 1) return GRAPES_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = f % 4 == 0 && grapes_aligned16(dout) && grapes_aligned16(g0) && (!g1 || grapes_aligned16(g1)) && (!out || grapes_aligned16(out)) &&
                     (!g2 || grapes_aligned16(g2));
    if (vec) hipLaunchKernelGGL(gcn2_mix_bwd_k<4>, dim3(flat_grid(n, f, 4)), dim3(256), 0, s, dout, out, relu, c0, c1, c2, g0, g1, g2, n, d_n, f);
    else hipLaunchKernelGGL(gcn2_mix_bwd_k<1>, dim3(flat_grid(n, f, 1)), dim3(256), 0, s, dout, out, relu, c0, c1, c2, g0, g1, g2, n, d_n, f);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
