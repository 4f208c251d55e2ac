// The aggregation SAGEConv and ClusterGCNConv share (grapes_rootsum_aggregate_fwd / _bwd), on the plain-sum gather of row_sum.h over
// the CSRs grapes_gcn_prepare builds (duplicates by multiplicity):
//   out[i] = act(s_i (sum_{j in row i} src[j] + c_i src[i]) + add[i] + bias),  c_i = loops[i] + (self_term ? self_weight : 0),
//   s_i = 1 (GRAPES_ROOTSUM_SCALE_NONE), 1 / deg_i (_MEAN; 0 for deg_i = 0) or 1 / (1 + deg_i) (_MEAN_PLUS_ONE),
//   deg_i = (rowptr[i + 1] - rowptr[i]) + loops[i]: the scale is applied ONCE per row, there is no per-edge weight.
// SAGEConv [PyG-recall: torch_geometric 2.5.2]: the stored loops, no self term, mean or none (sum); an empty row aggregates to 0.
// ClusterGCNConv [PyG-recall]: loops = NULL (the CSRs are loop-free), the self term with self_weight = 1 + diag_lambda, mean-plus-one.
// src, add, out (and copy: copy[i] = src[i], the root operand of the aggregate-first form) have their own leading dimensions, so
// halves of one GEMM output are used in place.
//   row_sum_rows_k / row_sum_chunks_k / row_sum_combine_k   the shared kernels; RootSumEpi below is their epilogue
//   row_gate_k / row_colsum_k      backward (row_gate.h): g = dout gated by relu_out > 0, dadd = g, gs = s g, and the column sums of g as
//                                  per-slab partials added in a fixed order
// The backward propagation is the SAME gather over the by-source CSR on the pre-scaled rows gs, with s = 1.  No float atomics: every
// sum has a fixed order (entry order inside a row, chunk order across work items, slab order for the bias), two runs are
// bit-identical.  No kernel waits on another workgroup.
#include "row_sum.h"
#include "row_gate.h"

// s of a row of deg entries (its stored loops counted): 1, 1 / deg (0 for an empty row) or 1 / (1 + deg) — one division
__device__ __forceinline__ float rootsum_scale(int scale, int deg) {
    if (scale == GRAPES_ROOTSUM_SCALE_NONE) return 1.f;
    const int d = scale == GRAPES_ROOTSUM_SCALE_MEAN_PLUS_ONE ? 1 + deg : deg;
    return d > 0 ? 1.0f / (float)d : 0.f;
}

// The epilogue of the shared row sum (row_sum.h), p = the row's sum + loops[row] src[row]:
//   out[row] = act(s (p + self_weight src[row]) + add[row] + bias);  copy[row] = src[row] (every row, long or not).  The self term runs
//   iff self_term, whatever self_weight holds (a weight of 0 still multiplies: signed zeros and non-finite rows keep their bits), and
//   src[row] is not read without it.  add, bias, loops and copy are optional.
struct RootSumEpi {
    const float* src; long long ld_src;
    const int32_t* loops;
    const float* add; long long ld_add;
    const float* bias;
    float* out; long long ld_out;
    float* copy; long long ld_copy;
    float self_weight;
    int self_term, scale, relu;

    template <int VEC, int LPR, int NS>
    __device__ __forceinline__ void pre(int row, int F, int l) const {
        if (!copy) return;
        float xr[NS][VEC];
        row_load_ld<VEC, LPR, NS>(src, row, ld_src, F, l, xr);
        row_store_ld<VEC, LPR, NS>(copy, row, ld_copy, F, l, xr);
    }
    template <int VEC, int LPR, int NS>
    __device__ __forceinline__ void finish(float (&acc)[NS][VEC], int row, int deg, int F, int l) const {
        const float sc = rootsum_scale(scale, deg);
        float ad[NS][VEC];
        if (self_term) {
            float xr[NS][VEC];
            row_load_ld<VEC, LPR, NS>(src, row, ld_src, F, l, xr);
            slab_fma<VEC, NS>(self_weight, xr, acc);
        }
        if (add) row_load_ld<VEC, LPR, NS>(add, row, ld_add, F, l, ad);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float o = acc[s][v] * sc;
                if (add) o += ad[s][v];
                const int f = (s * LPR + l) * VEC + v;
                if (bias && f < F) o += bias[f];
                acc[s][v] = relu ? fmaxf(o, 0.f) : o;
            }
        row_store_ld<VEC, LPR, NS>(out, row, ld_out, F, l, acc);
    }
    __device__ __forceinline__ void finish_col(float a, int row, int deg, int, int f) const {
        if (self_term) a = fmaf(self_weight, src[(long long)row * ld_src + f], a);
        float o = a * rootsum_scale(scale, deg);
        if (add) o += add[(long long)row * ld_add + f];
        if (bias) o += bias[f];
        out[(long long)row * ld_out + f] = relu ? fmaxf(o, 0.f) : o;
    }
};

// s of a row for the backward's gate pass (row_gate.h): always from the by-target row pointers
struct RootSumScale {
    const int32_t* loops; const int32_t* rowptr_t; int scale;
    __device__ __forceinline__ float operator()(int row) const {
        if (scale == GRAPES_ROOTSUM_SCALE_NONE) return 1.f;
        return rootsum_scale(scale, (rowptr_t[row + 1] - rowptr_t[row]) + (loops ? loops[row] : 0));
    }
};

// ------------------------------------------------------------------------------------------------------------ host side

static inline bool rootsum_vec_ok(const void* p, int64_t ld) { return !p || (grapes_aligned16(p) && ld % 4 == 0); }
static inline bool rootsum_scale_ok(int32_t scale) {
    return scale == GRAPES_ROOTSUM_SCALE_NONE || scale == GRAPES_ROOTSUM_SCALE_MEAN || scale == GRAPES_ROOTSUM_SCALE_MEAN_PLUS_ONE;
}

// workspace: [pacc item_cap f] [gs n f] [part slabs f]
extern "C" size_t grapes_rootsum_aggregate_workspace_bytes(int32_t n, int32_t item_cap, int32_t f) {
    const size_t N = n > 0 ? (size_t)n : 0, I = item_cap > 0 ? (size_t)item_cap : 0, F = f > 0 ? (size_t)f : 1;
    return grapes_round16(I * F * sizeof(float)) + grapes_round16(N * F * sizeof(float)) +
           grapes_round16(row_gate_slabs(n) * F * sizeof(float)) + 16;
}

extern "C" int grapes_rootsum_aggregate_fwd(const float* src, int64_t ld_src, const float* add, int64_t ld_add, const float* bias,
                                            const int32_t* loops, const int32_t* rowptr_t, const int32_t* csr_src, float self_weight,
                                            int32_t self_term, int32_t scale, int32_t relu, float* out, int64_t ld_out, float* copy_out,
                                            int64_t ld_copy, int32_t n, const int32_t* d_n, int32_t f, const int32_t* long_items,
                                            const int32_t* d_n_items, int32_t item_cap, void* workspace, int32_t* status,
                                            grapes_stream_t stream) {
    if (!src || !rowptr_t || !csr_src || !out || n < 0 || f < 1 || !rootsum_scale_ok(scale)) return GRAPES_EINVAL;
    if (ld_src < f || ld_out < f || (add && ld_add < f) || (copy_out && ld_copy < f)) return GRAPES_EINVAL;
    if (out == src || copy_out == src || (copy_out && copy_out == out)) return GRAPES_EINVAL;
    const bool use_items = long_items && d_n_items && workspace && item_cap > 0;
    if (use_items && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const int shape = gather_shape(f, rootsum_vec_ok(src, ld_src) && rootsum_vec_ok(add, ld_add) && rootsum_vec_ok(out, ld_out) &&
                                    rootsum_vec_ok(copy_out, ld_copy) && (!bias || grapes_aligned16(bias)));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    RootSumEpi epi;
    epi.src = src; epi.ld_src = ld_src; epi.loops = loops; epi.add = add; epi.ld_add = ld_add; epi.bias = bias;
    epi.out = out; epi.ld_out = ld_out; epi.copy = copy_out; epi.ld_copy = ld_copy; epi.self_weight = self_weight;
    epi.self_term = self_term ? 1 : 0; epi.scale = scale; epi.relu = relu ? 1 : 0;
    return row_sum_propagate<4>(epi, rowptr_t, csr_src, n, d_n, f, shape == 0, use_items ? long_items : nullptr, d_n_items, item_cap,
                                (float*)workspace, status, (hipStream_t)stream);
}

extern "C" int grapes_rootsum_aggregate_bwd(const float* dout, int64_t ld_dout, const float* relu_out, int64_t ld_relu,
                                            const int32_t* loops, const int32_t* rowptr_t, const int32_t* rowptr_s,
                                            const int32_t* csr_dst, float self_weight, int32_t self_term, int32_t scale, const float* add,
                                            int64_t ld_add, float* dsrc, int64_t ld_dsrc, float* dadd, int64_t ld_dadd, float* dbias,
                                            int32_t n, const int32_t* d_n, int32_t f, const int32_t* items_s, const int32_t* d_n_items_s,
                                            int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (!dout || !rowptr_t || n < 0 || f < 1 || ld_dout < f || !rootsum_scale_ok(scale)) return GRAPES_EINVAL;
    if (dsrc && (!rowptr_s || !csr_dst || ld_dsrc < f || dsrc == dout || dsrc == dadd)) return GRAPES_EINVAL;
    if ((relu_out && ld_relu < f) || (add && ld_add < f) || (dadd && (ld_dadd < f || dadd == dout))) return GRAPES_EINVAL;
    const bool pass = scale != GRAPES_ROOTSUM_SCALE_NONE || relu_out || dadd || dbias;   // the row-local pass; without it dsrc gathers dout itself
    const bool use_items = dsrc && items_s && d_n_items_s && item_cap > 0;
    if ((pass || use_items) && !workspace) return GRAPES_EINVAL;
    if (workspace && !grapes_aligned16(workspace)) return GRAPES_EALIGN;
    const bool src_ok = pass ? true : rootsum_vec_ok(dout, ld_dout);
    const int shape = gather_shape(f, src_ok && rootsum_vec_ok(add, ld_add) && rootsum_vec_ok(dsrc, ld_dsrc));
    if (shape < 0) return shape;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const size_t I = item_cap > 0 ? (size_t)item_cap : 0;
    float* pacc = (float*)workspace;
    float* gs = workspace ? (float*)((char*)workspace + grapes_round16(I * f * sizeof(float))) : nullptr;
    float* part = workspace ? (float*)((char*)gs + grapes_round16((size_t)n * f * sizeof(float))) : nullptr;
    if (pass) {
        const RootSumScale row_scale{loops, rowptr_t, scale};
        const int rc = row_gate_launch(dout, (long long)ld_dout, relu_out, (long long)ld_relu, row_scale, dsrc ? gs : (float*)nullptr, dadd,
                                       (long long)ld_dadd, part, dbias, n, d_n, f, s);
        if (rc) return rc;
    }
    if (!dsrc) return 0;
    RootSumEpi epi;
    epi.src = pass ? gs : dout; epi.ld_src = pass ? f : ld_dout; epi.loops = loops; epi.add = add; epi.ld_add = ld_add; epi.bias = nullptr;
    epi.out = dsrc; epi.ld_out = ld_dsrc; epi.copy = nullptr; epi.ld_copy = 0; epi.self_weight = self_weight;
    epi.self_term = self_term ? 1 : 0; epi.scale = GRAPES_ROOTSUM_SCALE_NONE; epi.relu = 0;
    return row_sum_propagate<4>(epi, rowptr_s, csr_dst, n, d_n, f, shape == 0, use_items ? items_s : nullptr, d_n_items_s, item_cap, pacc,
                                status, s);
}
