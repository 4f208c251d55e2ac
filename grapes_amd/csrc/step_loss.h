// The pieces of the step's loss launch (loss_kernels.hip: step_losses_mb_k) that the classifier's last aggregation runs as well
// when it carries the losses itself (spmm_kernels.hip: gcn_aggregate_losses_k): the GFlowNet loss, one target row by one
// wavefront, the log-Z sum of one workgroup and the last workgroup's sum of the row losses.  One text, so that both launches
// give the same bits.
#pragma once                 // (after common.h)
#include "row_loss.h"

#define LOSS_MAX_B 4096
#define LOSS_MB_THREADS 256
#define LOSS_MB_MAXROWS 65536

// main.py:272-282 for one thread.  stats: [hops][stride] floats, stats[h*stride + 4] = sum of hop h's log-probs
__device__ __forceinline__ void gflownet_loss_eval(bool has_z, float log_z_raw, float log_z_init,
                                                   const float* __restrict__ stats, int hops, int stride, float cost,
                                                   float loss_coef, int reinforce, float* __restrict__ out) {
    float tot = stats[4];
    for (int h = 1; h < hops; ++h) tot = __fadd_rn(tot, stats[h * stride + 4]);   // main.py:276
    const float lz = has_z ? __fsub_rn(log_z_raw, log_z_init) : 0.f;
    float loss, scale;
    if (reinforce) {
        loss = __fmul_rn(-tot, cost);                                             // main.py:279
        scale = -cost;
    } else {
        const float inner = __fadd_rn(__fadd_rn(lz, tot), __fmul_rn(loss_coef, cost));
        loss = __fmul_rn(inner, inner);                                           // main.py:282
        scale = __fmul_rn(2.0f, inner);
    }
    out[0] = loss; out[1] = scale; out[2] = lz; out[3] = tot;
}

// What grapes_step_losses adds to the classifier loss in the same workgroup: the mean of the log-Z head's output
// (main.py:228, the sum exactly as reduce_sum_k forms it) and the GFlowNet loss that needs both (main.py:272-282).
struct GfnTail {
    float* out4;                    // NULL = classifier loss only
    const float* zout; int nz; const int32_t* d_nz; float log_z_init;
    const float* stats; int hops, stride; float loss_coef; int reinforce;
    const float* loss_extra;        // NULL, or one float added to the classifier loss (the regulariser of main.py:260-261)
};

// One target row by one wavefront: loss of the row (every lane), its gradient row written.  CrossEntropy or BCE.
__device__ __forceinline__ float loss_row(const float* __restrict__ logits, float* __restrict__ dlogits, int n_rows, int C,
                                          int row, long long gid, const int64_t* __restrict__ labels,
                                          const float* __restrict__ labels_f, int multilabel, float inv, int lane) {
    float loss = 0.f;
    if ((unsigned)row < (unsigned)n_rows) {
        const RowStrided r{logits + (long long)row * C, dlogits + (long long)row * C, C, lane};
        loss = multilabel ? row_loss_bce(r, labels_f + gid * C, inv)
                          : row_loss_ce(r, (int)labels[gid], inv);
    }
    return loss;
}

// where the log-Z sum waits for the last workgroup: one double behind the B row losses (8-byte aligned)
__device__ __forceinline__ double* losses_zslot(float* row_loss, int B) { return reinterpret_cast<double*>(row_loss + ((B + 1) & ~1)); }

// The log-Z sum by ONE workgroup of LOSS_MB_THREADS threads, published to zslot: summed exactly as reduce_sum_k does
// (1024 virtual threads).  dred: 16 doubles of LDS.  All threads must call it.
__device__ __forceinline__ void losses_z_sum(const GfnTail& gt, double* zslot, double* dred) {
    const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
    if (gt.out4 && gt.zout) {     // virtual thread v = tid + 256 q sums x[v], x[v + 1024], ...; virtual wave = v / 64
        const int nz = eff_count(gt.d_nz, gt.nz);
        double zs[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i0 = 0; i0 < nz; i0 += 8 * 1024) {          // 32 independent loads in flight, added in index order
            float xv[8][4];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = i0 + 1024 * u + tid + 256 * q;
                    xv[u][q] = gt.zout[i < nz ? i : nz - 1];   // unconditional, clamped
                }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q) { if (i0 + 1024 * u + tid + 256 * q < nz) zs[q] += (double)xv[u][q]; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { const double w = wave_sum_d(zs[q]); if (lane == 0) dred[wid + 4 * q] = w; }
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < 16; ++w) t += dred[w];
            publish_f64(zslot, t);
        }
    }
}

// The last workgroup (LOSS_MB_THREADS threads) to finish: sum of the published row losses in block_sum_fixed's order for 1024
// threads (virtual thread v owns rows v, v + 1024, ...; butterfly inside a virtual wave; virtual waves in index order), the
// classifier loss, the GFlowNet loss, and the ticket back to zero.  fred: 16 floats of LDS.  All threads must call it.
__device__ __forceinline__ void losses_finish(const float* row_loss, int B, float inv, const GfnTail& gt, const double* zslot,
                                              float* __restrict__ loss_out, unsigned* __restrict__ ticket, float* fred) {
    const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < B; i0 += 1024) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + tid + 256 * q;
            if (i < B) ls[q] += __int_as_float(__hip_atomic_load((const int*)(row_loss + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float w = wave_sum(ls[q]); if (lane == 0) fred[wid + 4 * q] = w; }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += fred[w];
        const float loss = t * inv + (gt.loss_extra ? *gt.loss_extra : 0.f);
        *loss_out = loss;
        *ticket = 0u;
        if (gt.out4) {
            float zmean = 0.f;
            if (gt.zout) {
                const int nz = eff_count(gt.d_nz, gt.nz);
                const double zt = __longlong_as_double(__hip_atomic_load((const long long*)zslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                zmean = (float)(nz > 0 ? zt / (double)nz : 0.0 / 0.0);
            }
            gflownet_loss_eval(gt.zout != nullptr, zmean, gt.log_z_init, gt.stats, gt.hops, gt.stride, loss, gt.loss_coef,
                               gt.reinforce, gt.out4);
        }
    }
}
