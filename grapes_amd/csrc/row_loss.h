// The loss of ONE row of logits by ONE wavefront, and its gradient row: mean cross-entropy's softmax minus one-hot, and the stable
// BCE-with-logits row  max(z, 0) - z y + log1p(exp(-|z|))  with  sigmoid(z) - y.  The loss kernels call these two routines; what
// differs between the kernels — how a wavefront HOLDS its row — is the Row argument:
//   RowStrided   lane l reads columns l, l + 64, ... from memory on every pass and stores the gradient as it is formed
//                (loss_row of the step's loss kernels)
//   RowSlots     lane l holds column l + 64 k in register slot k, already transformed (the dropout in front of rl_loss_rows_k); the
//                gradient goes to register slots too
// A Row has  each(f): f(k, c) for every (slot, column) the lane holds;  get(k, c);  put(k, c, gradient).  A call site reads
//     const RowStrided r{z_row, g_row, C, lane};   loss = row_loss_ce(r, label, 1.f / rows);
// Label reading and checking, dropout, dinv and row masks, and the reduction over rows stay with the kernels.  All 64 lanes call;
// the row's loss comes back to every lane.  `inv` scales the gradient (1 / rows, or 1 / (rows C)), not the returned loss.
#pragma once                 // (after common.h: wave_max, wave_sum)

struct RowStrided {
    const float* __restrict__ x; float* __restrict__ g; int C, lane;
    template <class F> __device__ __forceinline__ void each(F f) const { for (int c = lane; c < C; c += 64) f(0, c); }
    __device__ __forceinline__ float get(int, int c) const { return x[c]; }
    __device__ __forceinline__ void put(int, int c, float v) const { g[c] = v; }
};
template <int KMAX>
struct RowSlots {
    const float (&x)[KMAX]; float (&g)[KMAX]; int KC, C, lane;          // KC <= KMAX live slots
    template <class F> __device__ __forceinline__ void each(F f) const {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { const int c = lane + 64 * k; if (k < KC && c < C) f(k, c); }
    }
    __device__ __forceinline__ float get(int k, int) const { return x[k]; }
    __device__ __forceinline__ void put(int k, int, float v) const { g[k] = v; }
};
// Cross-entropy rows are formed shift first, as torch's log_softmax:  lsm = (x - m) - log(se),  p = exp(lsm),  loss = -lsm[y].  The
// row maximum is never added back (lse = m + log(se), p = exp(x - lse)): that sum is rounded at the size of m, so a common offset of
// the row would reach the softmax — 2^-24 |m| of error in every p.

// y outside [0, C): no column matches — loss 0 and the plain softmax as the gradient (the callers that refuse such a label do so first).
template <class Row>
__device__ __forceinline__ float row_loss_ce(const Row& r, long long y, float inv) {
    float m = -INFINITY;
    r.each([&](int k, int c) { m = fmaxf(m, r.get(k, c)); });
    m = wave_max(m);
    float se = 0.f;
    r.each([&](int k, int c) { se += expf(r.get(k, c) - m); });
    se = wave_sum(se);
    const float lse = logf(se);
    float loss = 0.f;
    r.each([&](int k, int c) {
        const float lsm = (r.get(k, c) - m) - lse;                             // log_softmax
        if (c == y) loss = -lsm;
        r.put(k, c, (expf(lsm) - (c == y ? 1.0f : 0.0f)) * inv);
    });
    return wave_sum(loss);                                                     // (one lane holds column y: the others add 0)
}

// t: the row's C targets.
template <class Row>
__device__ __forceinline__ float row_loss_bce(const Row& r, const float* __restrict__ t, float inv) {
    float loss = 0.f;
    r.each([&](int k, int c) {
        const float v = r.get(k, c), y = t[c];
        loss += fmaxf(v, 0.f) - v * y + log1pf(expf(-fabsf(v)));              // stable BCE-with-logits
        r.put(k, c, (1.0f / (1.0f + expf(-v)) - y) * inv);
    });
    return wave_sum(loss);
}
