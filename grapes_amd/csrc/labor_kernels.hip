// LABOR, the layer-neighbour sampler [Balin and Catalyurek, NeurIPS 2023; LABOR-recall: DGL's LaborSampler]: neighbour sampling's
// per-row estimator with ONE uniform per candidate vertex, shared by every row that sees it, so that rows agree on which neighbours
// to keep and a layer's union of sources stays small.  The rule written here (and in include/grapes_hip.h) is the contract; the CPU
// oracle (tests/labor_oracle.py) reproduces the kept sets bit for bit.
//
// ---- the sampler (grapes_labor_sample_layer).  For list row r, s = rows[r], d_s = deg(s), fanout k, stored entry t (a GLOBAL id):
//   r_t = keys[t] when keys (one word per NODE) is given, else 32-bit word t & 3 of philox4x32_10(base + (t >> 2), seed);
//   d_s <= k: every entry is kept (p = 1);
//   LABOR-0 (c, pi NULL):  kept iff (uint64) r_t d_s < (uint64) k << 32 — integers only;
//   LABOR-i (c, pi given): kept iff u_t < p_st, u_t = (r_t >> 8) 2^-24, p_st = fminf(1, c[r] * pi[t]) — ONE fp32 multiply (this file is
//                          compiled with -ffp-contract=off), so a CPU given the same c and pi keeps the same entries;
//   Hajek weights w_st = (1 / p_st) / sum over the kept entries of the row of 1 / p_st (LABOR-0: 1 / kept_s).
// The test on an entry depends on that entry alone: there is no selection pass, and a long row is simply cut.  A work item is
// LABOR_CHUNK = GRAPES_LONG_ROW = 64 consecutive entries of one list row, one per lane:
//   labor_items_k  ONE workgroup: every row's chunk count and its exclusive prefix -> item_off (list_scan_tiles of row_list.h)
//   labor_count_k  a wavefront per item: finds its row (lower_bound over item_off), tests its 64 entries — a lane computes a Philox
//                  call only for the entry it tests — and stores the kept lanes as one 64-bit mask (+ the chunk's sum of 1 / p)
//   labor_scan_k   ONE workgroup: the exclusive prefix of the masks' popcounts over ALL items — the chunks of a long row feed the same
//                  prefix as the short rows — the edge count and the overflow bit
//   labor_write_k  a wavefront per item: the kept lanes behind the item's offset in lane order (= CSR order), so the list is in row
//                  order and within a row in CSR order; the row's 1 / p sum = its chunks' sums added in chunk order
//
// ---- the importance iterations (grapes_labor_importance), pi^(0) = 1:
//   c_s(pi) solves sum_{t in N(s)} 1 / min(1, c pi_t) = d_s^2 / k for a row with d_s > k;  pi_t <- pi_t max_{s: d_s > k, t in N(s)} c_s(pi),
//   `iters` times, then c_s once more for the final pi.  One wavefront per list row; every row sum has a fixed order (lane l adds the
//   entries l, l + 64, ... in that order, then a butterfly); the maximum is an integer atomicMax on the bit patterns of the positive
//   floats, which is order-independent: two runs give the same bits.  No float atomics.
//   labor_pi_init_k  pi[t] = 1 for every column the rows touch     labor_pi_scatter_k  c_s, max into the N-sized table (zero at rest)
//   labor_pi_apply_k pi[t] *= the maximum, by the ONE lane whose atomicExch takes it, which also zeroes the table again
//   labor_c_k        the final c
// No kernel waits on another workgroup.
#include "philox.h"
#include "row_list.h"

#define LABOR_CHUNK GRAPES_LONG_ROW
#define LABOR_MAX_ITERS 8
static_assert(LABOR_CHUNK == 64, "a work item is one entry per lane and its kept set one 64-bit mask");

// r_t: the word of node t (t inside [0, N))
__device__ __forceinline__ uint32_t labor_word(const uint32_t* __restrict__ keys, uint64_t seed, uint64_t base, int t) {
    return keys ? keys[t] : philox_word_at(seed, base, (long long)t);
}

// p_st of an entry of a row with d_s > k under the importance rule: ONE multiply, then the clamp
__device__ __forceinline__ float labor_p(float c_s, float pi_t) { return fminf(1.f, c_s * pi_t); }

// ONE workgroup.  item_off[r] = the chunks of the list rows before r, item_off[m] = their total, both clamped to item_cap (more raise
// GRAPES_STATUS_EDGE_OVERFLOW).  A row id outside [0, N) counts as an empty row and raises GRAPES_STATUS_BAD_INDEX.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void labor_items_k(const int64_t* __restrict__ rowptr, int N,
                                                                   const int32_t* __restrict__ rows, int m_host,
                                                                   const int32_t* __restrict__ d_m, int item_cap,
                                                                   int32_t* __restrict__ item_off, int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int live = eff_count(d_m, m_host);
    bool bad = false;
    auto chunks = [&](int i0, int (&v)[LIST_SCAN_PER]) {
        long long deg[LIST_SCAN_PER];
        list_row_degrees(rowptr, N, rows, i0, live, deg, bad);                // (live <= m_host)
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) {
            const long long nch = (deg[q] + LABOR_CHUNK - 1) / LABOR_CHUNK;
            v[q] = (int)(nch < 0x7fffffffll ? nch : 0x7fffffffll);
        }
    };
    const unsigned long long total = list_scan_tiles<int>(chunks, m_host, (unsigned long long)item_cap, item_off, lds);
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    list_scan_finish(total, item_cap, item_off + m_host, nullptr, status);
}

// The item of this wavefront: its list row and the entry of this lane.  false: no such item (whole wavefronts leave).
struct LaborItem { int r; ListRow R; long long t; };
__device__ __forceinline__ bool labor_item(LaborItem& I, int it, const int64_t* __restrict__ rowptr, int N,
                                           const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                           const int32_t* __restrict__ item_off, int lane) {
    if (it >= item_off[m_host]) return false;
    // the last row with item_off[r] <= it: rows without an entry own no item and are stepped over
    I.r = lower_bound<int32_t, int, int>(item_off, m_host, it + 1) - 1;
    I.R = list_row(rowptr, N, rows, I.r, eff_count(d_m, m_host), nullptr);
    I.t = (long long)(it - item_off[I.r]) * LABOR_CHUNK + lane;
    return true;
}

// A wavefront per item: mask[it] = the kept lanes; rsum[it] = the sum of 1 / p over them (importance rule only).  A column outside
// [0, N) raises GRAPES_STATUS_BAD_INDEX and is never kept.
__global__ __launch_bounds__(256) void labor_count_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                     const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                     int fanout, const uint32_t* __restrict__ keys, uint64_t seed, uint64_t base,
                                                     const float* __restrict__ c, const float* __restrict__ pi,
                                                     const int32_t* __restrict__ item_off, int item_cap,
                                                     unsigned long long* __restrict__ mask, float* __restrict__ rsum, int32_t* status) {
    const int it = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (it >= item_cap) return;
    LaborItem I;
    if (!labor_item(I, it, rowptr, N, rows, m_host, d_m, item_off, lane)) return;
    const long long deg = I.R.deg;
    const bool in = I.t < deg;
    const int cj = in ? col[I.R.a + I.t] : 0;
    const bool ok = in && (unsigned)cj < (unsigned)N;
    if (in && !ok && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    bool keep = ok;
    float invp = 1.f;
    if (ok && deg > (long long)fanout) {
        const uint32_t w = labor_word(keys, seed, base, cj);
        if (c) {
            const float p = labor_p(c[I.r], pi[cj]);
            keep = (float)(w >> 8) * 5.9604644775390625e-08f < p;              // u_t = (r_t >> 8) 2^-24, exact in fp32
            invp = 1.f / p;
        } else {
            keep = (uint64_t)w * (uint64_t)deg < ((uint64_t)fanout << 32);
        }
    }
    const unsigned long long bal = __ballot(keep);
    if (c) {
        const float s = wave_sum(keep ? invp : 0.f);
        if (lane == 0) rsum[it] = s;
    }
    if (lane == 0) mask[it] = bal;
}

// ONE workgroup.  off[it] = min(the kept entries of the items before it, e_cap), off[n_items] = *d_e = min(their total, e_cap).
__global__ __launch_bounds__(LIST_SCAN_THREADS) void labor_scan_k(const unsigned long long* __restrict__ mask,
                                                                  const int32_t* __restrict__ item_off, int m_host, int e_cap,
                                                                  int32_t* __restrict__ off, int32_t* __restrict__ d_e, int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int n_items = item_off[m_host];
    auto kept = [&](int i0, int (&v)[LIST_SCAN_PER]) {
        unsigned long long w[LIST_SCAN_PER];
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) w[q] = i0 + q < n_items ? mask[i0 + q] : 0ull;
#pragma unroll
        for (int q = 0; q < LIST_SCAN_PER; ++q) v[q] = __popcll(w[q]);
    };
    const unsigned long long total = list_scan_tiles<int>(kept, n_items, (unsigned long long)e_cap, off, lds);
    list_scan_finish(total, e_cap, off + n_items, d_e, status);
}

// A wavefront per item: its kept lanes behind off[it], in lane order; nothing is written at or past e_cap.
__global__ __launch_bounds__(256) void labor_write_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                     const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                     int fanout, const float* __restrict__ c, const float* __restrict__ pi,
                                                     const int32_t* __restrict__ item_off, int item_cap,
                                                     const unsigned long long* __restrict__ mask, const float* __restrict__ rsum,
                                                     const int32_t* __restrict__ off, int e_cap, int32_t* __restrict__ edge_src,
                                                     int32_t* __restrict__ edge_dst, int64_t* __restrict__ edge_pos,
                                                     float* __restrict__ edge_weight) {
    const int it = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (it >= item_cap) return;
    LaborItem I;
    if (!labor_item(I, it, rowptr, N, rows, m_host, d_m, item_off, lane)) return;
    const unsigned long long bal = mask[it];
    int base = off[it];
    if (bal == 0ull || base >= e_cap) return;
    const bool keep = (bal >> lane) & 1ull;
    const int p = wave_compact_slot(keep, lane, base);
    const int i0 = item_off[I.r], i1 = item_off[I.r + 1];
    float w = 0.f;
    if (edge_weight) {
        if (c) {                                                              // the row's chunks in chunk order
            float s = 0.f;
            for (int j = i0 + lane; j < i1; j += 64) s += rsum[j];
            s = wave_sum(s);
            const int cj = keep ? col[I.R.a + I.t] : 0;
            const float invp = (keep && I.R.deg > (long long)fanout) ? 1.f / labor_p(c[I.r], pi[cj]) : 1.f;
            w = invp / s;
        } else {
            w = 1.f / (float)(off[i1] - off[i0]);                             // 1 / kept_s
        }
    }
    if (keep && p < e_cap) {
        edge_src[p] = col[I.R.a + I.t];
        edge_dst[p] = I.R.i;
        if (edge_pos) edge_pos[p] = (int64_t)(I.R.a + I.t);
        if (edge_weight) edge_weight[p] = w;
    }
}

// mask uint64[item_cap] | item_off int32[m + 1] | off int32[item_cap + 1] | rsum float[item_cap]
extern "C" size_t grapes_labor_sample_layer_workspace_bytes(int32_t m, int32_t item_cap) {
    const size_t M = m > 0 ? (size_t)m : 1, I = item_cap > 0 ? (size_t)item_cap : 1;
    return I * 8 + (M + 1) * 4 + (I + 1) * 4 + I * 4 + 16;
}

extern "C" int grapes_labor_sample_layer(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m,
                                         const int32_t* d_m, int32_t fanout, const uint32_t* keys, uint64_t philox_seed,
                                         uint64_t philox_base, const float* c, const float* pi, int32_t item_cap, int32_t e_cap,
                                         int32_t* edge_src, int32_t* edge_dst, int64_t* edge_pos, float* edge_weight, int32_t* d_e,
                                         void* workspace, int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || m <= 0 || e_cap <= 0 || item_cap <= 0 || fanout < 1) return GRAPES_EINVAL;
    if (item_cap > (1 << 24)) return GRAPES_EINVAL;                           // (64 item_cap threads in one grid)
    if (!rowptr || !col || !rows || !edge_src || !edge_dst || !d_e || !workspace || ((c != nullptr) != (pi != nullptr)))
        return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 7) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* mask = (unsigned long long*)workspace;
    int32_t* item_off = (int32_t*)(mask + item_cap);
    int32_t* off = item_off + (m + 1);
    float* rsum = (float*)(off + (item_cap + 1));
    const dim3 grid(grapes_div_up((int64_t)item_cap * 64, 256));
    hipLaunchKernelGGL(labor_items_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, rowptr, num_nodes, rows, m, d_m, item_cap, item_off,
                       status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(labor_count_k, grid, dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, fanout, keys, philox_seed,
                       philox_base, c, pi, (const int32_t*)item_off, item_cap, mask, rsum, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(labor_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, (const unsigned long long*)mask,
                       (const int32_t*)item_off, m, e_cap, off, d_e, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(labor_write_k, grid, dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, fanout, c, pi,
                       (const int32_t*)item_off, item_cap, (const unsigned long long*)mask, (const float*)rsum, (const int32_t*)off,
                       e_cap, edge_src, edge_dst, edge_pos, edge_weight);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the importance iterations

// c_s(pi) of a row with d_s > k by the monotone fixed point, without a sort:
//   J = {};  c = (sum_{t not in J} 1 / pi_t) / (d_s^2 / k - |J|);  J <- {t : c pi_t >= 1};  until J stops growing.
// Proof that c never decreases and that at most d_s rounds run.  Write D = d_s^2 / k and f(c) = sum_t 1 / min(1, c pi_t), which
// decreases in c; the solution c* has f(c*) = D.  For a set J with c = S_J / (D - |J|), S_J = sum_{t not in J} 1 / pi_t, moving one t
// with c pi_t >= 1 into J gives c' = (S_J - 1 / pi_t) / (D - |J| - 1), and c' >= c  <=>  S_J - 1 / pi_t >= c (D - |J|) - c = S_J - c
// <=>  1 / pi_t <= c, which is the condition for the move.  So c never decreases, hence an entry that entered J stays in it: J only
// grows, and it has at most d_s entries, so at most d_s rounds change it.  The denominator stays positive: |J| <= d_s < d_s^2 / k since
// d_s > k.  Every iterate stays at or below c*: for c = S_J / (D - |J|), f(c) >= sum_{t not in J} 1 / (c pi_t) + |J| = D = f(c*), and f
// decreases.  The loop ends at a fixed point, J = {t : c pi_t >= 1} with sum_{t not in J} 1 / (c pi_t) + |J| = D, that is f(c) = D, and f
// is strictly decreasing while an entry is unsaturated: the fixed point is c*.  In fp32 a rounding may keep the count from growing one
// round early; the loop ends whenever the count does not grow, so it always ends.
// All 64 lanes call it with the same row and return the same bits: lane l adds the entries l, l + 64, ... in order, then a butterfly.
__device__ __forceinline__ float labor_solve_c(const int32_t* __restrict__ col, int64_t a, long long deg, int N,
                                               const float* __restrict__ pi, int fanout, int lane) {
    const float D = ((float)deg * (float)deg) / (float)fanout;
    float s = 0.f;
    for (long long t = lane; t < deg; t += 64) {
        const int cj = col[a + t];
        if ((unsigned)cj < (unsigned)N) s += 1.f / pi[cj];
    }
    float c = wave_sum(s) / D;
    unsigned long long nJ = 0ull;
    for (long long round = 0; round < deg; ++round) {
        unsigned long long j = 0ull;
        s = 0.f;
        for (long long t = lane; t < deg; t += 64) {
            const int cj = col[a + t];
            if ((unsigned)cj < (unsigned)N) {
                const float q = pi[cj];
                if (c * q >= 1.f) ++j; else s += 1.f / q;
            }
        }
        j = wave_sum_u64(j);
        if (j <= nJ) break;
        nJ = j;
        c = wave_sum(s) / (D - (float)nJ);
    }
    return c;
}

// one wavefront per list row
#define LABOR_ROW_HEAD()                                                                                                   \
    const int r = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;                    \
    if (r >= m_host) return;                                                                                               \
    bool bad = false;                                                                                                      \
    const ListRow R = list_row(rowptr, N, rows, r, eff_count(d_m, m_host), &bad)

__global__ __launch_bounds__(256) void labor_pi_init_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                       const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                       float* __restrict__ pi, int32_t* status) {
    LABOR_ROW_HEAD();
    for (long long t = lane; t < R.deg; t += 64) {
        const int cj = col[R.a + t];
        if ((unsigned)cj < (unsigned)N) pi[cj] = 1.f; else bad = true;
    }
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
}

__global__ __launch_bounds__(256) void labor_pi_scatter_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                          const int32_t* __restrict__ rows, int m_host,
                                                          const int32_t* __restrict__ d_m, int fanout, const float* __restrict__ pi,
                                                          uint32_t* __restrict__ mx) {
    LABOR_ROW_HEAD();
    if (R.deg <= (long long)fanout) return;                                   // p = 1: takes no part in the maximum
    const uint32_t bits = __float_as_uint(labor_solve_c(col, R.a, R.deg, N, pi, fanout, lane));   // c > 0: its bits order as it does
    for (long long t = lane; t < R.deg; t += 64) {
        const int cj = col[R.a + t];
        if ((unsigned)cj < (unsigned)N) atomicMax(&mx[cj], bits);
    }
}

__global__ __launch_bounds__(256) void labor_pi_apply_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                        const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                        float* __restrict__ pi, uint32_t* __restrict__ mx) {
    LABOR_ROW_HEAD();
    for (long long t = lane; t < R.deg; t += 64) {
        const int cj = col[R.a + t];
        if ((unsigned)cj >= (unsigned)N) continue;
        const uint32_t old = atomicExch(&mx[cj], 0u);                         // ONE lane takes the maximum; the table is zero again
        if (old) pi[cj] = pi[cj] * __uint_as_float(old);
    }
}

__global__ __launch_bounds__(256) void labor_c_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                 const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                 int fanout, const float* __restrict__ pi, float* __restrict__ c) {
    LABOR_ROW_HEAD();
    const float cs = R.deg > (long long)fanout ? labor_solve_c(col, R.a, R.deg, N, pi, fanout, lane) : 0.f;
    if (lane == 0) c[r] = cs;
}

// the N-sized table of maxima: zero on entry, zero again on return
extern "C" size_t grapes_labor_importance_workspace_bytes(int32_t num_nodes) {
    return grapes_round16((size_t)(num_nodes > 0 ? num_nodes : 1) * 4);
}

extern "C" int grapes_labor_importance(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m,
                                       const int32_t* d_m, int32_t fanout, int32_t iters, float* c, float* pi, void* workspace,
                                       int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || m <= 0 || fanout < 1 || iters < 0 || iters > LABOR_MAX_ITERS) return GRAPES_EINVAL;
    if (!rowptr || !col || !rows || !c || !pi || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* mx = (uint32_t*)workspace;
    const dim3 grid(grapes_div_up((int64_t)m * 64, 256));
    hipLaunchKernelGGL(labor_pi_init_k, grid, dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, pi, status);
    GRAPES_LAUNCH_CHECK();
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(labor_pi_scatter_k, grid, dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, fanout, (const float*)pi, mx);
        GRAPES_LAUNCH_CHECK();
        hipLaunchKernelGGL(labor_pi_apply_k, grid, dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, pi, mx);
        GRAPES_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(labor_c_k, grid, dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, fanout, (const float*)pi, c);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
