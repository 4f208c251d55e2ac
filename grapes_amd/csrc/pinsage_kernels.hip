// PinSAGE [Ying et al., KDD 2018 — recalled; DGL-recall: RandomWalkNeighborSampler / PinSAGESampler]: a node's neighbourhood is the T
// nodes that R short restarting walks from it visit most often, and the visit counts are the aggregation weights.  The rule written
// in include/grapes_hip.h is the contract; tests/pinsage_oracle.py reproduces it bit for bit.
//
// grapes_pinsage_neighbors: ONE launch (and a one-thread tail that advances a device stream offset, when the caller gave one).
//   pinsage_neighbors_k   256 threads own G consecutive roots, G = pinsage_group(R, V): as many as fill the lanes with walks and fit
//                     the LDS budget, at most 8 — a function of R and V alone, and the result does not depend on it: a draw is a
//                     function of (root id, walk, step, offset, seed).  (The cap: with all 26 roots that fill the lanes at R = 10
//                     a wavefront selects seven roots one after the other and 512 roots are 20 workgroups: measured 48.3 us per call
//                     at (R, L, T) = (10, 2, 3) against 22.6 us at (50, 2, 10), whose G is 6.)
//     walk phase      flat over the workgroup's G R walks, a lane per walk (in trips past 256): every step is two dependent memory
//                     trips (the row-pointer pair of the current node, then the chosen col entry), the L steps of a walk are
//                     sequential, so the parallelism is across walks.  One Philox call serves an even step and the odd one behind
//                     it.  A step's visit (or the empty mark) goes straight into the owning root's V LDS slots.
//     select phase    a wavefront per root (two trips at G = 8).  SORT, not a hash table: the wavefront sorts the root's P >= V
//                     ids in LDS (bitonic, P the power of two at or above V), a lane that holds the head of a run finds the run's
//                     end by a binary search of the sorted ids — log2 P reads, whatever the run's length, and no scan — and forms
//                     the key (V - count) << 32 | id; everything else holds the all-ones key.  A second bitonic pass over the
//                     64-bit keys puts them in rule order.  Chosen over an open-addressing table of integer LDS atomics because it
//                     needs no table beside the V ids and V keys the output already asks for (the table would have to hold 2 V
//                     entries and be compacted before its sort anyway), no atomic at all, and its cost does not depend on how the
//                     visits collide: a star's leaves all visit the hub, which a hash serialises on one slot.
//     output          lane t writes slot t + 1 from the sorted keys' prefix, coalesced; slot 0 and the slots past cnt hold (root, 0).
//   LDS: 12 P bytes per root (P ids, P keys), at most 48 KiB per workgroup (four roots at V = 1024), requested per launch.
//   Integers only, no global atomic beyond the status OR, no workspace: two runs give the same bits.
//
// grapes_relu_l2norm_fwd / _bwd: PinSAGE's layer epilogue out = relu(s) / max(|relu(s)|_2, eps) and its gradient, a group of lanes
// per row on the row-gather scaffold (row_gather.h): the row is read once, the sum of squares (backward: <g, out>) is an fma chain
// over a lane's slabs and a butterfly over the group — a fixed order, no atomics — then IEEE sqrtf and division.  One launch per
// direction in place of three elementwise torch launches and a reduction.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): pinsage_neighbors_k 54 VGPRs, 80 SGPRs, no scratch, occupancy 8 waves per
// SIMD by registers; its LDS is the 12 G P bytes above (3 KiB at (R, L) = (10, 2), 9 KiB at (50, 2), 24 KiB at (200, 3), 48 KiB at
// V = 1024 with R <= 64).  The relu_l2norm kernels use no LDS: 21 - 37 VGPRs forward, 24 - 49 backward, occupancy 8.
// Measured (profiles/pinsage_bench.json; products-shaped synthetic, 512 roots, p = 0.5): 15.4 us per call at (R, L, T) = (10, 2, 3),
// 22.6 at (50, 2, 10), 93.8 at (200, 3, 50), 94.3 at (256, 4, 50) — at V > 512 the two single-wavefront sorts of 1024 entries are the
// long pole — against 450 - 660 us for the cheapest torch form found; relu_l2norm on 5 000 rows 7.5 us forward and 17 us forward +
// backward against 31 and 190 - 200 us for the torch expression.
#include "philox.h"
#include "row_gather.h"

#define PINSAGE_THREADS 256
#define PINSAGE_MAX_V 1024
#define PINSAGE_MAX_T 1023
#define PINSAGE_MAX_G 8                      // roots of one workgroup at most: two select trips per wavefront (see the file header)
#define PINSAGE_LDS_BUDGET (48 * 1024)
#define PINSAGE_EMPTY 0xffffffffu            // no visit: sorts behind every id

// A wavefront's own LDS traffic, in program order for the compiler too (the hardware keeps a wavefront's LDS accesses in order).
__device__ __forceinline__ void pinsage_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a[0 .. P) ascending, P a power of two, by ONE wavefront: a lane per compare-exchange pair, so no lane idles while P >= 128
template <class T>
__device__ __forceinline__ void pinsage_wave_sort(T* a, int P, int lane) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;    // (bit j of i is clear)
                const T u = a[i], w = a[x];
                if ((u > w) == ((i & k) == 0)) { a[i] = w; a[x] = u; }
            }
            pinsage_wave_sync();
        }
    }
}

__global__ __launch_bounds__(PINSAGE_THREADS) void pinsage_neighbors_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                       int N, const int32_t* __restrict__ roots, int m_host,
                                                                       const int32_t* __restrict__ d_m, int R, int L, uint32_t term_q,
                                                                       int T, uint64_t seed, uint64_t off_host,
                                                                       const uint64_t* __restrict__ d_off, int G, int P,
                                                                       int32_t* __restrict__ nbr, uint32_t* __restrict__ visits,
                                                                       int32_t* __restrict__ cnt, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pinsage_lds[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(pinsage_lds);           // [G][P]
    uint32_t* ids = reinterpret_cast<uint32_t*>(keys + (size_t)G * P);                       // [G][P]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int V = R * L, K = T + 1;
    const int b0 = blockIdx.x * G;
    const int g_here = m_host - b0 < G ? m_host - b0 : G;                       // (workgroup-uniform, at least 1: the grid is ceil(m / G))
    const int live = eff_count(d_m, m_host);
    const uint64_t off = d_off ? *d_off : off_host;

    // ---- walk phase
    const int pad = P - V;
    for (int i = tid; i < g_here * pad; i += PINSAGE_THREADS) {
        const int g = i / pad;
        ids[g * P + V + (i - g * pad)] = PINSAGE_EMPTY;
    }
    bool bad = false;
    for (int w = tid; w < g_here * R; w += PINSAGE_THREADS) {
        const int g = w / R, j = w - g * R, b = b0 + g;
        uint32_t* slot = ids + g * P + j * L;
        const int v = b < live ? roots[b] : -1;
        bool alive = (unsigned)v < (unsigned)N;
        int c = v;
        Philox4 p{};
        for (int t = 0; t < L; ++t) {
            uint32_t visit = PINSAGE_EMPTY;
            if (alive) {
                const long long beg = rowptr[c], deg = rowptr[c + 1] - beg;
                if (!(t & 1)) p = philox4x32_10_wide((uint64_t)(uint32_t)v | ((uint64_t)(uint32_t)j << 32), off + (uint64_t)(t >> 1), seed);
                const uint32_t a = (t & 1) ? p.v[2] : p.v[0], s = (t & 1) ? p.v[3] : p.v[1];
                if (a < term_q || deg <= 0) {
                    alive = false;
                } else {
                    const int nc = col[beg + (long long)(((unsigned long long)s * (unsigned long long)deg) >> 32)];
                    if ((unsigned)nc >= (unsigned)N) { alive = false; bad = true; }          // (never a row pointer read outside the table)
                    else { c = nc; if (c != v) visit = (uint32_t)c; }
                }
            }
            slot[t] = visit;
        }
    }
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    __syncthreads();

    // ---- select phase: a wavefront per root
    for (int g = wid; g < g_here; g += PINSAGE_THREADS / 64) {
        const int b = b0 + g;
        const int v = b < live ? roots[b] : -1;
        int32_t* nb = nbr + (size_t)b * K;
        uint32_t* vs = visits + (size_t)b * K;
        if ((unsigned)v >= (unsigned)N) {                                       // (wavefront-uniform) no node: empty slots
            for (int i = lane; i < K; i += 64) { nb[i] = -1; vs[i] = 0u; }
            if (lane == 0) {
                cnt[b] = 0;
                if (b < live && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
            }
            continue;
        }
        uint32_t* id = ids + g * P;
        unsigned long long* key = keys + (size_t)g * P;
        pinsage_wave_sort<uint32_t>(id, P, lane);
        int heads = 0;
        for (int i = lane; i < P; i += 64) {
            const uint32_t u = id[i];
            unsigned long long k = ~0ull;
            if (u != PINSAGE_EMPTY && (i == 0 || id[i - 1] != u)) {             // the head of a run: its end by bisection
                int lo = i + 1, hi = P;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (id[mid] <= u) lo = mid + 1; else hi = mid;
                }
                k = ((unsigned long long)(uint32_t)(V - (lo - i)) << 32) | u;
                ++heads;
            }
            key[i] = k;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) heads += __shfl_xor(heads, d, 64);
        pinsage_wave_sync();
        pinsage_wave_sort<unsigned long long>(key, P, lane);
        const int n_sel = heads < T ? heads : T;
        for (int i = lane; i < K; i += 64) {
            int x = v;
            uint32_t c = 0u;
            if (i >= 1 && i <= n_sel) {
                const unsigned long long k = key[i - 1];
                x = (int)(uint32_t)k;
                c = (uint32_t)V - (uint32_t)(k >> 32);
            }
            nb[i] = x; vs[i] = c;
        }
        if (lane == 0) cnt[b] = 1 + n_sel;
    }
}

// the one-thread tail: every workgroup of the launch before it has read the offset
__global__ void pinsage_advance_k(uint64_t* d_off, uint64_t by) { *d_off += by; }

static inline int pinsage_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
// the roots of one workgroup: as many as fill its lanes with walks, inside the LDS budget — a function of R and V alone
static inline int pinsage_group(int R, int V) {
    int g = (PINSAGE_THREADS + R - 1) / R;
    const int cap = PINSAGE_LDS_BUDGET / (12 * pinsage_pow2(V));
    if (g > cap) g = cap;
    if (g > PINSAGE_MAX_G) g = PINSAGE_MAX_G;
    return g < 1 ? 1 : g;
}

extern "C" int grapes_pinsage_neighbors(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m,
                                        const int32_t* d_m, int32_t R, int32_t L, uint32_t term_q, int32_t T, uint64_t philox_seed,
                                        uint64_t philox_offset, uint64_t* d_philox_offset, int32_t* nbr, uint32_t* visits, int32_t* cnt,
                                        int32_t* status, grapes_stream_t stream) {
    if (num_nodes < 1 || m < 1 || R < 1 || L < 1 || R > PINSAGE_MAX_V || L > PINSAGE_MAX_V || R * L > PINSAGE_MAX_V) return GRAPES_EINVAL;
    if (T < 1 || T > PINSAGE_MAX_T || (long long)m * (T + 1) >= (1ll << 31)) return GRAPES_EINVAL;
    if (!rowptr || !col || !roots || !nbr || !visits || !cnt) return GRAPES_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int V = R * L, P = pinsage_pow2(V), G = pinsage_group(R, V);
    hipLaunchKernelGGL(pinsage_neighbors_k, dim3(grapes_div_up(m, G)), dim3(PINSAGE_THREADS), (size_t)G * P * 12, s, rowptr, col, num_nodes,
                       roots, m, d_m, R, L, term_q, T, philox_seed, philox_offset, (const uint64_t*)d_philox_offset, G, P, nbr, visits,
                       cnt, status);
    GRAPES_LAUNCH_CHECK();
    if (d_philox_offset) {
        hipLaunchKernelGGL(pinsage_advance_k, dim3(1), dim3(1), 0, s, d_philox_offset, (uint64_t)((L + 1) / 2));
        GRAPES_LAUNCH_CHECK();
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ relu + L2 normalisation
template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void relu_l2norm_fwd_k(const float* __restrict__ s, long long ld_s, int m, int F, float eps,
                                                         float* __restrict__ out, long long ld_out, float* __restrict__ nrm) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int r = blockIdx.x * G + threadIdx.x / LPR; r < m; r += gridDim.x * G) {
        float z[NS][VEC];
        row_load_ld<VEC, LPR, NS>(s, r, ld_s, F, l, z);
        float q = 0.f;
#pragma unroll
        for (int a = 0; a < NS; ++a)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                z[a][v] = z[a][v] > 0.f ? z[a][v] : 0.f;
                q = fmaf(z[a][v], z[a][v], q);
            }
        const float n = sqrtf(grp_sum<LPR>(q));
        const float d = fmaxf(n, eps);
#pragma unroll
        for (int a = 0; a < NS; ++a)
#pragma unroll
            for (int v = 0; v < VEC; ++v) z[a][v] = z[a][v] / d;
        row_store_ld<VEC, LPR, NS>(out, r, ld_out, F, l, z);
        if (l == 0) nrm[r] = n;
    }
}

template <int VEC, int LPR, int NS>
__global__ __launch_bounds__(256) void relu_l2norm_bwd_k(const float* __restrict__ g, long long ld_g, const float* __restrict__ out,
                                                         long long ld_out, const float* __restrict__ nrm, const float* __restrict__ s,
                                                         long long ld_s, int m, int F, float eps, float* __restrict__ ds, long long ld_ds) {
    const int l = threadIdx.x % LPR, G = 256 / LPR;
    for (int r = blockIdx.x * G + threadIdx.x / LPR; r < m; r += gridDim.x * G) {
        float gv[NS][VEC], ov[NS][VEC], sv[NS][VEC];
        row_load_ld<VEC, LPR, NS>(g, r, ld_g, F, l, gv);
        row_load_ld<VEC, LPR, NS>(out, r, ld_out, F, l, ov);
        row_load_ld<VEC, LPR, NS>(s, r, ld_s, F, l, sv);
        const float n = nrm[r];
        const float dot = grp_sum<LPR>(slab_dot<VEC, NS>(gv, ov));
        const float c = n >= eps ? dot : 0.f, d = fmaxf(n, eps);
#pragma unroll
        for (int a = 0; a < NS; ++a)
#pragma unroll
            for (int v = 0; v < VEC; ++v) gv[a][v] = sv[a][v] > 0.f ? (gv[a][v] - ov[a][v] * c) / d : 0.f;
        row_store_ld<VEC, LPR, NS>(ds, r, ld_ds, F, l, gv);
    }
}

static inline bool relu_l2norm_aligned(const void* p, int64_t ld) { return grapes_aligned16(p) && ld % 4 == 0; }

extern "C" int grapes_relu_l2norm_fwd(const float* s, int64_t ld_s, int32_t m, int32_t f, float eps, float* out, int64_t ld_out, float* nrm,
                                      grapes_stream_t stream) {
    if (!s || !out || !nrm || m < 1 || f < 1 || ld_s < f || ld_out < f || !(eps > 0.f)) return GRAPES_EINVAL;
    const int shape = gather_shape(f, relu_l2norm_aligned(s, ld_s) && relu_l2norm_aligned(out, ld_out));
    if (shape < 0) return shape;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = shape == 0;
    ROW_LAUNCH(relu_l2norm_fwd_k, 4, vec, f, m, st, s, (long long)ld_s, m, f, eps, out, (long long)ld_out, nrm);
    return 0;
}

extern "C" int grapes_relu_l2norm_bwd(const float* g, int64_t ld_g, const float* out, int64_t ld_out, const float* nrm, const float* s,
                                      int64_t ld_s, int32_t m, int32_t f, float eps, float* ds, int64_t ld_ds, grapes_stream_t stream) {
    if (!g || !out || !nrm || !s || !ds || m < 1 || f < 1 || ld_g < f || ld_out < f || ld_s < f || ld_ds < f || !(eps > 0.f)) return GRAPES_EINVAL;
    const int shape = gather_shape(f, relu_l2norm_aligned(g, ld_g) && relu_l2norm_aligned(out, ld_out) && relu_l2norm_aligned(s, ld_s) &&
                                          relu_l2norm_aligned(ds, ld_ds));
    if (shape < 0) return shape;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = shape == 0;
    ROW_LAUNCH(relu_l2norm_bwd_k, 4, vec, f, m, st, g, (long long)ld_g, out, (long long)ld_out, nrm, s, (long long)ld_s, m, f, eps, ds,
               (long long)ld_ds);
    return 0;
}
