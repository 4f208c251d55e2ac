// Layer-wise importance sampling: LADIES and FastGCN [LADIES-recall: acbull/LADIES pytorch_ladies.py, ladies_sampler /
// fastgcn_sampler].  V = A + I over the DeviceGraph CSR (a stored (i, i) makes v_ii = 2), P = D^-1 V with
// D_i = (rowptr[i + 1] - rowptr[i]) + 1.
//
//   ladies_importance_k   one wavefront per candidate j: pi_j = sum over the rows i of a set (a bitmap, or every row) of P_ij^2,
//                         by a walk of row j of A^T; logit_j = logf(pi_j) - C, C = 20 + logf(float(rows in the set))
//   ladies_count_k        one wavefront per row i of the layer: the kept columns of row i of V (a bitmap) and s_i = sum v_ij / pi_j
//   ladies_scan_k         ONE workgroup: exclusive scan of the counts (block_excl_scan_u64), the edge count, the overflow bit
//   ladies_write_k        one wavefront per row: (j, i, (v_ij / pi_j) / s_i) in ascending j, the diagonal at its sorted place
//
// Sum order (both sums): lane l of the wavefront adds the terms l, l + 64, l + 128, ... of the walk one after the other, the 64
// partial sums meet in the xor butterfly of wave_sum (32, 16, ..., 1), and the importance adds its diagonal term last.  No float
// atomics: every output is a function of the input.  A long row (a hub) is walked by the same loop — 64 entries per trip, every
// lane busy; there is no item list, since a layer has a few thousand rows at the most and a walk reads 4 bytes per entry.
//
// No kernel waits on another workgroup of its own launch.
#include "row_list.h"

#define LADIES_SCAN_THREADS 1024

__device__ __forceinline__ bool ladies_bit(const unsigned long long* __restrict__ bits, int v) {
    return (bits[v >> 6] >> (v & 63)) & 1ull;
}

// 1 / D_i in fp32, D_i = (rowptr[i + 1] - rowptr[i]) + 1 (below 2^31 + 1: the wrappers refuse larger graphs)
__device__ __forceinline__ float ladies_inv_deg(const int64_t* __restrict__ rowptr, int i) {
    return 1.0f / (float)(rowptr[i + 1] - rowptr[i] + 1);
}

__global__ __launch_bounds__(256) void ladies_importance_k(
        const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t, int N,
        const int32_t* __restrict__ ids, int n_host, const int32_t* __restrict__ d_n, const unsigned long long* __restrict__ prev_bits,
        int m_host, const int32_t* __restrict__ d_m, float* __restrict__ pi, float* __restrict__ logit, float* __restrict__ pi_table,
        int32_t* status) {
    const int k = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (k >= n_host) return;                                             // (whole wavefronts leave)
    if (k >= eff_count(d_n, n_host)) return;                             // entries past the live count stay untouched
    const int j = ids ? ids[k] : k;
    if ((unsigned)j >= (unsigned)N) {
        if (lane == 0) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); pi[k] = 0.f; logit[k] = -INFINITY; }
        return;
    }
    const float C = 20.0f + logf((float)eff_count(d_m, m_host));
    const int64_t a = rowptr_t[j], e = rowptr_t[j + 1];
    float acc = 0.f;
    bool loop = false;
    for (int64_t t = a + lane; t < e; t += 64) {
        const int i = col_t[t];
        if ((unsigned)i >= (unsigned)N) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); continue; }
        if (i == j) { loop = true; continue; }                           // the stored (j, j): part of the diagonal term
        if (prev_bits && !ladies_bit(prev_bits, i)) continue;
        const float p = ladies_inv_deg(rowptr, i);
        acc += p * p;
    }
    acc = wave_sum(acc);
    if (!prev_bits || ladies_bit(prev_bits, j)) {
        const float p = (__any(loop) ? 2.0f : 1.0f) * ladies_inv_deg(rowptr, j);
        acc += p * p;
    }
    if (lane == 0) {
        pi[k] = acc;
        logit[k] = logf(acc) - C;
        if (pi_table) pi_table[j] = acc;
    }
}

// The walk of row i of V restricted to nothing yet: virtual position q of deg + ins positions, where pos = the first stored column
// >= i and ins = 1 when (i, i) is not stored (the diagonal is then inserted at pos).  Returns the column (or -1 past the end) and v.
__device__ __forceinline__ int ladies_entry(const int32_t* __restrict__ crow, int deg, int i, int pos, int ins, int q, float& v) {
    v = 1.f;
    if (q >= deg + ins) return -1;
    if (ins && q == pos) return i;
    const int j = crow[q - (ins && q > pos ? 1 : 0)];
    if (j == i) v = 2.f;                                                  // the stored loop folded into the diagonal
    return j;
}

// list_row plus the diagonal's place; false: no row (bad = an id outside [0, N))
struct LadiesRow { int i; int deg; int pos; int ins; const int32_t* crow; };

__device__ __forceinline__ bool ladies_row(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                           const int32_t* __restrict__ rows, int r, int live, LadiesRow& R, bool* bad) {
    const ListRow L = list_row(rowptr, N, rows, r, live, bad);
    if (L.i < 0) return false;
    R.i = L.i;
    R.deg = (int)L.deg;
    R.crow = col + L.a;
    R.pos = lower_bound(R.crow, R.deg, R.i);
    R.ins = (R.pos < R.deg && R.crow[R.pos] == R.i) ? 0 : 1;
    return true;
}

__global__ __launch_bounds__(256) void ladies_count_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                      const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                      const unsigned long long* __restrict__ keep, const float* __restrict__ pi_table,
                                                      int32_t* __restrict__ cnt, float* __restrict__ rsum, int32_t* status) {
    const int r = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (r >= m_host) return;
    LadiesRow R;
    bool bad = false;
    if (!ladies_row(rowptr, col, N, rows, r, eff_count(d_m, m_host), R, &bad)) {
        if (lane == 0) {
            cnt[r] = 0; rsum[r] = 0.f;
            if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        }
        return;
    }
    int c = 0;
    float acc = 0.f;
    for (int q = lane; q < R.deg + R.ins; q += 64) {
        float v;
        const int j = ladies_entry(R.crow, R.deg, R.i, R.pos, R.ins, q, v);
        if ((unsigned)j >= (unsigned)N) { if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); continue; }
        if (!ladies_bit(keep, j)) continue;
        ++c;
        acc += v / pi_table[j];
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    acc = wave_sum(acc);
    if (lane == 0) { cnt[r] = c; rsum[r] = acc; }
}

// ONE workgroup: off[r] = min(sum of cnt[0 .. r), e_cap) for r < m_host; *d_e = min(total, e_cap); the overflow bit
// (Its own prefix, a thread walking its span, not row_list.h's tiled one: on that the layer call measured 0.6 - 2 % slower at 512 and
// 574 rows, above the spread between runs of the parent — profiles/row_list_ab.json.)
__global__ __launch_bounds__(LADIES_SCAN_THREADS) void ladies_scan_k(const int32_t* __restrict__ cnt, int m_host, int e_cap,
                                                                     int32_t* __restrict__ off, int32_t* __restrict__ d_e,
                                                                     int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int per = (m_host + LADIES_SCAN_THREADS - 1) / LADIES_SCAN_THREADS;
    const int lo = min((int)threadIdx.x * per, m_host), hi = min(lo + per, m_host);
    unsigned long long s = 0ull;
    for (int r = lo; r < hi; ++r) s += (unsigned long long)cnt[r];
    unsigned long long total;
    unsigned long long run = block_excl_scan_u64(s, lds, &total);
    for (int r = lo; r < hi; ++r) {
        off[r] = run < (unsigned long long)e_cap ? (int)run : e_cap;
        run += (unsigned long long)cnt[r];
    }
    list_scan_finish(total, e_cap, nullptr, d_e, status);
}

__global__ __launch_bounds__(256) void ladies_write_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                      const int32_t* __restrict__ rows, int m_host, const int32_t* __restrict__ d_m,
                                                      const unsigned long long* __restrict__ keep, const float* __restrict__ pi_table,
                                                      const int32_t* __restrict__ cnt, const float* __restrict__ rsum,
                                                      const int32_t* __restrict__ off, int e_cap, int32_t* __restrict__ edge_src,
                                                      int32_t* __restrict__ edge_dst, float* __restrict__ weight) {
    const int r = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (r >= m_host) return;
    if (cnt[r] == 0) return;                                              // (a row past the live count or with a bad id counted 0)
    LadiesRow R;
    if (!ladies_row(rowptr, col, N, rows, r, eff_count(d_m, m_host), R, nullptr)) return;
    const float s = rsum[r];
    int base = off[r];
    for (int q0 = 0; q0 < R.deg + R.ins; q0 += 64) {
        if (base >= e_cap) break;                                         // (wavefront-uniform)
        float v;
        const int j = ladies_entry(R.crow, R.deg, R.i, R.pos, R.ins, q0 + lane, v);
        const bool kept = (unsigned)j < (unsigned)N && ladies_bit(keep, j);
        const int p = wave_compact_slot(kept, lane, base);
        if (kept && p < e_cap) {
            edge_src[p] = j; edge_dst[p] = R.i;
            weight[p] = (v / pi_table[j]) / s;
        }
    }
}

extern "C" int grapes_ladies_importance(const int64_t* rowptr, const int64_t* rowptr_t, const int32_t* col_t, int32_t num_nodes,
                                        const int32_t* ids, int32_t n, const int32_t* d_n, const uint64_t* prev_bits, int32_t m,
                                        const int32_t* d_m, float* pi, float* logit, float* pi_table, int32_t* status,
                                        grapes_stream_t stream) {
    if (num_nodes <= 0 || n <= 0 || m <= 0 || (!ids && n > num_nodes)) return GRAPES_EINVAL;
    if (!rowptr || !rowptr_t || !col_t || !pi || !logit) return GRAPES_EINVAL;
    hipLaunchKernelGGL(ladies_importance_k, dim3(grapes_div_up((int64_t)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, rowptr,
                       rowptr_t, col_t, num_nodes, ids, n, d_n, (const unsigned long long*)prev_bits, m, d_m, pi, logit, pi_table,
                       status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// cnt int32[m] | off int32[m] | rsum fp32[m]
extern "C" size_t grapes_ladies_layer_workspace_bytes(int32_t m) {
    return (size_t)(m > 0 ? m : 1) * 12;
}

extern "C" int grapes_ladies_layer(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m,
                                   const int32_t* d_m, const uint64_t* keep_bits, const float* pi_table, int32_t e_cap,
                                   int32_t* edge_src, int32_t* edge_dst, float* weight, int32_t* d_e, void* workspace,
                                   int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || m <= 0 || e_cap <= 0) return GRAPES_EINVAL;
    if (!rowptr || !col || !rows || !keep_bits || !pi_table || !edge_src || !edge_dst || !weight || !d_e || !workspace)
        return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* cnt = (int32_t*)workspace;
    int32_t* off = cnt + m;
    float* rsum = (float*)(off + m);
    const unsigned long long* keep = (const unsigned long long*)keep_bits;
    const int grid = grapes_div_up((int64_t)m * 64, 256);
    hipLaunchKernelGGL(ladies_count_k, dim3(grid), dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, keep, pi_table, cnt, rsum,
                       status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(ladies_scan_k, dim3(1), dim3(LADIES_SCAN_THREADS), 0, s, (const int32_t*)cnt, m, e_cap, off, d_e, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(ladies_write_k, dim3(grid), dim3(256), 0, s, rowptr, col, num_nodes, rows, m, d_m, keep, pi_table,
                       (const int32_t*)cnt, (const float*)rsum, (const int32_t*)off, e_cap, edge_src, edge_dst, weight);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
