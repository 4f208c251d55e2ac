// GraphSAINT random-walk sampling and the masked batch loss (reference graphsaint.py:104 GraphSAINTRandomWalkSampler with
// batch_size B, walk_length L, num_steps 1, sample_coverage 0; graphsaint.py:31-34 the loss over the batch's train rows).
//
//   saint_walk_nodes_k   ONE workgroup: B walks of L steps (torch_cluster random_walk, p = q = 1), then the ascending
//                        duplicate-free node set of the B (L + 1) visited ids (walks.view(-1).unique()), sorted in LDS, its
//                        count and node_map[node_idx[i]] = i; advances the device Philox offset last.
//   saint_colcount_k / saint_blockw_k / saint_roww_scan_k   the edge sampler's one-time weight table (PyG GraphSAINTEdgeSampler:
//                        entry (r, c) weighs colcount[r] + rowcount[c]): entries per column (int32 atomics), per row the inclusive
//                        weight prefix of its 64-entry blocks, and (ONE workgroup) the exclusive prefix of the row weights
//   saint_draw_k         one wavefront per draw of the node sampler (PyG GraphSAINTNodeSampler: the row of a uniform entry) or
//                        the edge sampler: a 64-ary search of rowptr / roww, then of the row's block prefixes, then one scan of
//                        the block's 64 recomputed weights — a draw never walks a hub row
//   saint_unique_ids_k   ONE workgroup: the drawn ids' node set, count and node_map (the walk's tail, saint_sort_unique), then
//                        advances the device Philox offset
//   saint_edge_count_k   one wavefront per local row: entries of the row whose column is in the node set
//   saint_edge_scan_k    ONE workgroup: exclusive scan of those counts -> local row pointers, edge count (clamped to e_cap)
//   saint_edge_write_k   one wavefront per local row: the induced edges (local row, local column) in CSR order
//   saint_masked_loss_k  ONE workgroup: mean CE / BCE over the batch rows that are training rows, and d loss / d logits
//   saint_coverage_count_k   GraphSAINT's normalisation [PyG-recall: GraphSAINTSampler._compute_norm]: one wavefront per local row
//                        bumps node_count[v] and edge_count[j] of the row's member entries; one thread adds the set's size to a total
//   saint_norms_k        one wavefront per CSR row (grid-stride): edge_norm and node_norm from the counts
//   saint_edge_write_k<true>   the write kernel that also stores every edge's global entry position and its edge_norm
//   saint_masked_loss_weighted_k   ONE workgroup: sum over the training rows of node_norm[v] * row loss, and d loss / d logits
//
// No kernel waits on another workgroup of its own launch.
//
// RNG contract (stream (seed, off), off = *d_offset when given): word i of the stream is word i & 3 of
// philox4x32_10(off + i / 4, seed).  Root b (b < B) is (uint64(word b) * N) >> 32 — all 32 bits, so every node of a graph with
// up to 2^32 nodes can be drawn.  The uniform of walk b's step t (t < L) is philox_uniform_at(seed, off, B + b L + t): 24 bits,
// like torch.rand.  The launch advances *d_offset by ceil(B (L + 1) / 4) counters.
//
// RNG contract of the node and edge samplers (same stream): draw b (b < B) takes the 64-bit word (stream word 2b) << 32 | (stream
// word 2b + 1) — both are words of philox4x32_10(off + b / 2, seed) — and t = mulhi64(word, total), an integer in [0, total):
// total = nnz = rowptr[N] (node sampler) or the total weight roww[N] (edge sampler).  t selects the stored entry e whose weight
// interval [cum(e - 1), cum(e)) holds it (cum: inclusive prefix of the entry weights in CSR order; all 1 for the node sampler), so an
// entry of weight 0 is never drawn.  Integer arithmetic throughout: no float enters the choice.  saint_unique_ids_k advances
// *d_offset by ceil(2 B / 4) counters after every workgroup of saint_draw_k has read it (the next launch on the stream).
//
// Membership of the node set is tested as a sparse set: v is in the set iff m = node_map[v] < count and node_idx[m] == v, so
// node_map needs no clearing (stale entries of other nodes are never trusted).
#include "philox.h"
#include "row_list.h"

#define SAINT_THREADS 1024
#define SAINT_MAX_IDS 16384          // B (L + 1) <= this: the node set is sorted in 64 KiB of LDS
#define SAINT_ANY_ID 0x7fffffff      // list_row's N for the edge kernels: node_idx is this library's own output and is not validated

// The tail the walk and the draw share (one workgroup of SAINT_THREADS): ids[0 .. M) in LDS, written by this workgroup and not yet
// fenced; P = M rounded up to a power of two (<= SAINT_MAX_IDS).  Sorts them, writes their ascending duplicate-free set to node_idx
// and node_map[node_idx[i]] = i, and returns the set's size to every thread.
__device__ __forceinline__ int saint_sort_unique(int32_t* ids, int* wsum, int M, int P, int32_t* __restrict__ node_idx,
                                                 int32_t* __restrict__ node_map) {
    const int tid = threadIdx.x;
    for (int i = M + tid; i < P; i += blockDim.x) ids[i] = 0x7fffffff;       // padding sorts last
    __syncthreads();
    // bitonic sort of the P (a power of two) ids
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += blockDim.x) {
                const int p = i ^ j;
                if (p > i) {
                    const int a = ids[i], c = ids[p];
                    const bool up = (i & k) == 0;
                    if ((a > c) == up) { ids[i] = c; ids[p] = a; }
                }
            }
            __syncthreads();
        }
    }
    // unique: thread t owns the contiguous chunk [t * per, (t + 1) * per)
    const int per = (P + SAINT_THREADS - 1) / SAINT_THREADS;
    const int lo = tid * per, hi = min(lo + per, M);
    int heads = 0;
    for (int i = lo; i < hi; ++i) heads += (i == 0 || ids[i] != ids[i - 1]) ? 1 : 0;
    int total;
    int pos = block_excl_scan(heads, wsum, &total);
    for (int i = lo; i < hi; ++i) {
        if (i == 0 || ids[i] != ids[i - 1]) {
            const int v = ids[i];
            node_idx[pos] = v;
            node_map[v] = pos;
            ++pos;
        }
    }
    return total;
}

// torch_cluster random_walk step (CPU, p = q = 1): a node without neighbours stays; otherwise
// next = col[rowptr[v] + int64(u * deg)] with the product in fp32.  For deg > 2^24 the product can round up to deg: the index is
// clamped to deg - 1.
__device__ __forceinline__ int saint_step(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int v, float u) {
    const int64_t a = rowptr[v], deg = rowptr[v + 1] - a;
    if (deg <= 0) return v;
    const float prod = u * (float)deg;
    int64_t k = (int64_t)prod;
    if (k > deg - 1) k = deg - 1;
    return col[a + k];
}

__global__ __launch_bounds__(SAINT_THREADS) void saint_walk_nodes_k(
        const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N, int B, int L, const int32_t* __restrict__ roots,
        const float* __restrict__ uniforms, uint64_t seed, uint64_t offset, uint64_t* d_offset, int32_t* __restrict__ walks,
        int32_t* __restrict__ node_idx, int32_t* __restrict__ d_count, int32_t* __restrict__ node_map, int P, int32_t* status) {
    __shared__ int32_t ids[SAINT_MAX_IDS];
    __shared__ int wsum[SAINT_THREADS / 64 + 1];
    const int tid = threadIdx.x;
    const uint64_t off = d_offset ? *d_offset : offset;
    const int W = L + 1, M = B * W;
    for (int b = tid; b < B; b += blockDim.x) {
        int v;
        if (roots) {
            v = roots[b];
            if ((unsigned)v >= (unsigned)N) { atomicOr(status, GRAPES_STATUS_BAD_INDEX); v = 0; }
        } else {
            const uint32_t word = philox4x32_10(off + (uint64_t)(b >> 2), seed).v[b & 3];
            v = (int)(((uint64_t)word * (uint64_t)N) >> 32);
        }
        walks[(int64_t)b * W] = v;
        ids[b * W] = v;
        for (int t = 0; t < L; ++t) {
            const int64_t ui = (int64_t)b * L + t;
            const float u = uniforms ? uniforms[ui] : philox_uniform_at(seed, off, (long long)B + ui);
            v = saint_step(rowptr, col, v, u);
            walks[(int64_t)b * W + t + 1] = v;
            ids[b * W + t + 1] = v;
        }
    }
    const int total = saint_sort_unique(ids, wsum, M, P, node_idx, node_map);
    if (tid == 0) {
        *d_count = total;
        if (d_offset) *d_offset = off + (uint64_t)((M + 3) >> 2);
    }
}

// ---------------------------------------------------------------------------------------- node and edge samplers
// Weight of the stored entry (r, c): colcount[r] + rowcount[c] in uint32 (the launcher refuses 2^31 entries or more); a column
// outside [0, N) weighs 0, so such an entry is never drawn.  The table kernel and the draw compute it with this one function.
__device__ __forceinline__ uint32_t saint_entry_weight(const int64_t* __restrict__ rowptr, uint32_t colcount_r, int c, int N) {
    if ((unsigned)c >= (unsigned)N) return 0u;
    return colcount_r + (uint32_t)(rowptr[c + 1] - rowptr[c]);
}

// colcount[c] += 1 for every stored entry with column c (colcount zeroed by the launcher): int32 atomics, any order, one result
__global__ __launch_bounds__(256) void saint_colcount_k(const int32_t* __restrict__ col, int64_t nnz, int N,
                                                        int32_t* __restrict__ colcount, int32_t* status) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nnz; j += stride) {
        const int c = col[j];
        if ((unsigned)c < (unsigned)N) atomicAdd(&colcount[c], 1);
        else if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    }
}

// one wavefront per row r: blockw[(rowptr[r] >> 6) + r + k] = weight of the row's entries [0, 64 (k + 1)) (inclusive prefix over its
// 64-entry blocks); roww[r + 1] = the row's weight (saint_roww_scan_k turns these into the prefix over rows)
__global__ __launch_bounds__(256) void saint_blockw_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                      const int32_t* __restrict__ colcount, int64_t* __restrict__ blockw,
                                                      int64_t* __restrict__ roww) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= N) return;
    const int64_t a = rowptr[r], e = rowptr[r + 1];
    const uint32_t cr = (uint32_t)colcount[r];
    int64_t* bw = blockw + (a >> 6) + r;
    unsigned long long run = 0ull;
    for (int64_t j0 = a; j0 < e; j0 += 64) {
        const int64_t j = j0 + lane;
        const unsigned long long w = j < e ? (unsigned long long)saint_entry_weight(rowptr, cr, col[j], N) : 0ull;
        run += wave_sum_u64(w);
        if (lane == 0) bw[(j0 - a) >> 6] = (int64_t)run;
    }
    if (lane == 0) {
        roww[r + 1] = (int64_t)run;
        if (r == 0) roww[0] = 0;
    }
}

// ONE workgroup: roww[1 .. N] (the rows' weights) -> their inclusive prefix in place, 8 consecutive rows per thread and round
__global__ __launch_bounds__(SAINT_THREADS) void saint_roww_scan_k(int64_t* __restrict__ roww, int N) {
    __shared__ int64_t ws[SAINT_THREADS / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < N; t0 += 8 * SAINT_THREADS) {
        const int64_t i0 = t0 + 8 * (int64_t)tid;
        int64_t v[8], s = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) { v[q] = i0 + q < N ? roww[1 + i0 + q] : 0; s += v[q]; }
        // (block_excl_scan_u64 in its private form: the shared one is 8 % slower here — profiles/block_prims_ab.txt)
        const int64_t inc = (int64_t)wave_incl_scan64((unsigned long long)s);
        if (lane == 63) ws[w] = inc;
        __syncthreads();
        if (w == 0) {
            const int64_t x = lane < SAINT_THREADS / 64 ? ws[lane] : 0;
            const int64_t xi = (int64_t)wave_incl_scan64((unsigned long long)x);
            if (lane < SAINT_THREADS / 64) ws[lane] = xi - x;
            if (lane == SAINT_THREADS / 64 - 1) ws[SAINT_THREADS / 64] = xi;
        }
        __syncthreads();
        int64_t run = carry + ws[w] + inc - s;
        carry += ws[SAINT_THREADS / 64];
#pragma unroll
        for (int q = 0; q < 8; ++q) { run += v[q]; if (i0 + q < N) roww[1 + i0 + q] = run; }
        __syncthreads();
    }
}

// One wavefront per draw b < B.  t = draws[b], or mulhi64(word, total) of the 64-bit word (stream word 2b) << 32 | (stream word
// 2b + 1); total = cdf[N] with cdf = rowptr (node sampler) or roww (edge sampler).  Node sampler: the row that holds entry t.
// Edge sampler: the row by roww, the row's block by blockw, the entry by a scan of the block's recomputed weights; both endpoints.
__global__ __launch_bounds__(256) void saint_draw_k(
        const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N, int B, const int32_t* __restrict__ colcount,
        const int64_t* __restrict__ blockw, const int64_t* __restrict__ roww, const int64_t* __restrict__ draws, uint64_t seed,
        uint64_t offset, const uint64_t* d_offset, int32_t* __restrict__ ids, int64_t* __restrict__ entries, int32_t* status) {
    const int b = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;                                                   // (whole wavefronts leave: the scans below need all 64 lanes)
    const bool edge = roww != nullptr;
    const int64_t* cdf = edge ? roww : rowptr;
    const int64_t total = cdf[N];
    int64_t t;
    if (draws) {
        t = draws[b];
    } else {
        const uint64_t off = d_offset ? *d_offset : offset;
        const Philox4 p = philox4x32_10(off + (uint64_t)(b >> 1), seed);
        const uint64_t word = ((uint64_t)p.v[(2 * b) & 3] << 32) | (uint64_t)p.v[(2 * b + 1) & 3];
        t = (int64_t)__umul64hi(word, (uint64_t)(total > 0 ? total : 0));
    }
    bool bad = t < 0 || t >= total;
    int r = 0, c = 0;
    int64_t ent = 0;
    if (!bad) {                                                           // (wavefront-uniform)
        r = (int)wave_search64(cdf, 0, N, t);
        if (!edge) {
            ent = t;
        } else {
            const int64_t a = rowptr[r], e = rowptr[r + 1], base = (a >> 6) + r;
            int64_t u = t - roww[r];
            const int64_t k = wave_search64(blockw + base, -1, (e - a + 63) >> 6, u);
            if (k > 0) u -= blockw[base + k - 1];
            const int64_t j = a + 64 * k + lane;
            const int cj = j < e ? col[j] : -1;
            const uint32_t w = saint_entry_weight(rowptr, (uint32_t)colcount[r], cj, N);
            // 64 weights below 2^32: their prefix as two int scans of 16-bit halves
            const int64_t inc = ((int64_t)wave_incl_scan((int)(w >> 16)) << 16) + (int64_t)wave_incl_scan((int)(w & 0xffffu));
            const uint64_t hit = __ballot(inc > u);
            if (hit == 0ull) {
                bad = true;                                               // a table that is not this graph's
            } else {
                const int l = __ffsll((unsigned long long)hit) - 1;
                c = __shfl(cj, l, 64);
                ent = a + 64 * k + l;
            }
        }
    }
    if (lane == 0) {
        if (bad) { r = 0; c = 0; ent = 0; if (status) atomicOr(status, GRAPES_STATUS_BAD_INDEX); }
        if (edge) { ids[2 * b] = r; ids[2 * b + 1] = c; } else { ids[b] = r; }
        entries[b] = ent;
    }
}

// ONE workgroup, after saint_draw_k: the ascending duplicate-free set of the M drawn ids, its count and node_map, as the walk's tail;
// advances the device Philox offset (the draw's workgroups have all read it by now)
__global__ __launch_bounds__(SAINT_THREADS) void saint_unique_ids_k(const int32_t* __restrict__ drawn, int M, int P, uint64_t advance,
                                                                    uint64_t* d_offset, int32_t* __restrict__ node_idx,
                                                                    int32_t* __restrict__ d_count, int32_t* __restrict__ node_map) {
    __shared__ int32_t ids[SAINT_MAX_IDS];
    __shared__ int wsum[SAINT_THREADS / 64 + 1];
    for (int i = threadIdx.x; i < M; i += blockDim.x) ids[i] = drawn[i];
    const int total = saint_sort_unique(ids, wsum, M, P, node_idx, node_map);
    if (threadIdx.x == 0) {
        *d_count = total;
        if (d_offset) *d_offset += advance;
    }
}

// one wavefront per local row i < count: cnt[i] = entries of node_idx[i]'s CSR row whose column is in the node set
__global__ __launch_bounds__(256) void saint_edge_count_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const int32_t* __restrict__ node_idx, const int32_t* __restrict__ d_count,
                                                          const int32_t* __restrict__ node_map, int n_cap, int32_t* __restrict__ cnt) {
    const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (i >= n_cap) return;
    const int n = eff_count(d_count, n_cap);
    if (i >= n) { if (lane == 0) cnt[i] = 0; return; }
    const ListRow R = list_row(rowptr, SAINT_ANY_ID, node_idx, i, n, nullptr);
    const int64_t a = R.a, e = R.a + R.deg;
    int c = 0;
    for (int64_t j = a + lane; j < e; j += 64) {
        const int u = col[j];
        const int m = node_map[u];
        c += ((unsigned)m < (unsigned)n && node_idx[m] == u) ? 1 : 0;
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if (lane == 0) cnt[i] = c;
}

// ONE workgroup: rowptr_l[i] = sum of cnt[0 .. i) for i <= n_cap (rows at or past the count are empty); *d_e = min(total, e_cap)
// (Its own 32-bit prefix, a thread walking its span, not row_list.h's tiled 64-bit one: on that saint_subgraph measured 1 - 2 % slower at
// 256 and 768 ids, above the spread between runs of the parent — profiles/row_list_ab.json.)
__global__ __launch_bounds__(SAINT_THREADS) void saint_edge_scan_k(const int32_t* __restrict__ cnt, const int32_t* __restrict__ d_count,
                                                                   int n_cap, int e_cap, int32_t* __restrict__ rowptr_l,
                                                                   int32_t* __restrict__ d_e, int32_t* status) {
    __shared__ int wsum[SAINT_THREADS / 64 + 1];
    const int n = eff_count(d_count, n_cap);
    const int per = (n_cap + SAINT_THREADS - 1) / SAINT_THREADS;
    const int lo = threadIdx.x * per, hi = min(lo + per, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    int total;
    int run = block_excl_scan(s, wsum, &total);
    for (int i = lo; i < min(lo + per, n_cap); ++i) {
        rowptr_l[i] = i < n ? run : total;
        if (i < n) run += cnt[i];
    }
    if (threadIdx.x == 0) rowptr_l[n_cap] = total;                        // (row pointers: not clamped)
    list_scan_finish((unsigned long long)total, e_cap, nullptr, d_e, status);
}

// one wavefront per local row: the row's member entries, in CSR order, at rowptr_l[i] ..; nothing at or past e_cap is written
// IDS: also edge_id[p] = j (the entry's position in col) and edge_norm_b[p] = edge_norm[j], each when its pointer is given
template <bool IDS>
__global__ __launch_bounds__(256) void saint_edge_write_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const int32_t* __restrict__ node_idx, const int32_t* __restrict__ d_count,
                                                          const int32_t* __restrict__ node_map, int n_cap,
                                                          const int32_t* __restrict__ rowptr_l, int e_cap,
                                                          int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                          int64_t* __restrict__ edge_id, const float* __restrict__ edge_norm,
                                                          float* __restrict__ edge_norm_b) {
    const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (i >= n_cap) return;
    const int n = eff_count(d_count, n_cap);
    const ListRow R = list_row(rowptr, SAINT_ANY_ID, node_idx, i, n, nullptr);
    const int64_t a = R.a, e = R.a + R.deg;
    int base = rowptr_l[i];
    for (int64_t j0 = a; j0 < e; j0 += 64) {
        const int64_t j = j0 + lane;
        int m = -1;
        if (j < e) {
            const int u = col[j];
            const int mm = node_map[u];
            if ((unsigned)mm < (unsigned)n && node_idx[mm] == u) m = mm;
        }
        const int p = wave_compact_slot(m >= 0, lane, base);
        if (m >= 0 && p < e_cap) {
            src[p] = i; dst[p] = m;
            if (IDS) {
                if (edge_id) edge_id[p] = j;
                if (edge_norm_b) edge_norm_b[p] = edge_norm[j];
            }
        }
        if (base >= e_cap) break;
    }
}

// saint_masked_loss_k stays out of block_prims.h and row_loss.h: on block_excl_scan and the shared row routines the launch measured
// 1 % slower in every arrangement tried (profiles/block_prims_ab.txt), so it keeps its own scan (inclusive, one value per thread,
// blockDim.x == SAINT_THREADS; *total = the sum) and its own rows, shift first as row_loss.h's (lsm = (z - mx) - log(se))
__device__ __forceinline__ int saint_block_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = wave_incl_scan(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    if (w == 0) {
        int s = lane < nw ? wsum[lane] : 0;
        int si = wave_incl_scan(s);
        if (lane < nw) wsum[lane] = si - s;          // exclusive prefix of the wavefront totals
        if (lane == nw - 1) wsum[SAINT_THREADS / 64] = si;
    }
    __syncthreads();
    inc += wsum[w];
    *total = wsum[SAINT_THREADS / 64];
    __syncthreads();
    return inc;
}

// ONE workgroup.  Rows i < count of z [n_cap, ldz] are the batch's logits (row i = node node_idx[i]); the training rows are those
// with train_mask[node_idx[i]] != 0, T of them.  CE (labels int64[N]): loss = sum_train (log(se) - (z[y] - max)) / T,
// g = (softmax - onehot) / T.  BCE (labels_f fp32[N, C]): loss = sum_train sum_c (max(z, 0) - z y + log1p(exp(-|z|))) / (T C),
// g = (sigmoid(z) - y) / (T C).  Other rows (and rows >= count) get g = 0.  T = 0: loss = 0 / 0 = NaN and g = 0, as torch's
// mean over an empty selection.  Wavefront w sums rows w, w + 16, ... in double in that order; the 16 sums are added in wavefront
// order: a fixed summation order, no float atomics.
__global__ __launch_bounds__(SAINT_THREADS) void saint_masked_loss_k(
        const float* __restrict__ z, int64_t ldz, int C, const int32_t* __restrict__ node_idx, const int32_t* __restrict__ d_count,
        int n_cap, const uint8_t* __restrict__ train_mask, const int64_t* __restrict__ labels, const float* __restrict__ labels_f,
        float* __restrict__ g, int64_t ldg, float* __restrict__ loss_out, int32_t* __restrict__ d_train, int32_t* status) {
    __shared__ int wsum[SAINT_THREADS / 64 + 1];
    __shared__ double lsum[SAINT_THREADS / 64];
    const int n = eff_count(d_count, n_cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    int t = 0;
    for (int i = tid; i < n; i += blockDim.x) t += train_mask[node_idx[i]] ? 1 : 0;
    int T;
    (void)saint_block_scan(t, wsum, &T);
    const double denom = labels_f ? (double)T * (double)C : (double)T;
    const float inv = T > 0 ? (float)(1.0 / denom) : 0.f;
    double acc = 0.0;
    for (int i = w; i < n_cap; i += nw) {
        float* gr = g + (int64_t)i * ldg;
        const int v = i < n ? node_idx[i] : -1;
        if (v < 0 || !train_mask[v]) {
            for (int c = lane; c < C; c += 64) gr[c] = 0.f;
            continue;
        }
        const float* zr = z + (int64_t)i * ldz;
        if (labels_f) {
            const float* yr = labels_f + (int64_t)v * C;
            float rl = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float x = zr[c], y = yr[c];
                rl += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
                gr[c] = (1.f / (1.f + expf(-x)) - y) * inv;
            }
            acc += (double)wave_sum(rl);
        } else {
            const int64_t y = labels[v];
            if (y < 0 || y >= C) {
                if (lane == 0 && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
                for (int c = lane; c < C; c += 64) gr[c] = 0.f;
                continue;
            }
            float mx = -INFINITY;
            for (int c = lane; c < C; c += 64) mx = fmaxf(mx, zr[c]);
            for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
            float se = 0.f;
            for (int c = lane; c < C; c += 64) se += expf(zr[c] - mx);
            se = wave_sum(se);
            const float lse = logf(se);
            for (int c = lane; c < C; c += 64) gr[c] = (expf((zr[c] - mx) - lse) - (c == y ? 1.f : 0.f)) * inv;
            acc += (double)(lse - (zr[y] - mx));
        }
    }
    if (lane == 0) lsum[w] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int q = 0; q < nw; ++q) s += lsum[q];
        *loss_out = (float)(s / denom);             // T = 0: 0 / 0 = NaN
        if (d_train) *d_train = T;
    }
}

// ------------------------------------------------------------------------ GraphSAINT normalisation (sample_coverage > 0)
// [PyG-recall: GraphSAINTSampler._compute_norm]  One wavefront per local row i < count of ONE drawn batch: lane 0 bumps
// node_count[v], v = node_idx[i]; the lanes walk v's CSR row in strides of 64 and bump edge_count[j] of every entry whose column is
// in the node set (the sparse-set test of the subgraph kernels).  Within a batch every v and every j is touched by one thread, and
// batches are serial on the stream: plain read-add-writes, no atomics, one result.  Thread 0 of row 0 adds the set's size to *d_total.
__global__ __launch_bounds__(256) void saint_coverage_count_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              int N, const int32_t* __restrict__ node_idx,
                                                              const int32_t* __restrict__ d_count, const int32_t* __restrict__ node_map,
                                                              int n_cap, uint32_t* __restrict__ node_count,
                                                              uint32_t* __restrict__ edge_count, int64_t* __restrict__ d_total) {
    const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (i >= n_cap) return;
    const int n = eff_count(d_count, n_cap);
    if (i >= n) return;
    const int v = node_idx[i];
    if ((unsigned)v >= (unsigned)N) return;
    if (lane == 0) {
        node_count[v] += 1u;
        if (i == 0) *d_total += (int64_t)n;
    }
    const int64_t a = rowptr[v], e = rowptr[v + 1];
    for (int64_t j = a + lane; j < e; j += 64) {
        const int u = col[j];
        if ((unsigned)u >= (unsigned)N) continue;
        const int m = node_map[u];
        if ((unsigned)m < (unsigned)n && node_idx[m] == u) edge_count[j] += 1u;
    }
}

// One wavefront per CSR row r (grid-stride over the rows), so row(j) is free; the lanes walk the row in strides of 64 (a row
// shorter than a wavefront leaves lanes idle, a longer one takes several strides).
//   edge_norm[j] = fp32(node_count[r]) / fp32(edge_count[j]) clamped to [0, 1e4], a NaN (0 / 0) -> 0.1 (so x / 0 -> 1e4);
//   node_norm[r] = (fp32(num_samples) / c) / fp32(N), c = fp32(node_count[r]) or 0.1 where the count is 0.
// The fp32 divisions are the compiler's correctly rounded ones (the default of this build: no fast-math flag).
__global__ __launch_bounds__(256) void saint_norms_k(const int64_t* __restrict__ rowptr, int N, const uint32_t* __restrict__ node_count,
                                                     const uint32_t* __restrict__ edge_count, float num_samples,
                                                     float* __restrict__ edge_norm, float* __restrict__ node_norm) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < N; r += waves) {
        const uint32_t nc = node_count[r];
        const float ncf = (float)nc;
        if (lane == 0) node_norm[r] = (num_samples / (nc ? ncf : 0.1f)) / (float)N;
        const int64_t a = rowptr[r], e = rowptr[r + 1];
        for (int64_t j = a + lane; j < e; j += 64) {
            float q = ncf / (float)edge_count[j];
            if (q != q) q = 0.1f;
            else if (q > 1e4f) q = 1e4f;
            else if (q < 0.f) q = 0.f;
            edge_norm[j] = q;
        }
    }
}

// ONE workgroup; saint_masked_loss_k with a per-node weight table w = node_norm[N], read through node_idx like train_mask
// [PyG-recall: examples/graph_saint.py, (loss * node_norm)[train_mask].sum()].  loss = sum over the training rows i of
// w_i * rowloss_i, NOT divided by T.  CE: rowloss = log(se) - (z[y] - max), g = w_i (softmax - onehot).  BCE: rowloss = the mean over the C
// columns of max(z, 0) - z y + log1p(exp(-|z|)), g = w_i (sigmoid(z) - y) / C.  Other rows (and rows >= count) get g = 0.  T = 0:
// loss = 0 and g = 0.  Same fixed summation order: wavefront w sums rows w, w + 16, ... in double, the 16 sums are added in
// wavefront order; no float atomics.  With w = 1 / T everywhere this is saint_masked_loss_k's loss.
__global__ __launch_bounds__(SAINT_THREADS) void saint_masked_loss_weighted_k(
        const float* __restrict__ z, int64_t ldz, int C, const int32_t* __restrict__ node_idx, const int32_t* __restrict__ d_count,
        int n_cap, const uint8_t* __restrict__ train_mask, const float* __restrict__ node_norm, const int64_t* __restrict__ labels,
        const float* __restrict__ labels_f, float* __restrict__ g, int64_t ldg, float* __restrict__ loss_out,
        int32_t* __restrict__ d_train, int32_t* status) {
    __shared__ int wsum[SAINT_THREADS / 64 + 1];
    __shared__ double lsum[SAINT_THREADS / 64];
    const int n = eff_count(d_count, n_cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    if (d_train) {                                                        // (workgroup-uniform)
        int t = 0;
        for (int i = tid; i < n; i += blockDim.x) t += train_mask[node_idx[i]] ? 1 : 0;
        int T;
        (void)saint_block_scan(t, wsum, &T);
        if (tid == 0) *d_train = T;
    }
    double acc = 0.0;
    for (int i = w; i < n_cap; i += nw) {
        float* gr = g + (int64_t)i * ldg;
        const int v = i < n ? node_idx[i] : -1;
        if (v < 0 || !train_mask[v]) {
            for (int c = lane; c < C; c += 64) gr[c] = 0.f;
            continue;
        }
        const float* zr = z + (int64_t)i * ldz;
        const float wi = node_norm[v];
        if (labels_f) {
            const float* yr = labels_f + (int64_t)v * C;
            const float wc = wi / (float)C;
            float rl = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float x = zr[c], y = yr[c];
                rl += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
                gr[c] = (1.f / (1.f + expf(-x)) - y) * wc;
            }
            acc += (double)wi * ((double)wave_sum(rl) / (double)C);
        } else {
            const int64_t y = labels[v];
            if (y < 0 || y >= C) {
                if (lane == 0 && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
                for (int c = lane; c < C; c += 64) gr[c] = 0.f;
                continue;
            }
            float mx = -INFINITY;
            for (int c = lane; c < C; c += 64) mx = fmaxf(mx, zr[c]);
            for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
            float se = 0.f;
            for (int c = lane; c < C; c += 64) se += expf(zr[c] - mx);
            se = wave_sum(se);
            const float lse = logf(se);
            for (int c = lane; c < C; c += 64) gr[c] = (expf((zr[c] - mx) - lse) - (c == y ? 1.f : 0.f)) * wi;
            acc += (double)wi * (double)(lse - (zr[y] - mx));
        }
    }
    if (lane == 0) lsum[w] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int q = 0; q < nw; ++q) s += lsum[q];
        *loss_out = (float)s;                         // no training row: 0
    }
}

static int saint_pow2(int m) { int p = 64; while (p < m) p <<= 1; return p; }

extern "C" int grapes_saint_walk_nodes(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, int32_t B, int32_t L,
                                       const int32_t* roots, const float* uniforms, uint64_t philox_seed, uint64_t philox_offset,
                                       uint64_t* d_philox_offset, int32_t* walks, int32_t* node_idx, int32_t* d_count,
                                       int32_t* node_map, int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || B <= 0 || L < 0 || (int64_t)B * (L + 1) > SAINT_MAX_IDS) return GRAPES_EINVAL;
    if (!rowptr || !col || !walks || !node_idx || !d_count || !node_map || (roots && !status)) return GRAPES_EINVAL;
    hipLaunchKernelGGL(saint_walk_nodes_k, dim3(1), dim3(SAINT_THREADS), 0, (hipStream_t)stream, rowptr, col, num_nodes, B, L, roots,
                       uniforms, philox_seed, philox_offset, d_philox_offset, walks, node_idx, d_count, node_map,
                       saint_pow2(B * (L + 1)), status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t grapes_saint_subgraph_workspace_bytes(int32_t n_cap) {
    return (size_t)(n_cap > 0 ? n_cap : 1) * 4;
}

extern "C" int grapes_saint_subgraph(const int64_t* rowptr, const int32_t* col, const int32_t* node_idx, const int32_t* d_count,
                                     const int32_t* node_map, int32_t n_cap, int32_t e_cap, int32_t* rowptr_l, int32_t* edge_src,
                                     int32_t* edge_dst, int32_t* d_e, int64_t* edge_id, const float* edge_norm, float* edge_norm_b,
                                     void* workspace, int32_t* status, grapes_stream_t stream) {
    if (n_cap <= 0 || n_cap > SAINT_MAX_IDS || e_cap <= 0) return GRAPES_EINVAL;
    if (!rowptr || !col || !node_idx || !d_count || !node_map || !rowptr_l || !edge_src || !edge_dst || !d_e || !workspace)
        return GRAPES_EINVAL;
    if ((edge_norm == nullptr) != (edge_norm_b == nullptr)) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* cnt = (int32_t*)workspace;
    const int grid = grapes_div_up((int64_t)n_cap * 64, 256);
    hipLaunchKernelGGL(saint_edge_count_k, dim3(grid), dim3(256), 0, s, rowptr, col, node_idx, d_count, node_map, n_cap, cnt);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(saint_edge_scan_k, dim3(1), dim3(SAINT_THREADS), 0, s, (const int32_t*)cnt, d_count, n_cap, e_cap, rowptr_l,
                       d_e, status);
    GRAPES_LAUNCH_CHECK();
    if (edge_id || edge_norm)
        hipLaunchKernelGGL(saint_edge_write_k<true>, dim3(grid), dim3(256), 0, s, rowptr, col, node_idx, d_count, node_map, n_cap,
                           (const int32_t*)rowptr_l, e_cap, edge_src, edge_dst, edge_id, edge_norm, edge_norm_b);
    else
        hipLaunchKernelGGL(saint_edge_write_k<false>, dim3(grid), dim3(256), 0, s, rowptr, col, node_idx, d_count, node_map, n_cap,
                           (const int32_t*)rowptr_l, e_cap, edge_src, edge_dst, (int64_t*)nullptr, (const float*)nullptr,
                           (float*)nullptr);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_saint_edge_weights(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, int64_t nnz, int32_t* colcount,
                                         int64_t* blockw, int64_t* roww, int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || nnz < 0 || nnz >= ((int64_t)1 << 31)) return GRAPES_EINVAL;
    if (!rowptr || !col || !colcount || !blockw || !roww) return GRAPES_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = grapes_zero_async(colcount, (size_t)num_nodes * 4, s);
    if (e != hipSuccess) return (int)e;
    if (nnz > 0) {
        int grid = grapes_div_up(nnz, 256 * 8);
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL(saint_colcount_k, dim3(grid), dim3(256), 0, s, col, nnz, num_nodes, colcount, status);
        GRAPES_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(saint_blockw_k, dim3(grapes_div_up((int64_t)num_nodes * 64, 256)), dim3(256), 0, s, rowptr, col, num_nodes,
                       (const int32_t*)colcount, blockw, roww);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(saint_roww_scan_k, dim3(1), dim3(SAINT_THREADS), 0, s, roww, num_nodes);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_saint_draw_nodes(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, int32_t B, const int32_t* colcount,
                                       const int64_t* blockw, const int64_t* roww, const int64_t* draws, uint64_t philox_seed,
                                       uint64_t philox_offset, uint64_t* d_philox_offset, int32_t* ids, int64_t* entries,
                                       int32_t* node_idx, int32_t* d_count, int32_t* node_map, int32_t* status, grapes_stream_t stream) {
    const bool edge = roww != nullptr;
    if (num_nodes <= 0 || B <= 0 || (int64_t)B * (edge ? 2 : 1) > SAINT_MAX_IDS) return GRAPES_EINVAL;
    if (!rowptr || !col || !ids || !entries || !node_idx || !d_count || !node_map || (draws && !status)) return GRAPES_EINVAL;
    if (edge != (colcount != nullptr) || edge != (blockw != nullptr)) return GRAPES_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int M = edge ? 2 * B : B;
    hipLaunchKernelGGL(saint_draw_k, dim3(grapes_div_up((int64_t)B * 64, 256)), dim3(256), 0, s, rowptr, col, num_nodes, B, colcount,
                       blockw, roww, draws, philox_seed, philox_offset, (const uint64_t*)d_philox_offset, ids, entries, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(saint_unique_ids_k, dim3(1), dim3(SAINT_THREADS), 0, s, (const int32_t*)ids, M, saint_pow2(M),
                       (uint64_t)((2 * (int64_t)B + 3) >> 2), d_philox_offset, node_idx, d_count, node_map);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_saint_coverage_count(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* node_idx,
                                           const int32_t* d_count, const int32_t* node_map, int32_t n_cap, uint32_t* node_count,
                                           uint32_t* edge_count, int64_t* d_total, grapes_stream_t stream) {
    if (num_nodes <= 0 || n_cap <= 0 || n_cap > SAINT_MAX_IDS) return GRAPES_EINVAL;
    if (!rowptr || !col || !node_idx || !d_count || !node_map || !node_count || !edge_count || !d_total) return GRAPES_EINVAL;
    hipLaunchKernelGGL(saint_coverage_count_k, dim3(grapes_div_up((int64_t)n_cap * 64, 256)), dim3(256), 0, (hipStream_t)stream,
                       rowptr, col, num_nodes, node_idx, d_count, node_map, n_cap, node_count, edge_count, d_total);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_saint_norms(const int64_t* rowptr, int32_t num_nodes, const uint32_t* node_count, const uint32_t* edge_count,
                                  int64_t num_samples, float* edge_norm, float* node_norm, grapes_stream_t stream) {
    if (num_nodes <= 0 || num_samples < 0) return GRAPES_EINVAL;
    if (!rowptr || !node_count || !edge_count || !edge_norm || !node_norm) return GRAPES_EINVAL;
    int grid = grapes_div_up((int64_t)num_nodes * 64, 256);
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(saint_norms_k, dim3(grid), dim3(256), 0, (hipStream_t)stream, rowptr, num_nodes, node_count, edge_count,
                       (float)num_samples, edge_norm, node_norm);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

extern "C" int grapes_saint_masked_loss(const float* z, int64_t ldz, int32_t C, const int32_t* node_idx, const int32_t* d_count,
                                        int32_t n_cap, const uint8_t* train_mask, const float* node_norm, const int64_t* labels,
                                        const float* labels_f, float* g, int64_t ldg, float* loss_out, int32_t* d_train,
                                        int32_t* status, grapes_stream_t stream) {
    if (C <= 0 || n_cap <= 0 || ldz < C || ldg < C) return GRAPES_EINVAL;
    if (!z || !node_idx || !train_mask || !g || !loss_out || ((labels == nullptr) == (labels_f == nullptr))) return GRAPES_EINVAL;
    if (node_norm)
        hipLaunchKernelGGL(saint_masked_loss_weighted_k, dim3(1), dim3(SAINT_THREADS), 0, (hipStream_t)stream, z, ldz, C, node_idx,
                           d_count, n_cap, train_mask, node_norm, labels, labels_f, g, ldg, loss_out, d_train, status);
    else
        hipLaunchKernelGGL(saint_masked_loss_k, dim3(1), dim3(SAINT_THREADS), 0, (hipStream_t)stream, z, ldz, C, node_idx, d_count,
                           n_cap, train_mask, labels, labels_f, g, ldg, loss_out, d_train, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
