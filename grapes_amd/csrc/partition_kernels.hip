// A graph partitioner for Cluster-GCN: deterministic, integers-only, size-constrained SYNCHRONOUS label propagation that refines a
// balanced starting assignment.  The rule written in include/grapes_hip.h is the contract; tests/partition_oracle.py reproduces every
// integer.  A round is grapes_partition_propose, then grapes_partition_admit; grapes_partition_cut judges the result.  The driver
// (modules/cluster.py: refine_partition) reads `moved` and the cut once per round: this is one-time preprocessing, the eager form.
//
// ---- the proposal (grapes_partition_propose): one pass over every stored entry with the dependent load part[col[j]].
//   part_propose_rows_k  a wavefront per row.  A row of at most 64 entries counts in registers, one entry per lane: a ballot on "my
//                        label equals the first remaining lane's label" per distinct label — its popcount is that label's count, the
//                        same in every lane, so the maximum, the smallest label at the maximum and count[cur] are carried as
//                        wavefront-uniform values and need no reduction.  A longer row is appended to one of two lists (an integer
//                        atomic cursor: the lists' order varies from run to run, what is computed per row does not)
//   part_propose_mid_k   rows of 65 .. PART_LDS_ROW (2048) entries, a 256-thread workgroup per listed row, every 64-entry piece on its own
//                        wavefront (a thread's entries are loaded together): an LDS open-addressing table keyed by label with integer
//                        atomic counts.  The table has the first power of two >= 2 deg slots (128 .. PART_LDS_SLOTS = 4096), so at most
//                        half of it fills — a row has at most deg distinct labels — and a probe sequence always ends.  32 KB of LDS per
//                        workgroup: five workgroups per compute unit
//   part_propose_big_k   longer rows, PART_BIG_GROUPS (16) workgroups of 1024 threads, each with a P-sized int32 slab of the workspace
//                        that is zero at rest: walk 1 counts with integer atomics, walk 2 reads each entry's count back (the maximum and
//                        the smallest label among the maxima as one packed 64-bit max), walk 3 walks the row again to put the slab back
//                        to zero.  Exact for every degree below 2^31 and any number of distinct labels; a row of d entries costs 3 d /
//                        1024 dependent trips of one workgroup — the limit of this form: a graph whose hubs hold most entries is walked
//                        by 16 workgroups
//   The counts are merged exactly in every form; no form is taken by the labels, only by the row's degree.
//
// ---- the admission (grapes_partition_admit): part_admit_hist_k (an integer histogram of the proposers per destination),
//   part_admit_scan_k (ONE workgroup: counts -> offsets, list_scan_tiles), part_admit_scatter_k (the 64-bit keys into per-destination
//   buckets behind an integer cursor: a bucket's order varies, its set does not), part_admit_limit_k (a thread per destination: a
//   bucket of at most free keys admits all — limit ~0 —, free = 0 admits none — limit 0 —, a fuller bucket is listed),
//   part_admit_select_k (a 1024-thread workgroup per listed bucket: the free-th smallest key by an 8-bit radix select, most
//   significant digit first, eight passes over the bucket whatever its size — no ranking of pairs; keys are unique, so exactly free
//   keys are <= the limit) and part_admit_apply_k (a thread per proposer: key <= limit of its destination moves the node; integer
//   atomics on size and moved).
//
// ---- the cut (grapes_partition_cut): a wavefront per row walks rows of at most PART_CUT_WAVE_ROW (1024) entries 64 at a time, the
//   wavefronts of at most PART_CUT_GRID workgroups striding over the rows; longer rows are listed and taken by 256-thread workgroups.
//   64-bit integer sums, one atomic per workgroup into one of 64 slots.
//
// No floating point anywhere; integer atomics only; every output is bit-identical from run to run.  No kernel waits on another
// workgroup.
#include "row_list.h"

#define PART_CHUNK GRAPES_LONG_ROW
#define PART_LDS_ROW 2048
#define PART_LDS_SLOTS 4096
#define PART_MID_PER (PART_LDS_ROW / 256)      // the entries of one thread of part_propose_mid_k
#define PART_MID_GRID 4096
#define PART_BIG_GROUPS 16
#define PART_CUT_WAVE_ROW 1024
#define PART_CUT_SLOTS 64
#define PART_CUT_GRID 16384                    // workgroups of part_cut_rows_k: four wavefronts each, striding over the rows
#define PART_HDR 4
static_assert(PART_CHUNK == 64, "a short row is one entry per lane");
static_assert(PART_LDS_SLOTS >= 2 * PART_LDS_ROW, "the table of a listed row is at most half full");

// (count, label) packed so that the larger count wins, then the smaller label; 0 = no label seen
__device__ __forceinline__ unsigned long long part_pack(int count, int label) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)label);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}
// The workgroup's maximum to every thread; lds: one word per wavefront.  Two barriers, the first in front of the first LDS write.
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* lds) {
    v = wave_max_u64(v);
    __syncthreads();
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = 0ull;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m = lds[w] > m ? lds[w] : m;
    return m;
}

// Entry j of row v: the label of its column, or -1 for a stored loop and for a column outside [0, N) or a label outside [0, P), which
// set bad.
__device__ __forceinline__ int part_label(const int32_t* __restrict__ col, const int32_t* __restrict__ part, int64_t j, int v, int N,
                                          int P, bool& bad) {
    const int u = col[j];
    if ((unsigned)u >= (unsigned)N) { bad = true; return -1; }
    if (u == v) return -1;
    const int l = part[u];
    if ((unsigned)l >= (unsigned)P) { bad = true; return -1; }
    return l;
}

// The proposal of v from the packed best (count m, smallest label at m) and count[cur]
__device__ __forceinline__ void part_decide(unsigned long long best, int ccur, bool cur_ok, int v, int32_t* __restrict__ want,
                                            int32_t* __restrict__ gain) {
    const int m = (int)(best >> 32), lab = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    const bool stay = !cur_ok || m == 0 || ccur == m;
    want[v] = stay ? -1 : lab;
    gain[v] = stay ? 0 : m - ccur;
}

// hdr[0] = the rows of 65 .. PART_LDS_ROW entries, listed from the front of `list`; hdr[1] = the longer ones, listed from its back
__global__ __launch_bounds__(256) void part_propose_rows_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                           const int32_t* __restrict__ part, int P, int32_t* __restrict__ want,
                                                           int32_t* __restrict__ gain, int32_t* hdr, int32_t* __restrict__ list,
                                                           int32_t* status) {
    const int64_t v64 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (v64 >= (int64_t)N) return;                                             // (whole wavefronts leave)
    const int v = (int)v64;
    const int64_t a = rowptr[v];
    const long long deg = (long long)(rowptr[v + 1] - a);
    if (deg > PART_CHUNK) {
        if (lane == 0) {
            if (deg <= PART_LDS_ROW) list[atomicAdd(&hdr[0], 1)] = v;
            else list[N - 1 - atomicAdd(&hdr[1], 1)] = v;
        }
        return;
    }
    const int cur = part[v];
    const bool cur_ok = (unsigned)cur < (unsigned)P;
    bool bad = lane == 0 && !cur_ok;
    const int l = (long long)lane < deg ? part_label(col, part, a + lane, v, N, P, bad) : -1;
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    unsigned long long rem = __ballot(l >= 0), best = 0ull;
    int ccur = 0;
    while (rem) {                                                              // (one trip per distinct label; rem is uniform)
        const int lf = __shfl(l, __ffsll((long long)rem) - 1, 64);
        const unsigned long long eq = __ballot(l == lf);
        const int c = __popcll(eq);
        const unsigned long long pk = part_pack(c, lf);
        best = pk > best ? pk : best;
        if (lf == cur) ccur = c;
        rem &= ~eq;
    }
    if (lane == 0) part_decide(best, ccur, cur_ok, v, want, gain);
}

__global__ __launch_bounds__(256) void part_propose_mid_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                          const int32_t* __restrict__ part, int P, int32_t* __restrict__ want,
                                                          int32_t* __restrict__ gain, const int32_t* __restrict__ hdr,
                                                          const int32_t* __restrict__ list, int32_t* status) {
    __shared__ int keys[PART_LDS_SLOTS];
    __shared__ int cnt[PART_LDS_SLOTS];
    __shared__ unsigned long long red[4];
    __shared__ int s_ccur;
    const int tid = threadIdx.x;
    int n_mid = hdr[0];
    n_mid = n_mid < N ? n_mid : N;
    for (int h = blockIdx.x; h < n_mid; h += gridDim.x) {
        const int v = list[h];
        const int64_t a = rowptr[v];
        long long deg64 = (long long)(rowptr[v + 1] - a);
        const int deg = (int)(deg64 < PART_LDS_ROW ? deg64 : PART_LDS_ROW);   // (listed rows: 65 .. PART_LDS_ROW)
        int slots = 128, shift = 25;
        while (slots < 2 * deg) { slots <<= 1; --shift; }
        for (int s = tid; s < slots; s += 256) { keys[s] = -1; cnt[s] = 0; }
        if (tid == 0) s_ccur = 0;
        const int cur = part[v];
        const bool cur_ok = (unsigned)cur < (unsigned)P;
        bool bad = tid == 0 && !cur_ok;
        int lab[PART_MID_PER];
#pragma unroll
        for (int q = 0; q < PART_MID_PER; ++q) {                               // (a thread's loads are requested together)
            const int t = q * 256 + tid;
            lab[q] = t < deg ? part_label(col, part, a + t, v, N, P, bad) : -1;
        }
        if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PART_MID_PER; ++q) {
            if (lab[q] < 0) continue;
            unsigned s = ((unsigned)lab[q] * 2654435761u) >> shift;
            for (int probe = 0; probe < slots; ++probe) {                      // (ends at a free or own slot: the table is at most half full)
                const int old = atomicCAS(&keys[s], -1, lab[q]);
                if (old == -1 || old == lab[q]) { atomicAdd(&cnt[s], 1); break; }
                s = (s + 1) & (unsigned)(slots - 1);
            }
        }
        __syncthreads();
        unsigned long long best = 0ull;
        for (int s = tid; s < slots; s += 256) {
            const int k = keys[s];
            if (k < 0) continue;
            const int c = cnt[s];
            const unsigned long long pk = part_pack(c, k);
            best = pk > best ? pk : best;
            if (k == cur) s_ccur = c;                                          // (one slot holds cur)
        }
        best = block_max_u64(best, red);
        if (tid == 0) part_decide(best, s_ccur, cur_ok, v, want, gain);
        __syncthreads();                                                       // (the table and s_ccur are cleared by the next row)
    }
}

__global__ __launch_bounds__(1024) void part_propose_big_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                           const int32_t* __restrict__ part, int P, int32_t* __restrict__ want,
                                                           int32_t* __restrict__ gain, const int32_t* __restrict__ hdr,
                                                           const int32_t* __restrict__ list, int32_t* scratch, int32_t* status) {
    __shared__ unsigned long long red[16];
    const int tid = threadIdx.x;
    int32_t* slab = scratch + (size_t)blockIdx.x * (size_t)P;                  // zero at rest
    int n_big = hdr[1];
    n_big = n_big < N ? n_big : N;
    for (int h = blockIdx.x; h < n_big; h += gridDim.x) {
        const int v = list[N - 1 - h];
        const int64_t a = rowptr[v];
        const long long deg = (long long)(rowptr[v + 1] - a);
        const int cur = part[v];
        const bool cur_ok = (unsigned)cur < (unsigned)P;
        bool bad = tid == 0 && !cur_ok;
        for (long long t = tid; t < deg; t += 1024) {
            const int l = part_label(col, part, a + t, v, N, P, bad);
            if (l >= 0) atomicAdd(&slab[l], 1);
        }
        if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        unsigned long long best = 0ull;
        bool ignore = false;
        for (long long t = tid; t < deg; t += 1024) {
            const int l = part_label(col, part, a + t, v, N, P, ignore);
            if (l < 0) continue;
            const unsigned long long pk = part_pack(ld_agent(&slab[l]), l);
            best = pk > best ? pk : best;
        }
        const int ccur = (tid == 0 && cur_ok) ? ld_agent(&slab[cur]) : 0;
        best = block_max_u64(best, red);                                       // (its barriers: every read of the slab is behind us)
        if (tid == 0) part_decide(best, ccur, cur_ok, v, want, gain);
        __syncthreads();
        for (long long t = tid; t < deg; t += 1024) {
            const int l = part_label(col, part, a + t, v, N, P, ignore);
            if (l >= 0) st_agent(&slab[l], 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
}

// hdr int32[PART_HDR] | scratch int32[PART_BIG_GROUPS * P] | list int32[N]
extern "C" size_t grapes_partition_propose_workspace_bytes(int32_t num_nodes, int32_t num_parts) {
    const size_t N = num_nodes > 0 ? (size_t)num_nodes : 1, P = num_parts > 0 ? (size_t)num_parts : 1;
    return (PART_HDR + (size_t)PART_BIG_GROUPS * P + N) * 4 + 16;
}

extern "C" int grapes_partition_propose(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* part,
                                        int32_t num_parts, int32_t* want, int32_t* gain, void* workspace, int32_t* status,
                                        grapes_stream_t stream) {
    if (num_nodes <= 0 || num_parts <= 0 || num_parts > num_nodes) return GRAPES_EINVAL;
    if (!rowptr || !col || !part || !want || !gain || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 3) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* hdr = (int32_t*)workspace;
    int32_t* scratch = hdr + PART_HDR;
    int32_t* list = scratch + (size_t)PART_BIG_GROUPS * (size_t)num_parts;
    hipError_t e = grapes_zero_async(hdr, (PART_HDR + (size_t)PART_BIG_GROUPS * (size_t)num_parts) * 4, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(part_propose_rows_k, dim3(grapes_div_up((int64_t)num_nodes * 64, 256)), dim3(256), 0, s, rowptr, col, num_nodes,
                       part, num_parts, want, gain, hdr, list, status);
    GRAPES_LAUNCH_CHECK();
    const int mid_grid = num_nodes < PART_MID_GRID ? num_nodes : PART_MID_GRID;
    hipLaunchKernelGGL(part_propose_mid_k, dim3(mid_grid), dim3(256), 0, s, rowptr, col, num_nodes, part, num_parts, want, gain,
                       (const int32_t*)hdr, (const int32_t*)list, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_propose_big_k, dim3(PART_BIG_GROUPS), dim3(1024), 0, s, rowptr, col, num_nodes, part, num_parts, want, gain,
                       (const int32_t*)hdr, (const int32_t*)list, scratch, status);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the admission

// The destination of v when it proposes, else -1.  A destination outside [0, P), a gain below 1 beside one, or a current label outside
// [0, P) sets bad and v does not propose.
__device__ __forceinline__ int part_proposal(const int32_t* __restrict__ want, const int32_t* __restrict__ gain,
                                             const int32_t* __restrict__ part, int v, int P, bool& bad) {
    const int c = want[v];
    if (c < 0) return -1;
    if (c >= P || gain[v] < 1 || (unsigned)part[v] >= (unsigned)P) { bad = true; return -1; }
    return c;
}

__global__ __launch_bounds__(256) void part_admit_hist_k(const int32_t* __restrict__ want, const int32_t* __restrict__ gain,
                                                         const int32_t* __restrict__ part, int N, int P, int32_t* cnt, int32_t* status) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)N) return;
    bool bad = false;
    const int c = part_proposal(want, gain, part, (int)g, P, bad);
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    if (c >= 0) atomicAdd(&cnt[c], 1);
}

// ONE workgroup.  off[c] = the proposers to the destinations before c, off[P] = their number; *moved = 0.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void part_admit_scan_k(const int32_t* __restrict__ cnt, int P, int32_t* __restrict__ off,
                                                                       int32_t* __restrict__ moved) {
    __shared__ unsigned long long lds[17];
    auto counts = [&](int i0, int (&v)[LIST_SCAN_PER]) {
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) v[k] = i0 + k < P ? cnt[i0 + k] : 0;
    };
    const unsigned long long total = list_scan_tiles<int>(counts, P, LIST_NO_CAP, off, lds);
    if (threadIdx.x == 0) { off[P] = (int)total; *moved = 0; }
}

__global__ __launch_bounds__(256) void part_admit_scatter_k(const int32_t* __restrict__ want, const int32_t* __restrict__ gain,
                                                            const int32_t* __restrict__ part, int N, int P,
                                                            const int32_t* __restrict__ off, int32_t* cursor,
                                                            unsigned long long* __restrict__ keys) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)N) return;
    bool bad = false;
    const int v = (int)g, c = part_proposal(want, gain, part, v, P, bad);
    if (c < 0) return;
    const int at = off[c] + atomicAdd(&cursor[c], 1);
    keys[at] = ((unsigned long long)(0x7fffffffu - (unsigned)gain[v]) << 32) | (unsigned long long)(unsigned)v;
}

// A thread per destination: limit[c] = ~0 (all its proposers fit), 0 (no room: every key is above 0, a gain is below 2^31 - 1), or
// the bucket is listed for the selection; hdr[0] = the listed buckets.
__global__ __launch_bounds__(256) void part_admit_limit_k(const int32_t* __restrict__ off, const int32_t* __restrict__ size, int P, int cap,
                                                          unsigned long long* __restrict__ limit, int32_t* hdr,
                                                          int32_t* __restrict__ full) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)P) return;
    const int c = (int)g, n = off[c + 1] - off[c];
    const long long room = (long long)cap - (long long)size[c];
    unsigned long long lim = 0ull;
    if ((long long)n <= room) lim = ~0ull;
    else if (room > 0) full[atomicAdd(&hdr[0], 1)] = c;
    limit[c] = lim;
}

// A workgroup per listed bucket: limit[c] = its free-th smallest key, free = cap - size[c] (1 <= free < the bucket's keys).
__global__ __launch_bounds__(1024) void part_admit_select_k(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ off,
                                                            const int32_t* __restrict__ size, int P, int cap,
                                                            const int32_t* __restrict__ hdr, const int32_t* __restrict__ full,
                                                            unsigned long long* __restrict__ limit) {
    __shared__ int hist[256];
    __shared__ int lds[17];
    __shared__ int s_digit, s_k;
    const int tid = threadIdx.x, lane = tid & 63;
    int n_full = hdr[0];
    n_full = n_full < P ? n_full : P;
    for (int h = blockIdx.x; h < n_full; h += gridDim.x) {
        const int c = full[h], b0 = off[c], n = off[c + 1] - b0;
        int k = cap - size[c];                                                 // the rank wanted, 1-based, among the keys that match prefix
        unsigned long long prefix = 0ull;
        for (int pass = 7; pass >= 0; --pass) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int i0 = 0; i0 < n; i0 += 1024) {
                const int i = i0 + tid;
                const unsigned long long key = i < n ? keys[b0 + i] : 0ull;
                const bool in = i < n && (pass == 7 || (key >> (8 * (pass + 1))) == prefix);
                const int d = (int)((key >> (8 * pass)) & 0xffull);
                // the high digits are all but equal (a gain is small): a wavefront whose lanes agree adds once
                const unsigned long long act = __ballot(in);
                if (act) {
                    const int d0 = __shfl(d, __ffsll((long long)act) - 1, 64);
                    const unsigned long long same = __ballot(in && d == d0);
                    if (same == act) { if (lane == __ffsll((long long)act) - 1) atomicAdd(&hist[d0], __popcll(act)); }
                    else if (in) atomicAdd(&hist[d], 1);
                }
            }
            __syncthreads();
            const int mine = tid < 256 ? hist[tid] : 0;
            int tot;
            const int before = block_excl_scan(mine, lds, &tot);
            if (tid < 256 && before < k && k <= before + mine) { s_digit = tid; s_k = k - before; }
            __syncthreads();
            prefix = (prefix << 8) | (unsigned long long)s_digit;
            k = s_k;
            __syncthreads();                                                   // (s_digit, s_k and hist are written again by the next pass)
        }
        if (tid == 0) limit[c] = prefix;
    }
}

// A thread per proposer slot: the node moves when its key is at or below its destination's limit.
__global__ __launch_bounds__(256) void part_admit_apply_k(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ off,
                                                          int P, const int32_t* __restrict__ want,
                                                          const unsigned long long* __restrict__ limit, int32_t* __restrict__ part,
                                                          int32_t* size, int32_t* moved) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool go = false;
    if (g < (int64_t)off[P]) {
        const unsigned long long key = keys[g];
        const int v = (int)(key & 0xffffffffull), c = want[v];
        if (key <= limit[c]) {
            go = true;
            const int old = part[v];
            part[v] = c;
            atomicAdd(&size[c], 1);
            atomicSub(&size[old], 1);
        }
    }
    const unsigned long long bal = __ballot(go);
    if (bal && (threadIdx.x & 63) == __ffsll((long long)bal) - 1) atomicAdd(moved, __popcll(bal));
}

// keys u64[N] | limit u64[P] | hdr int32[PART_HDR] | cnt int32[P] | cursor int32[P] | off int32[P + 1] | full int32[P]
extern "C" size_t grapes_partition_admit_workspace_bytes(int32_t num_nodes, int32_t num_parts) {
    const size_t N = num_nodes > 0 ? (size_t)num_nodes : 1, P = num_parts > 0 ? (size_t)num_parts : 1;
    return (N + P) * 8 + (PART_HDR + 4 * P + 1) * 4 + 16;
}

extern "C" int grapes_partition_admit(const int32_t* want, const int32_t* gain, int32_t num_nodes, int32_t num_parts, int32_t* part,
                                      int32_t* size, int32_t cap, int32_t* moved, void* workspace, int32_t* status,
                                      grapes_stream_t stream) {
    if (num_nodes <= 0 || num_parts <= 0 || num_parts > num_nodes || cap < 0) return GRAPES_EINVAL;
    if (!want || !gain || !part || !size || !moved || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 7) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)num_nodes, P = (size_t)num_parts;
    unsigned long long* keys = (unsigned long long*)workspace;
    unsigned long long* limit = keys + N;
    int32_t* hdr = (int32_t*)(limit + P);
    int32_t* cnt = hdr + PART_HDR;
    int32_t* cursor = cnt + P;
    int32_t* off = cursor + P;
    int32_t* full = off + P + 1;
    hipError_t e = grapes_zero_async(hdr, (PART_HDR + 2 * P) * 4, s);
    if (e != hipSuccess) return (int)e;
    const int node_grid = grapes_div_up(num_nodes, 256), part_grid = grapes_div_up(num_parts, 256);
    hipLaunchKernelGGL(part_admit_hist_k, dim3(node_grid), dim3(256), 0, s, want, gain, (const int32_t*)part, num_nodes, num_parts, cnt,
                       status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_admit_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, (const int32_t*)cnt, num_parts, off, moved);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_admit_scatter_k, dim3(node_grid), dim3(256), 0, s, want, gain, (const int32_t*)part, num_nodes, num_parts,
                       (const int32_t*)off, cursor, keys);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_admit_limit_k, dim3(part_grid), dim3(256), 0, s, (const int32_t*)off, (const int32_t*)size, num_parts, cap,
                       limit, hdr, full);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_admit_select_k, dim3(num_parts < 1024 ? num_parts : 1024), dim3(1024), 0, s,
                       (const unsigned long long*)keys, (const int32_t*)off, (const int32_t*)size, num_parts, cap, (const int32_t*)hdr,
                       (const int32_t*)full, limit);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_admit_apply_k, dim3(node_grid), dim3(256), 0, s, (const unsigned long long*)keys, (const int32_t*)off,
                       num_parts, want, (const unsigned long long*)limit, part, size, moved);
    GRAPES_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the cut

// The workgroup's sum into one of the PART_CUT_SLOTS accumulators (an integer atomic: any order gives the same sum).
__device__ __forceinline__ void part_cut_add(unsigned long long mine, unsigned long long* lds, unsigned long long* acc) {
    unsigned long long tot;
    block_excl_scan_u64(mine, lds, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&acc[blockIdx.x % PART_CUT_SLOTS], tot);
}

// 1 when entry j of row v (label cur) is cut
__device__ __forceinline__ int part_cut_entry(const int32_t* __restrict__ col, const int32_t* __restrict__ part, int64_t j, int v, int cur,
                                              int N, int P, bool& bad) {
    const int l = part_label(col, part, j, v, N, P, bad);
    return l >= 0 && l != cur ? 1 : 0;
}

// A wavefront per row; hdr[0] = the rows of more than PART_CUT_WAVE_ROW entries, listed.
__global__ __launch_bounds__(256) void part_cut_rows_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                       const int32_t* __restrict__ part, int P, int32_t* hdr, int32_t* __restrict__ list,
                                                       unsigned long long* acc, int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned long long mine = 0ull;
    bool bad = false;
    for (int64_t v64 = wave; v64 < (int64_t)N; v64 += waves) {                  // (a capped grid: one atomic per workgroup, not per four rows)
        const int v = (int)v64;
        const int64_t a = rowptr[v];
        const long long deg = (long long)(rowptr[v + 1] - a);
        if (deg > PART_CUT_WAVE_ROW) {
            if (lane == 0) list[atomicAdd(&hdr[0], 1)] = v;
        } else if (deg > 0) {
            const int cur = part[v];
            if ((unsigned)cur >= (unsigned)P) bad = bad || lane == 0;
            else
                for (long long t = lane; t < deg; t += 64) mine += part_cut_entry(col, part, a + t, v, cur, N, P, bad);
        }
    }
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    part_cut_add(mine, lds, acc);
}

__global__ __launch_bounds__(256) void part_cut_long_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                       const int32_t* __restrict__ part, int P, const int32_t* __restrict__ hdr,
                                                       const int32_t* __restrict__ list, unsigned long long* acc, int32_t* status) {
    __shared__ unsigned long long lds[17];
    int n_long = hdr[0];
    n_long = n_long < N ? n_long : N;
    unsigned long long mine = 0ull;
    bool bad = false;
    for (int h = blockIdx.x; h < n_long; h += gridDim.x) {
        const int v = list[h];
        const int64_t a = rowptr[v];
        const long long deg = (long long)(rowptr[v + 1] - a);
        const int cur = part[v];
        if ((unsigned)cur >= (unsigned)P) { bad = true; continue; }
        for (long long t = threadIdx.x; t < deg; t += 256) mine += part_cut_entry(col, part, a + t, v, cur, N, P, bad);
    }
    if (bad && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    part_cut_add(mine, lds, acc);
}

__global__ __launch_bounds__(64) void part_cut_finish_k(const unsigned long long* __restrict__ acc, int64_t* __restrict__ cut) {
    const unsigned long long tot = wave_sum_u64(acc[threadIdx.x]);
    if (threadIdx.x == 0) *cut = (int64_t)tot;
}

// acc u64[PART_CUT_SLOTS] | hdr int32[PART_HDR] | list int32[N]
extern "C" size_t grapes_partition_cut_workspace_bytes(int32_t num_nodes) {
    const size_t N = num_nodes > 0 ? (size_t)num_nodes : 1;
    return PART_CUT_SLOTS * 8 + (PART_HDR + N) * 4 + 16;
}

extern "C" int grapes_partition_cut(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* part, int32_t num_parts,
                                    int64_t* cut, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || num_parts <= 0 || !rowptr || !col || !part || !cut || !workspace) return GRAPES_EINVAL;
    if ((uintptr_t)workspace & 7) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* acc = (unsigned long long*)workspace;
    int32_t* hdr = (int32_t*)(acc + PART_CUT_SLOTS);
    int32_t* list = hdr + PART_HDR;
    hipError_t e = grapes_zero_async(acc, PART_CUT_SLOTS * 8 + PART_HDR * 4, s);
    if (e != hipSuccess) return (int)e;
    const int64_t row_blocks = ((int64_t)num_nodes * 64 + 255) / 256;
    hipLaunchKernelGGL(part_cut_rows_k, dim3((unsigned)(row_blocks < PART_CUT_GRID ? row_blocks : PART_CUT_GRID)), dim3(256), 0, s, rowptr,
                       col, num_nodes, part, num_parts, hdr, list, acc, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_cut_long_k, dim3(num_nodes < 256 ? num_nodes : 256), dim3(256), 0, s, rowptr, col, num_nodes, part, num_parts,
                       (const int32_t*)hdr, (const int32_t*)list, acc, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_cut_finish_k, dim3(1), dim3(64), 0, s, (const unsigned long long*)acc, cut);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
