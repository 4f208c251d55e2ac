// Cluster-GCN [Chiang et al., KDD 2019; PyG-recall: ClusterData, ClusterLoader, ClusterGCNConv]: partition-based training.  The graph
// is cut into P clusters once; a batch is the subgraph induced on the union of q chosen clusters, so the edges between the chosen
// clusters come back.  The rule written in include/grapes_hip.h is the contract; tests/cluster_oracle.py reproduces every integer.
//
// ---- the batch (grapes_cluster_batch).  In cluster order the union's node set is q contiguous ranges of perm: it needs no sort and
// no N-sized node map.  where[u] = (cluster of u, position of u inside it) is one 8-byte load, stamp[c] = (serial, first local row of
// c in this batch) another: u is a member iff stamp[where[u].cluster].serial == serial, and its local row is base + position.  The
// table is never cleared between calls: the caller hands out a new serial per call.  The row-list pattern of row_list.h:
//   cluster_head_k   ONE workgroup: the q sizes and their exclusive prefix -> cptr (list_scan_tiles), the stamps, n, and the three
//                    refusals (a cluster id outside [0, P), a cluster listed twice, n > n_cap).  A duplicate is seen by the atomicExch
//                    that stamps the serial: exactly one of the two stores finds the serial already there, whichever wins, and the
//                    flag is read after the barrier, so the outcome does not depend on the race
//   cluster_rows_k   a thread per local row: its chosen cluster (lower_bound over cptr), node_idx, and the row's count of work items
//   cluster_items_k  ONE workgroup: the exclusive prefix of the item counts, in place -> item_off
//   cluster_count_k  a wavefront per item = 64 consecutive entries of one row, one per lane: col -> where -> stamp, the item's two
//                    dependent lookups in flight together; the member lanes as one 64-bit mask
//   cluster_scan_k   ONE workgroup: the exclusive prefix of the masks' popcounts over ALL items — the chunks of a hub row feed the same
//                    prefix as the short rows — the edge count and the overflow bit
//   cluster_write_k  a wavefront per item: the member lanes behind the item's offset in lane order (= CSR order); a thread per slot of
//                    rowptr_l: off[item_off[i]] for a live row, e for every slot from n to n_cap
// Integer code only, no global atomic beyond the status OR and the stamps, bit-identical runs, six launches, no host read.
//
// ClusterGCNConv's propagation is grapes_rootsum_aggregate_fwd / _bwd (rootsum_kernels.hip).
#include "row_list.h"

#define CLUSTER_CHUNK GRAPES_LONG_ROW
#define CLUSTER_MAX_BATCH_PARTS (1 << 20)
#define CLUSTER_ITEM_CAP_MAX (1 << 24)                                         // (64 item_cap threads in one grid)
static_assert(CLUSTER_CHUNK == 64, "a work item is one entry per lane and its member set one 64-bit mask");

// hdr[0] = n, the live rows (0 for a refused batch); hdr[1] = the live work items
#define CLUSTER_HDR 4

// ------------------------------------------------------------------------------------------------------------ the batch

// ONE workgroup.  cptr[k] = the rows of the chosen clusters before k, cptr[q] = n; stamp[c] = (serial, cptr[k]) for c = clusters[k].
// A refused batch — a bad or repeated cluster id (GRAPES_STATUS_BAD_INDEX), else n > n_cap (GRAPES_STATUS_NODE_OVERFLOW) — has
// cptr = 0 throughout and n = 0; its stamps carry this call's serial, which no later call uses.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void cluster_head_k(const int32_t* __restrict__ clusters, int Q, int P,
                                                                    const int32_t* __restrict__ partptr, int32_t* stamp, int serial,
                                                                    int n_cap, int32_t* cptr, int32_t* __restrict__ d_n,
                                                                    int32_t* __restrict__ hdr, int32_t* status) {
    __shared__ unsigned long long lds[17];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    auto sizes = [&](int i0, int (&v)[LIST_SCAN_PER]) {
        int c[LIST_SCAN_PER], a[LIST_SCAN_PER], b[LIST_SCAN_PER];
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) c[k] = i0 + k < Q ? clusters[i0 + k] : -1;
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) {
            const bool ok = i0 + k < Q && (unsigned)c[k] < (unsigned)P;
            bad = bad || (i0 + k < Q && !ok);
            a[k] = b[k] = 0;
            if (ok) {
                a[k] = partptr[c[k]]; b[k] = partptr[c[k] + 1];
                if (atomicExch(&stamp[2 * c[k]], serial) == serial) bad = true;   // listed twice: one of the two finds the serial
            }
        }
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) v[k] = b[k] > a[k] ? b[k] - a[k] : 0;
    };
    const unsigned long long total = list_scan_tiles<int>(sizes, Q, 0x7fffffffull, cptr, lds);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    const bool refused = s_bad != 0, over = !refused && total > (unsigned long long)n_cap;
    if (threadIdx.x == 0) {
        if (refused && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
        if (over && status) atomicOr(status, GRAPES_STATUS_NODE_OVERFLOW);
        const int n = (refused || over) ? 0 : (int)total;
        cptr[Q] = n; *d_n = n; hdr[0] = n;
    }
    // a thread revisits the positions it wrote in the scan
    for (int tile = 0; tile < Q; tile += LIST_SCAN_THREADS * LIST_SCAN_PER) {
        const int i0 = tile + (int)threadIdx.x * LIST_SCAN_PER;
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) {
            if (i0 + k >= Q) continue;
            if (refused || over) cptr[i0 + k] = 0;
            else stamp[2 * clusters[i0 + k] + 1] = cptr[i0 + k];
        }
    }
}

// A thread per local row i < n: node_idx[i] and, in item_off[i], the row's work items (until cluster_items_k scans them).
__global__ __launch_bounds__(256) void cluster_rows_k(const int64_t* __restrict__ rowptr, int N, const int32_t* __restrict__ perm,
                                                      const int32_t* __restrict__ partptr, const int32_t* __restrict__ clusters, int Q,
                                                      const int32_t* __restrict__ cptr, const int32_t* __restrict__ hdr,
                                                      int32_t* __restrict__ node_idx, int32_t* __restrict__ item_off, int32_t* status) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)hdr[0]) return;
    const int i = (int)g;
    const int k = lower_bound<int32_t, int, int>(cptr, Q + 1, i + 1) - 1;      // the last chosen cluster with cptr[k] <= i
    const long long at = (long long)partptr[clusters[k]] + (i - cptr[k]);
    const int v = (unsigned long long)at < (unsigned long long)N ? perm[at] : -1;   // (-1: tables that do not describe N nodes)
    node_idx[i] = v;
    long long nch = 0;
    if ((unsigned)v < (unsigned)N) {
        const long long deg = (long long)(rowptr[v + 1] - rowptr[v]);
        nch = deg > 0 ? (deg + CLUSTER_CHUNK - 1) / CLUSTER_CHUNK : 0;
    } else if (status) {
        atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    }
    item_off[i] = (int)(nch < 0x7fffffffll ? nch : 0x7fffffffll);
}

// ONE workgroup.  item_off[i] = min(the items of the rows before i, item_cap) in place, item_off[n] = hdr[1] = min(their total,
// item_cap); more raise GRAPES_STATUS_EDGE_OVERFLOW.
__global__ __launch_bounds__(LIST_SCAN_THREADS) void cluster_items_k(int32_t* __restrict__ hdr, int item_cap, int32_t* item_off,
                                                                     int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int n = hdr[0];
    auto items = [&](int i0, int (&v)[LIST_SCAN_PER]) {
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) v[k] = i0 + k < n ? item_off[i0 + k] : 0;
    };
    const unsigned long long total = list_scan_tiles<int>(items, n, (unsigned long long)item_cap, item_off, lds);
    list_scan_finish(total, item_cap, item_off + n, hdr + 1, status);
}

// The item of this wavefront: its local row r, the row's first entry a in col and the entry t of this lane (in: t is inside the row).
struct ClusterItem { int r; int64_t a; long long t; bool in; };
__device__ __forceinline__ ClusterItem cluster_item(int it, int r, const int64_t* __restrict__ rowptr, int N,
                                                    const int32_t* __restrict__ node_idx, const int32_t* __restrict__ item_off, int lane) {
    ClusterItem I; I.r = r; I.a = 0; I.in = false;
    I.t = (long long)(it - item_off[r]) * CLUSTER_CHUNK + lane;
    const int v = node_idx[r];
    if ((unsigned)v >= (unsigned)N) return I;                                  // (the bit was raised by cluster_rows_k)
    I.a = rowptr[v];
    I.in = I.t < (long long)(rowptr[v + 1] - I.a);
    return I;
}

// The local row of neighbour u, or -1 when u is in no chosen cluster: two dependent 8-byte loads.
__device__ __forceinline__ int cluster_local(int u, const int2* __restrict__ where, const int2* __restrict__ stamp, int P, int serial) {
    const int2 w = where[u];
    if ((unsigned)w.x >= (unsigned)P) return -1;
    const int2 st = stamp[w.x];
    return st.x == serial ? st.y + w.y : -1;
}

// A wavefront per item: mask[it] = the member lanes, item_row[it] = its local row.  A column outside [0, N) raises
// GRAPES_STATUS_BAD_INDEX and is dropped.
__global__ __launch_bounds__(256) void cluster_count_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                       const int2* __restrict__ where, const int2* __restrict__ stamp, int P, int serial,
                                                       const int32_t* __restrict__ node_idx, const int32_t* __restrict__ hdr,
                                                       const int32_t* __restrict__ item_off, unsigned long long* __restrict__ mask,
                                                       int32_t* __restrict__ item_row, int32_t* status) {
    const int it = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (it >= hdr[1]) return;                                                  // (whole wavefronts leave)
    const int n = hdr[0];
    const int r = lower_bound<int32_t, int, int>(item_off, n, it + 1) - 1;     // rows without an entry own no item and are stepped over
    const ClusterItem I = cluster_item(it, r, rowptr, N, node_idx, item_off, lane);
    const int u = I.in ? col[I.a + I.t] : 0;
    const bool ok = I.in && (unsigned)u < (unsigned)N;
    if (I.in && !ok && status) atomicOr(status, GRAPES_STATUS_BAD_INDEX);
    const bool keep = ok && cluster_local(u, where, stamp, P, serial) >= 0;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) { mask[it] = bal; item_row[it] = r; }
}

// ONE workgroup.  off[it] = min(the members of the items before it, e_cap), off[n_items] = *d_e = min(their total, e_cap).
__global__ __launch_bounds__(LIST_SCAN_THREADS) void cluster_scan_k(const unsigned long long* __restrict__ mask,
                                                                    const int32_t* __restrict__ hdr, int e_cap, int32_t* __restrict__ off,
                                                                    int32_t* __restrict__ d_e, int32_t* status) {
    __shared__ unsigned long long lds[17];
    const int n_items = hdr[1];
    auto kept = [&](int i0, int (&v)[LIST_SCAN_PER]) {
        unsigned long long w[LIST_SCAN_PER];
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) w[k] = i0 + k < n_items ? mask[i0 + k] : 0ull;
#pragma unroll
        for (int k = 0; k < LIST_SCAN_PER; ++k) v[k] = __popcll(w[k]);
    };
    const unsigned long long total = list_scan_tiles<int>(kept, n_items, (unsigned long long)e_cap, off, lds);
    list_scan_finish(total, e_cap, off + n_items, d_e, status);
}

// Thread g: rowptr_l[g] for g <= n_cap.  Wavefront g / 64: the member lanes of item g / 64 behind off[it], in lane order; nothing is
// written at or past e_cap.
__global__ __launch_bounds__(256) void cluster_write_k(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                                       const int2* __restrict__ where, const int2* __restrict__ stamp, int P, int serial,
                                                       const int32_t* __restrict__ node_idx, const int32_t* __restrict__ hdr,
                                                       const int32_t* __restrict__ item_off, const unsigned long long* __restrict__ mask,
                                                       const int32_t* __restrict__ item_row, const int32_t* __restrict__ off, int n_cap,
                                                       int e_cap, int32_t* __restrict__ rowptr_l, int32_t* __restrict__ edge_src,
                                                       int32_t* __restrict__ edge_dst, int64_t* __restrict__ edge_id) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int n = hdr[0], n_items = hdr[1];
    if (g <= (int64_t)n_cap) rowptr_l[g] = off[g < (int64_t)n ? item_off[g] : n_items];
    const int64_t it64 = g >> 6;
    if (it64 >= (int64_t)n_items) return;                                      // (whole wavefronts leave)
    const int it = (int)it64;
    const unsigned long long bal = mask[it];
    int base = off[it];
    if (bal == 0ull || base >= e_cap) return;
    const bool keep = (bal >> lane) & 1ull;
    const int p = wave_compact_slot(keep, lane, base);
    if (!keep || p >= e_cap) return;
    const int r = item_row[it];
    const ClusterItem I = cluster_item(it, r, rowptr, N, node_idx, item_off, lane);
    edge_src[p] = cluster_local(col[I.a + I.t], where, stamp, P, serial);
    edge_dst[p] = r;
    if (edge_id) edge_id[p] = (int64_t)(I.a + I.t);
}

// mask uint64[item_cap] | hdr int32[CLUSTER_HDR] | item_off int32[n_cap + 1] | off int32[item_cap + 1] | item_row int32[item_cap]
extern "C" size_t grapes_cluster_batch_workspace_bytes(int32_t n_cap, int32_t item_cap) {
    const size_t M = n_cap > 0 ? (size_t)n_cap : 1, I = item_cap > 0 ? (size_t)item_cap : 1;
    return I * 8 + CLUSTER_HDR * 4 + (M + 1) * 4 + (I + 1) * 4 + I * 4 + 16;
}

extern "C" int grapes_cluster_batch(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* perm,
                                    const int32_t* partptr, const int32_t* where, int32_t num_parts, const int32_t* clusters, int32_t q,
                                    int32_t* stamp, int32_t serial, int32_t n_cap, int32_t item_cap, int32_t e_cap, int32_t* cptr,
                                    int32_t* node_idx, int32_t* rowptr_l, int32_t* edge_src, int32_t* edge_dst, int64_t* edge_id,
                                    int32_t* d_n, int32_t* d_e, void* workspace, int32_t* status, grapes_stream_t stream) {
    if (num_nodes <= 0 || num_parts <= 0 || q <= 0 || q > CLUSTER_MAX_BATCH_PARTS || serial <= 0) return GRAPES_EINVAL;
    if (n_cap <= 0 || n_cap > 0x7ffffffe || e_cap <= 0 || item_cap <= 0 || item_cap > CLUSTER_ITEM_CAP_MAX) return GRAPES_EINVAL;
    if (!rowptr || !col || !perm || !partptr || !where || !clusters || !stamp || !cptr || !node_idx || !rowptr_l || !edge_src ||
        !edge_dst || !d_n || !d_e || !workspace)
        return GRAPES_EINVAL;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)where & 7) || ((uintptr_t)stamp & 7)) return GRAPES_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* mask = (unsigned long long*)workspace;
    int32_t* hdr = (int32_t*)(mask + item_cap);
    int32_t* item_off = hdr + CLUSTER_HDR;
    int32_t* off = item_off + ((size_t)n_cap + 1);
    int32_t* item_row = off + ((size_t)item_cap + 1);
    const int2* where2 = (const int2*)where;
    const int2* stamp2 = (const int2*)stamp;
    const int64_t item_threads = (int64_t)item_cap * 64, slot_threads = (int64_t)n_cap + 1;
    hipLaunchKernelGGL(cluster_head_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, clusters, q, num_parts, partptr, stamp, serial, n_cap, cptr,
                       d_n, hdr, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_rows_k, dim3(grapes_div_up(n_cap, 256)), dim3(256), 0, s, rowptr, num_nodes, perm, partptr, clusters, q,
                       (const int32_t*)cptr, (const int32_t*)hdr, node_idx, item_off, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_items_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, hdr, item_cap, item_off, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_count_k, dim3(grapes_div_up(item_threads, 256)), dim3(256), 0, s, rowptr, col, num_nodes, where2, stamp2,
                       num_parts, serial, (const int32_t*)node_idx, (const int32_t*)hdr, (const int32_t*)item_off, mask, item_row, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_scan_k, dim3(1), dim3(LIST_SCAN_THREADS), 0, s, (const unsigned long long*)mask, (const int32_t*)hdr, e_cap,
                       off, d_e, status);
    GRAPES_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_write_k, dim3(grapes_div_up(item_threads > slot_threads ? item_threads : slot_threads, 256)), dim3(256), 0,
                       s, rowptr, col, num_nodes, where2, stamp2, num_parts, serial, (const int32_t*)node_idx, (const int32_t*)hdr,
                       (const int32_t*)item_off, (const unsigned long long*)mask, (const int32_t*)item_row, (const int32_t*)off, n_cap,
                       e_cap, rowptr_l, edge_src, edge_dst, edge_id);
    GRAPES_LAUNCH_CHECK();
    return 0;
}
