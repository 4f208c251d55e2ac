/*
 * grapes_hip.h — C-ABI of libgrapes_hip.so: the MI355X (gfx950) implementation of GRAPES'
 * per-layer sample-then-aggregate training step.
 *
 * Every entry point replaces one piece of the reference's hot path (dfdazac/grapes; citations
 * are file:line in that repository).  The reference is pure Python, so the binding a maintainer
 * adds is a ctypes stub; grapes_amd/_lib.py is exactly that stub.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (hipMalloc / torch caching allocator) unless named h_*.
 *  - Node ids / local ids / CSR column indices are int32; CSR row pointers of the *graph* are
 *    int64 (ogbn-papers100M has 3.2e9 directed edges); per-hop CSRs use int32 row pointers.
 *  - Feature matrices are dense row-major fp32.
 *  - Dynamic sizes: a `const int32_t* d_x` argument, when non-NULL, points to the true element
 *    count on the device; the host argument next to it is then only the CAPACITY used to size the
 *    launch.  When NULL the host argument is the exact size.  No entry point synchronises the
 *    device or allocates memory: all of them only enqueue work on `stream` and are therefore
 *    legal inside hipGraph capture.
 *  - `status` (optional, may be NULL) is a device int32 word; kernels OR error bits into it
 *    (GRAPES_STATUS_*).  The caller reads it at its own synchronisation point.
 *  - Return value: 0 on success, a negative GRAPES_E* code for an invalid argument, or a positive
 *    hipError_t if a launch failed.  Nothing aborts.
 */
#ifndef GRAPES_HIP_H
#define GRAPES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version = 100 * MAJOR + MINOR.
 *   MAJOR changes when an entry point declared here changes its signature or meaning, or leaves the product surface: a binding
 *         written against another MAJOR must refuse to load the library.
 *   MINOR counts additions within a MAJOR: a binding written against MINOR m loads any library with MINOR >= m.
 * History: 1 (rounds 1-3, never bumped while entry points were added); 200 (round 4): the measurement-only entry points
 * (grapes_debug_*) left the product library for the diagnostic build (GRAPES_DIAG), the rider entry points were added, and the
 * product library stopped reading GRAPES_* environment switches;
 * 205: step chains (grapes_graph_chain_*); 206: grapes_linear_bwd_weight_gathered_split_multi;
 * 300 (round 5): grapes_draw_finish_args grew a field (stats_blocks) and grapes_sampler_hist_words() words now include the one-launch
 * draw's barrier words behind the histogram (callers that size d_hist by that call need no change; a binding that mirrors the struct
 * does); added: grapes_gumbel_topk_deferred_ext, grapes_frontier_expand_fused_ext; REMOVED (each a special case of an entry point that stays:
 * profiles/r05_entry_point_census.txt): grapes_frontier_expand_fused_counted / _finish (-> _ext), grapes_gumbel_topk_deferred (-> _deferred_ext),
 * grapes_linear_bwd_weight_bits_multi / _pair (-> _multi_cols / _pair_cols with dw_cols = 0), grapes_sampler_head_bwd_multi (-> _multi_phase, phase 0),
 * grapes_gate_bits_words;
 * 301: grapes_linear_fwd_row_scaled (full-batch inference: the dinv row scaling in the transform GEMM's epilogue);
 * 302: grapes_eval_predict; added within 302 (no signature of an earlier entry point changed): the full-batch path above 2^31
 * entries — grapes_csr_symmetric_check, grapes_csr_transpose, grapes_gcn_large_prepare, grapes_gcn_large_aggregate(_workspace_bytes);
 * and full-batch training over such graphs — grapes_rowlist_transpose(_workspace_bytes), grapes_rowlist_gather_t(_workspace_bytes),
 * grapes_dropout_rows, grapes_rowlist_loss(_workspace_bytes); GraphSAINT random-walk training — grapes_saint_walk_nodes,
 * grapes_saint_subgraph(_workspace_bytes), grapes_saint_masked_loss; the GAT classifier (modules/gcn.py:45-72) — grapes_gat_scores,
 * grapes_gat_aggregate_fwd / _bwd (+ _workspace_bytes each); the GCN2 classifier (modules/gcn.py:76-117) —
 * grapes_gcn2_loop_counts(_csr), grapes_gcn2_propagate_fwd / _bwd (+ _workspace_bytes), grapes_gcn2_mix_fwd / _bwd; the PNA
 * classifier (modules/gcn.py:120-149) — grapes_pna_aggregate_fwd / _bwd (+ _workspace_bytes each), grapes_pna_add_input_grad; GraphSAINT's node and edge
 * samplers — grapes_saint_edge_weights, grapes_saint_draw_nodes; GraphSAINT's normalisation — grapes_saint_coverage_count,
 * grapes_saint_norms; GCNConv with edge weights and with its improved / add_self_loops / normalize arguments —
 * grapes_wgcn_structure(_workspace_bytes), grapes_wgcn_loops(_workspace_bytes), grapes_wgcn_weights, grapes_wgcn_aggregate_fwd / _bwd
 * (+ _workspace_bytes each);
 * 303: five signatures grew the arguments of a twin that 302 had added beside them, and the twins left: grapes_wgcn_weights (loop_ptr,
 * loop_idx, mode, fill), grapes_wgcn_aggregate_fwd / _bwd (mode) <- their _mode forms; grapes_saint_subgraph (edge_id, edge_norm,
 * edge_norm_b) <- its _ids form; grapes_saint_masked_loss (node_norm) <- its _weighted form; added within 303 (no signature of an
 * earlier entry point changed): the LADIES / FastGCN layer-wise samplers — grapes_ladies_importance,
 * grapes_ladies_layer(_workspace_bytes); the AS-GCN adaptive sampler — grapes_asgcn_importance, grapes_asgcn_rows_workspace_bytes,
 * grapes_asgcn_variance, grapes_asgcn_logq_bwd; GraphSAGE — grapes_sage_sample_layer(_workspace_bytes),
 * grapes_sage_aggregate_fwd / _bwd, grapes_sage_aggregate_workspace_bytes; VR-GCN — grapes_vrgcn_aggregate_fwd / _bwd,
 * grapes_vrgcn_aggregate_workspace_bytes, grapes_vrgcn_long_row; LABOR — grapes_labor_sample_layer(_workspace_bytes),
 * grapes_labor_importance(_workspace_bytes); ShaDow-GNN — grapes_shadow_sample(_workspace_bytes), grapes_shadow_ppr_sample(_workspace_bytes), grapes_segment_mean_fwd / _bwd;
 * Cluster-GCN — grapes_cluster_batch(_workspace_bytes), grapes_cluster_aggregate_fwd / _bwd, grapes_cluster_aggregate_workspace_bytes; its graph partitioner —
 * grapes_partition_propose, grapes_partition_admit, grapes_partition_cut (+ _workspace_bytes each); GNNAutoScale —
 * grapes_gas_resolve(_workspace_bytes), grapes_gas_aggregate_fwd / _bwd, grapes_gas_aggregate_workspace_bytes; PPRGo — grapes_pprgo_topk,
 * grapes_pprgo_batch(_workspace_bytes), grapes_pprgo_aggregate_fwd / _bwd (+ _workspace_bytes each); PinSAGE — grapes_pinsage_neighbors,
 * grapes_relu_l2norm_fwd / _bwd.
 * 304: grapes_sage_aggregate_fwd / _bwd and grapes_cluster_aggregate_fwd / _bwd were one layer written twice and left, with their two
 * _workspace_bytes: grapes_rootsum_aggregate_fwd / _bwd (loops, self_weight, self_term, scale) and
 * grapes_rootsum_aggregate_workspace_bytes compute both; added within 304 (no signature of an earlier entry point changed): LINKX's
 * adjacency embedding bag — grapes_bag_batch, grapes_bag_fwd, grapes_bag_bwd (+ _workspace_bytes each), grapes_bag_bwd_adam; the classifier's backward pass in three launches —
 * grapes_gcn_aggregate_bwd_input(_available), grapes_linear_bwd_weight_slabs_multi. */
#define GRAPES_ABI_VERSION 304

#define GRAPES_EINVAL (-1)   /* bad size / NULL pointer / unsupported shape */
#define GRAPES_EALIGN (-2)   /* pointer not aligned as required */

#define GRAPES_STATUS_EDGE_OVERFLOW 1   /* frontier produced more edges than e_cap */
#define GRAPES_STATUS_NODE_OVERFLOW 2   /* compaction produced more nodes than n_cap */
#define GRAPES_STATUS_BAD_INDEX 4       /* an index was outside its table */
#define GRAPES_STATUS_SYNC_TIMEOUT 8    /* a one-launch scan gave up waiting for another workgroup (results invalid) */
/* `sync` arguments: GRAPES_SYNC_WORDS 64-bit words of caller memory, ZERO before the first use; the kernels leave it
 * zero.  It carries the workgroup totals of the one-launch ordered scans; launches that share one must be
 * stream-ordered.  NULL selects the two-launch form of the same operation. */
#define GRAPES_SYNC_WORDS 256

typedef void* grapes_stream_t; /* hipStream_t */

int grapes_abi_version(void);
/* "gfx950" — the only architecture the code object is built for. */
const char* grapes_target_arch(void);
/* "product" (libgrapes_hip.so: one configuration, no environment switches, no measurement-only entry points) or "diag"
 * (libgrapes_hip_diag.so, built with -DGRAPES_DIAG: the same kernels + the A/B switches and probes profiles/ uses). */
const char* grapes_build_flavor(void);

/* ------------------------------------------------------------------ A4: TensorMap
 * modules/utils.py:115-117  map_tensor[keys] = arange(len(keys)) */
int grapes_tensormap_update(int32_t* map, const int32_t* keys, int32_t n, const int32_t* d_n,
                            grapes_stream_t stream);
/* modules/utils.py:119-120  out = map_tensor[keys]  (also the edge relabel of main.py:195,254) */
int grapes_tensormap_map(const int32_t* map, const int32_t* keys, int32_t* out, int64_t n,
                         const int32_t* d_n, grapes_stream_t stream);

/* ------------------------------------------------------------------ A1: get_neighborhoods
 * modules/utils.py:74-82.  Two launches: offsets (row lengths + exclusive scan), then expand.
 * eoff[m+1]: eoff[i] = first output slot of nodes[i]; eoff[m] = e.  d_e_out receives e. */
int grapes_frontier_offsets(const int64_t* rowptr, const int32_t* nodes, int32_t m,
                            const int32_t* d_m, int32_t* eoff, int32_t* d_e_out,
                            grapes_stream_t stream);
/* src[t] = nodes[i] (queried node, global id), dst[t] = neighbour; order = query order then
 * ascending column.  src_pos (optional) = i.  Edges beyond e_cap are dropped and
 * GRAPES_STATUS_EDGE_OVERFLOW is raised. */
int grapes_frontier_expand(const int64_t* rowptr, const int32_t* col, const int32_t* nodes,
                           int32_t m, const int32_t* d_m, const int32_t* eoff, int32_t e_cap,
                           int32_t* src, int32_t* dst, int32_t* src_pos, int32_t* status,
                           grapes_stream_t stream);

/* Both steps in ONE launch for m <= 2048 queried nodes and e_cap < 2^23 - 1 (the step's <= B + K previous nodes): every workgroup
 * rebuilds the short row-length scan itself; eoff[m+1] and *d_e_out are published as by grapes_frontier_offsets. */
/* mark_bits (optional; with num_nodes): the expansion also does the hop's marks of grapes_bitmap_mark_hop below — queried
 * nodes -> mark_prev_bits (may be NULL), queried nodes with at least one edge and every neighbour -> mark_bits.
 * remark (optional, host struct): grapes_slice_remark (A3 below) in the same launch — its clear_bits must be a DIFFERENT
 * bitmap than mark_prev_bits (the step alternates two previous-node bitmaps from hop to hop). */
typedef struct {
    int32_t* mult;
    const int32_t* unmark_ids; int32_t n_unmark; const int32_t* d_n_unmark;
    const int32_t* mark_ids; int32_t n_mark; const int32_t* d_n_mark;
    uint64_t* clear_bits; const int32_t* clear_ids; int32_t n_clear; const int32_t* d_n_clear;
} grapes_slice_remark_args;
int grapes_frontier_expand_fused(const int64_t* rowptr, const int32_t* col, const int32_t* nodes, int32_t m,
                                 const int32_t* d_m, int32_t e_cap, int32_t* eoff, int32_t* d_e_out,
                                 int32_t* src, int32_t* dst, int32_t* status, uint64_t* mark_prev_bits,
                                 uint64_t* mark_bits, int32_t num_nodes, const grapes_slice_remark_args* remark,
                                 const int32_t* count_mult, int32_t* count_bsum, int32_t* slice_stage,
                                 grapes_stream_t stream);
/* slice_stage (optional, with count_mult; grapes_slice_stage_words(e_cap) int32 words, no clearing needed): the WHOLE edge side
 * of slice_adjacency (modules/utils.py:85-95, call main.py:241-243) over the edges this launch produces.  With W = ceil(e_cap/64):
 *   stage[wb]            number of surviving edges among the 64 edges t in [64 wb, 64 wb + 64)      (wb < ceil(e / 64))
 *   stage[W + wb]        their summed multiplicity count_mult[dst[t]]
 *   stage[2W + 64 wb + i], stage[2W + e_cap + ...], stage[2W + 2 e_cap + ...]   src / dst / multiplicity of the i-th survivor
 * in edge order.  grapes_gcn_prepare_small_batch(slice_stage = ...) assembles the filtered edge list from it inside the
 * classifier's graph build: no grapes_slice_filter launch. */
size_t grapes_slice_stage_words(int32_t e_cap);
/* count_mult + count_bsum (optional): the first half of grapes_slice_filter over the edges this launch produces —
 * count_bsum[t / 1024] += count_mult[dst[t]] (count_bsum zero on entry: the workspace of a later
 * grapes_slice_filter(counted = 1)); `remark` must then not re-mark count_mult (its clear part is fine: the two id lists
 * belong in grapes_frontier_compact's `remark`, one launch earlier). */

/* ------------------------------------------------------------------ A8 (K2/K3): frontier compaction
 * main.py:183-195.  Replaces the reference's O(N) boolean masks (one byte per node, rebuilt and scanned per hop)
 * by a bitmap over node ids, bits[(N+63)/64] (all-zero at rest; the compaction clears what it consumes): N/8 bytes
 * streamed twice per hop.  `bits1` (a summary level used by earlier versions) is optional everywhere and ignored
 * by the compaction; pass NULL.
 * mark: set the bits of ids[0..n).  */
int grapes_bitmap_mark(uint64_t* bits, uint64_t* bits1 /* may be NULL: level-0 only */,
                       const int32_t* ids, int64_t n, const int32_t* d_n, int32_t num_nodes,
                       int32_t* status, grapes_stream_t stream);
/* mark_rows: set the bit of nodes[i] for every queried node with at least one out-edge
 * (eoff[i+1] > eoff[i], eoff from grapes_frontier_offsets): the source endpoints of main.py:186, one
 * atomic per node instead of one per edge. */
int grapes_bitmap_mark_rows(uint64_t* bits, uint64_t* bits1, const int32_t* nodes, int32_t m,
                            const int32_t* d_m, const int32_t* eoff, int32_t num_nodes,
                            int32_t* status, grapes_stream_t stream);
/* clear: zero the words holding ids[0..n) (level-0 only bitmaps, e.g. the `previous` set). */
int grapes_bitmap_clear(uint64_t* bits, const int32_t* ids, int64_t n, const int32_t* d_n,
                        grapes_stream_t stream);
size_t grapes_frontier_compact_workspace_bytes(int32_t n_cap, int32_t num_nodes);
/* Emits, in ASCENDING GLOBAL ID order (main.py:189-190):
 *   batch_nodes[0..nb)      = ids set in `bits`
 *   neighbor_nodes[0..nn)   = ids set in `bits` and not in `prev_bits`      (main.py:187)
 *   nb_local[0..nn)         = rank of each neighbour inside batch_nodes     (main.py:213)
 *   node_map[id] = rank     for every batch node (main.py:194; node_map may be NULL)
 *   counts[0] = nb, counts[1] = nn.
 * Consumes (zeroes) `bits`/`bits1`; `prev_bits` (may be NULL) is left untouched. */
/* ind_code (optional): also sets indicator bit `ind_bit` of every emitted neighbour (main.py:191), with the
 * epoch convention of grapes_indicator_mark. */
int grapes_frontier_compact(uint64_t* bits, uint64_t* bits1, const uint64_t* prev_bits,
                            int32_t num_nodes, int32_t n_cap, int32_t* batch_nodes,
                            int32_t* neighbor_nodes, int32_t* nb_local, int32_t* node_map,
                            int32_t* counts, uint32_t* ind_code, uint32_t epoch, const uint32_t* d_epoch,
                            int32_t ind_bit, int32_t* cand_pos, void* zero_a, size_t zero_a_words, void* zero_b,
                            size_t zero_b_words, void* zero_c, size_t zero_c_words,
                            const grapes_slice_remark_args* remark, void* workspace, uint64_t* sync,
                            int32_t* status, grapes_stream_t stream);
/* remark (optional): the un-mark / mark id lists of grapes_slice_remark applied by this launch (its clear part is ignored
 * here) — the slice marks of the hop that starts with this compaction. */
/* zero_a / zero_b / zero_c (optional): three ranges of 32-bit words cleared by the same launch — the scratch the NEXT operation wants
 * zeroed (grapes_gcn_prepare with GRAPES_PREP_PREZEROED: its counters and csr_dst; the count_bsum of the hop's expansion), so that it needs no clearing launch. */
/* cand_pos (optional) int32[n_cap]: the inverse of nb_local — position of batch node j in neighbor_nodes, -1 if it is a
 * previous node (used by the sampler's backward pass to write d log_prob / d logit densely). */
/* sync != NULL and at most GRAPES_SYNC_WORDS - 1 workgroups (num_nodes <= 255 * 65536): ONE launch. */
/* ---- The hop graph's degree counting folded into the launches either side of it (main.py:180-195 feeding modules/gcn.py:32's
 * gcn_norm): grapes_gcn_prepare spends two of its four launches on an in-degree histogram over the relabelled edges and a scan
 * of it.  Local ids are assigned in ascending GLOBAL id order, so both can ride on launches that exist anyway:
 *   grapes_frontier_expand_fused_ext(count) per produced edge u -> v (u != v): slot[t] = atomicAdd(indeg[v], 1) — the entry's place
 *       in v's by-target row — and +1 on the in-degree sum of v's bitmap word; per queried node its edge segment (first, length)
 *       and its out-degree on the word sums of the by-source side; self-loops: slot -1, loops[u] += 1.
 *   grapes_frontier_compact_counted        reads the two word sums next to the bitmap words it scans anyway (two more scanned
 *       quantities, a second look-back word), and per emitted node its in-degree (and, for a queried node, its segment): writes
 *       rowptr_t, rowptr_s, dinv, seg_first, row_loops, the long-row items and the edge count — what grapes_gcn_prepare's first
 *       two launches produce — and puts the counters back to zero.
 *   grapes_gcn_prepare_counted             the remaining two launches: entries placed at rowptr_t[dst] + slot (no atomics),
 *       by-source rows from the segments, canonical row order + head records (identical arrays to grapes_gcn_prepare's).
 * All counter tables are indexed by GLOBAL node id, zero at rest and left zero:  indeg int32[N], loops int32[N],
 * seginfo int32[2 N] (written for every queried node, never cleared), wsum int32[2 ceil(N / 64)].  sync2: a second look-back
 * scratch of GRAPES_SYNC_WORDS words (zero at rest).  n_long: the build's counters (words 0, 1 zeroed by the expansion,
 * word 2 = aggregated edges written by the compaction). */
typedef struct {
    int32_t* indeg; int32_t* loops; int32_t* seginfo; int32_t* wsum;
    int32_t* slot;            /* expansion output, int32[e_cap]; NULL: the in-degree atomics return nothing (cursor form below) */
    int32_t* n_long;          /* counters of the build that follows (may be NULL) */
} grapes_hop_count_args;
typedef struct {
    int32_t* indeg; int32_t* loops; const int32_t* seginfo; int32_t* wsum;
    int32_t* rowptr_t; int32_t* rowptr_s; float* dinv; int32_t* seg_first; int32_t* row_loops;   /* [n_cap + 1] x 2, [n_cap] x 3 */
    int32_t* long_items; int32_t* n_long; int32_t item_cap;    /* as grapes_gcn_prepare (may be NULL / NULL / 0) */
    uint64_t* sync2;
    int32_t* cursor;          /* optional int32[n_cap]: a copy of rowptr_t for the CURSOR form of grapes_gcn_prepare_counted (slot = NULL:
                                 entries take their place with an atomic on the row's cursor, as grapes_gcn_prepare's fill does) */
} grapes_hop_degree_args;
/* ... and the END of the draw that produced `nodes` (grapes_gumbel_topk_deferred): the draw's last launch then has no tail — no
 * ticket, no last workgroup — and ONE extra workgroup of this expansion, which runs after it on the stream anyway, adds the
 * draw's log-prob partial sums in the draw's own fixed order into stats[4] and puts the draw-wide histogram back to zero
 * (main.py:276 reads that sum only when the GFlowNet loss is formed).  finish: filled by grapes_gumbel_topk_deferred (host struct,
 * device pointers into that draw's workspace, which must still be alive); NULL: no draw is finished here. */
typedef struct {
    const double* parts_keys;     /* keep-all draws (n <= k): the keys launch's partials, stride 5 doubles, keys_blocks of them */
    const double* parts_emit;     /* exact-k draws: one partial per emit workgroup */
    const uint32_t* sel;          /* sel[2] != 0: the draw kept everything */
    int32_t keys_blocks, emit_block, n_host; const int32_t* d_n;
    float* stats;                 /* stats[4] <- the sum (may be NULL) */
    uint32_t* hist; int32_t hist_words;     /* zeroed (may be NULL / 0) */
    int32_t stats_blocks;         /* > 0 (the one-launch draw): stats[0..3] are formed HERE from stats_blocks per-workgroup partials
                                     (min, max, sum, sum of squares) at parts_keys - 4, stride 5 doubles; 0: the draw wrote them */
} grapes_draw_finish_args;
/* ... and the queried rows' EXTENTS from memory (round 5): node_ext[2 i], node_ext[2 i + 1] = rowptr[nodes[i]], rowptr[nodes[i] + 1],
 * 16-byte aligned, written by whoever wrote `nodes` (grapes_gumbel_topk_deferred_ext for a hop's  cat(targets, kept)  list) — the
 * launch then reads ids, extents and the live count in ONE round trip instead of two dependent ones (modules/utils.py:78: the row
 * lookup of get_neighborhoods).  node_ext_out (optional): the extents this launch worked out itself (node_ext == NULL), for the
 * later lists that begin with the same ids (main.py:236: every hop's list starts with the targets).  NULL / NULL:
 * the plain launch with the draw's end / the degree counting riding in it. */
int grapes_frontier_expand_fused_ext(const int64_t* rowptr, const int32_t* col, const int32_t* nodes, int32_t m,
                                     const int32_t* d_m, int32_t e_cap, int32_t* eoff, int32_t* d_e_out,
                                     int32_t* src, int32_t* dst, int32_t* status, uint64_t* mark_prev_bits,
                                     uint64_t* mark_bits, int32_t num_nodes, const grapes_slice_remark_args* remark,
                                     const int32_t* count_mult, int32_t* count_bsum, int32_t* slice_stage,
                                     const grapes_hop_count_args* count, const grapes_draw_finish_args* finish,
                                     const int64_t* node_ext, int64_t* node_ext_out, grapes_stream_t stream);
int grapes_frontier_compact_counted(uint64_t* bits, uint64_t* bits1, const uint64_t* prev_bits,
                                    int32_t num_nodes, int32_t n_cap, int32_t* batch_nodes,
                                    int32_t* neighbor_nodes, int32_t* nb_local, int32_t* node_map,
                                    int32_t* counts, uint32_t* ind_code, uint32_t epoch, const uint32_t* d_epoch,
                                    int32_t ind_bit, int32_t* cand_pos, void* zero_a, size_t zero_a_words, void* zero_b,
                                    size_t zero_b_words, void* zero_c, size_t zero_c_words,
                                    const grapes_slice_remark_args* remark, void* workspace, uint64_t* sync,
                                    int32_t* status, const grapes_hop_degree_args* degrees, grapes_stream_t stream);
/* edge_src / edge_dst: GLOBAL ids as the expansion wrote them, node_map the compaction's relabel table; tmp_src: int32[e]
 * scratch; head_ids / row_head, prefetch_* as grapes_gcn_prepare_prefetching (helpers ride in the first of the two launches). */
int grapes_gcn_prepare_counted(const int32_t* edge_src, const int32_t* edge_dst, const int32_t* slot, int32_t e,
                               const int32_t* d_e, const int32_t* node_map, int32_t n, const int32_t* d_n,
                               const int32_t* rowptr_t, const int32_t* rowptr_s, const int32_t* seg_first,
                               const int32_t* row_loops, const float* dinv, int32_t* csr_src, int32_t* csr_dst,
                               int32_t* tmp_src, const int32_t* head_ids, int32_t* row_head, int32_t* status,
                               const float* prefetch_X, int64_t prefetch_pitch, int32_t prefetch_row_floats,
                               int32_t* cursor, grapes_stream_t stream);

/* The three marks of one hop in one launch (main.py:183-187): previous -> prev_bits; queried nodes with at least
 * one edge (eoff) and every neighbour dst[0..e) -> bits / bits1. */
int grapes_bitmap_mark_hop(uint64_t* prev_bits, uint64_t* bits, uint64_t* bits1, const int32_t* previous,
                           int32_t m, const int32_t* d_m, const int32_t* eoff, const int32_t* dst, int32_t e,
                           const int32_t* d_e, int32_t num_nodes, int32_t* status, grapes_stream_t stream);
/* Up to four id lists into one bitmap in one launch (main.py:221,252: all_nodes = targets + every hop's samples);
 * a list with n == 0 is skipped.  unmark_mult (optional): also zero the slice multiplicity table (A3 below) at every
 * listed id — the last un-mark of a step whose hops used grapes_slice_remark. */
int grapes_bitmap_mark_lists(uint64_t* bits, uint64_t* bits1, const int32_t* ids0, int32_t n0,
                             const int32_t* d_n0, const int32_t* ids1, int32_t n1, const int32_t* d_n1,
                             const int32_t* ids2, int32_t n2, const int32_t* d_n2, const int32_t* ids3,
                             int32_t n3, const int32_t* d_n3, int32_t num_nodes, int32_t* status,
                             int32_t* unmark_mult, grapes_stream_t stream);

/* all_nodes of a step in ONE launch when the lists are small (main.py:221,252): the ascending, duplicate-free union of up
 * to four id lists with n0 + n1 + n2 + n3 <= 4096 (host capacities) -> out_ids[0..counts[0]); node_map[id] = rank
 * (optional); unmark_mult as in grapes_bitmap_mark_lists.  Same result as marking the lists into a bitmap and compacting it.
 * More than n_cap distinct ids raise GRAPES_STATUS_NODE_OVERFLOW. */
int grapes_union_sorted(const int32_t* ids0, int32_t n0, const int32_t* d_n0, const int32_t* ids1, int32_t n1,
                        const int32_t* d_n1, const int32_t* ids2, int32_t n2, const int32_t* d_n2, const int32_t* ids3,
                        int32_t n3, const int32_t* d_n3, int32_t num_nodes, int32_t n_cap, int32_t* out_ids,
                        int32_t* node_map, int32_t* counts, int32_t* unmark_mult, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ A3: slice_adjacency
 * modules/utils.py:85-95.  `mult` is an int32[N] scratch table, all-zero at rest.
 * Step 1 grapes_slice_mark(+1 per entry of cols), step 2 frontier_offsets/expand over `rows`,
 * step 3 grapes_slice_filter keeps edge t mult[dst[t]] times, step 4 grapes_slice_mark(unmark).
 * Output order: row-major over rows, ascending global column id inside a row. */
/* clear_bits (optional): also zero the bitmap words holding cols[0..c) — in the step, `cols` is the hop's
 * previous_nodes list whose prev_bits marks are no longer needed (== grapes_bitmap_clear in the same launch). */
int grapes_slice_mark(int32_t* mult, const int32_t* cols, int32_t c, const int32_t* d_c,
                      int32_t unmark, uint64_t* clear_bits, grapes_stream_t stream);
/* Steps 4 (of hop h-1) and 1 (of hop h) in one launch: previous_nodes goes from targets + samples(h-1) to targets +
 * samples(h) (main.py:236-247), and a hop samples only nodes outside its previous_nodes, so the list to un-mark (the
 * older samples) and the list to mark (the newer ones) are disjoint from each other and from the targets, whose marks
 * stay.  clear_ids/clear_bits: the bitmap words of a third list are zeroed as in grapes_slice_mark.  Any list may be
 * empty (n == 0).  The marks left at the end of the step are removed by grapes_bitmap_mark_lists(unmark_mult). */
int grapes_slice_remark(int32_t* mult, const int32_t* unmark_ids, int32_t n_unmark, const int32_t* d_n_unmark,
                        const int32_t* mark_ids, int32_t n_mark, const int32_t* d_n_mark, uint64_t* clear_bits,
                        const int32_t* clear_ids, int32_t n_clear, const int32_t* d_n_clear, grapes_stream_t stream);
size_t grapes_slice_filter_workspace_bytes(int32_t e_cap);
/* sync (optional, see GRAPES_SYNC_WORDS): one launch instead of two for e <= 255 * 4096. */
int grapes_slice_filter(const int32_t* mult, const int32_t* src, const int32_t* dst, int32_t e,
                        const int32_t* d_e, int32_t out_cap, int32_t* out_src, int32_t* out_dst,
                        int32_t* d_out_count, void* workspace, uint64_t* sync, int32_t counted, int32_t* status,
                        grapes_stream_t stream);
/* counted != 0: `workspace` already holds the survivor count of every 1024-edge block (grapes_frontier_expand_fused's
 * count_bsum): only the emitting launch runs. */

/* ------------------------------------------------------------------ A8 (K4): feature gather
 * main.py:168,191,199-204.  ind_code[N] packs (epoch << 8 | indicator bits); a node whose epoch
 * differs from `epoch` has all indicators 0, so nothing is zeroed per batch (main.py:167). */
/* epoch: host value, or *d_epoch when d_epoch != NULL (a captured hipGraph replays with a new epoch).
 * advance_epoch != 0 (needs d_epoch): a new batch starts (main.py:167) — the marks carry *d_epoch + 1 and the kernel
 * stores that value back, so the counter needs no launch of its own. */
int grapes_indicator_mark(uint32_t* ind_code, const int32_t* ids, int32_t n, const int32_t* d_n,
                          uint32_t epoch, uint32_t* d_epoch, int32_t bit, int32_t advance_epoch,
                          grapes_stream_t stream);
/* The first launch of a captured step that feeds itself (main.py:126,157-168 without the host): targets[0..batch) =
 * ids[start..start+batch) with start = ((*d_cursor * stride + offset) * batch) mod max(1, n_ids - batch) — the unshuffled
 * sequential chunks of the reference's DataLoader, a different stripe per rank —, then *d_cursor += 1; with ind_code: the
 * grapes_indicator_mark(advance_epoch) of those targets; with totals: totals[j] += counters[j * counter_stride] (the
 * previous step's per-graph edge counters, about to be overwritten), skipped while *d_cursor == 0. */
int grapes_step_begin(uint32_t* ind_code, uint32_t* d_epoch, int32_t bit, const int32_t* ids, int32_t n_ids,
                      int32_t* d_cursor, int32_t stride, int32_t offset, int32_t batch, int32_t* targets,
                      const int32_t* counters, int32_t counter_stride, int32_t n_counters, int64_t* totals,
                      grapes_stream_t stream);
/* out[i, 0:F] = X[ids[i], :], out[i, F+j] = indicator j of ids[i]  (num_ind may be 0). */
int grapes_gather_rows(const float* X, int32_t F, const int32_t* ids, int32_t n,
                       const int32_t* d_n, const uint32_t* ind_code, uint32_t epoch,
                       const uint32_t* d_epoch,
                       int32_t num_ind, float* out, grapes_stream_t stream);

/* ------------------------------------------------------------------ A6: gcn_norm + per-hop CSRs
 * PyG gcn_norm (torch_geometric 2.5.2, not in the reference tree): self-loops are
 * dropped, one unit self-loop per node is implied, deg = in-degree on the target index + 1,
 * dinv = deg^-1/2.  Builds the CSR by TARGET (rowptr_t/csr_src: forward aggregation) and by
 * SOURCE (rowptr_s/csr_dst: backward), neighbour ids ascending inside each row (deterministic
 * summation order). */
/* flags: GRAPES_PREP_SRC_GROUPED — the edge list is in the order frontier_expand / slice_filter
 * emit (one contiguous segment per source, destinations ascending inside it): source degrees come
 * from the segment bounds and the by-source CSR is written directly — no same-address atomics and
 * no sorting on hub sources.  A list that is not grouped raises GRAPES_STATUS_BAD_INDEX.
 * long_items / n_long (optional, both or neither): work items for rows with more than
 * GRAPES_LONG_ROW entries.  An item is the int32 pair (row, chunk) = GRAPES_LONG_ROW consecutive
 * entries of that row; the items of one row occupy consecutive slots in chunk order.
 * long_items = int32[2][cap][2] (first half: by-target rows, second half: by-source rows,
 * cap = grapes_gcn_long_items_capacity(e)); n_long is int32[4]: [0],[1] = number of items per half,
 * [2] = number of aggregated (non-self-loop) edges, [3] reserved. */
/* head_ids / row_head (optional, both or neither): head_ids[local id] = row of the resident feature matrix (the hop's
 * batch_nodes); row_head = int32[n][12] receives one record per by-target row
 *   { len, head_ids[r], dinv[r]^2, dinv[r], (head_ids[src_j], dinv[src_j]*dinv[r]) for the first 4 entries }
 * (floats stored by bit pattern; unused entry slots = (head_ids[r], 0)) for grapes_gcn_aggregate_gather_fwd. */
#define GRAPES_PREP_SRC_GROUPED 1
#define GRAPES_PREP_PREZEROED 2   /* see grapes_gcn_prepare_zero_words */
#define GRAPES_LONG_ROW 64
size_t grapes_gcn_prepare_workspace_bytes(int32_t n_cap, int32_t e_cap);
int32_t grapes_gcn_long_items_capacity(int32_t e_cap);
/* node_map (optional): edge_src / edge_dst hold GLOBAL ids and are relabelled through it first — the TensorMap
 * lookup of main.py:195,254 (local_neighborhoods / local_edge_indices) folded into the build.
 * Graphs of at most 2048 nodes in grouped mode are built by ONE workgroup in one launch.
 * GRAPES_PREP_PREZEROED: an earlier launch of the caller (grapes_frontier_compact's zero_* arguments) has zeroed the first
 * grapes_gcn_prepare_zero_words(n) 32-bit words of `workspace` and, in grouped mode, csr_dst[0..e): the build then skips
 * its own clearing launch and applies node_map inside its per-edge kernels.
 * sync (optional, see GRAPES_SYNC_WORDS): the row-pointer scan of larger graphs (n <= 255 * 1024) takes one launch
 * instead of two. */
size_t grapes_gcn_prepare_zero_words(int32_t n);
int grapes_gcn_prepare(const int32_t* edge_src, const int32_t* edge_dst, int32_t e,
                       const int32_t* d_e, const int32_t* node_map, int32_t n, const int32_t* d_n, int32_t flags,
                       int32_t* rowptr_t, int32_t* csr_src, int32_t* rowptr_s, int32_t* csr_dst,
                       float* dinv, int32_t* long_items, int32_t* n_long, const int32_t* head_ids,
                       int32_t* row_head, void* workspace, uint64_t* sync, int32_t* status, grapes_stream_t stream);
/* grapes_gcn_prepare that ALSO touches the feature rows  prefetch_X[head_ids[r], 0:prefetch_row_floats]  (row pitch prefetch_pitch
 * floats; general path with head records) from extra workgroups of its first launch — the rows the hop's gather-SpMM
 * (grapes_gcn_aggregate_gather_fwd; reference main.py:199-204 + modules/gcn.py:32) reads next — so that they are Infinity-Cache
 * hits by then.  prefetch_X == NULL: exactly grapes_gcn_prepare.  No state is kept between calls. */
int grapes_gcn_prepare_prefetching(const int32_t* edge_src, const int32_t* edge_dst, int32_t e, const int32_t* d_e,
                                   const int32_t* node_map, int32_t n, const int32_t* d_n, int32_t flags,
                                   int32_t* rowptr_t, int32_t* csr_src, int32_t* rowptr_s, int32_t* csr_dst,
                                   float* dinv, int32_t* long_items, int32_t* n_long, const int32_t* head_ids,
                                   int32_t* row_head, void* workspace, uint64_t* sync, int32_t* status, const float* prefetch_X,
                                   int64_t prefetch_pitch, int32_t prefetch_row_floats, grapes_stream_t stream);

/* count (<= 8) small graphs over the SAME n <= 2048 nodes (the classifier's per-layer sampled subgraphs,
 * main.py:252-256), grouped edge lists, in ONE launch (one workgroup per graph).  The pointer arguments are HOST arrays
 * of device pointers; workspaces[i] as for grapes_gcn_prepare(n, e[i]). */
int grapes_gcn_prepare_small_batch(int32_t count, const int32_t* const* edge_src, const int32_t* const* edge_dst,
                                   const int32_t* e, const int32_t* const* d_e, const int32_t* node_map,
                                   int32_t n, const int32_t* d_n, int32_t* const* rowptr_t,
                                   int32_t* const* csr_src, int32_t* const* rowptr_s, int32_t* const* csr_dst,
                                   float* const* dinv, int32_t* const* long_items, int32_t* const* n_long,
                                   const int32_t* head_ids, int32_t* const* row_head, void* const* workspaces,
                                   const int32_t* const* slice_stage, const int32_t* const* d_fe, const int32_t* fe_cap,
                                   int32_t* status, grapes_stream_t stream);
/* slice_stage (optional host array; entry i may be NULL): graph i's edge list is first ASSEMBLED, by its workgroup, from the
 * stage a grapes_frontier_expand_fused(slice_stage = ...) launch left (fe_cap[i] = that launch's e_cap, d_fe[i] = its edge
 * count): edge_src[i] / edge_dst[i] (capacity e[i]) and *d_e[i] are then OUTPUTS of this call — the list and count
 * grapes_slice_filter would have produced — before they are read as the build's input. */

/* Full-graph variant (evaluation over the whole adjacency, eval.py:47-70): `rowptr` is an int32 CSR
 * by target with ascending columns and NO self-loops; only dinv and the hub-row work items are computed. */
int grapes_gcn_prepare_from_csr(const int32_t* rowptr, int32_t n, float* dinv, int32_t* items,
                                int32_t* n_items, int32_t item_cap, grapes_stream_t stream);

/* ------------------------------------------------------------------ A7: GCNConv arithmetic
 * H = X Wᵀ (GCNConv.lin, no bias) — fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32 fma chain. */
int grapes_linear_fwd(const float* x, const float* w, float* h, int32_t n, const int32_t* d_n,
                      int32_t f_in, int32_t f_out, grapes_stream_t stream);
/* H = diag(row_scale) X Wᵀ — the transform of a full-batch inference layer (modules/gcn.py:32 via eval.py:50; N1) with
 * grapes_scale_rows' pass in the GEMM's epilogue: the rows leave the launch pre-scaled by dinv, the operand
 * grapes_gcn_aggregate_fwd_prescaled reads.  Bit-identical to grapes_linear_fwd followed by grapes_scale_rows; f_out > 1. */
int grapes_linear_fwd_row_scaled(const float* x, const float* w, const float* row_scale, float* h, int32_t n,
                                 const int32_t* d_n, int32_t f_in, int32_t f_out, grapes_stream_t stream);
size_t grapes_linear_bwd_weight_workspace_bytes(int32_t n_cap, int32_t f_in, int32_t f_out);
/* dW[f_out,f_in] (+)= dHᵀ X  (split over rows, slabs reduced in fixed order: deterministic). */
int grapes_linear_bwd_weight(const float* dh, const float* x, float* dw, int32_t n,
                             const int32_t* d_n, int32_t f_in, int32_t f_out, int32_t accumulate,
                             void* workspace, grapes_stream_t stream);
/* Aggregate-first form of a GCNConv whose input needs no gradient and has F_in < F_out
 * (out = act((Â X) Wᵀ + b): same result as PyG's transform-then-aggregate up to fp32 rounding, with the
 * SpMM on the narrow side):  forward = GEMM with fused bias + ReLU epilogue. */
int grapes_linear_bias_act_fwd(const float* x, const float* w, const float* bias, int32_t relu,
                               float* out, int32_t n, const int32_t* d_n, int32_t f_in,
                               int32_t f_out, grapes_stream_t stream);
/* The same layer followed by the XW step of a 1-wide GCNConv head (modules/gcn.py:32 with out_channels = 1):
 * head_out[i] = sum_n out[i][n] * head_w[n], summed from the output tiles of the GEMM (one launch) where the bf16x3
 * kernel applies, else computed by a second launch.  The summation order is fixed but is not grapes_linear_fwd's. */
int grapes_linear_bias_act_head_fwd(const float* x, const float* w, const float* bias, int32_t relu, float* out,
                                    const float* head_w, float* head_out, int32_t n, const int32_t* d_n,
                                    int32_t f_in, int32_t f_out, grapes_stream_t stream);
/* Strided-input forms (bf16x3 kernels only; GRAPES_EINVAL where grapes_split_gemm_available() is 0): x rows are x_stride
 * floats apart (x_stride >= f_in, a multiple of 4), so a layer can read the leading f_in columns of a wider matrix that is
 * already there — at hop 0 the log-Z net's first layer (main.py:227: data.x[batch_nodes], the same rows as the sampler
 * net's input minus the indicator columns) reads the feature columns of the sampler net's aggregated input  Â [X | ind]
 * instead of aggregating the same rows again.  head_w / head_out may both be NULL.  The workspace of the dW form is
 * grapes_linear_bwd_weight_gated_workspace_bytes(n, f_in, f_out). */
int32_t grapes_split_gemm_available(int32_t n, int32_t f_in, int32_t f_out);
int grapes_linear_bias_act_head_fwd_strided(const float* x, int32_t x_stride, const float* w, const float* bias,
                                            int32_t relu, float* out, const float* head_w, float* head_out, int32_t n,
                                            const int32_t* d_n, int32_t f_in, int32_t f_out, grapes_stream_t stream);
int grapes_linear_bwd_weight_gated_strided(const float* gate, const float* x, int32_t x_stride, const float* row_scale,
                                           int32_t n, const int32_t* d_n, const float* col_vec, float* dw, float* dbias,
                                           float* dw_head, int32_t f_in, int32_t f_out, int32_t accumulate,
                                           void* workspace, grapes_stream_t stream);
/* Few-row weight gradients of SEVERAL layers with ONE slab reduction (the classifier's backward pass, main.py:267: its
 * layers all see the same ~B + hops*K rows).  grapes_linear_bwd_weight_slabs launches only the partial products of
 * dW = (dout ⊙ [gate > 0])ᵀ x (gate may be NULL) per 128 rows — slabs [ceil(n/128)][f_out * f_in] at `workspace`, and with
 * want_bias the column sums of the gated dout, [ceil(n/128)][f_out], right behind them; GRAPES_EINVAL when (n, f_in, f_out)
 * is not a shape of the few-row kernel (use grapes_linear_bwd_weight / _gated then).  grapes_slab_reduce_sets then sums up
 * to 8 such sets over the same n in slab order: outs[q][i] (+)= sum_z slabs[q][z * counts[q] + i]. */
size_t grapes_linear_bwd_weight_slabs_bytes(int32_t n, int32_t f_in, int32_t f_out);
int grapes_linear_bwd_weight_slabs(const float* dout, const float* gate, const float* x, int32_t n, const int32_t* d_n,
                                   int32_t f_in, int32_t f_out, int32_t want_bias, void* workspace, grapes_stream_t stream);
/* ... and the same slabs launch with the layer's input gradient dx = dout w  (modules/gcn.py:32,36 backward: the weight
 * and input gradients of one GCNConv's linear map read the same dout and do not depend on each other) as a second problem
 * of the SAME launch: workgroups [0, A) run the slab products, the rest the few-row dx GEMM.  w [f_out, f_in], dx [n, f_in].
 * GRAPES_EINVAL when either half's shape is not one of its few-row kernel (call the two entry points separately then). */
int grapes_linear_bwd_weight_slabs_and_input(const float* dout, const float* gate, const float* x, const float* w, float* dx,
                                             int32_t n, const int32_t* d_n, int32_t f_in, int32_t f_out, int32_t want_bias,
                                             void* workspace, grapes_stream_t stream);
/* grapes_linear_bwd_weight_slabs for 1..4 layers over the SAME n rows (one d_n) as ONE launch, each layer's workgroups side by
 * side: problem q = (dout[q], gate[q] or NULL, x[q], f_in[q], f_out[q], want_bias[q], workspace[q]) exactly as that entry point
 * takes them; the same slabs.  GRAPES_EINVAL (nothing launched) when a shape is not one of the few-row kernel. */
int grapes_linear_bwd_weight_slabs_multi(int32_t count, const float* const* dout, const float* const* gate, const float* const* x,
                                         int32_t n, const int32_t* d_n, const int32_t* f_in, const int32_t* f_out,
                                         const int32_t* want_bias, void* const* workspace, grapes_stream_t stream);
int grapes_slab_reduce_sets(int32_t nsets, const float* const* slabs, float* const* outs, const int64_t* counts, int32_t n,
                            const int32_t* d_n, int32_t accumulate, grapes_stream_t stream);
/* Gate-word forms of  layer -> ReLU -> 1-wide head  (reference modules/gcn.py:31-36 with hidden_dims = [H, 1]: the sampler
 * net main.py:112-113,210 and the log-Z net main.py:114,227), for callers whose only use of the hidden activations is that
 * head: the forward pass writes head_out [n] and gate_bits [n][f_out / 32] (bit 16 h + 4 q + u of word [r][c / 32] is
 * act[r][32 (c / 32) + 8 q + 4 h + u] > 0) INSTEAD of the n x f_out activations, and the backward pass forms
 *     dW1 (+)= col_vec ⊙ S,  db1 (+)= col_vec ⊙ T,  dW2 (+)= rowwise <S, w1> + b1 ⊙ T,
 *     S[m][:] = sum_r [bit(r, m)] row_scale[r] x[r][:],   T[m] = sum_r [bit(r, m)] row_scale[r]
 * over up to four row sets that share the weights (what torch autograd computes for d(head)/d(W1, b1, W2) given
 * d head_out = row_scale and W2 = col_vec; w1 / b1 are the layer's current parameters, [f_out][f_in] dense and [f_out]).
 * bf16x3 kernels only: GRAPES_EINVAL where grapes_split_gemm_available(n, f_in, f_out) is 0.  x rows may be strided
 * (x_stride[h] floats, 0 / NULL = dense).  Workspace: grapes_linear_bwd_weight_gated_workspace_bytes(1, f_in, f_out).
 * Range of the bf16x3 weight gradient (these entries and the rank-1 gated ones on the split kernel; tests/
 * test_split_dw_accuracy_gpu.py): each product v = row_scale[r] x[r][k] is formed in fp32 and split into three bf16 terms.
 *   - |v| >= 3.3962e38 (finite in fp32) rounds to bf16 inf: the lower terms become -inf and NaN, and column k of dW1 is NaN
 *     for EVERY unit (a 0 of the mask times inf is NaN too), with dW2 of the gate-word form (derived from dW1's sums);
 *     db1 and the other columns are unaffected.  The fp32 kernels give a finite answer there.  Not guarded: activations
 *     that large mean training has already diverged.
 *   - |v| below about 2^-109 (1.6e-33) is held by the three terms only to bf16's smallest subnormal step, 2^-133 (an error
 *     of at most 2^-134 per product instead of 2^-24 |v|); the matrix pipe keeps bf16 subnormals. */
int grapes_linear_relu_head_fwd_bits(const float* x, int32_t x_stride, const float* w, const float* bias,
                                     const float* head_w, uint32_t* gate_bits, float* head_out, int32_t n,
                                     const int32_t* d_n, int32_t f_in, int32_t f_out, grapes_stream_t stream);
/* TWO such layers over the same n rows in one launch (same f_out, f_in / f_in_b in the same multiple of 16): the sampler net's
 * and the log-Z net's first layers at hop 0 (main.py:199-210 and 223-228 read the same batch rows) — each alone leaves most of
 * its launch to its prologue; side by side on half the workgroups each the pair costs one.  Outputs bit-identical to two
 * grapes_linear_relu_head_fwd_bits calls.  GRAPES_EINVAL where either shape is outside the kernel (call them separately). */
int grapes_linear_relu_head_fwd_bits_pair(const float* x, int32_t x_stride, const float* w, const float* bias,
                                          const float* head_w, uint32_t* gate_bits, float* head_out,
                                          const float* x_b, int32_t x_stride_b, const float* w_b, const float* bias_b,
                                          const float* head_w_b, uint32_t* gate_bits_b, float* head_out_b, int32_t f_in_b,
                                          int32_t n, const int32_t* d_n, int32_t f_in, int32_t f_out, grapes_stream_t stream);
/* ... plus ONE more row set that belongs to a different layer of the same f_out (entry nseg of the operand arrays, which then
 * hold nseg + 1 <= 4 entries; its own f_in_b <= f_in, head weight, parameters and gradient buffers): the log-Z net's first
 * layer beside the sampler net's (main.py:287 backpropagates through both) in one GEMM launch on disjoint workgroups and one
 * slab reduction.  Same workspace. */
/* The two entries above with dw in the PARAMETER's layout: dw is [f_out, dw_cols], f_in - 3 <= dw_cols <= f_in, when f_in is the
 * layer's input width rounded up to a multiple of 4 (ogbn-arxiv: 128 features + 3 indicators = 131 -> 132) and x / w1 carry the
 * zero pad column — the slab sum writes the parameter's gradient itself instead of a padded buffer that a strided copy_ then
 * publishes (modules/gcn.py:32 backward).  dw_cols = 0 means f_in.  A row set is addressed with 32-bit byte offsets from its base:
 * GRAPES_EINVAL when n_cap[h] * x_stride[h] * 4 >= 2^32 (a 4 GiB operand; the hop capacities of BASELINE's configs are 2 - 3 orders
 * of magnitude below). */
int grapes_linear_bwd_weight_bits_multi_cols(int32_t nseg, const uint32_t* const* gate_bits, const float* const* x,
                                             const int32_t* x_stride, const float* const* row_scale,
                                             const int32_t* const* d_n, const int32_t* n_cap, const float* col_vec,
                                             const float* w1, const float* b1, float* dw, int32_t dw_cols, float* dbias,
                                             float* dw_head, int32_t f_in, int32_t f_out, int32_t accumulate, void* workspace,
                                             grapes_stream_t stream);
int grapes_linear_bwd_weight_bits_pair_cols(int32_t nseg, const uint32_t* const* gate_bits, const float* const* x,
                                            const int32_t* x_stride, const float* const* row_scale,
                                            const int32_t* const* d_n, const int32_t* n_cap, const float* col_vec,
                                            const float* w1, const float* b1, float* dw, int32_t dw_cols, float* dbias,
                                            float* dw_head, int32_t f_in, const float* col_vec_b, const float* w1_b,
                                            const float* b1_b, float* dw_b, float* dbias_b, float* dw_head_b, int32_t f_in_b,
                                            int32_t f_out, int32_t accumulate, void* workspace, grapes_stream_t stream);
/* backward of the same layer in ONE split-K GEMM: dW (+)= (dout ⊙ [gate > 0])ᵀ x,
 * dbias (+)= column sums of the gated dout (gate = the layer's ReLU output, or NULL; dbias may be NULL). */
size_t grapes_linear_bwd_weight_gated_workspace_bytes(int32_t n_cap, int32_t f_in, int32_t f_out);
/* row_scale/col_vec (both or neither): dout is the rank-1 matrix row_scale[r]·col_vec[m] (the gradient a
 * 1-wide head sends back, dh2 ⊗ w2) and is formed while loading — `dout` itself is then ignored.
 * dw_head (optional, rank-1 mode only): dw_head[m] (+)= Σ_r row_scale[r]·gate[r][m] = the head's own weight gradient
 * dh2ᵀ·act (gate = the ReLU output act >= 0), summed while the gate tiles stream through the same GEMM. */
int grapes_linear_bwd_weight_gated(const float* dout, const float* gate, const float* x, float* dw,
                                   float* dbias, int32_t n, const int32_t* d_n, int32_t f_in,
                                   int32_t f_out, int32_t accumulate, const float* row_scale,
                                   const float* col_vec, float* dw_head, void* workspace, grapes_stream_t stream);
/* The rank-1 form for up to four hops that share the weights, in ONE split-K launch + ONE slab reduction: hop h
 * contributes gate[h], x[h], row_scale[h] with *d_n[h] live rows of n_cap[h] (host arrays of device pointers).
 * Workspace: grapes_linear_bwd_weight_gated_workspace_bytes(1, f_in, f_out) suffices. */
int grapes_linear_bwd_weight_gated_multi(int32_t nseg, const float* const* gate, const float* const* x,
                                         const float* const* row_scale, const int32_t* const* d_n,
                                         const int32_t* n_cap, const float* col_vec, float* dw, float* dbias,
                                         float* dw_head, int32_t f_in, int32_t f_out, int32_t accumulate,
                                         void* workspace, grapes_stream_t stream);
#ifdef GRAPES_DIAG   /* the diagnostic build only (make -C grapes_amd/csrc diag -> libgrapes_hip_diag.so): not a product surface */
/* diagnosis only: forward GEMM with parts switched off (dbg bits: 1 no stores, 2 no operand reloads, 4 no MFMAs) */
int grapes_debug_gemm_fwd(const float* x, const float* w, float* out, int32_t n, int32_t f_in,
                          int32_t f_out, int32_t dbg, grapes_stream_t stream);
/* measurement only (profiles/gather_bound_probe.py): stripped-down gathers over gcn_prepare's head records, pricing the
 * ingredients of grapes_gcn_aggregate_gather_fwd one at a time; results are NOT the product's (rows of <= 1 entry only).
 * variant bits: 1 five row loads (else two), 2 resident looping workgroups (grid_cap), 4 a row per wavefront. */
int grapes_debug_gather_probe(const float* X, int32_t x_stride, const int32_t* row_head, float* out, int32_t n,
                              int32_t f_out, int32_t variant, int32_t grid_cap, grapes_stream_t stream);
/* measurement only (profiles/tsplit_ablation.py): the gathered-operand bf16x3 GEMMs with parts switched off */
int grapes_debug_tsplit_fwd(const float* X, int32_t F, int32_t x_stride, const int32_t* ids, const void* w_image, float* h,
                            int32_t n, int32_t f_out, int32_t dbg, grapes_stream_t stream);
int grapes_debug_tsplit_dw(const float* dh, const float* X, int32_t F, int32_t x_stride, const int32_t* ids, int32_t n,
                           int32_t f_out, void* workspace, int32_t dbg, grapes_stream_t stream);
#endif
/* dX = dH W */
int grapes_linear_bwd_input(const float* dh, const float* w, float* dx, int32_t n,
                            const int32_t* d_n, int32_t f_in, int32_t f_out,
                            grapes_stream_t stream);
/* out[c] = Σ_{r in row c} (dinv[r]·dinv[c])·H[r] + dinv[c]²·H[c] + bias ; optional ReLU
 * (modules/gcn.py:32).  Gather-SpMM over the by-target CSR: one wavefront per destination row,
 * 16 B per lane coalesced row loads, 8 rows in flight; rows longer than GRAPES_LONG_ROW are
 * processed item by item (one workgroup each) into `workspace` and combined in chunk order.
 * long_items / d_n_items: one half of gcn_prepare's item table and its count (or NULL: every row
 * is handled by a single wavefront).  bias may be NULL. */
size_t grapes_gcn_aggregate_workspace_bytes(int32_t item_cap, int32_t f);
/* two 1-wide vectors over the same graph in one launch: out_a = Â h_a + bias_a, out_b = Â h_b + bias_b (the sampler net's
 * and the log-Z net's heads at hop 0: modules/gcn.py:36 on the [H, 1] layers of main.py:210,227); biases may be NULL */
int grapes_gcn_aggregate_narrow_pair(const float* h_a, const float* h_b, const int32_t* rowptr_t, const int32_t* csr_src,
                                     const float* dinv, const float* bias_a, const float* bias_b, float* out_a, float* out_b,
                                     int32_t n, const int32_t* d_n, grapes_stream_t stream);
int grapes_gcn_aggregate_fwd(const float* h, const int32_t* rowptr_t, const int32_t* csr_src,
                             const float* dinv, const float* bias, float* out, int32_t n,
                             const int32_t* d_n, int32_t f, int32_t relu,
                             const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap,
                             void* workspace, grapes_stream_t stream);
/* grapes_gcn_aggregate_fwd that also returns head_out[r] = out[r] . head_w [f] — the X W step of a 1-wide layer that follows
 * (modules/gcn.py:36 applied to main.py:210's [H, 1] layer), taken from the row while it is in registers instead of a launch
 * that reads the n x f activations back.  f > 16, f % 4 == 0, 16-byte aligned rows; every row is walked by its own wavefront.
 * gate_bits (optional; relu != 0, f <= 256): uint32[n][8], the ReLU gates of out — element e of row r is bit e % 32 of
 * gate_bits[8 r + e / 32] — for grapes_gcn_aggregate_bwd_rank1_bits. */
int grapes_gcn_aggregate_fwd_head(const float* h, const int32_t* rowptr_t, const int32_t* csr_src, const float* dinv,
                                  const float* bias, float* out, int32_t n, const int32_t* d_n, int32_t f, int32_t relu,
                                  const float* head_w, float* head_out, uint32_t* gate_bits, grapes_stream_t stream);
/* grapes_gcn_aggregate_fwd (no ReLU, no long-row items) and grapes_step_losses on its output `out` = the logits [n, f] in ONE
 * launch (main.py:256-282: the classifier's last GCNConv aggregation, loss_c, d loss_c / d logits, the log-Z mean, the GFlowNet
 * loss): the wavefront that has formed a row runs its loss or zero-fills its gradient row, one more workgroup forms the log-Z
 * sum, the last workgroup to finish sums the row losses.  out, dlogits, loss_out and out4 are bit-identical to the two calls'.
 * Covers the shapes grapes_gcn_aggregate_fwd walks with one float per lane: grapes_gcn_aggregate_fwd_losses_available(h, bias,
 * out, n, f) != 0 (f > 16, f % 4 != 0 or a base that is not 16-byte aligned, n <= 65536); GRAPES_EINVAL otherwise.  Arguments
 * as those two entry points' (workspace: grapes_step_losses_workspace_bytes(B), 8-byte aligned; d_ticket: one zero word, left
 * zero; no loss_extra).  Distinct target ids must map to distinct rows. */
int grapes_gcn_aggregate_fwd_losses_available(const float* h, const float* bias, const float* out, int32_t n, int32_t f);
int grapes_gcn_aggregate_fwd_losses(const float* h, const int32_t* rowptr_t, const int32_t* csr_src, const float* dinv,
                                    const float* bias, float* out, int32_t n, const int32_t* d_n, int32_t f,
                                    const int32_t* node_map, const int32_t* target_ids, const int64_t* labels,
                                    const float* labels_f, int32_t B, float* dlogits, float* loss_out, const float* z_out,
                                    int32_t nz, const int32_t* d_nz, float log_z_init, const float* hop_stats, int32_t hops,
                                    int32_t stats_stride, float loss_coef, int32_t reinforce, float* out4, void* workspace,
                                    uint32_t* d_ticket, grapes_stream_t stream);
/* The same two aggregations (head_w NULL: grapes_gcn_aggregate_fwd's, else grapes_gcn_aggregate_fwd_head's) driven by the graph
 * build's per-row head records taken over LOCAL ids (row_head of grapes_gcn_prepare* with head_ids = 0, 1, ..., n - 1): one
 * dependent round trip per row instead of three, pairs of rows per resident wavefront (modules/gcn.py:32,36 on Reddit-shaped
 * first layers: f = hidden_dim <= 256, f % 4 == 0).  Results are bit-identical to those entry points'. */
int grapes_gcn_aggregate_fwd_rec(const float* h, const int32_t* row_head, const int32_t* rowptr_t, const int32_t* csr_src,
                                 const float* dinv, const float* bias, float* out, int32_t n, const int32_t* d_n, int32_t f,
                                 int32_t relu, const float* head_w, float* head_out, uint32_t* gate_bits, grapes_stream_t stream);
/* Full-batch inference form (eval.py:47-70; N1): the rows of `hs` are PRE-SCALED by their own dinv (grapes_scale_rows), so an
 * aggregated entry needs no gather of dinv[source]:  out[c] = dinv[c] (sum_s hs[s] + hs[c]) + bias (+ReLU).  Same graph
 * arguments as grapes_gcn_aggregate_fwd; f > 16 and a multiple of 4, 16-byte aligned rows.  Rounding differs from the
 * w = dinv[s] dinv[c] form by an ulp or two.  Replaces: the same GCNConv call sites, modules/gcn.py:32,36 via eval.py:50. */
int grapes_gcn_aggregate_fwd_prescaled(const float* hs, const int32_t* rowptr_t, const int32_t* csr_src,
                                       const float* dinv, const float* bias, float* out, int32_t n,
                                       const int32_t* d_n, int32_t f, int32_t relu, const int32_t* long_items,
                                       const int32_t* d_n_items, int32_t item_cap, void* workspace,
                                       grapes_stream_t stream);
/* Backward of  GCNConv (transform first: out = Â (X Wᵀ) + b) -> ReLU -> GCNConv to ONE output  (the sampler / log-Z nets of
 * main.py:112-114 when F_in >= hidden: Reddit, Cora; call sites modules/gcn.py:32,36) given dh2 = Âᵀ d(head output) [n]:
 *   dw2[m] (+)= sum_r dh2[r] act[r][m]       db1[m] (+)= sum_r [act[r][m] > 0] dh2[r] w2[m]
 *   dh[s][:] = sum_{r in out(s)} w_sr dpre[r] + w_ss dpre[s]   with   dpre[r][m] = [act[r][m] > 0] dh2[r] w2[m]
 * — what outer product + ReLU-mask / bias-gradient pass + grapes_gcn_aggregate_bwd computed through two n x f temporaries,
 * with the same products and summation orders (bit-identical results).  act: the layer's ReLU output [n, f]; w2 [f]; f > 16,
 * f % 4 == 0.  by-source CSR and work items as grapes_gcn_aggregate_bwd.  dw2 / db1 may be NULL. */
size_t grapes_gcn_aggregate_bwd_rank1_workspace_bytes(int32_t item_cap, int32_t f);
int grapes_gcn_aggregate_bwd_rank1(const float* act, const float* dh2, const float* w2, const int32_t* rowptr_s,
                                   const int32_t* csr_dst, const float* dinv, float* dh, float* dw2, float* db1,
                                   int32_t accumulate, int32_t n, const int32_t* d_n, int32_t f,
                                   const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap,
                                   void* workspace, grapes_stream_t stream);
/* ... with the gates of the aggregated matrix read from gate_bits (32 bytes per row, written by grapes_gcn_aggregate_fwd_head)
 * instead of from the rows of act: the same products in the same order, bit-identical dh; act still feeds the two column sums
 * (dw2, db1).  f <= 256. */
int grapes_gcn_aggregate_bwd_rank1_bits(const float* act, const uint32_t* gate_bits, const float* dh2, const float* w2,
                                        const int32_t* rowptr_s, const int32_t* csr_dst, const float* dinv, float* dh,
                                        float* dw2, float* db1, int32_t accumulate, int32_t n, const int32_t* d_n,
                                        int32_t f, const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap,
                                        void* workspace, grapes_stream_t stream);
/* grapes_gcn_aggregate_bwd_rank1_bits for up to three INDEPENDENT problems of one width f in the same five launches (the hops of
 * the sampler net and the log-Z net at main.py:287: each launch of a chain is a few dependent round trips long whatever it moves).
 * Arrays are HOST arrays of `count` entries; workspace[q]: grapes_gcn_aggregate_bwd_rank1_workspace_bytes(item_cap[q], f) each.
 * Results equal, bit for bit, the calls one after the other in index order: problems that name the same dw2 / db1 are added in
 * that order, each with its own accumulate flag (dw2[q] and db1[q] are both given or both NULL). */
int grapes_gcn_aggregate_bwd_rank1_bits_multi(int32_t count, const float* const* act, const uint32_t* const* gate_bits,
                                              const float* const* dh2, const float* const* w2, const int32_t* const* rowptr_s,
                                              const int32_t* const* csr_dst, const float* const* dinv, float* const* dh,
                                              float* const* dw2, float* const* db1, const int32_t* accumulate, const int32_t* n,
                                              const int32_t* const* d_n, int32_t f, const int32_t* const* long_items,
                                              const int32_t* const* d_n_items, const int32_t* item_cap, void* const* workspace,
                                              grapes_stream_t stream);
/* hs[r, :] = dinv[r] * h[r, :] (hs may alias h); f a multiple of 4. */
int grapes_scale_rows(const float* h, const float* dinv, float* hs, int64_t n, int32_t f, grapes_stream_t stream);
/* Â · [X | indicators] straight from the resident feature matrix (fuses the feature gather of
 * main.py:199-204 into the aggregation): out[c] = Σ_s w_sc feat(ids[s]) + dinv[c]² feat(ids[c]),
 * feat(v) = [X[v,0:F], indicator bits of v, zero padding];  out is [n, Kp], Kp = F + num_ind rounded up to a multiple of 4
 * (reference widths: F + hops + 1 = 131 on ogbn-arxiv, 605 on Reddit, main.py:111-113).  x_stride = floats between rows of X,
 * a multiple of 4 (0 = F); when F is not a multiple of 4 the resident matrix is a copy padded to x_stride with ZERO columns. */
int grapes_gcn_aggregate_gather_fwd(const float* X, int32_t F, int32_t x_stride, const int32_t* ids,
                                    const uint32_t* ind_code, uint32_t epoch, const uint32_t* d_epoch,
                                    int32_t num_ind, const int32_t* rowptr_t, const int32_t* csr_src,
                                    const float* dinv, const int32_t* row_head, float* out, int32_t n,
                                    const int32_t* d_n, grapes_stream_t stream);
size_t grapes_gcn_aggregate_bwd_workspace_bytes(int32_t item_cap, int32_t f);
/* dpre = dout ⊙ (out > 0) if relu_out != NULL else dout;  dbias (+)= Σ_c dpre[c];
 * dh[r] = Σ_{c in row r of by-source CSR} (dinv[c]·dinv[r])·dpre[c] + dinv[r]²·dpre[r].
 * dpre is materialised in `dpre_buf` [n,f] (may alias dout when the caller owns dout).
 * d_ticket (optional): GRAPES_COLSUM_TICKETS zero words, left zero — with n <= 8192 the ReLU mask + bias gradient pass
 * is then one launch (last-workgroup combine in a fixed order) instead of two; with f <= 256 and no long_items the WHOLE
 * operation is one launch: the mask is applied to the gathered rows on the fly and dpre_buf is NOT written. */
#define GRAPES_COLSUM_TICKETS 16
int grapes_gcn_aggregate_bwd(const float* dout, const float* relu_out, const int32_t* rowptr_s,
                             const int32_t* csr_dst, const float* dinv, float* dpre_buf,
                             float* dh, float* dbias, int32_t accumulate_bias, int32_t n,
                             const int32_t* d_n, int32_t f, const int32_t* long_items,
                             const int32_t* d_n_items, int32_t item_cap, void* workspace,
                             uint32_t* d_ticket, grapes_stream_t stream);
/* The few-row launch of grapes_gcn_aggregate_bwd AND grapes_linear_bwd_input on its output as ONE launch: dt [n, f] = what
 * grapes_gcn_aggregate_bwd writes to dh, dx [n, f_in] = dt w (w [f, f_in]), dbias (+)= the gated column sums (NULL: none; else
 * workspace of grapes_gcn_aggregate_bwd_workspace_bytes(0, f) and d_ticket as above).  A workgroup forms 32 rows of dt and runs
 * the 32 x 64 tile of the few-row dx GEMM on them: every value is bit for bit the two calls'.  _available: 0 < n <= 2048 (graphs small enough that no row is split into long-row items),
 * 16 < f <= 256 (f <= 64 unless f % 4 == 0 with 16-byte aligned dout, relu_out and dt); rows of any length are walked by one
 * wavefront (no long-row items).  Recorded while a rider recording is open, like grapes_gcn_aggregate_bwd, and carried by the same
 * launches (grapes_sampler_head_bwd_multi_phase). */
int grapes_gcn_aggregate_bwd_input_available(const float* dout, const float* relu_out, const float* dt, int32_t n, int32_t f,
                                             int32_t f_in);
int grapes_gcn_aggregate_bwd_input(const float* dout, const float* relu_out, const int32_t* rowptr_s, const int32_t* csr_dst,
                                   const float* dinv, const float* w, float* dt, float* dx, float* dbias,
                                   int32_t accumulate_bias, int32_t n, const int32_t* d_n, int32_t f, int32_t f_in,
                                   void* workspace, uint32_t* d_ticket, grapes_stream_t stream);

/* ------------------------------------------------------------------ GATConv aggregation (csrc/gat_kernels.hip)
 * modules/gcn.py:45-72: GAT stacks GATConv(in_channels, out_channels) layers with PyG's defaults (torch_geometric 2.5.2, not in
 * the reference tree: heads = 1, negative_slope = 0.2, add_self_loops, no attention dropout).  With H = X W^T (grapes_linear_fwd):
 *   e_ij = LeakyReLU(s_src[j] + s_dst[i], 0.2)   alpha_ij = softmax over the edges j -> i   out_i = sum_j alpha_ij H_j + bias
 * over the edge set of grapes_gcn_prepare: stored self-loops dropped, one unit self-loop per node implied, duplicates kept.
 * Widths: any f <= 256; f % 4 == 0 with 16-byte aligned rows up to 1024.  Every sum has a fixed order (no floating-point
 * atomics): results are bit-identical from run to run.  status: GRAPES_STATUS_BAD_INDEX when a CSR entry is outside [0, n)
 * (the entry is dropped). */
/* modules/gcn.py:66,70 (the attention scores inside GATConv): s_src[r] = H[r] . a_src, s_dst[r] = H[r] . a_dst  (a_* [f]). */
int grapes_gat_scores(const float* h, const float* a_src, const float* a_dst, float* s_src, float* s_dst, int32_t n,
                      const int32_t* d_n, int32_t f, grapes_stream_t stream);
/* modules/gcn.py:66-67,70 (GATConv's propagate, + the ReLU of gcn.py:67 when relu != 0): edge softmax and weighted gather in
 * ONE pass over the by-target CSR (online softmax: running maximum, rescaled sum and accumulator in registers), bias and ReLU in
 * the epilogue.  row_ms [n][2] receives (row maximum, log of the softmax sum) for the backward.  long_items / d_n_items /
 * item_cap / workspace as grapes_gcn_aggregate_fwd (by-target half of gcn_prepare's item table; NULL: every row by one group of
 * lanes): rows longer than GRAPES_LONG_ROW are cut into items whose (max, sum, accumulator) are merged in chunk order.
 * workspace: grapes_gat_aggregate_workspace_bytes(item_cap, f), 16-byte aligned.  bias may be NULL. */
size_t grapes_gat_aggregate_workspace_bytes(int32_t item_cap, int32_t f);
int grapes_gat_aggregate_fwd(const float* h, const float* s_src, const float* s_dst, const int32_t* rowptr_t,
                             const int32_t* csr_src, const float* bias, float* out, float* row_ms, int32_t n,
                             const int32_t* d_n, int32_t f, int32_t relu, const int32_t* long_items,
                             const int32_t* d_n_items, int32_t item_cap, void* workspace, int32_t* status,
                             grapes_stream_t stream);
/* Backward of the above (autograd through modules/gcn.py:66-67,70).  With G = dout (gated by out > 0 when relu != 0),
 * c_i = G_i . (out_i - bias), slope_ij = 1 if s_src[j] + s_dst[i] > 0 else 0.2 and g_ij = alpha_ij (G_i . H_j - c_i) slope_ij:
 *   ds_src[j] = sum_i g_ij   ds_dst[i] = sum_j g_ij   dh[j] = sum_i alpha_ij G_i + ds_src[j] a_src + ds_dst[j] a_dst
 *   da_src = sum_j ds_src[j] H_j   da_dst = sum_i ds_dst[i] H_i   dbias = sum_i G_i        (each may be NULL)
 * alpha is recomputed from the scores and row_ms in a pass over the by-target CSR (ds_dst) and one over the by-source CSR
 * (dh, ds_src); the three column sums are per-workgroup partials added in a fixed tree.  out: the forward's output.
 * items_t / items_s: the two halves of gcn_prepare's item table with their counts (NULL: no row splitting).
 * workspace: grapes_gat_aggregate_bwd_workspace_bytes(n, item_cap, f), 16-byte aligned. */
size_t grapes_gat_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f);
int grapes_gat_aggregate_bwd(const float* dout, const float* out, const float* bias, int32_t relu, const float* h,
                             const float* s_src, const float* s_dst, const float* row_ms, const float* a_src,
                             const float* a_dst, const int32_t* rowptr_t, const int32_t* csr_src,
                             const int32_t* rowptr_s, const int32_t* csr_dst, float* dh, float* da_src, float* da_dst,
                             float* dbias, int32_t n, const int32_t* d_n, int32_t f, const int32_t* items_t,
                             const int32_t* d_n_items_t, const int32_t* items_s, const int32_t* d_n_items_s,
                             int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ GATv2Conv aggregation (csrc/gatv2_kernels.hip)
 * PyG's GATv2Conv (torch_geometric 2.5.2, not in the reference tree) with `heads` heads of `c` channels, f = heads c, LeakyReLU slope
 * negative_slope in [0, 1), add_self_loops, no attention dropout.  With x_l = lin_l(x), x_r = lin_r(x) (grapes_linear_fwd), [n, f]
 * viewed as [n, heads, c], and att [heads, c]:
 *   e_ij[h] = sum_c att[h, c] LeakyReLU(x_l[j, h, c] + x_r[i, h, c])   alpha_ij[h] = softmax over the edges j -> i, per head
 *   agg_i[h] = sum_j alpha_ij[h] x_l[j, h]   out_i = concat_h agg_i[h] + bias (concat != 0, [n, f]) or mean_h agg_i[h] + bias ([n, c])
 * over the edge set of grapes_gcn_prepare: stored self-loops dropped, one unit self-loop per node implied, duplicates kept.
 * Shapes: 1 <= heads <= 16; c % 4 == 0 with 16-byte aligned rows up to f = 1024, any c up to f = 256; GRAPES_EINVAL / GRAPES_EALIGN
 * otherwise.  Every sum has a fixed order (no floating-point atomics): results are bit-identical from run to run.  status:
 * GRAPES_STATUS_BAD_INDEX when a CSR entry is outside [0, n) (the entry is dropped). */
/* GATv2Conv.propagate (+ a ReLU on the result when relu != 0): the per-edge score, one online softmax per head and the weighted
 * gather in ONE pass over the by-target CSR, every row x_l[j] loaded once per edge; 1 / sum, head concat or mean, bias and ReLU
 * follow.  row_ms [n][heads][2] receives (maximum, log of the softmax sum) per head for the backward; agg [n][f] receives the
 * per-head aggregate before the mean and the bias when concat == 0 (NULL otherwise: it is out - bias).  long_items / d_n_items /
 * item_cap / workspace as grapes_gat_aggregate_fwd: rows longer than GRAPES_LONG_ROW are cut into items whose per-head (max, sum)
 * and accumulators are merged in chunk order.  workspace: grapes_gatv2_aggregate_workspace_bytes(item_cap, f, heads), 16-byte
 * aligned.  bias may be NULL. */
size_t grapes_gatv2_aggregate_workspace_bytes(int32_t item_cap, int32_t f, int32_t heads);
int grapes_gatv2_aggregate_fwd(const float* x_l, const float* x_r, const float* att, const int32_t* rowptr_t,
                               const int32_t* csr_src, const float* bias, float* out, float* agg, float* row_ms, int32_t n,
                               const int32_t* d_n, int32_t heads, int32_t c, int32_t concat, float negative_slope, int32_t relu,
                               const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap, void* workspace,
                               int32_t* status, grapes_stream_t stream);
/* Backward of the above (autograd through GATv2Conv.propagate).  With G = dout gated by out > 0 when relu != 0, viewed per head
 * (G / heads for every head when concat == 0), z_ij = x_l[j] + x_r[i], c[i, h] = G[i, h] . agg_i[h],
 * de_ij[h] = alpha_ij[h] (G[i, h] . x_l[j, h] - c[i, h]) and dz_ij[h, c] = de_ij[h] att[h, c] (z_ij > 0 ? 1 : negative_slope):
 *   dx_l[j] = sum_i alpha_ij G[i] + dz_ij   dx_r[i] = sum_j dz_ij   datt[h, c] = sum_ij de_ij[h] LeakyReLU(z_ij[h, c])
 *   dbias = sum_i dout_i (gated; [f] or [c])                                               (datt and dbias may be NULL)
 * Nothing is kept per edge: a pass over the by-target CSR (dx_r, datt) and one over the by-source CSR (dx_l) each recompute z, e
 * and alpha from x_l, x_r and row_ms; datt and dbias are per-workgroup partials added in a fixed tree.  out / agg: the forward's.
 * items_t / items_s: the two halves of gcn_prepare's item table with their counts (NULL: no row splitting).
 * workspace: grapes_gatv2_aggregate_bwd_workspace_bytes(n, item_cap, f, heads), 16-byte aligned. */
size_t grapes_gatv2_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f, int32_t heads);
int grapes_gatv2_aggregate_bwd(const float* dout, const float* out, const float* agg, const float* bias, int32_t relu,
                               const float* x_l, const float* x_r, const float* att, const float* row_ms,
                               const int32_t* rowptr_t, const int32_t* csr_src, const int32_t* rowptr_s, const int32_t* csr_dst,
                               float* dx_l, float* dx_r, float* datt, float* dbias, int32_t n, const int32_t* d_n, int32_t heads,
                               int32_t c, int32_t concat, float negative_slope, const int32_t* items_t,
                               const int32_t* d_n_items_t, const int32_t* items_s, const int32_t* d_n_items_s, int32_t item_cap,
                               void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ GCN2Conv / GCNII (csrc/gcn2_kernels.hip)
 * modules/gcn.py:76-117: GCN2 stacks GCN2Conv(channels, alpha, theta, layer, shared_weights, normalize=False) layers
 * (torch_geometric 2.5.2, not in the reference tree).  normalize=False: no gcn_norm and no added loop; with
 *   P_i = sum over the stored edges (j -> i) of x_j   (every occurrence counts: duplicates by multiplicity, a stored (i, i) like
 *   any edge, an isolated row gives 0),   S = (1 - alpha) P + alpha x0,   beta = log(theta / layer + 1)
 * the layer is  out = (1 - beta) S + beta S W1  (shared weights) or
 *   out = (1 - beta) S + beta ((1 - alpha) P W1 + alpha x0 W2)  (shared_weights=False), W1 / W2 [c][c] applied untransposed.
 * The edge set is grapes_gcn_prepare's, which drops stored self-loops: they come back as loops[i] x_i.  Widths: any f <= 1024
 * (float4 columns when f % 4 == 0 and the rows are 16-byte aligned, scalar columns otherwise).  Every sum has a fixed order (no
 * floating-point atomics): results are bit-identical from run to run.  status: GRAPES_STATUS_BAD_INDEX when a CSR entry is
 * outside [0, n) (the entry is dropped).  The products with W1 / W2 are grapes_linear_bwd_input (S W), grapes_linear_fwd (G W^T)
 * and grapes_linear_bwd_weight (S^T G): the square weights are read as stored, no transposed copy. */
/* loops[i] = number of stored edges (i, i), i < n, from the edge list grapes_gcn_prepare takes (same d_e / node_map / d_n). */
int grapes_gcn2_loop_counts(const int32_t* edge_src, const int32_t* edge_dst, int32_t e, const int32_t* d_e,
                            const int32_t* node_map, int32_t n, const int32_t* d_n, int32_t* loops, grapes_stream_t stream);
/* The same from a CSR with 64-bit row pointers (graph.DeviceGraph): loops[i] = number of entries of row i equal to i. */
int grapes_gcn2_loop_counts_csr(const int64_t* rowptr, const int32_t* col, int32_t n, int32_t* loops, grapes_stream_t stream);
/* modules/gcn.py:109,113 (GCN2Conv's propagate and its initial residual):
 *   s_out[i] = (1 - alpha) (sum_{j in row i of the by-target CSR} x[j] + loops[i] x[i]) + alpha x0[i]
 *   p_out[i] = the first term alone (optional: what W1 multiplies when shared_weights=False)
 * in ONE pass: a group of lanes per row, the sum in registers.  loops may be NULL (no stored loops).  long_items / d_n_items /
 * item_cap / workspace as grapes_gcn_aggregate_fwd (NULL: every row by one group): rows longer than GRAPES_LONG_ROW are cut into
 * items whose partial sums are merged in chunk order.  workspace: grapes_gcn2_propagate_workspace_bytes(n, item_cap, f),
 * 16-byte aligned.  s_out / p_out must not alias x or x0 (x and x0 may be the same matrix). */
size_t grapes_gcn2_propagate_workspace_bytes(int32_t n, int32_t item_cap, int32_t f);
int grapes_gcn2_propagate_fwd(const float* x, const float* x0, const int32_t* loops, const int32_t* rowptr_t,
                              const int32_t* csr_src, float alpha, float* s_out, float* p_out, int32_t n, const int32_t* d_n,
                              int32_t f, const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap,
                              void* workspace, int32_t* status, grapes_stream_t stream);
/* Backward of the above (autograd through modules/gcn.py:109,113).  With D = ds + ds_add (ds_add optional):
 *   dx[j]  = (1 - alpha) (sum_{i in row j of the by-source CSR} D[i] + loops[j] D[j])
 *   dx0[i] (+)= alpha D'[i] + dx0_add[i]      D' = D, or ds alone when add_is_p != 0; accumulate_x0: x0 feeds every layer
 * ds is the gradient of s_out; ds_add is a second share of it (add_is_p == 0: the identity-mapping GEMM's) or the gradient of
 * p_out (add_is_p != 0: it reaches x only); dx0_add (optional) is a gradient that reaches x0 directly (that of x0 W2).  A gather
 * over rowptr_s / csr_dst with the by-source items; with ds_add or dx0_add one streaming pass forms D and dx0 first.  dx0 may
 * be NULL.  workspace as for the forward (required with ds_add / dx0_add). */
int grapes_gcn2_propagate_bwd(const float* ds, const float* ds_add, int32_t add_is_p, const float* dx0_add, const int32_t* loops,
                              const int32_t* rowptr_s, const int32_t* csr_dst, float alpha, float* dx, float* dx0,
                              int32_t accumulate_x0, int32_t n, const int32_t* d_n, int32_t f, const int32_t* items_s,
                              const int32_t* d_n_items_s, int32_t item_cap, void* workspace, int32_t* status,
                              grapes_stream_t stream);
/* The identity-mapping blend (inside GCN2Conv.forward, + the torch.relu of gcn.py:109 when relu != 0):
 *   out = act(c0 s + c1 t1 + c2 t2)     t2 optional; shared weights: (c0, c1) = (1 - beta, beta), t1 = S W1. */
int grapes_gcn2_mix_fwd(const float* s, const float* t1, const float* t2, float c0, float c1, float c2, int32_t relu, float* out,
                        int32_t n, const int32_t* d_n, int32_t f, grapes_stream_t stream);
/* Its backward in one read of dout and out: g = dout gated by out > 0 (relu != 0), g0 = c0 g, g1 = c1 g, g2 = c2 g
 * (g1, g2 optional; out may be NULL when relu == 0). */
int grapes_gcn2_mix_bwd(const float* dout, const float* out, int32_t relu, float c0, float c1, float c2, float* g0, float* g1,
                        float* g2, int32_t n, const int32_t* d_n, int32_t f, grapes_stream_t stream);

/* ------------------------------------------------------------------ GCNConv with edge weights (csrc/wgcn_kernels.hip)
 * modules/gcn.py:9-42 builds its layers from PyG's GCNConv, whose forward is forward(x, edge_index, edge_weight=None)
 * (torch_geometric 2.5.2, not in the reference tree).  With weights, gcn_norm(edge_index, edge_weight, add_self_loops=True,
 * improved=False, flow='source_to_target') is
 *   add_remaining_self_loops(fill_value=1): non-loop entries keep their weights; every node gets ONE loop of weight lw[i] = 1,
 *     or the weight of its stored entry (i, i) — of the LAST one in input order when there are several (PyG assigns them by
 *     index-put; the rule is fixed here so that the result is a function of the input);
 *   deg[c] = lw[c] + sum of w_e over the non-loop entries into c;  dinv = deg^-1/2, inf -> 0.  A negative degree gives NaN, as in
 *     PyG; it is not checked;
 *   out[c] = dinv[c] sum_{e: r -> c} w_e dinv[r] H[r] + dinv[c]^2 lw[c] H[c] + bias   (duplicates each count; a weight 0 is legal)
 * over the CSRs of grapes_gcn_prepare (ascending neighbour ids per row, stored loops and out-of-range entries dropped).  Widths:
 * any f <= 256; f % 4 == 0 with 16-byte aligned rows up to 1024.  No floating-point atomics: every sum has a fixed order (slot
 * order inside a row, chunk order across work items, a fixed tree across partials) and duplicates sit in input order, so results
 * are bit-identical from run to run.  status: GRAPES_STATUS_BAD_INDEX when an entry finds no slot or a CSR entry is outside [0, n).
 * Operands are taken to be finite: a lane without an entry adds 0 * (the row's own operand), so an inf / NaN in H[c] (forward) or
 * G[r] (backward) reaches that row's sums even where its coefficient is 0. */
/* The structure pass, once per edge list (replaces the bookkeeping of add_remaining_self_loops, gcn_norm's first call): for input
 * entry i, pos_t[i] / pos_s[i] [e] = its slot in the by-target / by-source CSR (-1: a stored loop or a dropped entry), inv_t / inv_s
 * [e] the inverse maps (slot -> input entry), loop_src [n] = the input index of the stored loop that sets lw, or -1.  edge_src /
 * edge_dst / e / d_e / n / d_n: the list grapes_gcn_prepare was given (without a node_map).  Duplicates of one (r, c) take adjacent
 * slots in input order.  Cost: one binary search per entry, plus L reads per member of a run of L duplicates of one (r, c) — L^2 per
 * run, and the L claims of a run share one atomic counter: meant for multigraphs whose runs are short (a pair repeated 10^4 times
 * costs 10^8 reads, once per edge list).  workspace: grapes_wgcn_structure_workspace_bytes(e), 16-byte aligned. */
size_t grapes_wgcn_structure_workspace_bytes(int32_t e);
int grapes_wgcn_structure(const int32_t* edge_src, const int32_t* edge_dst, int32_t e, const int32_t* d_e, int32_t n,
                          const int32_t* d_n, const int32_t* rowptr_t, const int32_t* csr_src, const int32_t* rowptr_s,
                          const int32_t* csr_dst, int32_t* pos_t, int32_t* pos_s, int32_t* inv_t, int32_t* inv_s,
                          int32_t* loop_src, void* workspace, int32_t* status, grapes_stream_t stream);
/* GCNConv's other constructor arguments (PyG 2.5 GCNConv(improved, add_self_loops, normalize), as recalled): the CSRs never hold a
 * loop, so every mode is a rule for lw, and one of them drops the normalisation.
 *   GRAPES_WGCN_LOOP_FILL     add_self_loops=True: lw[i] = the weight of the last stored (i, i), or fill (1; improved=True: 2).
 *                             fill = 1 is the rule written out above.
 *   GRAPES_WGCN_LOOP_SUM      add_self_loops=False, normalize=True: nothing is added and a stored loop is an ordinary entry —
 *                             lw[i] = the weights of ALL stored (i, i), added in input order (0 without one), deg, dinv and the
 *                             formulas as above; a node without an incoming entry has dinv = 0 and outputs the bias.  dw: every
 *                             stored loop of i gets s_i^2 (G[i] . H[i]) + q_i.
 *   GRAPES_WGCN_UNNORMALIZED  normalize=False: lw as LOOP_SUM; no deg and no dinv (dinv may be NULL and is never read):
 *                             out[c] = sum_{e: r -> c} w_e H[r] + lw_c H[c] + bias,  dh[r] = sum_{e: r -> c} w_e G[c] + lw_r G[r],
 *                             dw[i] = p_e for a stored entry, G[i] . H[i] for a stored loop. */
#define GRAPES_WGCN_LOOP_FILL 0
#define GRAPES_WGCN_LOOP_SUM 1
#define GRAPES_WGCN_UNNORMALIZED 2
/* The structure pass of LOOP_SUM / UNNORMALIZED, once per edge list: the stored loops of every node as a list in input order —
 * loop_ptr [n + 1], loop_idx [e] (the first loop_ptr[n] places are written) = input indices.  Integer atomics count and claim, a
 * rank puts each node's claims in input order (L reads per member of a node with L stored loops).  workspace:
 * grapes_wgcn_loops_workspace_bytes(n, e), 16-byte aligned. */
size_t grapes_wgcn_loops_workspace_bytes(int32_t n, int32_t e);
int grapes_wgcn_loops(const int32_t* edge_src, const int32_t* edge_dst, int32_t e, const int32_t* d_e, int32_t n, const int32_t* d_n,
                      int32_t* loop_ptr, int32_t* loop_idx, void* workspace, grapes_stream_t stream);
/* The weight pass, per call (replaces gcn_norm's scatter of edge_weight into deg, its pow(-0.5) and its masked_fill): val_t / val_s
 * [e] = the weights in both CSR orders, lw [n] by the rule of `mode` (fill is read by LOOP_FILL alone), dinv [n] with deg summed in
 * by-target slot order.  edge_weight NULL: every weight is 1 (an unweighted call; no ones vector is formed) — in every mode,
 * LOOP_FILL with fill 1 included, which up to ABI 302 refused it.  loop_src is read by LOOP_FILL only, loop_ptr / loop_idx by the
 * other two (NULL where not read); UNNORMALIZED writes no dinv (NULL).  One launch. */
int grapes_wgcn_weights(const float* edge_weight, int32_t e, const int32_t* inv_t, const int32_t* inv_s, const int32_t* loop_src,
                        const int32_t* loop_ptr, const int32_t* loop_idx, const int32_t* rowptr_t, const int32_t* rowptr_s, int32_t n,
                        const int32_t* d_n, int32_t mode, float fill, float* val_t, float* val_s, float* lw, float* dinv,
                        grapes_stream_t stream);
/* GCNConv.propagate with the weights of that pass (+ bias, + ReLU when relu != 0) in ONE pass over the by-target CSR: a group of
 * lanes per row, each lane reads one column index and one val_t per batch, val * dinv[col] is broadcast with the index.  mode: the
 * one the weights were made by — LOOP_FILL and LOOP_SUM run the same kernels over their own lw and dinv; UNNORMALIZED runs
 * specialisations that never load dinv (one memory request per gathered entry less).
 * long_items / d_n_items / item_cap / workspace as grapes_gcn_aggregate_fwd (NULL: every row by one group): rows longer than
 * GRAPES_LONG_ROW are cut into items whose partial sums are merged in chunk order.  workspace:
 * grapes_wgcn_aggregate_workspace_bytes(item_cap, f), 16-byte aligned.  bias may be NULL; out must not alias h. */
size_t grapes_wgcn_aggregate_workspace_bytes(int32_t item_cap, int32_t f);
int grapes_wgcn_aggregate_fwd(const float* h, const int32_t* rowptr_t, const int32_t* csr_src, const float* val_t, const float* dinv,
                              const float* lw, const float* bias, float* out, int32_t n, const int32_t* d_n, int32_t f,
                              int32_t relu, int32_t mode, const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap,
                              void* workspace, int32_t* status, grapes_stream_t stream);
/* Backward of the above and of gcn_norm (autograd through GCNConv.forward with edge weights).  With G = dout gated by
 * relu_out > 0 (relu_out NULL: G = dout), s = dinv, p_e = G[c] . H[r], for LOOP_FILL (the modes above say where the others differ:
 * dw's loop rule; UNNORMALIZED forms no by-source / by-target sums and no q):
 *   dh[r] = s_r sum_{e: r -> c} w_e s_c G[c] + s_r^2 lw_r G[r]                       (by-source CSR)
 *   dbias = column sums of G (the gated column-sum pass of grapes_gcn_aggregate_bwd: partials added in a fixed order)
 *   t_i = sum_{e -> i} w_e s_r p_e + sum_{e: i -> c} w_e s_c p_e + 2 s_i lw_i (G[i] . H[i]),   q_i = -1/2 s_i^3 t_i (0 where s_i = 0)
 *   dw[i] = s_r s_c p_e + q_c for a stored entry; s_i^2 (G[i] . H[i]) + q_i for the loop that set lw[i]; 0 for an overridden loop
 *           and for a dropped entry                                                    (input order, through pos_t and loop_src)
 * dh, dbias and dw may each be NULL (not all three); h, edge_src / edge_dst / pos_t / loop_src, rowptr_t / csr_src / val_t and
 * items_t are needed for dw only.  items_t / items_s: the two halves of gcn_prepare's item table with their counts (NULL: no row
 * splitting).  workspace: grapes_wgcn_aggregate_bwd_workspace_bytes(n, e, item_cap, f), 16-byte aligned. */
size_t grapes_wgcn_aggregate_bwd_workspace_bytes(int32_t n, int32_t e, int32_t item_cap, int32_t f);
int grapes_wgcn_aggregate_bwd(const float* dout, const float* relu_out, const float* h, const int32_t* edge_src,
                              const int32_t* edge_dst, int32_t e, const int32_t* d_e, const int32_t* pos_t, const int32_t* loop_src,
                              const int32_t* rowptr_t, const int32_t* csr_src, const float* val_t, const int32_t* rowptr_s,
                              const int32_t* csr_dst, const float* val_s, const float* dinv, const float* lw, float* dh,
                              float* dbias, float* dw, int32_t n, const int32_t* d_n, int32_t f, int32_t mode,
                              const int32_t* items_t, const int32_t* d_n_items_t, const int32_t* items_s,
                              const int32_t* d_n_items_s, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ PNAConv (csrc/pna_kernels.hip)
 * modules/gcn.py:120-149: PNA stacks PNAConv(in_channels, out_channels, aggregators, scalers, deg) layers, every other argument
 * at its default (torch_geometric 2.5.2, not in the reference tree): towers = 1, pre_nn = Linear(2 f, f), post_nn =
 * Linear((n_agg n_scal + 1) f, c), lin = Linear(c, c).  The message of a stored edge (j -> i) is pre_nn([x_i | x_j]) =
 * a_i + b_j with a = x W_i^T + bias, b = x W_j^T (two GEMM outputs sharing the pitch ld; W_pre = [W_i | W_j]): no per-edge
 * tensor is formed.  Every occurrence of a stored edge counts, a stored (i, i) comes back through loops[i]
 * (grapes_gcn2_loop_counts), no loop is added, nothing is normalised.  With d_i = row length + loops[i], per feature:
 *   mean = sum m / max(d, 1);  min, max (0 when d = 0);  var = relu(mean(m^2) - mean(m)^2) computed CENTRED (Welford per entry,
 *   Chan's update across work items);  std = sqrt(var + 1e-5);  sum
 * Aggregator codes: 0 mean, 1 min, 2 max, 3 std, 4 var, 5 sum.  Scaler codes: 0 identity, 1 amplification log(d + 1) / avg_log,
 * 2 attenuation avg_log / log(max(d, 1) + 1), 3 linear d / avg_lin, 4 inverse_linear avg_lin / max(d, 1).  agg_code / scal_code
 * hold n_agg <= 6 / n_scal <= 5 codes of 3 bits each, the first in the low bits.  Any f >= 1 (float4 columns when f % 4 == 0,
 * ld % 4 == 0 and the rows are 16-byte aligned).  No floating-point atomics: results are bit-identical from run to run. */
/* z[i] = [x_i | scaler_1(agg_1 .. agg_k) | scaler_2(...) | ...]  ([n][(1 + n_agg n_scal) f]: post_nn's operand, written once),
 * stats[i] = [mean | min | max | var | ties_min | ties_max] of b over row i ([n][6][f]; ties = number of entries equal to the
 * extreme) for the backward.  ONE gather pass over the by-target CSR: a group of lanes per row, the statistics in registers.
 * long_items / d_n_items / item_cap / workspace as grapes_gcn2_propagate_fwd (NULL: every row by one group); workspace:
 * grapes_pna_aggregate_fwd_workspace_bytes(item_cap, f), 16-byte aligned.  z and stats must not alias the inputs. */
size_t grapes_pna_aggregate_fwd_workspace_bytes(int32_t item_cap, int32_t f);
int grapes_pna_aggregate_fwd(const float* x, const float* a, const float* b, int32_t ld, const int32_t* loops,
                             const int32_t* rowptr_t, const int32_t* csr_src, int32_t n_agg, int32_t agg_code, int32_t n_scal,
                             int32_t scal_code, float avg_log, float avg_lin, float* z, float* stats, int32_t n,
                             const int32_t* d_n, int32_t f, const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap,
                             void* workspace, int32_t* status, grapes_stream_t stream);
/* Backward of the above from dz = d z.  A row-local pass folds the scalers and the aggregators into four coefficients per (row,
 * feature) and writes  da[i] = gmean + gmin + gmax  (0 when d_i = 0); a gather over the by-source CSR (items_s as
 * grapes_gcn2_propagate_bwd) then writes
 *   db[j] = sum_{i <- j} gmean_i / d_i + 2 gvar_i (b_j - mean_i) / d_i + gmax_i [b_j == max_i] / ties_max_i
 *           + gmin_i [b_j == min_i] / ties_min_i          (+ loops[j] times the term with i = j)
 * gvar_i is gated by var_i > 0.  Bit-equal extremes share the gradient evenly.  da / db: [n][ld_d] (two halves of one matrix, or
 * two matrices with one pitch).  The columns dz[:, :f] (the gradient of the copy of x) are not read: grapes_pna_add_input_grad.
 * workspace (required): grapes_pna_aggregate_bwd_workspace_bytes(n, item_cap, f), 16-byte aligned. */
size_t grapes_pna_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f);
int grapes_pna_aggregate_bwd(const float* dz, const float* b, int32_t ld, const float* stats, const int32_t* loops,
                             const int32_t* rowptr_t, const int32_t* rowptr_s, const int32_t* csr_dst, int32_t n_agg,
                             int32_t agg_code, int32_t n_scal, int32_t scal_code, float avg_log, float avg_lin, float* da,
                             float* db, int32_t ld_d, int32_t n, const int32_t* d_n, int32_t f, const int32_t* items_s,
                             const int32_t* d_n_items_s, int32_t item_cap, void* workspace, int32_t* status,
                             grapes_stream_t stream);
/* dx[i][:f] += dz[i][:f] over the first n rows (dz with the pitch ld_z): the gradient that reaches x through its copy in z. */
int grapes_pna_add_input_grad(float* dx, const float* dz, int32_t ld_z, int32_t n, const int32_t* d_n, int32_t f,
                              grapes_stream_t stream);

/* ------------------------------------------------------------------ A2: sampler
 * modules/utils.py:13-71.  One launch: keys = log(sigmoid(l)) + Gumbel(u) with the portable
 * fp32 exp/log of oracle/portable_math.py (bit-identical on CPU and GPU), exact top-k by 4-pass
 * radix select (ties -> lowest position), position-ordered compaction, Bernoulli log-prob,
 * sampler statistics.
 *   logits: if logit_index != NULL the candidate's logit is logits[logit_index[i]] (main.py:213)
 *   uniforms: the torch.rand(n) of the reference's Gumbel draw; if NULL, Philox4x32-10 with
 *             (philox_seed, offset) generates them; offset = *d_philox_offset when non-NULL
 *             (and the kernel advances it), else philox_offset.
 *   mode: 0 = Gumbel-top-k (training, utils.py:37-44); 1 = greedy top-k of probs (eval.py:126-130)
 *   n <= k: every candidate is kept, log_prob = logsigmoid(l), no noise consumed (utils.py:31-33).
 * Outputs: mask[n] (1.0 / 0.0), kept_pos[min(n,k)] ascending candidate positions,
 *   kept_ids = candidate_ids[kept_pos] (optional), d_kept_count, log_prob[n] (optional),
 *   keys_out[n] (optional), stats[6] = {min_prob, max_prob, mean_entropy, std_entropy,
 *   sum(log_prob), valid(1/0)} (optional).
 *   union_ids (optional) = [prefix_ids[0:prefix_n] | kept ids], *d_union_count = prefix_n + kept count: the next
 *   hop's batch_nodes = cat(target_nodes, sampled nodes) (main.py:236-238) written by the same launches. */
size_t grapes_sampler_workspace_bytes(int32_t n_cap);
int grapes_gumbel_topk(const float* logits, const int32_t* logit_index, const float* uniforms,
                       uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset,
                       int32_t n, const int32_t* d_n, int32_t k, int32_t mode,
                       const int32_t* candidate_ids, float* mask, int32_t* kept_pos,
                       int32_t* kept_ids, int32_t* d_kept_count, float* log_prob, float* keys_out,
                       float* stats, const int32_t* prefix_ids, int32_t prefix_n, int32_t* union_ids,
                       int32_t* d_union_count, void* workspace, grapes_stream_t stream);
/* The same draw with ONE histogram of the order keys' top 12 bits for the whole draw (instead of per-workgroup rows of their top
 * byte): d_hist = grapes_sampler_hist_words() 32-bit words of caller memory, 16-byte aligned, ZERO before the first use and left
 * zero; draws sharing it must be stream-ordered.  The bin of the k-th largest key then holds ~0.3 % of the candidates, and the
 * selection every emit workgroup derives is a short scan + three short passes.  Results are bit-identical to grapes_gumbel_topk.
 * Replaces the same reference lines (modules/utils.py:37-71). */
int32_t grapes_sampler_hist_words(void);
int grapes_gumbel_topk_hist(const float* logits, const int32_t* logit_index, const float* uniforms,
                            uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset,
                            int32_t n, const int32_t* d_n, int32_t k, int32_t mode,
                            const int32_t* candidate_ids, float* mask, int32_t* kept_pos,
                            int32_t* kept_ids, int32_t* d_kept_count, float* log_prob, float* keys_out,
                            float* stats, const int32_t* prefix_ids, int32_t prefix_n, int32_t* union_ids,
                            int32_t* d_union_count, void* workspace, uint32_t* d_hist, grapes_stream_t stream);
/* grapes_gumbel_topk_hist whose last launch has NO TAIL: the kept count, the next query list's count, stats[5] and the Philox
 * advance are written by the launch's first workgroup as soon as it knows the selection; the sum of the log-probs (stats[4]) and
 * the histogram's return to zero are LEFT to the caller's next launch — *finish receives what grapes_frontier_expand_fused_ext
 * needs for them (pointers into `workspace`, which must stay alive until that launch has run).  Same results, bit for bit. */
/* grapes_gumbel_topk_deferred that also writes the next query list's ROW EXTENTS beside its ids (round 5): union_ext[2 j], [2 j + 1] =
 * rowptr[union_ids[j]], rowptr[union_ids[j] + 1]  (int64 pairs, 16-byte aligned, prefix_n + min(k, n) of them; prefix_ext: the prefix
 * ids' pairs, copied) for the adjacency `rowptr` the caller expands next — grapes_frontier_expand_fused_ext(node_ext = union_ext) then
 * needs one round trip less.  The draw requests every candidate's pair while it waits at its barrier; only the kept ones are stored.
 * Same draw, bit for bit (modules/utils.py:37-71; main.py:236-238 for the list). */
int grapes_gumbel_topk_deferred_ext(const float* logits, const int32_t* logit_index, const float* uniforms,
                            uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset,
                            int32_t n, const int32_t* d_n, int32_t k, int32_t mode,
                            const int32_t* candidate_ids, float* mask, int32_t* kept_pos,
                            int32_t* kept_ids, int32_t* d_kept_count, float* log_prob, float* keys_out,
                            float* stats, const int32_t* prefix_ids, int32_t prefix_n, int32_t* union_ids,
                            int32_t* d_union_count, void* workspace, uint32_t* d_hist, grapes_draw_finish_args* finish,
                            const int64_t* rowptr, const int64_t* prefix_ext, int64_t* union_ext, grapes_stream_t stream);
/* d logits[i] = g · (mask[i] − sigmoid(l_i)),  g = *d_grad_scale (device scalar) × grad_vec[i]
 * (either may be NULL = 1).  If dlogits_index != NULL the result is scattered:
 * dlogits[dlogits_index[i]] = value (destination pre-zeroed by the caller). */
/* sum_out (optional): (+)= Σ of the written values = the bias gradient of the 1-wide head producing these logits;
 * needs partials (fp32[2048] scratch) and d_ticket (a device word that is ZERO at rest; the kernel leaves it zero). */
int grapes_bernoulli_logprob_bwd(const float* logits, const int32_t* logit_index,
                                 const float* mask, const float* grad_vec,
                                 const float* d_grad_scale, float* dlogits, int32_t n,
                                 const int32_t* d_n, float* sum_out, int32_t accumulate_sum,
                                 float* partials, uint32_t* d_ticket, grapes_stream_t stream);
/* Philox4x32-10 uniforms in [0,1): out[i] from counter offset + i/4, lane i%4. */
int grapes_philox_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset,
                          grapes_stream_t stream);

/* ------------------------------------------------------------------ small helpers on the path */
/* out = Σ_{i<n} x[i] / (mean ? n : 1)   (main.py:228 log_z, main.py:276 tot_log_prob) */
int grapes_reduce_sum(const float* x, int32_t n, const int32_t* d_n, int32_t mean, float* out,
                      grapes_stream_t stream);
/* x[i] = value for i < n (count-aware fill; used for d(mean) broadcasts) */
/* sum_out (optional): (+)= n · value, the sum of what was written */
int grapes_fill(float* x, int32_t n, const int32_t* d_n, float value, const float* d_value,
                float scale_by_inv_n, float* sum_out, int32_t accumulate_sum, grapes_stream_t stream);

/* Backward of the sampler net's 1-wide head for up to four hops in TWO launches (the hops' weights are shared, and only
 * the backward passes of different hops are independent of each other):
 *   dlogits[q][r] = d_grad_scale * (mask[q][cand_pos[q][r]] - sigmoid(logits[q][r]))  for candidate rows, 0 otherwise —
 *                   utils.py:71 differentiated, written densely over the hop's *d_n[q] batch rows (no zero fill needed);
 *   sum_out (+)=    the sum of all of them (bias gradient of the head), combined in a fixed order;
 *   dh[q]         = Â_qᵀ dlogits[q]  (by-source CSR of grapes_gcn_prepare: rowptr_s / csr_dst / dinv).
 * Arrays are HOST arrays of `count` device pointers; logits[q] is the hop's [n_cap[q]] logit vector (per batch row),
 * mask[q] its draw (per candidate position).  A segment with mask[q] == NULL is a MEAN head instead (the log-Z net,
 * main.py:228): dlogits[q][r] = d_grad_scale / *d_n[q] on every live row, not part of sum_out; *mean_sum_out = their sum
 * (that head's bias gradient).  workspace: grapes_sampler_head_bwd_multi_workspace_bytes(); d_ticket: one zero word,
 * left zero. */
size_t grapes_sampler_head_bwd_multi_workspace_bytes(void);
/* The same in two calls: phase 1 = the d logits launch only, phase 2 = the aggregation launch only (0 = both, as above).
 * Between them the caller may issue independent launches of its own; each of the two launches carries a pending recorded
 * few-row backward aggregation of the classifier (grapes_gcn_aggregate_bwd while grapes_rider_record_begin is open) as extra
 * columns of its grid — main.py:267 and main.py:287 depend on the losses only, not on each other. */
int grapes_sampler_head_bwd_multi_phase(int32_t count, const float* const* logits, const float* const* mask,
                                        const int32_t* const* cand_pos, const int32_t* n_cap, const int32_t* const* d_n,
                                        const float* d_grad_scale, const int32_t* const* rowptr_s,
                                        const int32_t* const* csr_dst, const float* const* dinv, float* const* dlogits,
                                        float* const* dh, float* sum_out, int32_t accumulate_sum, float* mean_sum_out,
                                        void* workspace, uint32_t* d_ticket, int32_t phase, grapes_stream_t stream);

/* ------------------------------------------------------------------ losses + optimiser update
 * main.py:260,267: loss_c = CrossEntropyLoss (labels: int64 class of every node) or BCEWithLogitsLoss (labels_f:
 * fp32 [N, C]) over rows local_rows[0..B) of logits[n_rows, C], labels looked up at target_ids[b] (global ids);
 * dlogits[n_rows, C] = d loss_c / d logits (zero outside those rows — what loss_c.backward() feeds gcn_c).
 * Exactly one of labels / labels_f is non-NULL.  B <= 4096.  The target rows must be distinct. */
int grapes_classifier_loss(const float* logits, int32_t n_rows, int32_t C, const int32_t* local_rows,
                           const int32_t* target_ids, const int64_t* labels, const float* labels_f,
                           int32_t B, float* dlogits, float* loss_out, grapes_stream_t stream);
/* eval.py:154-155 (mini-batch evaluation, N1): pred[b] = argmax_c logits[node_map[targets[b]], c] — the first largest, a NaN the
 * largest (torch.argmax) — and rows_out[b, :] (optional) = that row.  A target whose map entry is not a row of logits raises
 * GRAPES_STATUS_BAD_INDEX in *status (optional).  Replaces: node_map.map + index_select + argmax (four framework launches). */
int grapes_eval_predict(const float* logits, int32_t n_rows, int32_t C, const int32_t* node_map, const int32_t* targets,
                        int32_t B, int64_t* pred, float* rows_out, int32_t* status, grapes_stream_t stream);
/* main.py:272-282.  hop_stats[h*stats_stride + 4] = sum of hop h's log-probs (the statistics row grapes_gumbel_topk
 * writes); log_z = *log_z_raw - log_z_init (log_z_raw may be NULL = 0).  out4 = {loss_gfn, d loss_gfn / d (log_z or
 * sum log-probs) [= 2·inner for trajectory balance, = -cost for REINFORCE (main.py:279)], log_z, sum log-probs}. */
int grapes_gflownet_loss(const float* log_z_raw, float log_z_init, const float* hop_stats, int32_t hops,
                         int32_t stats_stride, const float* loss_c, float loss_coef, int32_t reinforce,
                         float* out4, grapes_stream_t stream);
/* main.py:259-282 in ONE launch (one workgroup): grapes_classifier_loss with the target rows looked up as
 * node_map[target_ids[b]] (main.py:259), log_z = mean(z_out[0..nz)) - log_z_init (main.py:228; z_out may be NULL = 0;
 * the sum is formed exactly as grapes_reduce_sum forms it) and grapes_gflownet_loss on the loss just computed. */
/* workspace (grapes_step_losses_workspace_bytes(B), 8-byte aligned) + d_ticket (one zero word, left zero): the work is
 * spread over up to 65 workgroups (n_rows <= 65536), results bit-identical to the single-workgroup form that NULLs
 * select. */
size_t grapes_step_losses_workspace_bytes(int32_t B);
int grapes_step_losses(const float* logits, int32_t n_rows, int32_t C, const int32_t* node_map,
                       const int32_t* target_ids, const int64_t* labels, const float* labels_f, int32_t B,
                       float* dlogits, float* loss_out, const float* z_out, int32_t nz, const int32_t* d_nz,
                       float log_z_init, const float* hop_stats, int32_t hops, int32_t stats_stride,
                       float loss_coef, int32_t reinforce, float* out4, const float* loss_extra, void* workspace,
                       uint32_t* d_ticket, grapes_stream_t stream);
/* F.dropout(x, p, training=True) of modules/gcn.py:33,37 on the sampler's Philox stream: element i of the live [n, f] matrix is
 * kept iff philox_uniform(seed, offset, i) >= p (grapes_philox_uniform's generator) and scaled by 1 / (1 - p); keep[i] = 1 / 0.
 * With d_philox_offset the offset is read from the device and advanced by ceil(n f / 4) afterwards.  The backward pass is
 * dx = keep ? dy / (1 - p) : 0.  (The reference draws its mask from torch's generator: parity is statistical there and exact
 * against the oracle's Philox.) */
int grapes_dropout_fwd(const float* x, float* y, uint8_t* keep, int32_t n, const int32_t* d_n, int32_t f, float p,
                       uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, grapes_stream_t stream);
int grapes_dropout_bwd(const float* dy, const uint8_t* keep, float* dx, int32_t n, const int32_t* d_n, int32_t f, float p,
                       grapes_stream_t stream);
/* The regulariser of main.py:260-261,  reg * sum_r var(logits[r, :])  (torch.var: unbiased, over the classes, every row):
 * with `out` the term itself (one float: pass it to grapes_step_losses as loss_extra — it is then part of loss_out and of
 * the GFlowNet cost, main.py:274), with `dlogits` its gradient ADDED to dlogits (after grapes_step_losses has written them):
 * dlogits[r][c] += reg * 2 (logits[r][c] - mean_r) / (C - 1).  Either pointer may be NULL. */
int grapes_logit_var_reg(const float* logits, int32_t n, const int32_t* d_n, int32_t C, float reg, float* out, float* dlogits,
                         grapes_stream_t stream);
/* main.py:268,289: torch.optim.Adam (amsgrad off) for n_tensors tensors in ONE launch.  d_desc = device array of
 *   struct { float* p; const float* g; float* m; float* v; float* step; int64_t n;
 *            double lr, beta1, beta2, eps, weight_decay; int32_t maximize, pad;
 *            float* w_pad; void* img; int32_t K, ld_pad; } (grapes_adam_desc_bytes() each)
 * step = the optimiser's per-tensor step counter (fp32 scalar, as torch keeps it for capturable=True); the launch
 * uses step+1 and advances every distinct counter once.  d_ticket: n_tensors device words, zero at rest.
 * MIRRORS (round 4; both may be NULL): p is a contiguous [rows, K] weight (< 2^31 elements) and the launch writes every updated
 * element also into w_pad [rows, ld_pad] (the zero-padded fp32 copy a first layer with K % 4 != 0 computes on) and / or into img
 * (the bf16x3 split image of grapes_weight_split_image, rows <= 256) — the copies a step used to rebuild with launches of their own
 * follow the weights by themselves; their padding is written once by the caller and never touched. */
int32_t grapes_adam_desc_bytes(void);
int grapes_adam_step(const void* d_desc, int32_t n_tensors, int64_t max_numel, uint32_t* d_ticket,
                     grapes_stream_t stream);
/* The same launch with grapes_slab_reduce_sets folded in (the classifier's few-row weight gradients, main.py:267 -> :268): a
 * tensor whose gradient pointer equals grads[q] first gets  grad (+)= sum of its slabs (slabs[q]: [ceil(n/128)][numel], summed
 * in grapes_slab_reduce_sets' order: bit-identical), written back to the gradient, then the update.  Every grads[q] must be
 * the gradient of one of the n_tensors tensors (the caller checks).  nsets <= 8; n / d_n: the rows the slabs were formed over. */
int grapes_adam_step_slabs(const void* d_desc, int32_t n_tensors, int64_t max_numel, uint32_t* d_ticket, int32_t nsets,
                           const float* const* slabs, const float* const* grads, int32_t n, const int32_t* d_n,
                           int32_t accumulate, grapes_stream_t stream);

/* ------------------------------------------------------------------ 1-D node partition: either side of the RCCL
 * exchanges (distributes main.py:180 get_neighborhoods and main.py:199-204 x[batch_nodes]).
 * Rank r owns global ids [lo, hi) = [bounds[r], bounds[r+1]); its CSR rows are rebased to 0, its columns are
 * global ids.  Every capacity is equal on all ranks and every live count is on the device, so none of these
 * reads a size on the host (they sit between fixed-size all-gather / all-to-all calls).
 *
 * Adjacency rows.  req = the all-gathered query lists, int32[n_peers][cap+1] (cap ids, then the live count).
 * The owner writes, for each peer p, reply[p] = int32[reply_stride]:
 *   [0,cap) row length of query j (0 if not owned / beyond the count), [cap,2cap) offset of that row inside the
 *   slot's column area, [2cap, 2cap+e_slot) the columns (query order, ascending inside a row).
 * eoff int32[n_peers*cap+1] is scratch.  A rank may own nothing (lo == hi): its replies hold zero lengths / empty runs, and
 * col_local (X_local in grapes_exchange_serve_features) may then be NULL.  Words of a slot outside these three areas, and columns past the slot's total, are
 * not written; the padding of a query list beyond its count (clamped to [0, cap]) may hold anything.
 *
 * Edge overflow.  A slot whose rows hold more than e_slot columns raises GRAPES_STATUS_EDGE_OVERFLOW on the owner: every column
 * whose index inside the slot is below e_slot is written, nothing at or past it, and the len / off headers stay those of the
 * FULL rows.  The requester adds the lengths it reads: a total above e_cap raises GRAPES_STATUS_EDGE_OVERFLOW there, *d_e and
 * eoff are the TRUE (unclamped) totals, and (src, dst)[0 .. e_cap) is the exact prefix of the true edge list — edge t of the
 * list sits at an in-slot index <= t < e_cap, so with e_cap <= e_slot every column that prefix reads was written.
 * A requester's e_cap MUST NOT exceed the owners' e_slot: the requester does not know e_slot and reads in-slot indices up to
 * e_cap - 1 unguarded, which after an owner's overflow lie past the columns written and, for the last peer, past `back`.
 * grapes_exchange_recv_rows refuses reply_stride < 2 cap + e_cap (GRAPES_EINVAL) — all it can check of that rule. */
/* This rank's query message: query[0..n) = ids, query[cap] = min(*d_n, n) (n when d_n is NULL); query[n..cap) is padding
 * and is left as it is. */
int grapes_exchange_pack_query(const int32_t* ids, int32_t n, const int32_t* d_n, int32_t cap, int32_t* query,
                               grapes_stream_t stream);
int grapes_exchange_serve_rows(const int64_t* rowptr_local, const int32_t* col_local,
                               const int32_t* req, int32_t n_peers, int32_t cap, int32_t lo, int32_t hi,
                               int32_t* reply, int64_t reply_stride, int32_t e_slot, int32_t* eoff,
                               int32_t* status, grapes_stream_t stream);
/* Requester: back = the all-to-all'ed replies int32[n_peers][reply_stride]; nodes[cap] (first *d_m live) are this
 * rank's queries.  Output = the contract of grapes_frontier_offsets + grapes_frontier_expand on the full graph:
 * eoff[cap+1], (src, dst)[e_cap] in query order then ascending column, *d_e = edge count.  rowstart[cap] is scratch. */
int grapes_exchange_recv_rows(const int32_t* back, int64_t reply_stride, const int32_t* nodes, int32_t cap,
                              const int32_t* d_m, const int32_t* bounds, int32_t n_peers, int32_t e_cap,
                              int32_t* eoff, int32_t* rowstart, int32_t* src, int32_t* dst, int32_t* d_e,
                              int32_t* status, grapes_stream_t stream);
/* Halo feature rows.  req = all-gathered ASCENDING id lists int32[n_peers][cap+1]; the ids of [lo,hi) form one run of
 * each list; reply[p] = fp32[n_slot][F] holds the rows of peer p's run; slot rows past the run are not written.
 *
 * Node overflow.  A run longer than n_slot raises GRAPES_STATUS_NODE_OVERFLOW on the owner, which sends the run's first n_slot
 * rows.  The requester (grapes_exchange_assemble_features and grapes_exchange_halo_positions alike) clamps a row's position
 * inside its run to n_slot - 1, so every read stays inside the slot: rows among the first n_slot of their run are exact, every
 * later row of the run is a copy of the slot's last row (in the in-place form: has that row's position; the several ids that
 * share it then all write code_pos there and which of their words stays is unspecified).  The status word says so. */
int grapes_exchange_serve_features(const float* X_local, int32_t F, const int32_t* req, int32_t n_peers,
                                   int32_t cap, int32_t lo, int32_t hi, float* reply, int32_t n_slot,
                                   int32_t* status, grapes_stream_t stream);
/* Requester: out[i, 0:F] = row of ids[i] taken from back = fp32[n_peers][n_slot][F], out[i, F+j] = indicator j
 * (same packing as grapes_gather_rows); ids ascending, first *d_n live; rows of out past *d_n are not written.  The epoch an
 * indicator word (bits 8..31) is compared with is *d_epoch & 0xffffff when d_epoch is given, else `epoch`. */
int grapes_exchange_assemble_features(const float* back, int32_t F, int32_t n_slot, const int32_t* ids,
                                      int32_t n, const int32_t* d_n, const int32_t* bounds,
                                      int32_t n_peers, const uint32_t* ind_code, uint32_t epoch,
                                      const uint32_t* d_epoch, int32_t num_ind, float* out,
                                      grapes_stream_t stream);

/* ---- The same halo rows WITHOUT an exchange: peer shards read in place (replaces the all-gather + all-to-all of
 * grapes_exchange_serve_features / _assemble_features for aggregate-first first layers, main.py:199-204 + modules/gcn.py:32).
 * Every rank maps every other rank's shard of X into its address space once (hipIpc memory handles: the owner's HBM, reached
 * over xGMI by ordinary loads) and the fused gather-SpMM picks the shard of each row it reads from a table of at most
 * GRAPES_MAX_PEER_SHARDS (base pointer, first row) pairs held in registers.  No collective, no request/reply buffers, no
 * copy: a hop's halo costs the rows it touches, once, over the links they live behind.
 *   grapes_peer_export  handle[64] + byte offset of `ptr` inside its allocation, to be sent to the other ranks of the node
 *   grapes_peer_open    maps a peer's allocation into this process (lazily enabling peer access) -> its address of `ptr`
 *   grapes_peer_close   unmaps it (pass what grapes_peer_open returned and the same offset)
 * shard_base / shard_bounds of grapes_gcn_aggregate_gather_fwd_peers are HOST arrays (n_shards pointers; n_shards + 1 ascending
 * first-row numbers, shard_bounds[0] = 0): shard q holds rows [bounds[q], bounds[q + 1]) at pitch x_stride; row_head is
 * required (head records over GLOBAL row ids); everything else as grapes_gcn_aggregate_gather_fwd — results are bit-identical
 * to it on the concatenated matrix. */
#define GRAPES_MAX_PEER_SHARDS 8
#define GRAPES_PEER_HANDLE_BYTES 64
int grapes_peer_export(const void* ptr, void* handle, uint64_t* offset);
int grapes_peer_open(const void* handle, uint64_t offset, void** ptr);
int grapes_peer_close(void* ptr, uint64_t offset);
/* bytes from a mapped peer shard (or anywhere on a device) into local memory, on `stream` — start-up self-checks and tests */
int grapes_peer_copy(void* dst, const void* src, size_t bytes, grapes_stream_t stream);
int grapes_gcn_aggregate_gather_fwd_peers(const float* const* shard_base, const int32_t* shard_bounds, int32_t n_shards,
                                          int32_t F, int32_t x_stride, const int32_t* ids,
                                          const uint32_t* ind_code, uint32_t epoch, const uint32_t* d_epoch,
                                          int32_t num_ind, const int32_t* rowptr_t, const int32_t* csr_src,
                                          const float* dinv, const int32_t* row_head, float* out, int32_t n,
                                          const int32_t* d_n, grapes_stream_t stream);

/* Requester, in-place form: pos[i] = row of ids[i] inside back viewed as fp32[n_peers * n_slot][F] (rows past *d_n: 0) and,
 * with ind_code, code_pos[pos[i]] = ind_code[ids[i]] — grapes_gcn_aggregate_gather_fwd(X = back, ids = pos, ind_code =
 * code_pos, head records built with head_ids = pos) then aggregates the exchanged rows where they arrived.  Words of code_pos
 * that no live row maps to are not written; ind_code and code_pos come together or not at all (GRAPES_EINVAL); n = 0 writes
 * nothing.  dist.py. */
int grapes_exchange_halo_positions(const int32_t* ids, int32_t n, const int32_t* d_n, const int32_t* bounds,
                                   int32_t n_peers, int32_t n_slot, const uint32_t* ind_code, int32_t* pos,
                                   uint32_t* code_pos, grapes_stream_t stream);

/* Requester: where the rows of ids[0 .. *d_n) sit among the rows this rank has ALREADY received in this step —
 *   loc[ids[i]] = base + pos[row(i)],   row(i) = node_map[ids[i]]  (node_map != NULL)  or  idx_b[idx_a[i]]
 * with pos = grapes_exchange_halo_positions of the hop's batch and base = the hop's offset in one buffer holding every hop's
 * `back`.  node_map form: batch[0 .. *d_n_batch) are the hop's batch nodes; an id whose map entry does not point at itself there is
 * not a batch row (a target without any edge) and its entry of loc — written once from a replicated side table — is left alone.  all_nodes (main.py:252) are the targets and the kept nodes of the hops — batch rows of earlier fetches — so the
 * classifier's features (main.py:256) are a local gather through loc instead of a fourth request / reply.  loc: int32[N]. */
int grapes_exchange_note_rows(int32_t* loc, const int32_t* ids, int32_t n, const int32_t* d_n, const int32_t* node_map,
                              const int32_t* batch, int32_t n_batch, const int32_t* d_n_batch,
                              const int32_t* idx_a, const int32_t* idx_b, const int32_t* pos, int32_t base, grapes_stream_t stream);

/* A2 + A7: the draw with its logits produced on the way.  logits_out[r] = (Â head_in)[r] + *bias over the hop's n_rows batch
 * rows — the 1-wide last layer of the sampler net (main.py:210; head_in = act · w2ᵀ) — and every batch row that is a
 * candidate (cand_pos[r] >= 0: its position in neighbor_nodes; logit_index = nb_local, both from grapes_frontier_compact)
 * goes straight on to its key.  Two launches (aggregation + keys | selection + emit) instead of three; keys, masks and
 * log-probabilities are bit-identical to grapes_gcn_aggregate_fwd + grapes_gumbel_topk.  Other arguments as grapes_gumbel_topk. */
int grapes_gumbel_topk_from_aggregate(const float* head_in, const int32_t* rowptr_t, const int32_t* csr_src,
                                      const float* dinv, const float* bias, float* logits_out, int32_t n_rows,
                                      const int32_t* d_n_rows, const int32_t* cand_pos,
                                      const int32_t* logit_index, const float* uniforms,
                                      uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, int32_t n,
                                      const int32_t* d_n, int32_t k, int32_t mode, const int32_t* candidate_ids,
                                      float* mask, int32_t* kept_pos, int32_t* kept_ids, int32_t* d_kept_count,
                                      float* log_prob, float* keys_out, float* stats, const int32_t* prefix_ids,
                                      int32_t prefix_n, int32_t* union_ids, int32_t* d_union_count, void* workspace,
                                      grapes_stream_t stream);

/* ------------------------------------------------------------------ A7, first layers with F_in >= F_out (Reddit, Cora)
 * The reference order — transform, then aggregate (PyG GCNConv; modules/gcn.py:32) — with the transform reading its operand
 * feat(ids[r]) = [X[ids[r], 0:F] | indicator bits | 0-padding] (main.py:199-204) through the id list: the gathered matrix is
 * never written.  Kp = F + num_ind rounded up to a multiple of 4; w and dw are [f_out, Kp] (padding columns: ignored / zero).
 * X / x_stride as in grapes_gcn_aggregate_gather_fwd.  fp32 MFMA (v_mfma_f32_32x32x2_f32), fixed summation order. */
size_t grapes_linear_gathered_workspace_bytes(int32_t n_cap, int32_t k_pad, int32_t f_out);
int grapes_linear_fwd_gathered(const float* X, int32_t F, int32_t x_stride, const int32_t* ids,
                               const uint32_t* ind_code, uint32_t epoch, const uint32_t* d_epoch, int32_t num_ind,
                               const float* w, float* h, int32_t n, const int32_t* d_n, int32_t f_out,
                               void* workspace, grapes_stream_t stream);
int grapes_linear_bwd_weight_gathered(const float* dh, const float* X, int32_t F, int32_t x_stride,
                                      const int32_t* ids, const uint32_t* ind_code, uint32_t epoch,
                                      const uint32_t* d_epoch, int32_t num_ind, uint32_t ind_mask, float* dw,
                                      int32_t n, const int32_t* d_n, int32_t f_out, int32_t accumulate,
                                      void* workspace, grapes_stream_t stream);
/* ind_mask (0 = all): the indicator bits that count.  The indicator columns accumulate from hop to hop within a batch
 * (main.py:191), and a backward pass that re-reads them at the END of the step must see what its hop's forward pass saw:
 * bits 0..hop and the target bit (the reference keeps the hop's x tensor alive instead). */

/* The same two GEMMs on the bf16 matrix pipe at fp32 accuracy (exact 3-way bf16 operand splits, six cross products per
 * product, fp32 accumulation; csrc/gemm_tiled_split.hip): 128 x 256 output tiles, both operands streamed through split-plane
 * LDS images in K steps of 32.  The forward takes W as a pre-split IMAGE (grapes_weight_split_image, once per step, from the
 * [f_out, k] parameter itself: no padded copy); f_out <= 256, a multiple of 4.  GRAPES_GEMM_SPLIT=0 disables them
 * (grapes_split_gathered_available).
 * Range (these entries, the split-K / split-tail / several-problem forms below; tests/test_tsplit_accuracy_gpu.py:
 * test_tiled_split_range_edges): each OPERAND is split on its own — a gathered entry, a weight, a dH entry — not a product.
 *   - an entry >= 3.3962e38 (finite in fp32) rounds to bf16 inf: its m term is -inf and its l term NaN, so every output that
 *     contracts over it is NaN — the whole forward row of a gathered row holding it (every column, 0 x NaN included), the
 *     whole dW column of that feature (every unit).  A weight or a dH entry that large goes through the same split and
 *     takes its forward column / dW row the same way (untested).  Other rows / columns are unaffected.  The fp32 kernels give a finite answer there.  Not guarded: inputs that large
 *     mean training has already diverged.
 *   - an entry below about 2^-110 (1e-33) is held by its three terms only to bf16's smallest subnormal step, 2^-133 (an
 *     error of at most 2^-134 per entry instead of 2^-24 relative): measured at X = 1e-35 (fails the element-wise fp32
 *     criterion) against 1e-28 (meets it); the matrix pipe keeps bf16 subnormals. */
int32_t grapes_split_gathered_available(int32_t f_out);
size_t grapes_weight_split_image_bytes(int32_t k);
int grapes_weight_split_image(const float* w, int32_t ldw, int32_t f_out, int32_t k, void* image, grapes_stream_t stream);
/* ... that also writes w_pad [f_out, ld_pad] (k <= ld_pad <= k rounded up to 32), a zero-padded fp32 copy of w for the few-row
 * fp32 kernels, in the same launch (instead of a strided copy of its own per step). */
int grapes_weight_split_image_padded(const float* w, int32_t ldw, int32_t f_out, int32_t k, void* image, float* w_pad,
                                     int32_t ld_pad, grapes_stream_t stream);
/* ... for up to GRAPES_MAX_WEIGHT_IMAGES weights in ONE launch (host arrays of `count` entries; w_pad / ld_pad may be NULL, a
 * w_pad[q] may be NULL): the sampler net's, the log-Z net's and the classifier's first layers (main.py:199-205,227,245) are
 * refreshed together at the top of a step. */
#define GRAPES_MAX_WEIGHT_IMAGES 4
int grapes_weight_split_images(int32_t count, const float* const* w, const int32_t* ldw, const int32_t* f_out, const int32_t* k,
                               void* const* image, float* const* w_pad, const int32_t* ld_pad, grapes_stream_t stream);
/* grapes_linear_bwd_weight_gathered_split with the row pitch of dw given: dw_ld = 0 or ceil4(F + num_ind) — the padded layout —
 * or exactly F + num_ind — the parameter's own [f_out, F + num_ind] gradient (modules/gcn.py:32 backward), written by the slab
 * sum itself instead of a strided copy out of a padded buffer afterwards. */
int grapes_linear_bwd_weight_gathered_split_ld(const float* dh, const float* X, int32_t F, int32_t x_stride,
                                               const int32_t* ids, const uint32_t* ind_code, uint32_t epoch,
                                               const uint32_t* d_epoch, int32_t num_ind, uint32_t ind_mask, float* dw,
                                               int32_t dw_ld, int32_t n, const int32_t* d_n, int32_t f_out,
                                               int32_t accumulate, void* workspace, grapes_stream_t stream);
/* Several of these weight-gradient GEMMs in ONE launch + one slab sum (new design; main.py:271-283's backward reaches the sampler
 * net's first layer once per hop and the log-Z net's once, all over rows of the same X).  Problems q = 0..count-1 (count <= 4): HOST
 * arrays of dh / ids / ind_code / num_ind / ind_mask / dw / dw_ld / n / d_n / accumulate with the meaning of the one-problem entry
 * point.  Problems that name the same dw are summed into it together (same num_ind and layout; accumulate = the first one's).  The
 * slab budget is dealt out on the DEVICE by the live row counts.  Available when grapes_..._multi_available(f_out, k_pad) says so
 * for every problem's k_pad (f_out in (128, 256], k_pad mod 256 in (0, 128]: the tile shape this launch has); workspace:
 * ..._multi_workspace_bytes(distinct dw pointers, largest k_pad, f_out), 16-byte aligned. */
int32_t grapes_linear_bwd_weight_gathered_split_multi_available(int32_t f_out, int32_t k_pad);
size_t grapes_linear_bwd_weight_gathered_split_multi_workspace_bytes(int32_t outputs, int32_t k_pad_max, int32_t f_out);
int grapes_linear_bwd_weight_gathered_split_multi(int32_t count, const float* const* dh, const float* X, int32_t F,
                                                  int32_t x_stride, const int32_t* const* ids,
                                                  const uint32_t* const* ind_code, uint32_t epoch, const uint32_t* d_epoch,
                                                  const int32_t* num_ind, const uint32_t* ind_mask, float* const* dw,
                                                  const int32_t* dw_ld, const int32_t* n, const int32_t* const* d_n,
                                                  int32_t f_out, const int32_t* accumulate, void* workspace,
                                                  grapes_stream_t stream);
int grapes_linear_fwd_gathered_split(const float* X, int32_t F, int32_t x_stride, const int32_t* ids,
                                     const uint32_t* ind_code, uint32_t epoch, const uint32_t* d_epoch, int32_t num_ind,
                                     const void* w_image, float* h, int32_t n, const int32_t* d_n, int32_t f_out,
                                     grapes_stream_t stream);
/* The same transform for ONE or TWO nets over the same gathered rows (nprob = 2: the sampler net and the log-Z net at hop 0,
 * main.py:210 and main.py:227 — the second net finds the rows in L2) with a split tail: on 256 resident workgroups the units
 * (tiles x nets) that do not fill a whole round are cut along K into as many pieces as there are idle workgroups and their partial
 * tiles summed by a second launch, in piece order (Reddit: 597 tiles = three rounds for 2.33 -> 2.4; two nets x 182 tiles = two
 * rounds -> 1.5).  HOST arrays of nprob entries: ind_code / num_ind / w_image / h; the nets' K must cover the same number of
 * 32-wide steps.  A tile that is not cut equals grapes_linear_fwd_gathered_split's bit for bit; a cut tile differs by the order of
 * its K steps' additions (pieces summed in order: deterministic).  workspace: …_tail_workspace_bytes(f_out), 16-byte aligned. */
size_t grapes_linear_fwd_gathered_split_tail_workspace_bytes(int32_t f_out);
int grapes_linear_fwd_gathered_split_tail(const float* X, int32_t F, int32_t x_stride, const int32_t* ids, int32_t nprob,
                                          const uint32_t* const* ind_code, uint32_t epoch, const uint32_t* d_epoch,
                                          const int32_t* num_ind, const void* const* w_image, float* const* h, int32_t n,
                                          const int32_t* d_n, int32_t f_out, void* workspace, grapes_stream_t stream);
/* The same GEMM for FEW rows (the classifier's <= B + hops K rows, a small graph's frontier): 128-row tiles x slabs of K steps
 * on ~256 workgroups + the slabs' sum in index order (two launches) — a handful of tiles would otherwise walk the whole K alone
 * (Cora: 2.7k rows x K = 1436).  workspace: grapes_linear_fwd_gathered_split_k_workspace_bytes(n, ceil4(F + num_ind), f_out). */
size_t grapes_linear_fwd_gathered_split_k_workspace_bytes(int32_t n, int32_t kp, int32_t f_out);
int grapes_linear_fwd_gathered_split_k(const float* X, int32_t F, int32_t x_stride, const int32_t* ids,
                                       const uint32_t* ind_code, uint32_t epoch, const uint32_t* d_epoch, int32_t num_ind,
                                       const void* w_image, float* h, int32_t n, const int32_t* d_n, int32_t f_out,
                                       void* workspace, grapes_stream_t stream);
size_t grapes_linear_bwd_weight_gathered_split_workspace_bytes(int32_t k_pad, int32_t f_out);
int grapes_linear_bwd_weight_gathered_split(const float* dh, const float* X, int32_t F, int32_t x_stride,
                                            const int32_t* ids, const uint32_t* ind_code, uint32_t epoch,
                                            const uint32_t* d_epoch, int32_t num_ind, uint32_t ind_mask, float* dw,
                                            int32_t n, const int32_t* d_n, int32_t f_out, int32_t accumulate,
                                            void* workspace, grapes_stream_t stream);

/* ------------------------------------------------------------------ N3: ingest, edge_index -> CSR
 * main.py:134-136  adjacency = sp.csr_matrix((ones(E, bool), edge_index), (N, N)): duplicate (row, col) pairs collapse, the
 * columns of a row ascend, self-loops stay.  Counting placement (one atomic per edge) + per-row sort / de-duplication in
 * LDS windows (hub rows in place in global memory) + a scan; 64-bit offsets (ogbn-papers100M: 3.2e9 symmetrised edges).
 * edge_src / edge_dst: int64[num_edges] (torch.long edge_index rows); rowptr int64[num_nodes + 1]; col int32 with capacity
 * num_edges; *d_nnz (device) = stored entries.  Ids outside [0, num_nodes) are skipped and raise GRAPES_STATUS_BAD_INDEX.
 * workspace: grapes_csr_build_workspace_bytes, 256-byte aligned.  Not for use inside a stream capture. */
size_t grapes_csr_build_workspace_bytes(int64_t num_edges, int32_t num_nodes);
int grapes_csr_build(const int64_t* edge_src, const int64_t* edge_dst, int64_t num_edges, int32_t num_nodes,
                     int64_t* rowptr, int32_t* col, int64_t* d_nnz, void* workspace, int32_t* status,
                     grapes_stream_t stream);

/* ------------------------------------------------------------------ N1 above 2^31 entries: full-batch message passing over a
 * graph whose CSR needs 64-bit offsets (ogbn-papers100M: 3.2e9 symmetrised entries).  The int32 forms above
 * (grapes_gcn_prepare_from_csr, grapes_gcn_aggregate_fwd[_prescaled]) stay the path below 2^31; these read the graph's own
 * int64 rowptr / int32 col in place (no edge-list copy).  Replace, for such graphs: eval.py:47-70 (evaluate(full_batch=True))
 * and modules/gcn.py:32,36 (the GCNConv calls of GCN.forward on the whole adjacency, inference only).
 *
 * Symmetry check: *d_flag = 0 when every stored (r, c) with r != c has a stored (c, r) (binary search; columns ascend), bit 1
 * when one is missing, bit 2 when a column id is outside [0, n).  The CSR by target is then the graph itself. */
int grapes_csr_symmetric_check(const int64_t* rowptr, const int32_t* col, int32_t n, int32_t* d_flag, grapes_stream_t stream);
/* Transpose (r, c) -> (c, r) of a device CSR (the CSR by target of a directed graph): counting placement + the per-row sort of
 * grapes_csr_build (rows ascend, duplicates collapse).  rowptr_t int64[N+1], col_t int32[capacity nnz]; workspace:
 * grapes_csr_build_workspace_bytes(nnz, N), 256-byte aligned.  Not for use inside a stream capture. */
int grapes_csr_transpose(const int64_t* rowptr, const int32_t* col, int64_t nnz, int32_t num_nodes, int64_t* rowptr_t,
                         int32_t* col_t, void* workspace, int32_t* status, grapes_stream_t stream);
/* gcn_norm over the CSR by target (rowptr_t int64, col_t int32): dinv[r] = (1 + #entries of row r other than r)^-1/2 (stored
 * self-loops are skipped, the unit loop added: PyG's self-loop replacement) and *d_items (int64, device) = the number of
 * hub-row work items of the whole graph — rows with more than `chunk` entries (a multiple of 64), one item per `chunk` —
 * the item_cap that bounds every grapes_gcn_large_aggregate launch over distinct rows with the same chunk. */
int grapes_gcn_large_prepare(const int64_t* rowptr_t, const int32_t* col_t, int32_t n, int32_t chunk, float* dinv,
                             int64_t* d_items, grapes_stream_t stream);
/* out[i, :f] = dinv[r] (sum_{s in row r, s != r} w_s h[s] + w_r h[r]) + bias (+ReLU), r = rows ? rows[i] : r0 + i, i < m:
 * prescaled != 0 — h's rows are pre-scaled by their own dinv (w = 1, as grapes_gcn_aggregate_fwd_prescaled); else w_s = dinv[s].
 * One wavefront per row; rows with more than `chunk` entries are cut into items (one workgroup each, partials in `workspace`)
 * added in chunk order: two runs give bit-identical output.  f % 4 == 0, f <= 4096; ldh, ldo (row pitches in floats) >= f and
 * multiples of 4; h, out, bias 16-byte aligned; bias may be NULL.  item_cap: grapes_gcn_large_prepare's item count (0: every
 * row by its own wavefront); rows whose items no longer fit below item_cap (only a row list with repeats needs more) are
 * walked by their own wavefront — same value, another summation order — and raise GRAPES_STATUS_NODE_OVERFLOW in *status
 * (optional); no item slot is ever left unwritten.  workspace: grapes_gcn_large_aggregate_workspace_bytes, 256-byte aligned. */
size_t grapes_gcn_large_aggregate_workspace_bytes(int32_t m, int32_t item_cap, int32_t f);
int grapes_gcn_large_aggregate(const float* h, int64_t ldh, const int64_t* rowptr_t, const int32_t* col_t, const float* dinv,
                               int32_t prescaled, int32_t r0, const int32_t* rows, int32_t m, int32_t f, const float* bias,
                               int32_t relu, float* out, int64_t ldo, int32_t chunk, int32_t item_cap, void* workspace,
                               int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ full-batch training over the same graphs
 * Replace full-batch.py:100-105 (logits = gcn_c(x, edge_index) on the whole graph, loss_fn on the train rows, backward) for a
 * two-layer GCN, row-blocked with 64-bit offsets (grapes_amd/full_graph.py train_step).  Deterministic: fixed summation orders,
 * no float atomics.
 *
 * Row-list transpose of the CSR by target restricted to rows[0..m) (ascending, distinct): for rows[p] = r the entries (s, p) are
 * every stored s of row r with s != r, plus (r, p) (the unit self-loop).  Output, per source s that has any, in ascending s:
 * srcs[j] = s (capacity num_nodes), its entries' positions p ascending in pos[src_off[j] .. src_off[j+1]) (src_off capacity
 * num_nodes + 1; pos capacity e_cap), counts[0] = sources, counts[1] = entries (int64, device).  e_cap must be at least
 * sum over rows of (row length + 1).  workspace: grapes_rowlist_transpose_workspace_bytes(e_cap, num_nodes), 256-byte aligned. */
size_t grapes_rowlist_transpose_workspace_bytes(int64_t e_cap, int32_t num_nodes);
int grapes_rowlist_transpose(const int64_t* rowptr_t, const int32_t* col_t, int32_t num_nodes, const int32_t* rows, int32_t m,
                             int64_t e_cap, int32_t* srcs, int64_t* src_off, int32_t* pos, int64_t* counts, void* workspace,
                             int32_t* status, grapes_stream_t stream);
/* Transposed gather over that structure (the backward of the last aggregation on the loss rows):
 * out[j, :f] = dinv[srcs[j]] * sum_{k in [src_off[j], src_off[j+1])} g[pos[k], :f].  Sources with more than `chunk` entries are cut
 * into items (partials added in chunk order); item_cap >= 2 * entries / chunk + 1.  f % 4 == 0, ldg / ldo multiples of 4, g and
 * out 16-byte aligned; workspace: grapes_rowlist_gather_t_workspace_bytes(n_src, item_cap, f), 256-byte aligned. */
size_t grapes_rowlist_gather_t_workspace_bytes(int32_t n_src, int32_t item_cap, int32_t f);
int grapes_rowlist_gather_t(const float* g, int64_t ldg, const int32_t* srcs, const int64_t* src_off, const int32_t* pos,
                            const float* dinv, int32_t n_src, int32_t f, float* out, int64_t ldo, int32_t chunk, int32_t item_cap,
                            void* workspace, int32_t* status, grapes_stream_t stream);
/* Dropout (modules/gcn.py:33,37) on rows of an N x width matrix: y[i, c] = x[i, c] / (1 - p) if
 * philox_uniform(seed, offset, r * width + c) >= p else 0, r = rows ? rows[i] : r0 + i, c < f — the mask grapes_dropout_fwd
 * draws on the whole contiguous matrix, whatever the row block.  y may be x. */
int grapes_dropout_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int32_t r0, const int32_t* rows, int32_t m, int32_t f,
                        int64_t width, float p, uint64_t philox_seed, uint64_t philox_offset, grapes_stream_t stream);
/* full-batch.py:101 loss_fn(logits[train_mask], y[train_mask]) on m rows (z: their pre-dropout logits, row pitch ldz): dropout
 * with (p, seed, offset) on the N x C logits as grapes_dropout_rows draws it, then mean CrossEntropy (labels int64[N]) or mean
 * BCEWithLogits (labels_f fp32[N, C]).  *loss_out = the loss; g[i, c] = dinv[rows[i]] * dloss/dZ[i, c] (dropout's backward
 * applied; columns C .. ldg_cols - 1 written 0); dcol[c] = sum_i dloss/dZ[i, c] (the bias gradient), c < ldg_cols.
 * C <= ldg_cols <= 1024; g may be z.  workspace: grapes_rowlist_loss_workspace_bytes(m, ldg_cols), 256-byte aligned. */
size_t grapes_rowlist_loss_workspace_bytes(int32_t m, int32_t ldg_cols);
int grapes_rowlist_loss(const float* z, int64_t ldz, int32_t C, const int32_t* rows, int32_t m, const int64_t* labels,
                        const float* labels_f, const float* dinv, float p, uint64_t philox_seed, uint64_t philox_offset, float* g,
                        int64_t ldg, int32_t ldg_cols, float* dcol, float* loss_out, void* workspace, int32_t* status,
                        grapes_stream_t stream);

/* ------------------------------------------------------------------ GraphSAINT random-walk sampling (graphsaint.py:104)
 * GraphSAINTRandomWalkSampler(data, batch_size=B, walk_length=L) with num_steps 1, sample_coverage 0 (csrc/saint_kernels.hip).
 * Stream (seed, off), off = *d_philox_offset when non-NULL, else philox_offset: root b = (uint64(word b) * N) >> 32 of the raw
 * 32-bit Philox words (all 32 bits); walk b's step t uses philox_uniform(seed, off, B + b L + t) (24 bits, as torch.rand).
 * A step from v: v itself if deg(v) = 0, else col[rowptr[v] + min(int64(u * deg), deg - 1)], the product in fp32 (torch_cluster
 * random_walk, p = q = 1; the clamp only acts for deg > 2^24).  roots (int32[B]) / uniforms (fp32[B * L]), when non-NULL, replace
 * the draws (tests); a root outside [0, N) ORs GRAPES_STATUS_BAD_INDEX into status (required then) and walks from node 0.
 * ONE workgroup: walks int32[B, L + 1]; node_idx int32[>= B (L + 1)] = walks.view(-1).unique() (ascending), *d_count its size;
 * node_map[node_idx[i]] = i (other entries untouched: membership is node_map[v] < count && node_idx[node_map[v]] == v).
 * *d_philox_offset advances by ceil(B (L + 1) / 4).  B (L + 1) <= 16384. */
int grapes_saint_walk_nodes(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, int32_t B, int32_t L, const int32_t* roots, const float* uniforms, uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, int32_t* walks, int32_t* node_idx, int32_t* d_count, int32_t* node_map, int32_t* status, grapes_stream_t stream);
/* graphsaint.py:104 adj.saint_subgraph(node_idx): the induced subgraph on the *d_count (<= n_cap <= 16384) ids of node_idx with
 * node_map as written by grapes_saint_walk_nodes.  Edges (edge_src[k], edge_dst[k]) = (local row, local column) in CSR order —
 * local row ascending, then the graph's column order (ascending for a sorted CSR); stored self-loops stay.  rowptr_l
 * int32[n_cap + 1]: the local row pointers (rows at or past the count are empty).  *d_e = min(edges, e_cap); more than e_cap
 * edges ORs GRAPES_STATUS_EDGE_OVERFLOW into status and only the first e_cap are written.  Every edge's origin, when wanted (all
 * three NULL: not formed): edge_id[p] = j (int64[e_cap], may be NULL on its own), the position in col of the entry that became edge
 * p, and, with GraphSAINT's table edge_norm (fp32[nnz], grapes_saint_norms), edge_norm_b[p] = edge_norm[j] (fp32[e_cap]; both NULL or
 * both given) — written at the same slot p as edge_src / edge_dst, nothing at or past e_cap.  Three launches (per-row counts,
 * one-workgroup scan, per-row writes).  workspace: grapes_saint_subgraph_workspace_bytes(n_cap), 4-byte aligned. */
size_t grapes_saint_subgraph_workspace_bytes(int32_t n_cap);
int grapes_saint_subgraph(const int64_t* rowptr, const int32_t* col, const int32_t* node_idx, const int32_t* d_count, const int32_t* node_map, int32_t n_cap, int32_t e_cap, int32_t* rowptr_l, int32_t* edge_src, int32_t* edge_dst, int32_t* d_e, int64_t* edge_id, const float* edge_norm, float* edge_norm_b, void* workspace, int32_t* status, grapes_stream_t stream);
/* graphsaint.py:31-34 loss_fn(out[0][train_idx], y[train_idx]), train_idx = batch.train_mask.nonzero(): over rows i < *d_count of
 * the batch logits z [n_cap, ldz] (row i = node node_idx[i]) with train_mask[node_idx[i]] != 0 (uint8 / bool [N]), T of them
 * (counted on the device; *d_train = T when non-NULL).  rowloss is CrossEntropy (labels int64[N]) or the mean over the C columns
 * of the BCEWithLogits elements (labels_f fp32[N, C]); exactly one of the two is given.
 *   node_norm NULL: the mean — *loss_out = sum of rowloss / T, g [n_cap, ldg] = d loss / d z (0 on other rows).  T = 0:
 *     *loss_out = NaN and g = 0 (torch's mean over an empty selection).
 *   node_norm (fp32[N], read through node_idx like train_mask; grapes_saint_norms): the normalised step's loss — *loss_out = sum
 *     over the training rows i of node_norm[node_idx[i]] * rowloss_i, a sum, not divided by T; g row i = w_i (softmax - onehot) or
 *     w_i (sigmoid(z) - y) / C.  T = 0: *loss_out = 0 and g = 0.
 * A label outside [0, C) ORs GRAPES_STATUS_BAD_INDEX into status and the row counts nothing.  ONE workgroup, fixed summation
 * order, no float atomics. */
int grapes_saint_masked_loss(const float* z, int64_t ldz, int32_t C, const int32_t* node_idx, const int32_t* d_count, int32_t n_cap, const uint8_t* train_mask, const float* node_norm, const int64_t* labels, const float* labels_f, float* g, int64_t ldg, float* loss_out, int32_t* d_train, int32_t* status, grapes_stream_t stream);
/* GraphSAINT's other two samplers (the reference imports GraphSAINTNodeSampler at graphsaint.py:8; PyG 2.5 loader/graph_saint.py).
 * The one-time weight table of GraphSAINTEdgeSampler: the weight of the stored entry (r, c) is colcount[r] + rowcount[c] (PyG:
 * prob = 1 / deg_in[row] + 1 / deg_out[col] with deg_in = 1 / colcount, deg_out = 1 / rowcount), an integer below 2^32.
 * colcount int32[N]: entries per column (zeroed here, then int32 atomic adds).  blockw int64[(nnz >> 6) + N]: row r owns the slots
 * from (rowptr[r] >> 6) + r on, one per 64-entry block of the row, holding the inclusive prefix of the block weights inside the row
 * (slots no row owns are left as they are).  roww int64[N + 1]: exclusive prefix of the row weights; roww[N] = the total weight.
 * A column outside [0, N) weighs 0 and ORs GRAPES_STATUS_BAD_INDEX into status.  nnz < 2^31.  Four launches, stream-ordered. */
int grapes_saint_edge_weights(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, int64_t nnz, int32_t* colcount, int64_t* blockw, int64_t* roww, int32_t* status, grapes_stream_t stream);
/* One batch of GraphSAINTNodeSampler (roww == NULL: PyG adj.storage.row()[randint(0, E, (B,))]) or GraphSAINTEdgeSampler (colcount /
 * blockw / roww of grapes_saint_edge_weights: PyG's top-1 of rand(B, E).log() / prob per row, i.e. one weighted draw per row).
 * Draw b: t = draws[b] when draws != NULL (a value outside [0, total) ORs GRAPES_STATUS_BAD_INDEX and draws entry 0's row), else
 * t = mulhi64(word, total), word = (stream word 2b) << 32 | (stream word 2b + 1) of the stream (seed, off), off = *d_philox_offset
 * when non-NULL; total = rowptr[N] (node) or roww[N] (edge), read on the device.  Node: ids[b] = the row holding entry t,
 * entries[b] = t.  Edge: entries[b] = the entry e whose weight interval holds t, ids[2b] = its row, ids[2b + 1] = its column.
 * Then node_idx / *d_count / node_map as grapes_saint_walk_nodes writes them, over the B (node) or 2 B (edge) ids (<= 16384).
 * *d_philox_offset advances by ceil(2 B / 4).  Two launches: one wavefront per draw, then one workgroup. */
int grapes_saint_draw_nodes(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, int32_t B, const int32_t* colcount, const int64_t* blockw, const int64_t* roww, const int64_t* draws, uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, int32_t* ids, int64_t* entries, int32_t* node_idx, int32_t* d_count, int32_t* node_map, int32_t* status, grapes_stream_t stream);
/* GraphSAINT's normalisation (sample_coverage > 0) [PyG-recall: PyG 2.5 GraphSAINTSampler._compute_norm / __collate__ and
 * examples/graph_saint.py].  Stored entry j is position j of col; row(j) is the CSR row (the source) that holds it.
 * One drawn batch's share of the coverage counts: node_count[v] += 1 (uint32[N]) for every v of the node set (node_idx / *d_count /
 * node_map as the draw wrote them), edge_count[j] += 1 (uint32[nnz]) for every stored entry j whose row and column are both in the
 * set (stored loops and duplicate entries are each their own j), *d_total += the set's size (int64, on the device).  The caller
 * zeroes the three before the first batch.  One wavefront per local row; every v and every j is touched by one thread and batches
 * are serial on the stream, so there are no atomics and the counts are exact and deterministic.  The subgraph is not formed and
 * nothing is read back.  One launch. */
int grapes_saint_coverage_count(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* node_idx, const int32_t* d_count, const int32_t* node_map, int32_t n_cap, uint32_t* node_count, uint32_t* edge_count, int64_t* d_total, grapes_stream_t stream);
/* The two norm vectors from the counts of num_samples batches:
 *   edge_norm[j] = fp32(node_count[row(j)]) / fp32(edge_count[j]) clamped to [0, 1e4]; a NaN (0 / 0) becomes 0.1, so x / 0 with
 *     x > 0 gives 1e4;
 *   node_norm[v] = (fp32(num_samples) / c) / fp32(N), c = fp32(node_count[v]), or 0.1 where the count is 0.
 * One wavefront per CSR row, rows shorter and longer than a wavefront alike.  One launch. */
int grapes_saint_norms(const int64_t* rowptr, int32_t num_nodes, const uint32_t* node_count, const uint32_t* edge_count, int64_t num_samples, float* edge_norm, float* node_norm, grapes_stream_t stream);

/* ------------------------------------------------------------------ LADIES / FastGCN layer-wise importance sampling
 * (csrc/ladies_kernels.hip) [LADIES-recall: acbull/LADIES pytorch_ladies.py].  V = A + I over the CSR (rowptr int64[N + 1], col
 * int32, ascending, duplicate-free; a stored (i, i) makes v_ii = 2), P = D^-1 V, D_i = (rowptr[i + 1] - rowptr[i]) + 1.
 * The importance of n candidates [LADIES-recall: ladies_sampler, `pi = np.array(np.sum(U.multiply(U), axis=0))[0]` with
 * U = lap_matrix[previous_nodes, :]; fastgcn_sampler, the same over every row of lap_matrix]:
 *   pi[k] = sum over the rows i of the set of P_ij^2, j = ids[k] (ids NULL: j = k); logit[k] = logf(pi[k]) - C with
 *   C = 20 + logf(float(m)) — the shifted logits the existing draw (grapes_gumbel_topk*, mode 0) takes: there log sigmoid(l) = l in
 *   fp32, so its exact-k Gumbel draw samples without replacement in proportion to pi; pi_table[j] = pi[k] when given (fp32[N]; only
 *   candidates are written).
 * The set is the bitmap prev_bits (uint64[ceil(N / 64)], bit v & 63 of word v >> 6) of m (*d_m) rows, or every row (prev_bits NULL;
 * pass m = N).  rowptr_t / col_t: the CSR of the transpose (the graph's own arrays when it is symmetric); rowptr gives D_i.
 * n / d_n, m / d_m: capacity and optional device count, as everywhere; entries at or past *d_n are not written.  One wavefront per
 * candidate walks row j of the transpose 64 entries per trip (long rows by the same loop), lane-strided partial sums, a butterfly,
 * then the diagonal term (v_jj / D_j)^2 when j is in the set: a fixed order, no atomics.  An id outside [0, N) raises
 * GRAPES_STATUS_BAD_INDEX (its pi is 0, its logit -inf).  One launch. */
int grapes_ladies_importance(const int64_t* rowptr, const int64_t* rowptr_t, const int32_t* col_t, int32_t num_nodes, const int32_t* ids, int32_t n, const int32_t* d_n, const uint64_t* prev_bits, int32_t m, const int32_t* d_m, float* pi, float* logit, float* pi_table, int32_t* status, grapes_stream_t stream);
/* One layer's reweighted, row-normalised slice [LADIES-recall: ladies_sampler, `adj = U[:, after_nodes].multiply(1 / p[after_nodes])`
 * then `row_normalize(adj)`]: for the rows i = rows[r], r < m (*d_m), in that order, and within a row for ascending j, every
 * (i, j) with v_ij > 0 and j in keep_bits (the bitmap of the kept columns): edge_src[e] = j, edge_dst[e] = i (global ids),
 * weight[e] = (v_ij / pi_table[j]) / sum over the row's kept j' of v_ij' / pi_table[j'].  The diagonal entry sits at its sorted
 * place, a stored loop folded into it (v = 2).  A row without a kept column has no entries.  *d_e = the entry count; more than e_cap
 * raise GRAPES_STATUS_EDGE_OVERFLOW, *d_e = e_cap and nothing past e_cap is written.  An id outside [0, N) raises
 * GRAPES_STATUS_BAD_INDEX and is dropped.  Count, one-workgroup scan, write: three launches; the row sums in the importance's fixed
 * order.  workspace: grapes_ladies_layer_workspace_bytes(m), 4-byte aligned. */
size_t grapes_ladies_layer_workspace_bytes(int32_t m);
int grapes_ladies_layer(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m, const int32_t* d_m, const uint64_t* keep_bits, const float* pi_table, int32_t e_cap, int32_t* edge_src, int32_t* edge_dst, float* weight, int32_t* d_e, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ AS-GCN: the adaptive layer-wise sampler and its variance loss
 * (csrc/asgcn_kernels.hip) [AS-GCN-recall: Huang et al., "Adaptive Sampling Towards Fast Graph Representation Learning", NeurIPS
 * 2018; the layer-wise sampler with the self-dependent function g(x(u_j))], on the LADIES conventions above (V, P, D, the set as a
 * bitmap or every row, the transpose CSR, n / d_n, the status bits).  The sampler's parameters: w_g fp32[f], b_g fp32[1] (device).
 * For the n candidates j = ids[k] (ids NULL: j = k), with x fp32[N, f] whose rows are ldx >= f floats apart:
 *   c[k] = sum over the rows i of the set of P_ij (the column mass, > 0 for a candidate);  a[k] = <x_j, w_g> + b_g;
 *   g = max(a, 0) + 1;  q[k] = c g;  logq[k] = logf(q);  logit[k] = (logq[k] - M) - 20 with M = max over the live k of logq, exactly
 *   those two fp32 roundings: logit <= -20, where the existing draw (grapes_gumbel_topk*, mode 0) samples without replacement in
 *   proportion to q.  q_table[j] = q[k], a_table[j] = a[k] when given (fp32[N]; only candidates are written).
 * One wavefront per candidate: the transpose-row walk of grapes_ladies_importance (64 entries per trip, lane-strided partial sums, a
 * butterfly, the diagonal term last) and in the same wavefront the lane-strided dot product over the feature row — 16-byte loads
 * when f % 4 == 0, ldx % 4 == 0 and x and w_g are 16-byte aligned, scalar loads otherwise; any f >= 1.  Then one workgroup takes
 * the maximum and writes logit: two launches, a fixed order, no atomics — two calls give the same bits.  m / d_m are accepted as
 * grapes_ladies_importance takes them (m >= 1) and not read: the shift is the layer's maximum.  An id outside [0, N) raises
 * GRAPES_STATUS_BAD_INDEX (c = a = q = 0, logq = logit = -inf); entries at or past *d_n are not written. */
int grapes_asgcn_importance(const int64_t* rowptr, const int64_t* rowptr_t, const int32_t* col_t, int32_t num_nodes, const int32_t* ids, int32_t n, const int32_t* d_n, const uint64_t* prev_bits, int32_t m, const int32_t* d_m, const float* x, int64_t ldx, int32_t f, const float* w_g, const float* b_g, float* c, float* a, float* q, float* logq, float* logit, float* q_table, float* a_table, int32_t* status, grapes_stream_t stream);
/* The two calls below run over ONE layer's entry list in grapes_ladies_layer's order with LOCAL ids (the batch's ranks, below
 * n_local): e entries (edge_src[t] = j, edge_dst[t] = i, weight[t] = w_ij), row-contiguous, a row's sources ascending, and
 * rows int32[m] = the layer's rows in the list's order (distinct; a row may have no entry).  A small launch of their own finds each
 * row's offsets from the runs of edge_dst (not from a WeightedStructure's CSR, where the diagonal entry is no entry): the diagonal
 * is an ordinary entry here.  An id outside [0, n_local), or a target that is none of the rows, raises GRAPES_STATUS_BAD_INDEX and
 * is left out.  workspace: grapes_asgcn_rows_workspace_bytes(m, n_local), 4-byte aligned.
 * The variance term over h fp32[n_local, c] (the layer's transformed input, a constant here), s_i = the entries of row i:
 *   mu_i = sum_j w_ij h_j;  v[r] = s_i sum_j w_ij^2 |h_j|^2 - |mu_i|^2 (0 for a row without an entry);  l_var[0] = (sum_r v[r]) / m
 *   in a fixed order;  dw[t] = (2 / m) (s_i w_ij |h_j|^2 - <mu_i, h_j>), the gradient of l_var by the weights.
 * Widths: any c <= 256, multiples of 4 up to 1024.  One wavefront per row whatever its length, looping in batches: a first sweep
 * for mu_i, a second for the entries; lanes are (entry slot, channel) so that a narrow h fills the wavefront.  Four launches. */
size_t grapes_asgcn_rows_workspace_bytes(int32_t m, int32_t n_local);
int grapes_asgcn_variance(const int32_t* edge_src, const int32_t* edge_dst, const float* weight, int32_t e, const int32_t* rows, int32_t m, const float* h, int32_t n_local, int32_t c, float* v, float* l_var, float* dw, void* workspace, int32_t* status, grapes_stream_t stream);
/* d L / d logq from g[t] = d L / d w_ij: Gbar_i = sum_j g_ij w_ij per row, then t[j] += sum over the rows i, in the list's row order,
 * of w_ij (g_ij - Gbar_i) for every j < n_local (t fp32[n_local] is accumulated into: one array serves every layer of a batch);
 * d L / d logq_j = -t[j].  One wavefront per row for the means, one per column for the sums (lane l takes the rows l, l + 64, ...
 * and finds j in each by a binary search): a fixed order, no float atomics.  Four launches. */
int grapes_asgcn_logq_bwd(const int32_t* edge_src, const int32_t* edge_dst, const float* weight, const float* g, int32_t e, const int32_t* rows, int32_t m, int32_t n_local, float* t, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ GraphSAGE: the node-wise neighbour sampler and SAGEConv's
 * aggregation (csrc/sage_kernels.hip) [Hamilton et al., NeurIPS 2017; PyG-recall: torch_geometric 2.5.2 SAGEConv, NeighborLoader].
 * The sampler: for the rows i = rows[r], r < m (*d_m), of the CSR (rowptr int64[N + 1], col int32) keep min(deg_i, fanout) entries of
 * row i, uniformly without replacement, 1 <= fanout <= 64.  The rule (bit-reproducible on a CPU):
 *   off_r = the exclusive prefix over r, in list order, of deg(rows[r]); entry t of list row r has stream position p = off_r + t;
 *   its key is keys[p] when keys (uint32[n_keys]) is given, else raw 32-bit word p of the Philox stream (seed, off), off =
 *   *d_philox_offset when given else philox_offset: word p & 3 of philox4x32_10(off + p / 4, seed), as grapes_saint_draw_nodes
 *   indexes words;
 *   list row r keeps its min(deg, fanout) entries with the smallest composite (key << 32) | t — unique, so a tie in the word goes to
 *   the lower position and nothing depends on scheduling;
 *   kept entries are written for r ascending and within a row for t ascending: edge_src[e] = col entry (the neighbour), edge_dst[e] =
 *   the row (global ids: the direction of slice_adjacency and grapes_ladies_layer), edge_pos[e] = the entry's position in col
 *   (int64; edge_pos may be NULL);  *d_e = sum of min(deg, fanout).
 * A row listed twice draws twice, independently (its p differs).  A row with deg <= fanout keeps everything; its words are skipped
 * all the same, so p is the same on every path.  *d_philox_offset advances by ceil(sum deg / 4) (with keys too).  A row id outside
 * [0, N) raises GRAPES_STATUS_BAD_INDEX and is dropped (an empty row).  A column outside [0, N) raises it too and is dropped: its
 * slot holds -1 in edge_src, edge_dst and edge_pos, so that the list's layout never depends on the data.  A stream position at or
 * past n_keys raises it as well (key 0xffffffff).  More than e_cap entries raise GRAPES_STATUS_EDGE_OVERFLOW, *d_e = e_cap and
 * nothing is written past e_cap.  Positions are 64-bit on the device; a caller that knows sum deg refuses 2^31 or more
 * (ops.sage_sample_layer does).  Rows at or past *d_m write nothing.
 * Two launches.  One workgroup: the degrees, both prefixes, the count, the offset's advance.  Then one wavefront per list row:
 * deg <= fanout is a copy; deg <= 64 ranks one key per lane by broadcast compares in registers; a longer row is walked 256 stream
 * positions per trip (a lane takes the four words of one Philox call) by an 8-bit radix select on the word — a pass counts one digit
 * of the entries that match the prefix found so far in a wavefront-private 256-bin LDS histogram; once the entries at or below the
 * prefix fit 128 slots (after one pass for rows of up to about 16 000 entries) one more pass lists them in order and the row ends in
 * registers; words that tie beyond that take four passes and a fifth that writes every word below the threshold and the first
 * positions that equal it.  Two to five generations of a row's keys: linear in deg, no sort, nothing through global memory, no float
 * arithmetic.  workspace: grapes_sage_sample_layer_workspace_bytes(m), 8-byte aligned. */
size_t grapes_sage_sample_layer_workspace_bytes(int32_t m);
int grapes_sage_sample_layer(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m, const int32_t* d_m, int32_t fanout, const uint32_t* keys, int64_t n_keys, uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, int32_t e_cap, int32_t* edge_src, int32_t* edge_dst, int64_t* edge_pos, int32_t* d_e, void* workspace, int32_t* status, grapes_stream_t stream);
/* The aggregation SAGEConv and ClusterGCNConv share, over the CSRs grapes_gcn_prepare builds, used as stored: duplicate entries
 * count by multiplicity, and the stored self-loops the build drops come back through loops[i] (grapes_gcn2_loop_counts; NULL: none):
 *   out[i, :f] = act(s_i (sum_{j in row i of the by-target CSR} src[j, :f] + c_i src[i, :f]) + add[i, :f] + bias)
 *   c_i = loops[i] + (self_term != 0 ? self_weight : 0);  deg_i = (rowptr_t[i + 1] - rowptr_t[i]) + loops[i];
 *   s_i = 1 (scale = GRAPES_ROOTSUM_SCALE_NONE), 1 / deg_i (_MEAN; an empty row aggregates to 0) or 1 / (1 + deg_i) (_MEAN_PLUS_ONE);
 *   any other scale is GRAPES_EINVAL.
 * SAGEConv: the stored loops, self_term = 0, _MEAN (mean) or _NONE (sum) — no self-loop is added.  ClusterGCNConv [PyG-recall:
 * remove_self_loops followed by add_self_loops]: loops = NULL, self_term = 1 with self_weight = 1 + diag_lambda, _MEAN_PLUS_ONE.
 * The self term is computed whenever self_term != 0, whatever self_weight holds (0 still multiplies src[i]), and src[i] is not
 * read for it otherwise.  In fp32: p = the row's sum in entry order, p = fma(loops[i], src[i], p), p = fma(self_weight, src[i], p),
 * o = p s_i, o += add, o += bias, ReLU.
 * The scale is applied once per row: there is no per-edge weight.  add, bias and the ReLU (relu != 0) are optional.  copy_out
 * (optional): copy_out[i, :f] = src[i, :f], the root operand beside the aggregate in the aggregate-first form.  src, add, out and
 * copy_out are row-major with their own leading dimensions (ld_* >= f floats), so column blocks of one GEMM output are used in
 * place; out and copy_out must not alias src.  Widths: any f <= 256; up to 1024 when f % 4 == 0 and every matrix is 16-byte
 * aligned with ld % 4 == 0 (float4 columns), else GRAPES_EALIGN / GRAPES_EINVAL.  long_items / d_n_items / item_cap / workspace as
 * grapes_gcn2_propagate_fwd (NULL: every row by one group of lanes): rows longer than GRAPES_LONG_ROW are cut into items whose
 * partial sums are merged in chunk order.  Every sum has a fixed order, no floating-point atomics: two runs give the same bits.
 * status: GRAPES_STATUS_BAD_INDEX when a CSR entry is outside [0, n) (the entry is dropped).
 * workspace: grapes_rootsum_aggregate_workspace_bytes(0, item_cap, f) for the forward, (n, item_cap, f) for the backward; 16-byte
 * aligned. */
#define GRAPES_ROOTSUM_SCALE_NONE 0
#define GRAPES_ROOTSUM_SCALE_MEAN 1
#define GRAPES_ROOTSUM_SCALE_MEAN_PLUS_ONE 2
size_t grapes_rootsum_aggregate_workspace_bytes(int32_t n, int32_t item_cap, int32_t f);
int grapes_rootsum_aggregate_fwd(const float* src, int64_t ld_src, const float* add, int64_t ld_add, const float* bias, const int32_t* loops, const int32_t* rowptr_t, const int32_t* csr_src, float self_weight, int32_t self_term, int32_t scale, int32_t relu, float* out, int64_t ld_out, float* copy_out, int64_t ld_copy, int32_t n, const int32_t* d_n, int32_t f, const int32_t* long_items, const int32_t* d_n_items, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);
/* Backward of the above.  g = dout, gated by relu_out > 0 when relu_out (the forward's output) is given:
 *   dsrc[j] = sum_{i in row j of the by-source CSR} s_i g_i + c_j s_j g_j (+ add[j]);   dadd = g;   dbias = column sums of g.
 * One row-local pass writes dadd, the pre-scaled rows s g and per-128-row partial column sums (added in a fixed order by a second
 * launch); dsrc is then the forward's gather over rowptr_s / csr_dst on the pre-scaled rows with scale = _NONE and the caller's
 * loops, self_weight and self_term, with the by-source items.  The pass is left out when nothing needs it (scale = _NONE, no gate,
 * no dadd, no dbias): dsrc gathers dout itself.  add (optional) is a gradient that reaches the source rows directly (the root half
 * of the aggregate-first form).  dsrc, dadd and dbias may each be NULL; dsrc and dadd must not alias dout.  s_i always comes from
 * the by-target row pointers rowptr_t.  workspace: required unless the pass is left out and there are no items. */
int grapes_rootsum_aggregate_bwd(const float* dout, int64_t ld_dout, const float* relu_out, int64_t ld_relu, const int32_t* loops, const int32_t* rowptr_t, const int32_t* rowptr_s, const int32_t* csr_dst, float self_weight, int32_t self_term, int32_t scale, const float* add, int64_t ld_add, float* dsrc, int64_t ld_dsrc, float* dadd, int64_t ld_dadd, float* dbias, int32_t n, const int32_t* d_n, int32_t f, const int32_t* items_s, const int32_t* d_n_items_s, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ VR-GCN: the control-variate aggregation over historical
 * activations (csrc/vrgcn_kernels.hip) [Chen, Zhu and Song, ICML 2018].  The graph is a loop-free CSR (rowptr int64[N + 1], col
 * int32) with d_u stored entries in row u and dinv[u] = (d_u + 1)^-1/2 (float[N], the caller's table); a batch has n_local nodes,
 * node_idx[local id] = global id.  h [n_local, f] is the layer's input on local rows, hbar [N, f] its history on GLOBAL rows, read in
 * place.  For the m listed rows (u = rows_g[r], its local id rows_l[r]) and the layer's kept entries as the by-target CSR
 * grapes_gcn_prepare builds over the batch's local ids (rowptr_k int32[n_local + 1], csr_k: row loc u holds the local ids of its
 * k_u kept sources):
 *   out[r] = dinv_u (dinv_u h[loc u] + (d_u / k_u) sum_{kept v} dinv_v (h[loc v] - hbar[v]) + sum_{every entry v of row u} dinv_v hbar[v])
 * coef (optional, float[m]) receives (d_u / k_u) dinv_u (0 for k_u = 0), the backward's per-row factor.  A group of lanes owns a row
 * and keeps one accumulator in registers across both walks; d_u / k_u and dinv_u are applied once per row.  item_cap > 0: rows
 * with more than grapes_vrgcn_long_row() entries (a multiple of GRAPES_LONG_ROW) are cut into chunks of that many entries, one
 * group each, whose partial sums are added in chunk order (four launches instead of one); item_cap bounds the chunks of the
 * listed long rows (at most 2^20; more raise GRAPES_STATUS_EDGE_OVERFLOW and the result is invalid); item_cap = 0: every row by
 * one group.  No float atomics: two runs give the same bits.  Widths as grapes_rootsum_aggregate_fwd: any f <= 256, up to 1024 when
 * f % 4 == 0 and h, hbar, out are 16-byte aligned with ld % 4 == 0, else GRAPES_EALIGN / GRAPES_EINVAL.  An index outside its table
 * (a listed row, a kept source, its node_idx, a column) raises GRAPES_STATUS_BAD_INDEX and is dropped (a bad listed row gives
 * zeros).  workspace: grapes_vrgcn_aggregate_workspace_bytes(m, item_cap, f), 16-byte aligned; may be NULL with item_cap = 0. */
int32_t grapes_vrgcn_long_row(void);
size_t grapes_vrgcn_aggregate_workspace_bytes(int32_t m, int32_t item_cap, int32_t f);
int grapes_vrgcn_aggregate_fwd(const float* h, int64_t ld_h, const int32_t* node_idx, int32_t n_local, const float* hbar, int64_t ld_hbar, const float* dinv, const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows_g, const int32_t* rows_l, int32_t m, const int32_t* rowptr_k, const int32_t* csr_k, float* out, int64_t ld_out, float* coef, int32_t f, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);
/* Backward of the above with hbar a constant, over the by-source CSR of the same preparation (rowptr_s int32[n_local + 1], csr_dst:
 * row loc v holds the local ids of the rows that kept v); pos[local id] = the list position r of that node or -1:
 *   dh[loc v] = dinv_v sum_{kept (u, v)} coef[pos[loc u]] da[pos[loc u]] + dinv_v^2 da[pos[loc v]]   (the self term for listed v only)
 * for every local row (rows nothing reaches get zeros).  One launch, a group per local row, entries in the CSR's order: no float
 * atomics, two runs give the same bits.  A target that is none of the listed rows raises GRAPES_STATUS_BAD_INDEX and is dropped. */
int grapes_vrgcn_aggregate_bwd(const float* da, int64_t ld_da, const float* coef, const int32_t* pos, const int32_t* node_idx, const float* dinv, int32_t num_nodes, const int32_t* rowptr_s, const int32_t* csr_dst, float* dh, int64_t ld_dh, int32_t n_local, int32_t m, int32_t f, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ GNNAutoScale, "GAS": cluster batches that pull out-of-batch
 * neighbours from histories (csrc/gas_kernels.hip) [Fey, Lenssen, Weichert and Leskovec, ICML 2021; pyg_autoscale-recall: ScalableGNN,
 * History, SubgraphLoader — recalled, not read: the rule below is the contract; tests/gas_oracle.py reproduces it].
 *   graph    a symmetric loop-free CSR (rowptr int64[N + 1], col int32, fewer than 2^31 entries, duplicates counting once each):
 *            d_u = the stored entries of row u, dinv[u] = (d_u + 1)^-1/2 (float[N], the caller's table), P = D^-1/2 (A + I) D^-1/2.
 *   batch    grapes_cluster_batch's over that graph: n rows in cluster order, node_idx[i] = the global id of row i.
 *   history  a model of L layers keeps for l = 1 .. L - 1 a table Hbar^(l), fp32 [N, hidden_l] on global rows, zero at first.
 *   resolve  once per batch, for every batch row i, u = node_idx[i], and every stored entry v at position t of row u, in the CSR's
 *            order: code[rowptr_h[i] + t] = the local row of v when v is in the batch (stamp[where[v].cluster].serial == serial:
 *            stamp[..].base + where[v].position, as grapes_cluster_batch), else -1 - v.  rowptr_h int32[n + 1] = the prefix sum of
 *            the batch rows' global degrees; counts int64[2] = the in-batch and the out-of-batch entries.
 *   level 1  exact, the history of X being X: Z1 = (P X)[node_idx] W1^T + b1, P X computed once.
 *   level l + 1 >= 2, H = H^(l) [n, f] on local rows, Hbar = Hbar^(l) a constant for autograd:
 *            A[i] = dinv_u (dinv_u H[i] + sum_{t in row i of rowptr_h} dinv_{v_t} (code_t >= 0 ? H[code_t] : Hbar[-1 - code_t])),
 *            Z = A W^T + b; dinv_{v_t} from the global table (v_t = node_idx[code_t] for an in-batch entry).
 *   backward over the by-source CSR of the batch's INDUCED entries (grapes_gcn_prepare over the batch's edge list) — exact for any
 *            stored multiset, the code list is not assumed to be its own transpose:
 *            dH[j] = dinv_{v_j} (dinv_{v_j} dA[j] + sum_{i in by-source row j} dinv_{u_i} dA[i]);  dHbar = none.
 *   push     after the step's forward, for every level: Hbar^(l)[node_idx] = H^(l) (post-ReLU, all n rows; grapes_scatter_rows).
 *            In-batch nodes never read their own history inside a step.
 * grapes_gas_resolve runs after grapes_cluster_batch with the same stamp (int32[P][2], 8-byte aligned, as `where`) and serial: one
 * launch scans the degrees, one runs a wavefront per 64 entries of a row and writes the codes one per lane.  Integers only.  e_cap
 * bounds the code list: a larger total ORs GRAPES_STATUS_EDGE_OVERFLOW, nothing is written at or past e_cap and rowptr_h[n] still
 * holds the TRUE total, so the caller can retry; item_cap (1 .. 2^24) bounds the sum over the batch rows of ceil(d / 64), more
 * raise the same bit.  A row id or column id outside [0, N), or a `where` entry outside its table (cluster outside [0, P), local
 * row outside [0, n)), ORs GRAPES_STATUS_BAD_INDEX; such an entry's code is 2^31 - 1, which the aggregation drops, and neither
 * count includes it.  The counts cover every entry, also those past e_cap.  workspace:
 * grapes_gas_resolve_workspace_bytes(n) bytes, 4-byte aligned; counts 8-byte aligned. */
size_t grapes_gas_resolve_workspace_bytes(int32_t n);
int grapes_gas_resolve(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* node_idx, int32_t n, const int32_t* where, const int32_t* stamp, int32_t num_parts, int32_t serial, int32_t e_cap, int32_t item_cap, int32_t* rowptr_h, int32_t* code, int64_t* counts, void* workspace, int32_t* status, grapes_stream_t stream);
/* out [n, f] = A of the rule above from h [n, f] and hbar [N, f], both read in place: no halo is materialised.  e = the entries of
 * `code` (offsets of rowptr_h beyond it are clamped).  A group of lanes owns a row and keeps one accumulator in registers over one
 * walk; the source table and row are selected from the code without a branch, so several source rows are in flight; dinv_u is
 * applied once per row.  item_cap > 0: rows with more than grapes_vrgcn_long_row() codes are cut into chunks of that many, one group
 * each, whose partial sums are added in chunk order (four launches instead of one); item_cap bounds the chunks of the long rows (at
 * most 2^20; more raise GRAPES_STATUS_EDGE_OVERFLOW and the result is invalid); item_cap = 0: every row by one group.  No float
 * atomics: two runs give the same bits.  Widths as grapes_rootsum_aggregate_fwd: any f <= 256, up to 1024 when f % 4 == 0 and h, hbar,
 * out are 16-byte aligned with ld % 4 == 0, else GRAPES_EALIGN / GRAPES_EINVAL.  A code outside [-N, n) (or a node_idx outside
 * [0, N)) raises GRAPES_STATUS_BAD_INDEX and is dropped.  workspace: grapes_gas_aggregate_workspace_bytes(n, item_cap, f), 16-byte
 * aligned; may be NULL with item_cap = 0. */
size_t grapes_gas_aggregate_workspace_bytes(int32_t n, int32_t item_cap, int32_t f);
int grapes_gas_aggregate_fwd(const float* h, int64_t ld_h, const float* hbar, int64_t ld_hbar, const float* dinv, int32_t num_nodes, const int32_t* node_idx, int32_t n, const int32_t* rowptr_h, const int32_t* code, int32_t e, float* out, int64_t ld_out, int32_t f, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);
/* dh [n, f] of the backward above from da = d A [n, f], over rowptr_s int32[n + 1] / csr_dst of the batch's prepared induced entries.
 * One launch, a group per local row, entries in the CSR's order: no float atomics, two runs give the same bits. */
int grapes_gas_aggregate_bwd(const float* da, int64_t ld_da, const int32_t* node_idx, const float* dinv, int32_t num_nodes, const int32_t* rowptr_s, const int32_t* csr_dst, float* dh, int64_t ld_dh, int32_t n, int32_t f, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ LABOR: the layer-neighbour sampler (csrc/labor_kernels.hip)
 * [Balin and Catalyurek, NeurIPS 2023; LABOR-recall: DGL's LaborSampler].  Neighbour sampling's per-row estimator with ONE variate
 * per candidate vertex, shared by every row that sees it.  For the rows s = rows[r], r < m (*d_m), of the CSR (rowptr int64[N + 1],
 * col int32), d_s = deg(s), fanout k >= 1, and every stored entry t of row s (duplicates are separate entries, a stored loop is an
 * ordinary entry; t is a GLOBAL node id):
 *   r_t = keys[t] when keys (uint32[N], one word per NODE) is given, else 32-bit word t & 3 of philox4x32_10(philox_base + (t >> 2),
 *   philox_seed): every row sees the same r_t for the same t;
 *   d_s <= k: every entry is kept, p_st = 1;
 *   c == pi == NULL (LABOR-0): entry t is kept iff (uint64) r_t * d_s < (uint64) k << 32 — probability k / d_s, integers only;
 *   c (float[m], per list row) and pi (float[N], per node) given: kept iff u_t < p_st with u_t = (r_t >> 8) * 2^-24 and
 *   p_st = fminf(1, c[r] * pi[t]), ONE fp32 multiply contracted with nothing: a CPU given the same c and pi keeps the same entries;
 *   edge_weight (optional): the Hajek weights w_st = (1 / p_st) / sum_{t' kept in row s} (1 / p_st') — LABOR-0: 1 / kept_s; a row's sum
 *   is formed per 64-entry chunk (a butterfly over the lanes) and over its chunks in chunk order, in fp32: two runs give the same bits;
 *   kept entries are written for r ascending and within a row in CSR order: edge_src[e] = t, edge_dst[e] = s, edge_pos[e] = the
 *   entry's position in col (int64; may be NULL); *d_e = their number.  A row that keeps nothing has no entry.
 * A work item is GRAPES_LONG_ROW = 64 consecutive entries of one list row, one per lane: a longer row is cut over several wavefronts
 * and its chunks' counts feed the same prefix as every other row's.  item_cap bounds the items, sum over the rows of ceil(d_s / 64)
 * (at most m + (sum d_s) / 64; up to 2^24): more raise GRAPES_STATUS_EDGE_OVERFLOW and the list is incomplete.  More than e_cap kept
 * entries raise it too, *d_e = e_cap and nothing is written past e_cap.  A row id outside [0, N) raises GRAPES_STATUS_BAD_INDEX and
 * counts as an empty row; a column outside [0, N) raises it and is never kept.  Rows at or past *d_m write nothing.
 * Four launches: one workgroup (the rows' chunk counts and their prefix), a wavefront per item (its kept lanes as a 64-bit mask — a
 * lane computes a Philox call only for the entry it tests), one workgroup (the prefix of the masks' popcounts, the count, the
 * overflow bit), a wavefront per item (the write).  workspace: grapes_labor_sample_layer_workspace_bytes(m, item_cap), 8-byte
 * aligned. */
size_t grapes_labor_sample_layer_workspace_bytes(int32_t m, int32_t item_cap);
int grapes_labor_sample_layer(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m, const int32_t* d_m, int32_t fanout, const uint32_t* keys, uint64_t philox_seed, uint64_t philox_base, const float* c, const float* pi, int32_t item_cap, int32_t e_cap, int32_t* edge_src, int32_t* edge_dst, int64_t* edge_pos, float* edge_weight, int32_t* d_e, void* workspace, int32_t* status, grapes_stream_t stream);
/* LABOR's importance iterations for one layer (0 <= iters <= 8), from pi = 1 on every column the rows touch:
 *   c_s(pi), for a row with d_s > k, solves sum_{t in N(s)} 1 / min(1, c pi_t) = d_s^2 / k (pi = 1: c_s = k / d_s);
 *   one iteration: pi_t <- pi_t * max_{s listed, d_s > k, t in N(s)} c_s(pi); rows with d_s <= k take no part, and a column that only
 *   they see keeps its pi;  after `iters` iterations c_s is solved once more for the final pi.
 * Writes c[r] (float[m]; 0 for a row with d_s <= k, whose p is 1) and pi[t] (float[N]) for every column t the rows touch; other
 * entries of pi are left alone.  c_s is solved without a sort by the monotone fixed point J = {}, c = (sum_{t not in J} 1 / pi_t) /
 * (d_s^2 / k - |J|), J <- {t : c pi_t >= 1}, until J stops growing (c never decreases; at most d_s rounds).  fp32; one wavefront per
 * row, every row sum in a fixed order; the maximum is an integer atomic max on the bit patterns of the positive floats: no float
 * atomics, two runs give the same bits.  workspace: grapes_labor_importance_workspace_bytes(N) bytes, a table of one word per node
 * that must be ZERO on entry and is zero again on return (as the DeviceGraph's bitmaps are).  1 + 2 iters + 1 launches.  Bad ids as
 * above (dropped, GRAPES_STATUS_BAD_INDEX). */
size_t grapes_labor_importance_workspace_bytes(int32_t num_nodes);
int grapes_labor_importance(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m, const int32_t* d_m, int32_t fanout, int32_t iters, float* c, float* pi, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ ShaDow-GNN: the per-root ego-net sampler (csrc/shadow_kernels.hip)
 * [Zeng et al., NeurIPS 2021; PyG-recall: ShaDowKHopSampler(data, depth, num_neighbors) over torch_sparse's ego_k_hop_sample_adj].
 * Every root gets its OWN sampled ego-net; the batch is the disjoint union of the ego-nets, in root order.  The rule (integers only,
 * bit-reproducible on a CPU):
 *   inputs   the CSR (rowptr int64[N + 1], col int32, fewer than 2^31 entries); roots[b], b < m (*d_m), 1 <= m <= 4096; depth >= 1;
 *            fanout k, 1 <= k <= 64, one value for every hop; C = 1 + k + k^2 + ... + k^depth <= 1024, the ego-net cap (more:
 *            GRAPES_EINVAL).
 *   hops     S_0 = F_0 = {root}.  Hop h = 1 .. depth expands every v in F_{h-1}, the nodes first reached at hop h - 1: deg(v) <= k
 *            keeps every entry of v's row; deg(v) > k keeps the entries at the positions Cset chosen by Floyd's algorithm below;
 *            S_h = S_{h-1} united with {col[rowptr[v] + t] : t in Cset} over the expanded v;  F_h = S_h \ S_{h-1}.
 *   Floyd    for a row v with d = deg(v) > k: for s = 0 .. k - 1, j = d - k + s, t = ((uint64) w_s * (j + 1)) >> 32 — a 64-bit product
 *            of the 32-bit word w_s, so 0 <= t <= j; t joins Cset when it is absent, else j does (j is always absent).  k steps
 *            whatever the degree; every k-subset of the positions is equally likely [Floyd-recall: Bentley and Floyd, CACM 1987].
 *   words    w_s = word s & 3 of Philox4x32-10 under key philox_seed at the 128-bit counter whose low 64 bits are
 *            ((uint64) v << 4) | (s >> 2) and whose high 64 bits are off + b * depth + (h - 1); off = *d_philox_offset when given, else
 *            philox_offset.  The call advances *d_philox_offset by (*d_m) * depth.  A draw depends on (b, h, v) alone, so the result
 *            is a set that no scheduling order can change.
 *   hook     (the argument `words`, uint32[m][depth][k], optional, for tests): words[b][h - 1][s] replaces w_s for every row that root b
 *            expands at hop h; all zeros force the collision branch at every step and keep the positions {0, d - k + 1, ..., d - 1}.
 *   edges    the ego-net of b is the subgraph induced on S_depth: every stored entry (u, c) with both ends in the set is kept;
 *            stored self-loops and duplicate entries stay (as grapes_saint_subgraph keeps them).
 * Outputs, the ego-nets concatenated in root order: n_id int32[n_total] the global ids, ascending within an ego-net; ptr int32[m + 1];
 * batch int32[n_total] the ego-net of each row; root_n_id int32[m] the batch-local row of each root; edge_src / edge_dst
 * int32[e_total] batch-local ids, source = the neighbour and target = the row, ordered by ego-net, then local row ascending, then the
 * CSR's order within the row; e_id int64[e_total] (optional) each entry's position in col; *d_n = n_total, *d_e = e_total.
 * More than n_cap nodes raise GRAPES_STATUS_NODE_OVERFLOW, more than e_cap entries GRAPES_STATUS_EDGE_OVERFLOW: the counts (and ptr)
 * are clamped and nothing is written at or past a capacity.  A root outside [0, N) raises GRAPES_STATUS_BAD_INDEX and becomes an empty
 * ego-net (ptr[b + 1] = ptr[b], root_n_id[b] = -1), as does a root at or past *d_m (without the bit); a column outside [0, N) raises
 * it too and its entry is dropped.  A root listed twice gets two ego-nets with independent draws (its b differs).
 * Three launches: a workgroup per root builds the sorted set in LDS and counts the induced entries per member (a wavefront strides over
 * a member's row, the whole workgroup over a row of more than 256 entries); one workgroup turns the counts into ptr and the edge
 * offsets; a workgroup per root writes.  No float, no global atomic beyond the status OR: two runs give the same bits.
 * workspace: grapes_shadow_sample_workspace_bytes(m, depth, fanout) bytes (0 for arguments outside the rule), 4-byte aligned. */
size_t grapes_shadow_sample_workspace_bytes(int32_t m, int32_t depth, int32_t fanout);
int grapes_shadow_sample(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m, const int32_t* d_m, int32_t depth, int32_t fanout, const uint32_t* words, uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, int32_t n_cap, int32_t e_cap, int32_t* n_id, int32_t* ptr, int32_t* batch, int32_t* root_n_id, int32_t* edge_src, int32_t* edge_dst, int64_t* e_id, int32_t* d_n, int32_t* d_e, void* workspace, int32_t* status, grapes_stream_t stream);
/* ShaDow-GNN's other scope: the k best nodes of an approximate personalised PageRank from the root, by synchronous forward push
 * [Zeng et al., NeurIPS 2021 for the PPR scope; Andersen, Chung, Lang, FOCS 2006 for the push — both recalled].  The push is stated in
 * FIXED POINT: integer adds commute, so a synchronous round has one result whatever the scheduling.  The rule (integers only,
 * bit-reproducible on a CPU; ONE = 2^30 is the unit of mass, T = 4096 the touched-set capacity — the result depends on T, so T is
 * part of the rule and not a tuning knob):
 *   inputs   the CSR (rowptr int64[N + 1], col int32, fewer than 2^31 entries); roots[b], b < m (*d_m), 1 <= m <= 4096; k, the scope
 *            size, 1 <= k <= 1023; alpha_q, the teleport probability in units of 2^-16, 1 <= alpha_q <= 65535; thr, the push threshold
 *            per stored entry in units of 2^-30, 1 <= thr <= 2^30; 1 <= max_rounds <= 1024 (outside: GRAPES_EINVAL).  No random
 *            numbers: the result is a function of the graph and the root.
 *   state    per root a set S of touched nodes, each with r_v and p_v (uint32); S = {root}, r_root = ONE, p_root = 0 at the start;
 *            sum r + sum p <= ONE always, so nothing overflows.  deg(v) is the stored length of row v: loops and duplicates count,
 *            each by multiplicity.
 *   round    F = {v in S : r_v > 0 and r_v >= thr * deg(v)} (a 64-bit product).  In this order: F empty — stop, code 0;
 *            rounds == max_rounds — stop, code 1; |S| + sum over F of deg(v) > T — stop, code 2 (the round could overflow the table,
 *            so it is not run; all three quantities are fixed at a round boundary, so the stop is reproducible).  Otherwise: snapshot
 *            (v, r_v) for v in F and set those r_v = 0; a snapshot entry with deg(v) = 0 gives p_v += r_v; every other one gives
 *            keep = (r_v * alpha_q) >> 16 (a 64-bit product), p_v += keep, share = (r_v - keep) / deg(v) (integer division, the
 *            remainder is dropped), and every stored entry u of row v joins S if absent (r = p = 0, also when share = 0) and gets
 *            r_u += share; an entry u = v pays v back.  A column outside [0, N) is dropped, loses its share and raises
 *            GRAPES_STATUS_BAD_INDEX.  rounds += 1.
 *   score    score_v = p_v + ((r_v * alpha_q) >> 16) for v in S: what p would be if every node kept once more without spreading;
 *            it gives residual-only nodes a rank.
 *   members  the root, and the k nodes v != root with score_v > 0 that have the largest (score_v, -v): score descending, then id
 *            ascending; fewer when fewer exist.
 *   edges    the subgraph induced on the members, exactly as grapes_shadow_sample defines it.
 * Outputs: everything grapes_shadow_sample returns, in the same order and with the same capacity, overflow and bad-root behaviour (the
 * ego-net cap is C = k + 1); score uint32[n_total] (optional) aligned with n_id, the root's own score included; rounds int32[m] and
 * stop int32[m] (optional): the rounds run and the stop code of each root, 0 and 0 for an empty ego-net.
 * Three launches: a workgroup per root runs the rounds with the touched table in LDS (an 8192-slot hash, integer LDS atomics only; a
 * round is two dependent memory trips whatever the frontier's size), selects by one bitonic sort of 64-bit keys and counts the induced
 * entries; then the scan and the write of grapes_shadow_sample.  No float, no global atomic beyond the status OR: two runs give the
 * same bits.
 * workspace: grapes_shadow_ppr_sample_workspace_bytes(m, k) bytes (0 for arguments outside the rule), 4-byte aligned. */
size_t grapes_shadow_ppr_sample_workspace_bytes(int32_t m, int32_t k);
int grapes_shadow_ppr_sample(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m, const int32_t* d_m, int32_t k, uint32_t alpha_q, uint32_t thr, int32_t max_rounds, int32_t n_cap, int32_t e_cap, int32_t* n_id, int32_t* ptr, int32_t* batch, int32_t* root_n_id, int32_t* edge_src, int32_t* edge_dst, int64_t* e_id, uint32_t* score, int32_t* rounds, int32_t* stop, int32_t* d_n, int32_t* d_e, void* workspace, int32_t* status, grapes_stream_t stream);
/* PPRGo [Bojchevski et al., KDD 2020 — recalled]: logits_b = sum_t w[b][t] MLP(x)[nbr[b][t]] over the root and its k best PPR nodes.
 * There is no graph between a batch's nodes, so the ego-net half of grapes_shadow_ppr_sample is not run.
 * grapes_pprgo_topk: the arguments of grapes_shadow_ppr_sample up to max_rounds with the same ranges; the push, the three stops, score
 * and the member order are THAT rule word for word (T = 4096 included).  Outputs in fixed slots, K = k + 1: nbr int32[m][K], score
 * uint32[m][K], cnt int32[m], rounds / stop int32[m] (optional).  Slot 0 is the root with its own score; slots 1 .. cnt[b] - 1 the best
 * nodes, score descending, then id ascending; slots t >= cnt[b] hold nbr = root, score = 0 (a union over all slots may ignore cnt;
 * nothing else reads them).  A root outside [0, N) raises GRAPES_STATUS_BAD_INDEX and gives cnt = 0, nbr = -1, score = 0, rounds = stop
 * = 0; a root at or past *d_m the same without the bit.  One launch (a workgroup per root writes the sorted keys' prefix in rank
 * order), no workspace, no scan, integers only, no global atomic beyond the status OR: two runs give the same bits. */
int grapes_pprgo_topk(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m, const int32_t* d_m, int32_t k, uint32_t alpha_q, uint32_t thr, int32_t max_rounds, int32_t* nbr, uint32_t* score, int32_t* cnt, int32_t* rounds, int32_t* stop, int32_t* status, grapes_stream_t stream);
/* grapes_pprgo_batch: the batch structure of slot tables nbr / cnt [m][K] (1 <= m <= 4096, 2 <= K <= 1024; a slot t < cnt[b] is live,
 * cnt is clamped to [0, K], dead slots are not read).
 *   node_idx int32[n]   the ascending, duplicate-free union of the live slots' ids; *d_n = n
 *   loc int32[m][K]     the rank of nbr[b][t] in node_idx for a live slot; a dead slot repeats slot 0's value (-1 where cnt[b] = 0)
 *   tptr int32[n + 1], tslot int32[E]   the by-source inverted index: for local row u the flat slot indices s = b K + t of the live
 *                       slots with loc = u, ASCENDING; *d_e = E = the live slots; *d_seg_max (optional) = the longest segment, so
 *                       that a caller who reads it beside n and E can spare the backward its chunked form (item_cap = 0)
 * More than n_cap nodes raise GRAPES_STATUS_NODE_OVERFLOW, more than e_cap slots GRAPES_STATUS_EDGE_OVERFLOW: the counts (and tptr) are
 * clamped, nothing is written at or past a capacity, and the structure is then incomplete (a slot of a dropped node has loc = -1).  A
 * live id outside [0, N) raises GRAPES_STATUS_BAD_INDEX, gets loc = -1 and is in no segment; so does a source listed more than 4096
 * times, whose segment stays unordered.
 * The caller's scratch: bits uint64[ceil(N / 64)], ZERO on entry and zero again on return; node_map int32[N], any state on entry (it
 * holds the ranks of this batch's ids afterwards).  Integers only; two runs give the same bits.
 * workspace: grapes_pprgo_batch_workspace_bytes(n_cap, num_nodes) bytes, 4-byte aligned. */
size_t grapes_pprgo_batch_workspace_bytes(int32_t n_cap, int32_t num_nodes);
int grapes_pprgo_batch(const int32_t* nbr, const int32_t* cnt, int32_t m, int32_t K, int32_t num_nodes, uint64_t* bits, int32_t* node_map, int32_t n_cap, int32_t e_cap, int32_t* node_idx, int32_t* loc, int32_t* tptr, int32_t* tslot, int32_t* d_n, int32_t* d_e, int32_t* d_seg_max, void* workspace, int32_t* status, grapes_stream_t stream);
/* The weighted gathers of PPRGo's readout, row-major fp32, widths as the row gathers (f % 4 == 0 with 16-byte aligned rows up to 1024,
 * any f up to 256).
 *   forward   out[b, :f] = sum_{t < cnt[b]} w[b][t] z[loc[b][t], :f], b < m; w fp32[m][K], z [n, f].  Slots at or past cnt[b] are never
 *             read, neither w nor loc.
 *   backward  dz[u, :f] = sum_{s in tslot[tptr[u] .. tptr[u + 1])} w[s] g[s / K, :f] in ascending s, for EVERY u < n (e = tptr[n]);
 *             w carries no gradient.
 * A row of more than grapes_vrgcn_long_row() entries (the forward: K above it) is cut into chunks of that many, one group of lanes each,
 * and the partial sums are added in chunk order.  No float atomics: every sum has a fixed order, two runs give the same bits.  An index
 * outside its table raises GRAPES_STATUS_BAD_INDEX and the entry is dropped.  item_cap (backward): the chunks behind the first of the
 * long segments the call has room for, at most 2^22 (0: every segment by one group); more raise GRAPES_STATUS_EDGE_OVERFLOW.
 * workspace: the _workspace_bytes of the direction (forward: may be NULL while K is no long row), 16-byte aligned. */
size_t grapes_pprgo_aggregate_fwd_workspace_bytes(int32_t m, int32_t K, int32_t f);
int grapes_pprgo_aggregate_fwd(const float* z, int32_t n, const float* w, const int32_t* loc, const int32_t* cnt, int32_t m, int32_t K, int32_t f, float* out, void* workspace, int32_t* status, grapes_stream_t stream);
size_t grapes_pprgo_aggregate_bwd_workspace_bytes(int32_t n, int32_t item_cap, int32_t f);
int grapes_pprgo_aggregate_bwd(const float* g, int32_t m, const float* w, int32_t K, const int32_t* tptr, const int32_t* tslot, int32_t n, int32_t e, int32_t f, float* dz, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);
/* PinSAGE [Ying et al., KDD 2018 — recalled; DGL-recall: RandomWalkNeighborSampler / PinSAGESampler]: a root's neighbourhood is the T
 * nodes that R restarting walks of at most L steps from it visit most often; the visit counts are the aggregation weights.
 * grapes_pinsage_neighbors — the rule, integers only (a CPU reproduces every output bit):
 *   Ranges (else GRAPES_EINVAL): 1 <= R, 1 <= L, V = R L <= 1024; 1 <= T <= 1023, K = T + 1 (the tables fit grapes_pprgo_batch);
 *   m >= 1 and m K < 2^31; the graph holds fewer than 2^31 entries; term_q is any uint32 — the termination probability in units of
 *   2^-32, min(2^32 - 1, round(p 2^32)) for 0 <= p < 1.
 *   Stream offset: off = *d_philox_offset when that pointer is non-NULL, else philox_offset.  A non-NULL *d_philox_offset advances by
 *   ceil(L / 2) per call, in a ONE-THREAD TAIL launch behind the kernel (every workgroup has read the offset by then); without the
 *   pointer the call is one launch.
 *   One step: walk j < R of a root with global id v, step t < L, from the current node c (c = v at t = 0):
 *     P = philox4x32_10 over the 128-bit counter (low 64 bits = uint64(v) | uint64(j) << 32, high 64 bits = off + (t >> 1)) under the
 *     key philox_seed; a = P.v[2 (t & 1)], s = P.v[2 (t & 1) + 1].  The walk ENDS before the move if a < term_q or deg(c) = 0 (deg =
 *     rowptr[c + 1] - rowptr[c]); otherwise c <- col[rowptr[c] + ((uint64(s) deg(c)) >> 32)].  The new c is one VISIT unless c = v:
 *     returns to the root are not counted, the root has its own term in the layer (DGL keeps them: a stated deviation).  A col entry
 *     outside [0, N) ends the walk uncounted and raises GRAPES_STATUS_BAD_INDEX.
 *   A draw depends on (v, j, t, off, seed) alone — not on the root's position, on m, or on how the kernel tiles the roots: a repeated
 *   root gets identical rows.
 *   Selection: count[u] = the visits to u over the root's R walks; kept are the min(T, distinct) nodes with the smallest key
 *   ((V - count[u]) << 32) | u: count descending, then id ascending.
 *   Outputs, in grapes_pprgo_topk's slot convention (grapes_pprgo_batch runs on them unchanged): nbr int32[m][K], visits uint32[m][K],
 *   cnt int32[m].  Slot 0 is (root, 0); slots 1 .. cnt[b] - 1 the kept nodes in key order with their counts; slots t >= cnt[b] hold
 *   (root, 0).  A root outside [0, N) raises GRAPES_STATUS_BAD_INDEX and gets cnt = 0, nbr = -1, visits = 0; a root at or past *d_m
 *   (optional, clamped to m) the same without the bit.
 * No float, no global atomic beyond the status OR, no workspace: two runs give the same bits. */
int grapes_pinsage_neighbors(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* roots, int32_t m, const int32_t* d_m, int32_t R, int32_t L, uint32_t term_q, int32_t T, uint64_t philox_seed, uint64_t philox_offset, uint64_t* d_philox_offset, int32_t* nbr, uint32_t* visits, int32_t* cnt, int32_t* status, grapes_stream_t stream);
/* PinSAGE's layer epilogue over the rows of s [m, f] (rows ld_s floats apart; every ld >= f), eps > 0:
 *   forward   z = max(s, 0) (a NaN reads as 0); nrm[b] = sqrtf(sum_c z[b, c]^2); out[b, c] = z[b, c] / max(nrm[b], eps)
 *   backward  ds[b, c] = [s[b, c] > 0] (g[b, c] - out[b, c] <g[b], out[b]> [nrm[b] >= eps]) / max(nrm[b], eps), with out and nrm as
 *             the forward wrote them
 * Widths as the row gathers: f % 4 == 0 up to 1024 where every matrix is 16-byte aligned with ld % 4 == 0, any f up to 256 otherwise
 * (GRAPES_EALIGN where alignment alone stands in the way).  A group of lanes owns a row; the sums are an fma chain over a lane's
 * columns and a butterfly over the group — a fixed order, no atomics, two runs give the same bits; IEEE sqrtf and division.  Columns
 * at or past f of a row are neither read nor written.  One launch each, no workspace. */
int grapes_relu_l2norm_fwd(const float* s, int64_t ld_s, int32_t m, int32_t f, float eps, float* out, int64_t ld_out, float* nrm, grapes_stream_t stream);
int grapes_relu_l2norm_bwd(const float* g, int64_t ld_g, const float* out, int64_t ld_out, const float* nrm, const float* s, int64_t ld_s, int32_t m, int32_t f, float eps, float* ds, int64_t ld_ds, grapes_stream_t stream);
/* The mean over contiguous row segments, ShaDow's pooled readout: out[b, :f] = the mean of h[ptr[b] .. ptr[b + 1], :f] for b <
 * num_segments, 0 for an empty segment; h is [n_rows, f] row-major, 1 <= f <= 1024.  A thread owns a column and adds the segment's
 * rows in row order, then divides once: n_b - 1 additions and one division in a fixed order, no atomics.  The backward writes
 * dh[r, :f] = g[b, :f] / n_b for every row r of segment b — one division, so it is exact up to that rounding — and 0 for the rows in
 * front of the first segment and behind the last.  A segment that is not a run inside [0, n_rows] raises GRAPES_STATUS_BAD_INDEX and
 * counts as empty.  One launch each. */
int grapes_segment_mean_fwd(const float* h, const int32_t* ptr, int32_t num_segments, int32_t n_rows, int32_t f, float* out, int32_t* status, grapes_stream_t stream);
int grapes_segment_mean_bwd(const float* g, const int32_t* ptr, int32_t num_segments, int32_t n_rows, int32_t f, float* dh, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ LINKX: the adjacency embedding bag (csrc/bag_kernels.hip)
 * [Lim et al., NeurIPS 2021; PyG-recall: LINKX, SparseLinear].  A node's row of the adjacency matrix is a feature vector of length N
 * pushed through a learned table W fp32 [N, H]:  h_A[i] = b + sum_{t in row(i)} W[col[t]].  Nothing is sampled; a batch is m rows of A.
 * The graph is the CSR as stored (rowptr int64[N + 1], col int32, fewer than 2^31 entries): directed graphs are allowed, and
 * duplicates and loops count as often as they are stored.
 * grapes_bag_batch — the batch tables of rows[m], 1 <= m <= 4096; ids may repeat, each occurrence is its own batch row.  Integers only:
 *   bptr int32[m + 1]   the exclusive prefix of the batch rows' stored lengths in batch order; bptr[m] = e, the TRUE total whatever e_cap
 *   uniq int32[n_u]     the distinct column ids over all batch rows, ascending
 *   tptr int32[n_u + 1], trow int32[e]   for column uniq[s] the batch-row indices b whose row stores it, ASCENDING in b; a column
 *                       stored c times in one row appears c times, adjacent
 *   d_counts int32[4]   (n_u, e, the longest segment, the longest batch row): the TRUE totals also past a capacity.  e = bptr[m]
 *                       counts every stored entry; tptr[n_u] counts the entries that sit in a segment.  The two are equal unless
 *                       GRAPES_STATUS_BAD_INDEX was raised for a column id (such an entry is in no segment: tptr[n_u] < e) or a
 *                       capacity was passed
 * More than u_cap distinct columns raise GRAPES_STATUS_NODE_OVERFLOW, more than e_cap entries GRAPES_STATUS_EDGE_OVERFLOW: nothing is
 * written at or past a capacity (uniq holds u_cap ids, tptr u_cap + 1 offsets clamped to e_cap, trow e_cap values), the structure is
 * then incomplete, and the caller retries with the totals d_counts reports.  A row id outside [0, N) raises GRAPES_STATUS_BAD_INDEX
 * and is an empty row; so does a column id outside [0, N), which is in no segment, and a column stored more than 4096 times over
 * the batch, whose segment stays unordered.
 * The caller's scratch: bits uint64[ceil(N / 64)], ZERO on entry and zero again on return; node_map int32[N], any state on entry —
 * the entries this call wrote (those of uniq) are put back to 0, so a map that was zero is returned zero.  Two runs give the same
 * bits.  workspace: grapes_bag_batch_workspace_bytes(m, u_cap, num_nodes) bytes, 4-byte aligned. */
size_t grapes_bag_batch_workspace_bytes(int32_t m, int32_t u_cap, int32_t num_nodes);
int grapes_bag_batch(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m, uint64_t* bits, int32_t* node_map, int32_t u_cap, int32_t e_cap, int32_t* bptr, int32_t* uniq, int32_t* tptr, int32_t* trow, int32_t* d_counts, void* workspace, int32_t* status, grapes_stream_t stream);
/* grapes_bag_fwd: out[b, :h] = bias + sum_t W[col[t], :h] over the stored entries t of row rows[b], b < m, in stored order: the
 * accumulator starts at bias (0 without one) and the rows are added one after the other.  W rows ld_w floats apart, out ld_out.
 * Widths as the row gathers: h % 4 == 0 up to 1024 where W, out and bias are 16-byte aligned with ld % 4 == 0, any h up to 256 otherwise
 * (GRAPES_EALIGN where alignment alone stands in the way).  item_cap > 0: a row of more than grapes_vrgcn_long_row() entries is cut
 * into chunks of that many, one group of lanes each; chunk 0 starts at bias, the further chunks at 0, and their partial sums are added
 * to chunk 0's in chunk order.  item_cap bounds the chunks behind the first (at most 2^22; more raise GRAPES_STATUS_EDGE_OVERFLOW);
 * 0: every row by one group.  An empty row gives bias; so does a row id outside [0, N), which raises GRAPES_STATUS_BAD_INDEX; a column
 * id outside [0, N) raises it and is dropped.  No float atomics, two runs give the same bits.
 * workspace: grapes_bag_fwd_workspace_bytes(m, item_cap, h) bytes, 16-byte aligned (may be NULL with item_cap = 0). */
size_t grapes_bag_fwd_workspace_bytes(int32_t m, int32_t item_cap, int32_t h);
int grapes_bag_fwd(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* rows, int32_t m, const float* w, int64_t ld_w, const float* bias, int32_t h, float* out, int64_t ld_out, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);
/* The backward over the batch tables, G = d out fp32 [m, h] (rows ld_g apart):  g_s = sum_{q in [tptr[s], tptr[s + 1])} G[trow[q]]
 * for every s < n_u, in segment order and COMPENSATED: with the sum S = 0 and its error term c = 0, every entry x does
 * y = x - c; t = S + y; c = (t - S) - y; S = t (Kahan), each operation rounded once to fp32, and g_s = S.  item_cap > 0: a segment of
 * more than grapes_vrgcn_long_row() entries is cut into chunks of that many, each summed so by its own group, and the chunks' sums are
 * added in chunk order by the same rule from (0, 0); item_cap bounds the chunks of such segments, the first included (at most 2^22;
 * floor(e / 32) cannot overflow).  The compensation is what keeps a long segment's sum within an ulp of the exact one: the plain
 * fixed-order sum of 300 entries measured up to 12.7 times the error of a correctly rounded fp32 sum in the update below.
 * The argument e of the two calls bounds what is read of trow: every segment must lie inside [0, e], else it is refused with
 * GRAPES_STATUS_BAD_INDEX and counts as empty.  tptr[n_u] is the exact value; grapes_bag_batch's e = bptr[m] is never below it, and
 * trow holds at least that many values, so either may be passed.  No float atomics; widths and alignment as the forward.
 *   grapes_bag_bwd       grad[s, :h] = g_s: the values of the row-sparse gradient of W whose indices are uniq.
 *   grapes_bag_bwd_adam  writes no gradient.  With g = g_s in registers, row j = uniq[s] of W (p), exp_avg (m) and exp_avg_sq (v) is
 *                        read once and written once, each operation rounded once to fp32 (no contraction), IEEE sqrtf and division:
 *                            m' = m + one_minus_beta1 (g - m);   v' = v + one_minus_beta2 (g g - v);
 *                            p' = p - step_size (m' / (sqrtf(v') + eps))
 *                        which is torch.optim.SparseAdam's rule with step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t) formed by the
 *                        caller in double and passed as one fp32; t counts calls, not touches.  LAZY semantics: rows outside uniq are
 *                        neither read nor written — their moments do not decay.  A row is updated exactly once: uniq is
 *                        duplicate-free, a short segment is finished by the rows kernel and a long one by the combine pass.  An
 *                        entry of uniq outside [0, N) raises GRAPES_STATUS_BAD_INDEX and is skipped.  exp_avg and exp_avg_sq rows
 *                        are ld_state floats apart.
 * workspace: grapes_bag_bwd_workspace_bytes(n_u, item_cap, h) bytes, 16-byte aligned (may be NULL with item_cap = 0). */
size_t grapes_bag_bwd_workspace_bytes(int32_t n_u, int32_t item_cap, int32_t h);
int grapes_bag_bwd(const float* g, int64_t ld_g, int32_t m, const int32_t* tptr, const int32_t* trow, int32_t n_u, int32_t e, int32_t h, float* grad, int64_t ld_grad, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);
int grapes_bag_bwd_adam(const float* g, int64_t ld_g, int32_t m, const int32_t* tptr, const int32_t* trow, const int32_t* uniq, int32_t n_u, int32_t e, int32_t num_nodes, int32_t h, float* w, int64_t ld_w, float* exp_avg, float* exp_avg_sq, int64_t ld_state, float one_minus_beta1, float one_minus_beta2, float eps, float step_size, int32_t item_cap, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ Cluster-GCN: cluster-union batches (csrc/cluster_kernels.hip)
 * [Chiang et al., KDD 2019; PyG-recall: ClusterData, ClusterLoader, ClusterGCNConv].  The graph is cut into P clusters once; a batch is
 * the subgraph induced on the union of q chosen clusters.  The rule (integers only, bit-reproducible on a CPU):
 *   inputs   the CSR (rowptr int64[N + 1], col int32, fewer than 2^31 entries); the partition tables, built once: perm int32[N] the node
 *            ids in cluster order, ascending id inside a cluster; partptr int32[P + 1]; where int32[N][2] = (cluster of v, position of
 *            v inside its cluster), 8-byte aligned so that the pair is one load; clusters int32[q], 1 <= q <= 2^20, taken IN THE GIVEN
 *            ORDER; stamp int32[P][2], 8-byte aligned, the caller's scratch membership table, and serial >= 1; the capacities n_cap
 *            (<= 2^31 - 2), item_cap (<= 2^24) and e_cap.
 *   nodes    *d_n = n = the sum of the chosen clusters' sizes; cptr int32[q + 1]: the rows of chosen cluster k are cptr[k] ..
 *            cptr[k + 1] (an empty cluster has an empty range); node_idx[cptr[k] + t] = perm[partptr[clusters[k]] + t].
 *   edges    for local row i ascending, then the entries j of row node_idx[i] in col's stored order: an entry whose u = col[j] lies in a
 *            chosen cluster becomes edge p: edge_src[p] = the local row of u, the neighbour (cptr[slot of where[u].cluster] +
 *            where[u].position); edge_dst[p] = i; edge_id[p] = j (edge_id may be NULL).  Stored self-loops and duplicates stay.
 *            *d_e = min(e, e_cap).  rowptr_l int32[n_cap + 1]: the first edge of local row i for i < n, and min(e, e_cap) for
 *            EVERY slot n <= i <= n_cap — written by the call, so a caller may hand rowptr_l on with n_cap rows.
 *   status   more than e_cap edges OR GRAPES_STATUS_EDGE_OVERFLOW: exactly the first e_cap edges in that order are written, nothing at
 *            or past e_cap.  n > n_cap ORs GRAPES_STATUS_NODE_OVERFLOW; a cluster id outside [0, P) or a cluster listed twice ORs
 *            GRAPES_STATUS_BAD_INDEX (it takes precedence over the node overflow): either way the batch is empty — *d_n = *d_e = 0,
 *            cptr and rowptr_l all zero, no row or edge written — whichever thread wins a race.  A col entry outside [0, N) ORs
 *            GRAPES_STATUS_BAD_INDEX and is dropped.  A row is cut into work items of 64 entries; a batch of more than item_cap items
 *            ORs GRAPES_STATUS_EDGE_OVERFLOW and keeps the edges of the first item_cap items alone (the sum over the batch's rows of
 *            ceil(deg / 64) never exceeds a cap taken from the partition: ClusterLoader's default).
 *   stamps   stamp[c] = (serial, first local row of c) for every chosen c; u is a member iff stamp[where[u].cluster].serial ==
 *            serial.  The table is NOT cleared between calls: the caller zeroes it once and passes a serial no call has used since
 *            (1, 2, ...; zero it again before a serial would repeat).  A refused call leaves its serial in the table like any other.
 * Six launches: one workgroup turns the q sizes into cptr, the stamps and n; a thread per row finds node_idx and the row's items; one
 * workgroup scans the items; a wavefront per item tests its 64 entries (col -> where -> stamp: an item's lookups are in flight
 * together, and a hub row is cut over many wavefronts); one workgroup scans the kept counts; a wavefront per item writes.  No float,
 * no host read, no global atomic beyond the status OR and the stamps: two runs give the same bits.
 * workspace: grapes_cluster_batch_workspace_bytes(n_cap, item_cap) bytes, 8-byte aligned. */
size_t grapes_cluster_batch_workspace_bytes(int32_t n_cap, int32_t item_cap);
int grapes_cluster_batch(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* perm, const int32_t* partptr, const int32_t* where, int32_t num_parts, const int32_t* clusters, int32_t q, int32_t* stamp, int32_t serial, int32_t n_cap, int32_t item_cap, int32_t e_cap, int32_t* cptr, int32_t* node_idx, int32_t* rowptr_l, int32_t* edge_src, int32_t* edge_dst, int64_t* edge_id, int32_t* d_n, int32_t* d_e, void* workspace, int32_t* status, grapes_stream_t stream);

/* ------------------------------------------------------------------ the graph partitioner of Cluster-GCN (csrc/partition_kernels.hip)
 * Size-constrained SYNCHRONOUS label propagation that refines a starting assignment.  Integers only, bit-reproducible on a CPU
 * (tests/partition_oracle.py).  The rule, for the CSR (rowptr int64[N + 1], col int32, fewer than 2^31 entries), P clusters, part
 * int32[N] in [0, P), cap = the largest size a cluster may reach; one round is a proposal and an admission:
 *   propose  every node v, every round, from part as it stood at the start of the round: count the labels part[u] over the stored
 *            entries u of row v with u != v (a duplicate entry counts once each).  cur = part[v], m = the largest count.  v stays when
 *            the row has no such entry or count[cur] == m: want[v] = -1, gain[v] = 0.  Otherwise want[v] = the smallest label among
 *            those with count m and gain[v] = m - count[cur] >= 1.
 *   admit    size[c] = the size of c at the start of the round, free[c] = max(cap - size[c], 0): nodes that leave in this round are
 *            not credited, so no cluster ever exceeds cap.  Among the proposers to c, the free[c] with the smallest 64-bit key
 *            ((0x7fffffff - gain) << 32) | v are admitted — the larger gain first, then the smaller node id; keys are unique, so the
 *            admitted set does not depend on the order in which the proposers were gathered.  An admitted v takes part[v] = want[v];
 *            size is updated at both ends; *moved = the nodes admitted.
 *   cut      the stored entries (v, u) with u != v and part[v] != part[u], an exact int64.
 * The driver (modules/cluster.py: refine_partition) evaluates the cut of the start and after every round, returns the assignment of
 * the earliest round with the smallest cut — synchronous propagation can oscillate; the result is never worse than the start — and
 * stops when a round moves nothing.  Once clusters sit at cap the rule stalls: there is no swap or rebalancing phase.
 *   status   a column outside [0, N) or a label outside [0, P) ORs GRAPES_STATUS_BAD_INDEX and the entry is dropped; a node whose own
 *            label is outside [0, P) ORs it and stays (propose), counts nothing (cut).  grapes_partition_admit ORs it for a proposal
 *            with want >= P, gain < 1 or such a label, and ignores the proposal.
 * grapes_partition_propose: rows of at most 64 entries on one wavefront in registers; rows of 65 .. 2048 entries by a workgroup with an
 * LDS table keyed by label; longer rows by 16 workgroups of 1024 threads over P-sized slabs of the workspace.  grapes_partition_admit:
 * histogram, one-workgroup scan, scatter of the keys, the limit of every destination (a fuller bucket by an 8-bit radix select over its
 * keys), apply; part and size are updated in place.  grapes_partition_cut: one pass, 64-bit integer sums.  No floating point; integer
 * atomics only; two runs give the same bits.  Workspaces: the _workspace_bytes companions; 8-byte aligned. */
size_t grapes_partition_propose_workspace_bytes(int32_t num_nodes, int32_t num_parts);
int grapes_partition_propose(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* part, int32_t num_parts, int32_t* want, int32_t* gain, void* workspace, int32_t* status, grapes_stream_t stream);
size_t grapes_partition_admit_workspace_bytes(int32_t num_nodes, int32_t num_parts);
int grapes_partition_admit(const int32_t* want, const int32_t* gain, int32_t num_nodes, int32_t num_parts, int32_t* part, int32_t* size, int32_t cap, int32_t* moved, void* workspace, int32_t* status, grapes_stream_t stream);
size_t grapes_partition_cut_workspace_bytes(int32_t num_nodes);
int grapes_partition_cut(const int64_t* rowptr, const int32_t* col, int32_t num_nodes, const int32_t* part, int32_t num_parts, int64_t* cut, void* workspace, int32_t* status, grapes_stream_t stream);

#ifdef GRAPES_DIAG
/* ------------------------------------------------------------------ pre-split feature planes (round 4; DIAGNOSTIC BUILD ONLY:
 * measured slower than splitting in the K loop — Reddit 1.418 against 1.366 ms/step — and kept as an A/B form)
 * The gathered-operand bf16x3 GEMMs of the transform-first first layers (grapes_linear_fwd_gathered_split[_k],
 * grapes_linear_bwd_weight_gathered_split[_ld]; modules/gcn.py:32 on main.py:199-204's rows) split every gathered fp32 row into
 * its three bf16 terms inside their K loops.  X is constant for a whole run (main.py:66): the caller may split it ONCE —
 * planes: grapes_feature_planes_bytes(n, x_stride) bytes, 24 per 4-column chunk [h0..h3 | m0..m3 | l0..l3], 8-byte aligned —
 * and REGISTER the planes for that matrix (host-side table keyed by the X pointer and row stride; planes NULL forgets it);
 * those entry points then read the planes of the rows they gather.  Results are bit-identical (the same split, done earlier).
 * The planes must be rebuilt when X changes (learned embeddings: do not register). */
size_t grapes_feature_planes_bytes(int64_t n, int32_t x_stride);
int grapes_feature_split_planes(const float* X, int64_t n, int32_t x_stride, void* planes, grapes_stream_t stream);
int grapes_feature_planes_register(const float* X, int32_t x_stride, const void* planes);
#endif

/* ------------------------------------------------------------------ learned node embeddings (--embed_nodes)
 * main.py:89-100,116: data.x is an nn.Parameter optimised by optimizer_c; the backward of `data.x[all_nodes]` (main.py:256)
 * accumulates the rows' gradients into a dense [N, F] gradient.  dst[ids[i], 0:F] (+)= src[i, 0:F]; accumulate = 0 overwrites
 * the addressed rows (the step's id lists are duplicate-free and the gradient was zeroed); atomic != 0 adds with float
 * atomics (id lists with duplicates: the drop-in autograd function). */
int grapes_scatter_rows(float* dst, int64_t dst_stride, const int32_t* ids, const float* src, int64_t src_stride, int32_t F,
                        int32_t n, const int32_t* d_n, int32_t accumulate, int32_t atomic, grapes_stream_t stream);

/* ------------------------------------------------------------------ measurement: kernel clock table
 * bench.py's roofline numbers are taken INSIDE the replayed hipGraph (HIP events cannot bracket a graph node on this ROCm):
 * while a table is enabled, every launch of the roofline kernels (gcn_aggregate_k<4>, gcn_aggregate_gather*_k,
 * gemm_wsplit_f32_k, ...) reserves one (begin, end) pair of 100 MHz s_memrealtime stamps per wavefront — at enqueue / capture
 * time, in launch order — and its wavefronts write them on every execution.  Launch i's duration = (max end - min begin) /
 * rate over its pairs.  With no table (the default, and the timed region of bench.py) no stamp executes.
 * table: device memory of `words` 64-bit words (NULL disables and forgets the launch log). */
int grapes_kernel_clock_enable(uint64_t* table, int64_t words);
int32_t grapes_kernel_clock_launches(void);
/* kernel64: caller buffer of 64 chars (NUL-terminated name); offset_words into the table; pairs = wavefronts of the launch */
int grapes_kernel_clock_entry(int32_t i, char* kernel64, int64_t* offset_words, int32_t* pairs);
int32_t grapes_kernel_clock_rate_khz(void);

/* ------------------------------------------------------------------ riders: two problems side by side in one launch
 * (new design; no reference counterpart — reference main.py:157-291 runs its steps strictly one after the other)
 * The step's small index kernels leave most of the chip idle, and on this stack neither a second stream nor a branch of a
 * hipGraph overlaps them for free (profiles/r04_overlap_probe.txt: a second hardware queue taxes every dispatch of the first).
 * What does overlap is work of the SAME kernel carried as extra workgroups of one launch.  While RECORDING, the launches of
 * grapes_step_begin, grapes_frontier_expand_fused[_ext], grapes_frontier_compact[_counted], grapes_gcn_prepare_counted and
 * grapes_gcn_aggregate_gather_fwd[_peers] are not issued but appended to a PROGRAM (their arguments are kept by value: the
 * buffers must stay alive).  While a program is ATTACHED, the next launch of the same kernel (same variant and workgroup
 * size) by those entry points carries the program's next record as additional workgroups ("host" and "rider" never share
 * scratch: give the rider's compaction its own sync words); records that cannot ride (grapes_step_begin, other kernel
 * variants) are issued on their own, in recorded order, as soon as they are at the head of the program; detach issues what
 * is left.  Every record is issued exactly once per attach, in recorded order.  step_graph uses this to run the NEXT training
 * step's weight-independent prelude (next batch, hop 0's expansion / compaction / graph build / gather-SpMM) inside the
 * current step's hop-1 launches.  Host-side state, one recording / one attachment at a time, not thread-safe. */
int grapes_rider_record_begin(void);
int32_t grapes_rider_record_end(void);                              /* -> program handle (>= 0) or -1 */
int32_t grapes_rider_count(int32_t program);                        /* records in the program, -1: no such program */
/* hold != 0: the early phase — only a recorded grapes_step_begin may be taken (as one more workgroup of the next expansion);
 * everything else waits for grapes_rider_release.  hold == 0: all records may ride from now on (the leading ones that cannot
 * ride are issued at once). */
int grapes_rider_attach(int32_t program, int32_t hold, grapes_stream_t stream);
int grapes_rider_release(grapes_stream_t stream);
/* -> records issued on their own during this attachment (>= 0), or a negative error; *paired = records that rode */
int grapes_rider_detach(grapes_stream_t stream, int32_t* paired);
int grapes_rider_launch(int32_t program, grapes_stream_t stream);   /* the whole program on its own, in order */
int grapes_rider_free(int32_t program);

/* ------------------------------------------------------------------ step chains: several captured steps, one hipGraphLaunch
 * (new design; reference main.py:157 `for batch in loader` launches its steps one by one — here the loop body is a captured
 * hipGraph, and between two hipGraphLaunch calls the queue idles for ~20 us: 4 % of a 0.5 ms step)
 * graphs: n hipGraph_t handles (HOST array; e.g. torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph()) of captured steps.
 * The chain is a NEW executable graph holding copies of their kernel (/ memset / empty) nodes with the SAME arguments, segment
 * after segment in the given order, the whole sequence `repeat` times; a segment starts when the one before has finished.
 * The source graphs are not changed and stay launchable; their buffers must outlive the chain.  A graph with any other node
 * kind (copies, host functions, events) -> GRAPES_EINVAL.  *chain_out: opaque handle; *nodes_out (optional): nodes in it. */
int grapes_graph_chain_create(void* const* graphs, int32_t n, int32_t repeat, void** chain_out, int32_t* nodes_out);
int grapes_graph_chain_launch(void* chain, grapes_stream_t stream);
int grapes_graph_chain_destroy(void* chain);

#ifdef __cplusplus
}
#endif
#endif /* GRAPES_HIP_H */
