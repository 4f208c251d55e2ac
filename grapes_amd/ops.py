"""Tensor-level wrappers over the C-ABI (include/grapes_hip.h).

PyTorch is used here only as plumbing: device memory (caching allocator), the current HIP stream
and dtype/shape checks.  Every function enqueues HIP kernels on torch's current stream and
returns without synchronising; `d_*` arguments are optional int32 device scalars carrying the
true sizes of capacity-padded buffers (see the header for the convention).
"""
from __future__ import annotations

from typing import List, Optional

import ctypes as _C
import os

import torch

from . import _lib
from ._lib import diag_switch as _sw      # A/B switches: the default unless GRAPES_DIAG=1 (the product has one configuration)

_i32 = torch.int32
_i64 = torch.int64
_f32 = torch.float32


def lib():
    return _lib.load()


def _stream() -> int:
    """torch's current HIP stream as a raw pointer.  (torch.cuda.current_stream() builds a Stream object through several
    Python layers: ~10 us per call, 70 calls per eager step — profiles/eager_profile.py; the raw query is one C call.)"""
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:          # (another torch build: the public, slower way)
        return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: Optional[torch.Tensor], dtype, name: str, allow_none: bool = False):
    if t is None:
        if allow_none:
            return
        raise TypeError(f"{name} is required")
    if not t.is_cuda:
        raise _lib.GrapesHipError(f"{name} must live in HBM (cuda tensor); grapes_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


_KEEP = [None]        # while launches are RECORDED as riders (rider_keep): the temporaries they will use later must outlive the call


def rider_keep(on: bool):
    """on=True: from now on every scratch tensor of the wrappers below is also appended to a list (launches recorded by
    grapes_rider_record_begin run LATER, every step: a workspace freed when the wrapper returns would be somebody else's memory
    by then); on=False: stop and return that list — the caller keeps it for as long as the recorded program lives."""
    if on:
        _KEEP[0] = []
        return None
    kept, _KEEP[0] = _KEEP[0], None
    return kept


def _tmp(t: torch.Tensor) -> torch.Tensor:
    if _KEEP[0] is not None:
        _KEEP[0].append(t)
    return t


def _ws(nbytes: int, device) -> torch.Tensor:
    return _tmp(torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device))


_SYNC = {}
_ONE_LAUNCH_PREP = _sw("GRAPES_ONE_LAUNCH_PREP", "1") != "0"      # A/B switches for the look-back forms
_ONE_LAUNCH_SLICE = _sw("GRAPES_ONE_LAUNCH_SLICE", "0") != "0"    # measured slower (4 edges per thread): off
_PREFETCH_ROWS = _sw("GRAPES_PREFETCH_ROWS", "1") != "0"          # A/B: the hop build touches the gather-SpMM's rows of X
# GRAPES_PREP_FUSED=1 (read by the library): the grouped, pre-zeroed hop-graph build as ONE cooperative launch with grid
# barriers instead of four launches — measured slower (profiles/r03_prep_fused_ab.txt): off


_LANE = [0]


def set_scratch_lane(lane: int) -> int:
    """Selects which copy of the per-device `sync` scratch the next calls bake into their launches; returns the previous lane.
    Launches that may run AT THE SAME TIME on two streams (step_graph's prelude pipeline: the next step's weight-independent
    index chain under the current step) must not share it; within a lane calls are stream-ordered."""
    old, _LANE[0] = _LANE[0], int(lane)
    return old


def sync_scratch(device) -> torch.Tensor:
    """The per-device `sync` scratch of the one-launch scans (include/grapes_hip.h: GRAPES_SYNC_WORDS): zero at rest,
    left zero by every kernel that uses it.  Shared by all calls of a lane on the device (set_scratch_lane), which therefore
    have to be stream-ordered (they are: the index pipeline of a lane runs on one stream); pass your own `sync=` tensor
    otherwise."""
    dev = torch.device(device)
    t = _SYNC.get((dev, _LANE[0]))
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("sync_scratch: first use inside a stream capture; run one eager step first")
        t = torch.zeros(256, dtype=_i64, device=dev)
        _SYNC[(dev, _LANE[0])] = t
    return t


# ------------------------------------------------------------------------------- learned node embeddings (--embed_nodes)
def scatter_rows(dst, ids, src, d_n=None, accumulate=False, atomic=False, F=None):
    """dst[ids[i], :F] (+)= src[i, :F]  (backward of a feature-row gather into a dense gradient; main.py:89-100,256)."""
    _chk(dst, _f32, "dst"); _chk(ids, _i32, "ids"); _chk(d_n, _i32, "d_n", True)
    if src.dtype != _f32 or not src.is_cuda or src.stride(1) != 1:
        raise TypeError("scatter_rows: src must be a float32 cuda matrix with unit column stride")
    F = int(min(dst.shape[1], src.shape[1]) if F is None else F)
    _lib.check(lib().grapes_scatter_rows(_p(dst), dst.stride(0), _p(ids), _p(src), src.stride(0), F, ids.numel(), _p(d_n),
                                         1 if accumulate else 0, 1 if atomic else 0, _stream()), "scatter_rows")
    return dst


class GatherRowsFn(torch.autograd.Function):
    """x = [X[ids] | indicators]  with a gradient for X (learned node embeddings, main.py:89-100): forward = gather_rows,
    backward = the rows' gradients added into a dense [N, F] gradient (float atomics: an id may repeat)."""

    @staticmethod
    def forward(ctx, X, ids, ind_code, epoch, num_ind):
        ctx.save_for_backward(ids)
        ctx.shape = X.shape
        return gather_rows(X.detach(), ids, ind_code, epoch, num_ind)

    @staticmethod
    def backward(ctx, dx):
        (ids,) = ctx.saved_tensors
        g = torch.zeros(ctx.shape, dtype=_f32, device=dx.device)
        if ids.numel():
            scatter_rows(g, ids, dx.contiguous(), atomic=True, F=ctx.shape[1])
        return g, None, None, None, None


# ------------------------------------------------------------------------------- TensorMap
def tensormap_update(map_t, keys, d_n=None):
    _chk(map_t, _i32, "map"); _chk(keys, _i32, "keys"); _chk(d_n, _i32, "d_n", True)
    _lib.check(lib().grapes_tensormap_update(_p(map_t), _p(keys), keys.numel(), _p(d_n), _stream()), "tensormap_update")


def tensormap_map(map_t, keys, out=None, d_n=None):
    _chk(map_t, _i32, "map"); _chk(keys, _i32, "keys"); _chk(d_n, _i32, "d_n", True)
    if out is None:
        out = torch.empty_like(keys)
    _chk(out, _i32, "out")
    _lib.check(lib().grapes_tensormap_map(_p(map_t), _p(keys), _p(out), keys.numel(), _p(d_n), _stream()), "tensormap_map")
    return out


# ------------------------------------------------------------------------------- frontier
def frontier_offsets(rowptr, nodes, d_m=None):
    """eoff int32[m+1] (eoff[m] = e) and a 1-element device tensor holding e."""
    _chk(rowptr, _i64, "rowptr"); _chk(nodes, _i32, "nodes"); _chk(d_m, _i32, "d_m", True)
    m = nodes.numel()
    eoff = torch.empty(m + 1, dtype=_i32, device=nodes.device)
    d_e = torch.empty(1, dtype=_i32, device=nodes.device)
    _lib.check(lib().grapes_frontier_offsets(_p(rowptr), _p(nodes), m, _p(d_m), _p(eoff), _p(d_e), _stream()),
               "frontier_offsets")
    return eoff, d_e


def frontier_expand(rowptr, col, nodes, eoff, e_cap, d_m=None, want_pos=False, status=None):
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(nodes, _i32, "nodes"); _chk(eoff, _i32, "eoff")
    dev = nodes.device
    src = torch.empty(e_cap, dtype=_i32, device=dev)
    dst = torch.empty(e_cap, dtype=_i32, device=dev)
    pos = torch.empty(e_cap, dtype=_i32, device=dev) if want_pos else None
    _lib.check(lib().grapes_frontier_expand(_p(rowptr), _p(col), _p(nodes), nodes.numel(), _p(d_m), _p(eoff), e_cap,
                                            _p(src), _p(dst), _p(pos), _p(status), _stream()), "frontier_expand")
    return src, dst, pos


class _SliceRemarkArgs(_C.Structure):
    """include/grapes_hip.h: grapes_slice_remark_args"""
    _fields_ = [("mult", _C.c_void_p), ("unmark_ids", _C.c_void_p), ("n_unmark", _C.c_int32), ("d_n_unmark", _C.c_void_p),
                ("mark_ids", _C.c_void_p), ("n_mark", _C.c_int32), ("d_n_mark", _C.c_void_p), ("clear_bits", _C.c_void_p),
                ("clear_ids", _C.c_void_p), ("n_clear", _C.c_int32), ("d_n_clear", _C.c_void_p)]


def _remark_args(remark):
    """dict(mult=, unmark=(ids, d_n)|None, mark=..., clear=..., clear_bits=) -> (ctypes struct kept alive, byref) or (None, None)"""
    if remark is None:
        return None, None
    import ctypes as C
    _chk(remark.get("mult"), _i32, "mult", True); _chk(remark.get("clear_bits"), _i64, "clear_bits", True)
    a = _SliceRemarkArgs()
    a.mult = _p(remark.get("mult"))
    for key, f_ids, f_n, f_dn in (("unmark", "unmark_ids", "n_unmark", "d_n_unmark"), ("mark", "mark_ids", "n_mark", "d_n_mark"),
                                  ("clear", "clear_ids", "n_clear", "d_n_clear")):
        ids, dn = remark.get(key) or (None, None)
        _chk(ids, _i32, key, True)
        setattr(a, f_ids, _p(ids)); setattr(a, f_n, 0 if ids is None else ids.numel()); setattr(a, f_dn, _p(dn))
    a.clear_bits = _p(remark.get("clear_bits"))
    return a, C.byref(a)


class _DrawFinishArgs(_C.Structure):
    """include/grapes_hip.h: grapes_draw_finish_args (filled by grapes_gumbel_topk_deferred)"""
    _fields_ = [("parts_keys", _C.c_void_p), ("parts_emit", _C.c_void_p), ("sel", _C.c_void_p), ("keys_blocks", _C.c_int32),
                ("emit_block", _C.c_int32), ("n_host", _C.c_int32), ("d_n", _C.c_void_p), ("stats", _C.c_void_p),
                ("hist", _C.c_void_p), ("hist_words", _C.c_int32), ("stats_blocks", _C.c_int32)]


class _HopCountArgs(_C.Structure):
    """include/grapes_hip.h: grapes_hop_count_args"""
    _fields_ = [("indeg", _C.c_void_p), ("loops", _C.c_void_p), ("seginfo", _C.c_void_p), ("wsum", _C.c_void_p),
                ("slot", _C.c_void_p), ("n_long", _C.c_void_p)]


class _HopDegreeArgs(_C.Structure):
    """include/grapes_hip.h: grapes_hop_degree_args"""
    _fields_ = [("indeg", _C.c_void_p), ("loops", _C.c_void_p), ("seginfo", _C.c_void_p), ("wsum", _C.c_void_p),
                ("rowptr_t", _C.c_void_p), ("rowptr_s", _C.c_void_p), ("dinv", _C.c_void_p), ("seg_first", _C.c_void_p),
                ("row_loops", _C.c_void_p), ("long_items", _C.c_void_p), ("n_long", _C.c_void_p), ("item_cap", _C.c_int32),
                ("sync2", _C.c_void_p), ("cursor", _C.c_void_p)]


class HopCounters:
    """Per-graph counter tables of the counted hop build (include/grapes_hip.h: grapes_hop_count_args), indexed by GLOBAL node
    id, zero at rest and left zero by the launches that use them: in-degrees, self-loop counts, edge segments of the queried
    nodes, per-bitmap-word degree sums, and the second look-back scratch of the compaction."""

    def __init__(self, num_nodes, device):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("HopCounters: first use inside a stream capture; run one eager step first")
        W = (int(num_nodes) + 63) // 64
        self.num_nodes = int(num_nodes)
        self.indeg = torch.zeros(num_nodes, dtype=_i32, device=device)
        self.loops = torch.zeros(num_nodes, dtype=_i32, device=device)
        self.seginfo = torch.zeros(2 * num_nodes, dtype=_i32, device=device)
        self.wsum = torch.zeros(2 * W, dtype=_i32, device=device)
        self.sync2 = torch.zeros(256, dtype=_i64, device=device)


class HopBuild:
    """Arrays of ONE counted hop-graph build: the expansion fills `slot`, the compaction the row starts / dinv / segments, and
    PreparedGraph.counted() the CSRs and head records (two launches instead of grapes_gcn_prepare's four)."""

    def __init__(self, n_cap, e_cap, device, counters=None, cursor_form=None):
        self.n_cap, self.e_cap = int(n_cap), int(e_cap)
        # cursor form (A/B: GRAPES_HOP_CURSOR): the expansion's in-degree atomics return nothing and the fill takes an entry's place
        # from a per-row cursor the compaction wrote; else the atomic's return value IS the place (`slot`) and the fill has no atomic
        if cursor_form is None:
            cursor_form = _sw("GRAPES_HOP_CURSOR", "0") != "0"
        self.slot = None if cursor_form else torch.empty(max(e_cap, 1), dtype=_i32, device=device)
        self.cursor = torch.empty(max(n_cap, 1), dtype=_i32, device=device) if cursor_form else None
        self.rowptr_t = torch.empty(n_cap + 1, dtype=_i32, device=device)
        self.rowptr_s = torch.empty(n_cap + 1, dtype=_i32, device=device)
        self.dinv = torch.empty(max(n_cap, 1), dtype=_f32, device=device)
        self.seg_first = torch.empty(max(n_cap, 1), dtype=_i32, device=device)
        self.row_loops = torch.empty(max(n_cap, 1), dtype=_i32, device=device)
        self.csr_dst = torch.empty(max(e_cap, 1), dtype=_i32, device=device)      # (cleared by the compaction: zero= list)
        self.item_cap = int(lib().grapes_gcn_long_items_capacity(e_cap))
        self.long_items = torch.empty(4 * self.item_cap, dtype=_i32, device=device)
        self.n_long = counters if counters is not None else torch.empty(4, dtype=_i32, device=device)

    def count_args(self, hc: "HopCounters"):
        a = _HopCountArgs()
        a.indeg, a.loops, a.seginfo, a.wsum = _p(hc.indeg), _p(hc.loops), _p(hc.seginfo), _p(hc.wsum)
        a.slot, a.n_long = _p(self.slot), _p(self.n_long)
        return a

    def degree_args(self, hc: "HopCounters"):
        a = _HopDegreeArgs()
        a.indeg, a.loops, a.seginfo, a.wsum = _p(hc.indeg), _p(hc.loops), _p(hc.seginfo), _p(hc.wsum)
        a.rowptr_t, a.rowptr_s, a.dinv = _p(self.rowptr_t), _p(self.rowptr_s), _p(self.dinv)
        a.seg_first, a.row_loops = _p(self.seg_first), _p(self.row_loops)
        a.long_items, a.n_long, a.item_cap = _p(self.long_items), _p(self.n_long), self.item_cap
        a.sync2 = _p(hc.sync2)
        a.cursor = _p(self.cursor)
        return a


def slice_stage(e_cap, device):
    """Scratch for frontier_expand_fused(slice_stage=) -> PreparedGraph.small_batch(stages=): no clearing needed."""
    return torch.empty(int(lib().grapes_slice_stage_words(e_cap)), dtype=_i32, device=device)


def frontier_expand_fused(rowptr, col, nodes, e_cap, d_m=None, status=None, mark_prev_bits=None, mark_bits=None,
                          num_nodes=0, remark=None, count_mult=None, count_bsum=None, slice_stage=None, count=None, finish=None,
                          node_ext=None, node_ext_out=None):
    """frontier_offsets + frontier_expand in one launch (<= 2048 queried nodes): (src, dst, d_e, eoff).
    mark_bits (+ mark_prev_bits, num_nodes): also the hop's bitmap marks (bitmap_mark_hop) in the same launch.
    remark = dict(mult=, unmark=(ids, d_n)|None, mark=(ids, d_n)|None, clear=(ids, d_n)|None, clear_bits=): slice_remark in
    the same launch (clear_bits must not be mark_prev_bits).  count_mult + count_bsum: also slice_filter's counting half
    over the produced edges (count_bsum zeroed by the caller; pass it to slice_filter(bsum=...))."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(nodes, _i32, "nodes")
    _chk(mark_prev_bits, _i64, "mark_prev_bits", True); _chk(mark_bits, _i64, "mark_bits", True)
    m, dev = nodes.numel(), nodes.device
    eoff = torch.empty(m + 1, dtype=_i32, device=dev)
    d_e = torch.empty(1, dtype=_i32, device=dev)
    src = torch.empty(e_cap, dtype=_i32, device=dev)
    dst = torch.empty(e_cap, dtype=_i32, device=dev)
    _keep, rm = _remark_args(remark)
    _chk(count_mult, _i32, "count_mult", True); _chk(count_bsum, _i32, "count_bsum", True); _chk(slice_stage, _i32, "slice_stage", True)
    if slice_stage is not None and slice_stage.numel() < int(lib().grapes_slice_stage_words(e_cap)):
        raise ValueError("frontier_expand_fused: slice_stage needs grapes_slice_stage_words(e_cap) words")
    # node_ext int64[2 m]: the queried rows' (rowptr[id], rowptr[id + 1]) written by the draw that produced `nodes`
    # (gumbel_topk(ext=...)["union_ext"]): one dependent round trip less; node_ext_out int64[2 m]: the extents this launch finds itself
    _chk(node_ext, _i64, "node_ext", True); _chk(node_ext_out, _i64, "node_ext_out", True)
    if (node_ext is not None and node_ext.numel() < 2 * m) or (node_ext_out is not None and node_ext_out.numel() < 2 * m):
        raise ValueError("frontier_expand_fused: node_ext / node_ext_out hold two int64 per queried node")
    if finish is not None or node_ext is not None or node_ext_out is not None or count is not None:
        # finish = gumbel_topk(defer_finish=True)["finish"]: one more workgroup ends that draw;
        # count = (HopCounters, HopBuild): the hop graph's degree counting rides in this launch
        import ctypes as C
        ca = None
        if count is not None:
            if count[1].e_cap < e_cap:
                raise ValueError("frontier_expand_fused: the HopBuild's slot array is smaller than e_cap")
            ca = count[1].count_args(count[0])
        _lib.check(lib().grapes_frontier_expand_fused_ext(_p(rowptr), _p(col), _p(nodes), m, _p(d_m), e_cap, _p(eoff), _p(d_e),
                                                          _p(src), _p(dst), _p(status), _p(mark_prev_bits), _p(mark_bits),
                                                          int(num_nodes), rm, _p(count_mult), _p(count_bsum), _p(slice_stage),
                                                          C.byref(ca) if ca is not None else None,
                                                          C.byref(finish[0]) if finish is not None else None,
                                                          _p(node_ext), _p(node_ext_out), _stream()),
                   "frontier_expand_fused_ext")
        return src, dst, d_e, eoff
    _lib.check(lib().grapes_frontier_expand_fused(_p(rowptr), _p(col), _p(nodes), m, _p(d_m), e_cap, _p(eoff), _p(d_e),
                                                  _p(src), _p(dst), _p(status), _p(mark_prev_bits), _p(mark_bits), int(num_nodes),
                                                  rm, _p(count_mult), _p(count_bsum), _p(slice_stage), _stream()), "frontier_expand_fused")
    return src, dst, d_e, eoff


# ------------------------------------------------------------------------------- bitmaps / compaction
def bitmap_mark(bits, bits1, ids, num_nodes, d_n=None, status=None):
    _chk(bits, _i64, "bits"); _chk(bits1, _i64, "bits1", True); _chk(ids, _i32, "ids")
    _lib.check(lib().grapes_bitmap_mark(_p(bits), _p(bits1), _p(ids), ids.numel(), _p(d_n), num_nodes, _p(status),
                                        _stream()), "bitmap_mark")


def bitmap_mark_rows(bits, bits1, nodes, eoff, num_nodes, d_m=None, status=None):
    """Marks the queried nodes that have >= 1 out-edge (the source endpoints of the frontier)."""
    _chk(bits, _i64, "bits"); _chk(bits1, _i64, "bits1", True); _chk(nodes, _i32, "nodes"); _chk(eoff, _i32, "eoff")
    _lib.check(lib().grapes_bitmap_mark_rows(_p(bits), _p(bits1), _p(nodes), nodes.numel(), _p(d_m), _p(eoff), num_nodes,
                                             _p(status), _stream()), "bitmap_mark_rows")


def bitmap_clear(bits, ids, d_n=None):
    _chk(bits, _i64, "bits"); _chk(ids, _i32, "ids")
    _lib.check(lib().grapes_bitmap_clear(_p(bits), _p(ids), ids.numel(), _p(d_n), _stream()), "bitmap_clear")


def bitmap_mark_hop(prev_bits, bits, bits1, previous, eoff, dst, num_nodes, d_m=None, d_e=None, status=None):
    """The three marks of a hop in one launch (== bitmap_mark(prev) + bitmap_mark_rows + bitmap_mark(dst))."""
    _chk(prev_bits, _i64, "prev_bits"); _chk(bits, _i64, "bits"); _chk(bits1, _i64, "bits1", True)
    _chk(previous, _i32, "previous"); _chk(eoff, _i32, "eoff"); _chk(dst, _i32, "dst")
    _lib.check(lib().grapes_bitmap_mark_hop(_p(prev_bits), _p(bits), _p(bits1), _p(previous), previous.numel(), _p(d_m),
                                            _p(eoff), _p(dst), dst.numel(), _p(d_e), num_nodes, _p(status), _stream()),
               "bitmap_mark_hop")


def bitmap_mark_lists(bits, bits1, lists, num_nodes, status=None, unmark_mult=None):
    """lists: up to four (ids, d_n or None) pairs marked in one launch.  unmark_mult: the slice multiplicity table, zeroed
    at every listed id in the same launch (see slice_remark)."""
    _chk(bits, _i64, "bits"); _chk(bits1, _i64, "bits1", True); _chk(unmark_mult, _i32, "unmark_mult", True)
    if len(lists) > 4:
        raise ValueError("at most four lists per launch")
    args = []
    for ids, d_n in list(lists) + [(None, None)] * (4 - len(lists)):
        _chk(ids, _i32, "ids", True)
        args += [_p(ids), 0 if ids is None else ids.numel(), _p(d_n)]
    _lib.check(lib().grapes_bitmap_mark_lists(_p(bits), _p(bits1), *args, num_nodes, _p(status), _p(unmark_mult), _stream()),
               "bitmap_mark_lists")


def union_sorted(lists, num_nodes, n_cap, node_map=None, status=None, unmark_mult=None):
    """Ascending duplicate-free union of up to four (ids, d_n or None) lists with at most 4096 ids in all, by one workgroup:
    (all_ids[n_cap], counts[2]); node_map[id] = rank; unmark_mult zeroed at the ids."""
    if not (1 <= len(lists) <= 4) or sum(ids.numel() for ids, _ in lists) > 4096:
        raise ValueError("union_sorted: 1..4 lists, at most 4096 ids in all")
    _chk(node_map, _i32, "node_map", True); _chk(unmark_mult, _i32, "unmark_mult", True)
    dev = lists[0][0].device
    args = []
    for ids, d_n in list(lists) + [(None, None)] * (4 - len(lists)):
        _chk(ids, _i32, "ids", True)
        args += [_p(ids), 0 if ids is None else ids.numel(), _p(d_n)]
    out = torch.empty(n_cap, dtype=_i32, device=dev)
    counts = torch.empty(2, dtype=_i32, device=dev)
    _lib.check(lib().grapes_union_sorted(*args, num_nodes, n_cap, _p(out), _p(node_map), _p(counts), _p(unmark_mult), _p(status),
                                         _stream()), "union_sorted")
    return out, counts


def frontier_compact(bits, bits1, prev_bits, num_nodes, n_cap, node_map=None, status=None, ind_code=None, epoch=0,
                     d_epoch=None, ind_bit=0, sync=None, one_launch=True, want_cand_pos=False, zero=(), remark=None,
                     degrees=None):
    """Returns (batch_nodes[n_cap], neighbor_nodes[n_cap], nb_local[n_cap], counts[2]) — ascending ids.
    ind_code: also set indicator bit `ind_bit` of every emitted neighbour (main.py:191)."""
    _chk(ind_code, _i32, "ind_code", True)
    _chk(bits, _i64, "bits"); _chk(bits1, _i64, "bits1", True); _chk(prev_bits, _i64, "prev_bits", True)
    _chk(node_map, _i32, "node_map", True)
    dev = bits.device
    batch = torch.empty(n_cap, dtype=_i32, device=dev)
    neigh = torch.empty(n_cap, dtype=_i32, device=dev)
    nbl = torch.empty(n_cap, dtype=_i32, device=dev)
    counts = torch.empty(2, dtype=_i32, device=dev)
    ws = _ws(lib().grapes_frontier_compact_workspace_bytes(n_cap, num_nodes), dev)
    if sync is None and one_launch:
        sync = sync_scratch(dev)
    _chk(sync, _i64, "sync", True)
    cand_pos = torch.empty(n_cap, dtype=_i32, device=dev) if want_cand_pos else None
    # zero: up to three (tensor, words) pairs the launch also clears (scratch of the operation that follows)
    _keep, crm = _remark_args(remark)
    zargs = []
    for zt, zw in list(zero)[:3] + [(None, 0)] * (3 - len(list(zero)[:3])):
        zargs += [_p(zt), int(zw)]
    if degrees is not None:    # degrees = (HopCounters, HopBuild): row starts, dinv and segments of the hop graph from this launch
        import ctypes as C
        if degrees[1].n_cap < n_cap:
            raise ValueError("frontier_compact: the HopBuild is smaller than n_cap")
        da = degrees[1].degree_args(degrees[0])
        _lib.check(lib().grapes_frontier_compact_counted(_p(bits), _p(bits1), _p(prev_bits), num_nodes, n_cap, _p(batch), _p(neigh),
                                                         _p(nbl), _p(node_map), _p(counts), _p(ind_code), epoch, _p(d_epoch),
                                                         ind_bit, _p(cand_pos), *zargs, crm, _p(ws), _p(sync), _p(status),
                                                         C.byref(da), _stream()), "frontier_compact_counted")
    else:
        _lib.check(lib().grapes_frontier_compact(_p(bits), _p(bits1), _p(prev_bits), num_nodes, n_cap, _p(batch), _p(neigh),
                                                 _p(nbl), _p(node_map), _p(counts), _p(ind_code), epoch, _p(d_epoch), ind_bit,
                                                 _p(cand_pos), *zargs, crm, _p(ws), _p(sync), _p(status), _stream()),
                   "frontier_compact")
    if want_cand_pos:
        return batch, neigh, nbl, counts, cand_pos
    return batch, neigh, nbl, counts


# ------------------------------------------------------------------------------- slice
def slice_mark(mult, cols, unmark=False, d_c=None, clear_bits=None):
    _chk(mult, _i32, "mult"); _chk(cols, _i32, "cols"); _chk(clear_bits, _i64, "clear_bits", True)
    _lib.check(lib().grapes_slice_mark(_p(mult), _p(cols), cols.numel(), _p(d_c), 1 if unmark else 0, _p(clear_bits),
                                       _stream()), "slice_mark")


def slice_remark(mult, unmark=None, mark=None, clear=None, clear_bits=None):
    """unmark / mark / clear: (ids, d_n or None) or None.  One launch: zero mult at `unmark`, +1 at `mark` (the two lists
    must be disjoint), zero the words of `clear_bits` holding `clear`."""
    _chk(mult, _i32, "mult"); _chk(clear_bits, _i64, "clear_bits", True)
    args = []
    for pair in (unmark, mark):
        ids, d_n = pair if pair is not None else (None, None)
        _chk(ids, _i32, "ids", True)
        args += [_p(ids), 0 if ids is None else ids.numel(), _p(d_n)]
    ids, d_n = clear if clear is not None else (None, None)
    _chk(ids, _i32, "clear ids", True)
    _lib.check(lib().grapes_slice_remark(_p(mult), *args, _p(clear_bits), _p(ids), 0 if ids is None else ids.numel(), _p(d_n),
                                         _stream()), "slice_remark")


def slice_filter_bsum(e_cap, device):
    """Zeroed per-1024-edge-block survivor counters for frontier_expand_fused(count_bsum=) + slice_filter(bsum=)."""
    return torch.zeros(max(int(lib().grapes_slice_filter_workspace_bytes(e_cap)) // 4, 1), dtype=_i32, device=device)


def slice_filter(mult, src, dst, out_cap, d_e=None, status=None, one_launch=None, bsum=None):
    """one_launch: the look-back form (default: GRAPES_ONE_LAUNCH_SLICE, off — 7 us/step slower than two launches).
    bsum: survivor counts already formed by the expansion that produced src / dst (only the emitting launch runs)."""
    if one_launch is None:
        one_launch = _ONE_LAUNCH_SLICE
    _chk(mult, _i32, "mult"); _chk(src, _i32, "src"); _chk(dst, _i32, "dst")
    dev = src.device
    out_src = torch.empty(out_cap, dtype=_i32, device=dev)
    out_dst = torch.empty(out_cap, dtype=_i32, device=dev)
    cnt = torch.empty(1, dtype=_i32, device=dev)
    _chk(bsum, _i32, "bsum", True)
    ws = bsum if bsum is not None else _ws(lib().grapes_slice_filter_workspace_bytes(src.numel()), dev)
    _lib.check(lib().grapes_slice_filter(_p(mult), _p(src), _p(dst), src.numel(), _p(d_e), out_cap, _p(out_src),
                                         _p(out_dst), _p(cnt), _p(ws), _p(sync_scratch(dev)) if one_launch else None,
                                         1 if bsum is not None else 0, _p(status), _stream()), "slice_filter")
    return out_src, out_dst, cnt


# ------------------------------------------------------------------------------- features
def indicator_mark(ind_code, ids, epoch, bit, d_n=None, d_epoch=None, advance_epoch=False):
    """advance_epoch: a new batch — marks with *d_epoch + 1 and stores that back (no separate counter launch)."""
    _chk(ind_code, _i32, "ind_code"); _chk(ids, _i32, "ids")
    _lib.check(lib().grapes_indicator_mark(_p(ind_code), _p(ids), ids.numel(), _p(d_n), epoch, _p(d_epoch), bit,
                                           1 if advance_epoch else 0, _stream()), "indicator_mark")


def step_begin(ids32, d_cursor, stride, offset, targets, ind_code=None, d_epoch=None, bit=0, counters=None, totals=None):
    """First launch of a self-feeding captured step: next batch of target ids from the device-resident id array, cursor and
    epoch advanced, target indicators marked, the previous step's edge counters (counters[:, col] view) added to totals."""
    _chk(ids32, _i32, "ids"); _chk(d_cursor, _i32, "d_cursor"); _chk(targets, _i32, "targets")
    _chk(ind_code, _i32, "ind_code", True); _chk(d_epoch, _i32, "d_epoch", True); _chk(totals, _i64, "totals", True)
    cs, nc = (int(counters.stride(0)), int(counters.numel())) if counters is not None else (1, 0)
    _lib.check(lib().grapes_step_begin(_p(ind_code), _p(d_epoch), bit, _p(ids32), ids32.numel(), _p(d_cursor), int(stride),
                                       int(offset), targets.numel(), _p(targets), _p(counters), cs, nc, _p(totals), _stream()),
               "step_begin")


def gather_rows(X, ids, ind_code=None, epoch=0, num_ind=0, d_n=None, out=None, d_epoch=None):
    _chk(X, _f32, "X"); _chk(ids, _i32, "ids"); _chk(ind_code, _i32, "ind_code", True)
    n, F = ids.numel(), X.shape[1]
    if out is None:
        out = torch.empty((n, F + num_ind), dtype=_f32, device=X.device)
    _lib.check(lib().grapes_gather_rows(_p(X), F, _p(ids), n, _p(d_n), _p(ind_code), epoch, _p(d_epoch), num_ind, _p(out),
                                        _stream()),
               "gather_rows")
    return out


# ------------------------------------------------------------------------------- GCN
_SMALL_GRAPH = 2048      # <= this many nodes (the classifier's sampled subgraphs): no split of long rows into work items


class PreparedGraph:
    """gcn_norm + CSR by target / by source of one (local) edge list."""

    __slots__ = ("n", "e", "d_n", "d_e", "rowptr_t", "csr_src", "rowptr_s", "csr_dst", "dinv", "status",
                 "long_items", "n_long", "item_cap", "items_t", "items_s", "n_items_t", "n_items_s",
                 "items_fwd", "row_head", "head_ids", "head_local", "loops")

    @staticmethod
    def scratch(n, e, device):
        """(workspace, csr_dst, [(tensor, words), ...]): the build's scratch allocated ahead of it, with the ranges an earlier
        launch (frontier_compact(zero=...)) has to clear for `prezeroed=True`."""
        ws = _ws(lib().grapes_gcn_prepare_workspace_bytes(n, e), device)
        csr_dst = torch.empty(max(e, 1), dtype=_i32, device=device)
        return ws, csr_dst, [(ws, lib().grapes_gcn_prepare_zero_words(n)), (csr_dst, e)]

    def __init__(self, edge_src, edge_dst, n, d_n=None, d_e=None, status=None, src_grouped=False, items_fwd=True,
                 node_map=None, head_ids=None, counters=None, scratch=None, prefetch=None, head_local=False):
        """node_map: edge_src / edge_dst are GLOBAL ids, relabelled through this table inside the build.
        head_local: head_ids is 0, 1, 2, ... — the head records then hold LOCAL ids and drive the record form of the
        aggregation over [n, f] activations (gcn_aggregate_fwd / _fwd_head -> grapes_gcn_aggregate_fwd_rec).
        head_ids: int32[n] feature-matrix row of every local node (the hop's batch_nodes): the build also writes the
        per-row head records the fused gather-SpMM (gcn_aggregate_gather) reads.
        counters: int32[4] to use for the build's device counters ([2] = aggregated edges), e.g. a row of a caller's table."""
        _chk(head_ids, _i32, "head_ids", True); _chk(counters, _i32, "counters", True)
        _chk(edge_src, _i32, "edge_src"); _chk(edge_dst, _i32, "edge_dst"); _chk(node_map, _i32, "node_map", True)
        dev = edge_src.device
        e = edge_src.numel()
        self.n, self.e, self.d_n, self.d_e, self.status = n, e, d_n, d_e, status
        # items_fwd=False: the forward (by-target) aggregation runs as ONE launch, every row by one wavefront —
        # right for frontier graphs, whose in-degrees are tiny (<= number of source rows); still correct otherwise
        self.items_fwd = items_fwd
        self.rowptr_t = torch.empty(n + 1, dtype=_i32, device=dev)
        self.rowptr_s = torch.empty(n + 1, dtype=_i32, device=dev)
        self.csr_src = torch.empty(max(e, 1), dtype=_i32, device=dev)
        self.csr_dst = scratch[1] if scratch is not None else torch.empty(max(e, 1), dtype=_i32, device=dev)
        self.dinv = torch.empty(max(n, 1), dtype=_f32, device=dev)
        self.item_cap = lib().grapes_gcn_long_items_capacity(e)
        self.long_items = torch.empty(4 * self.item_cap, dtype=_i32, device=dev)
        self.n_long = counters if counters is not None else torch.empty(4, dtype=_i32, device=dev)
        self.items_t, self.items_s = self.long_items[: 2 * self.item_cap], self.long_items[2 * self.item_cap:]
        self.n_items_t, self.n_items_s = self.n_long[0:1], self.n_long[1:2]
        self.head_ids = head_ids
        self.head_local = bool(head_local) and head_ids is not None
        self.row_head = torch.empty((max(n, 1), 12), dtype=_i32, device=dev) if (head_ids is not None and e > 0) else None
        ws = scratch[0] if scratch is not None else _ws(lib().grapes_gcn_prepare_workspace_bytes(n, e), dev)
        flags = (1 if src_grouped else 0) | (2 if scratch is not None else 0)
        args = (_p(edge_src), _p(edge_dst), e, _p(d_e), _p(node_map), n, _p(d_n), flags,
                _p(self.rowptr_t), _p(self.csr_src), _p(self.rowptr_s), _p(self.csr_dst),
                _p(self.dinv), _p(self.long_items), _p(self.n_long),
                _p(head_ids) if self.row_head is not None else None, _p(self.row_head),
                _p(ws), _p(sync_scratch(dev)) if _ONE_LAUNCH_PREP else None, _p(status))
        if prefetch is not None and head_ids is not None and _PREFETCH_ROWS:
            # prefetch = (X, row_floats): the build's first launch also touches X[head_ids] (the gather-SpMM's rows; see the header)
            _lib.check(lib().grapes_gcn_prepare_prefetching(*args, _p(prefetch[0]), int(prefetch[0].stride(0)), int(prefetch[1]),
                                                            _stream()), "gcn_prepare_prefetching")
        else:
            _lib.check(lib().grapes_gcn_prepare(*args, _stream()), "gcn_prepare")

    @classmethod
    def counted(cls, edge_src, edge_dst, hb: "HopBuild", n, d_n, d_e, node_map, status=None, head_ids=None, prefetch=None,
                head_local=False):
        """The hop graph from a COUNTED expansion + compaction (frontier_expand_fused(count=), frontier_compact(degrees=) over the
        same HopBuild): the two remaining launches of the build.  Same arrays as PreparedGraph(src_grouped=True, node_map=...)."""
        _chk(edge_src, _i32, "edge_src"); _chk(edge_dst, _i32, "edge_dst"); _chk(node_map, _i32, "node_map"); _chk(head_ids, _i32, "head_ids", True)
        dev = edge_src.device
        e = edge_src.numel()
        g = object.__new__(cls)
        g.n, g.e, g.d_n, g.d_e, g.status, g.items_fwd = n, e, d_n, d_e, status, False
        g.rowptr_t, g.rowptr_s, g.dinv, g.csr_dst = hb.rowptr_t, hb.rowptr_s, hb.dinv, hb.csr_dst
        g.csr_src = torch.empty(max(e, 1), dtype=_i32, device=dev)
        g.item_cap, g.long_items, g.n_long = hb.item_cap, hb.long_items, hb.n_long
        g.items_t, g.items_s = g.long_items[: 2 * g.item_cap], g.long_items[2 * g.item_cap:]
        g.n_items_t, g.n_items_s = g.n_long[0:1], g.n_long[1:2]
        g.head_ids = head_ids
        g.head_local = bool(head_local) and head_ids is not None
        g.row_head = torch.empty((max(n, 1), 12), dtype=_i32, device=dev) if head_ids is not None else None
        tmp = _tmp(torch.empty(max(e, 1), dtype=_i32, device=dev))
        pf = prefetch if (prefetch is not None and head_ids is not None and _PREFETCH_ROWS) else None
        _lib.check(lib().grapes_gcn_prepare_counted(_p(edge_src), _p(edge_dst), _p(hb.slot), e, _p(d_e), _p(node_map), n, _p(d_n),
                                                    _p(hb.rowptr_t), _p(hb.rowptr_s), _p(hb.seg_first), _p(hb.row_loops), _p(hb.dinv),
                                                    _p(g.csr_src), _p(g.csr_dst), _p(tmp), _p(head_ids), _p(g.row_head), _p(status),
                                                    _p(pf[0]) if pf else None, int(pf[0].stride(0)) if pf else 0,
                                                    int(pf[1]) if pf else 0, _p(hb.cursor), _stream()), "gcn_prepare_counted")
        return g

    @classmethod
    def small_batch(cls, edge_lists, n, d_n=None, status=None, node_map=None, head_ids=None, counters=None, stages=None):
        """Several graphs over the SAME n <= 2048 nodes in one launch (one workgroup each): edge_lists =
        [(edge_src, edge_dst, d_e), ...] in frontier (source-grouped) order.  Returns the PreparedGraphs.
        stages: per graph None or (slice_stage, d_fe, fe_cap) — the edge list (edge_src / edge_dst / d_e: outputs then) is
        first assembled from the stage a frontier_expand_fused(slice_stage=) launch left (slice_adjacency without a launch)."""
        import ctypes as C
        if not (1 <= len(edge_lists) <= 8) or n > _SMALL_GRAPH:
            raise ValueError("small_batch: 1..8 graphs of at most %d nodes" % _SMALL_GRAPH)
        outs, wss = [], []
        for gi, (es, ed, d_e) in enumerate(edge_lists):
            _chk(es, _i32, "edge_src"); _chk(ed, _i32, "edge_dst")
            dev, e = es.device, es.numel()
            g = object.__new__(cls)
            g.n, g.e, g.d_n, g.d_e, g.status, g.items_fwd = n, e, d_n, d_e, status, True
            g.rowptr_t = torch.empty(n + 1, dtype=_i32, device=dev); g.rowptr_s = torch.empty(n + 1, dtype=_i32, device=dev)
            g.csr_src = torch.empty(max(e, 1), dtype=_i32, device=dev); g.csr_dst = torch.empty(max(e, 1), dtype=_i32, device=dev)
            g.dinv = torch.empty(max(n, 1), dtype=_f32, device=dev)
            g.item_cap = lib().grapes_gcn_long_items_capacity(e)
            g.long_items = torch.empty(4 * g.item_cap, dtype=_i32, device=dev)
            g.n_long = counters[gi] if counters is not None else torch.empty(4, dtype=_i32, device=dev)
            g.items_t, g.items_s = g.long_items[: 2 * g.item_cap], g.long_items[2 * g.item_cap:]
            g.n_items_t, g.n_items_s = g.n_long[0:1], g.n_long[1:2]
            g.head_ids = head_ids
            g.head_local = False
            g.row_head = torch.empty((max(n, 1), 12), dtype=_i32, device=dev) if head_ids is not None else None
            outs.append(g)
            wss.append(_ws(lib().grapes_gcn_prepare_workspace_bytes(n, e), dev))
        k = len(outs)
        arr = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
        ecnt = (C.c_int32 * k)(*[g.e for g in outs])
        _lib.check(lib().grapes_gcn_prepare_small_batch(
            k, arr([el[0] for el in edge_lists]), arr([el[1] for el in edge_lists]), ecnt, arr([el[2] for el in edge_lists]),
            _p(node_map), n, _p(d_n), arr([g.rowptr_t for g in outs]), arr([g.csr_src for g in outs]),
            arr([g.rowptr_s for g in outs]), arr([g.csr_dst for g in outs]), arr([g.dinv for g in outs]),
            arr([g.long_items for g in outs]), arr([g.n_long for g in outs]), _p(head_ids),
            arr([g.row_head for g in outs]), arr(wss),
            arr([None if st is None else st[0] for st in stages]) if stages is not None else None,
            arr([None if st is None else st[1] for st in stages]) if stages is not None else None,
            (C.c_int32 * k)(*[0 if st is None else int(st[2]) for st in stages]) if stages is not None else None,
            _p(status), _stream()), "gcn_prepare_small_batch")
        return outs

    @classmethod
    def from_csr(cls, rowptr_t32, csr_src, n, rowptr_s32=None, csr_dst=None):
        """Full-graph form: an int32 CSR by target (ascending columns, no self-loops) and, for the backward
        pass, optionally the CSR by source (for a symmetric graph the same arrays)."""
        _chk(rowptr_t32, _i32, "rowptr_t"); _chk(csr_src, _i32, "csr_src")
        dev = rowptr_t32.device
        self = object.__new__(cls)
        e = csr_src.numel()
        self.n, self.e, self.d_n, self.d_e, self.status, self.items_fwd = n, e, None, None, None, True
        self.row_head = self.head_ids = None
        self.head_local = False
        self.rowptr_t, self.csr_src = rowptr_t32, csr_src
        self.rowptr_s, self.csr_dst = (rowptr_s32, csr_dst) if rowptr_s32 is not None else (rowptr_t32, csr_src)
        self.dinv = torch.empty(max(n, 1), dtype=_f32, device=dev)
        self.item_cap = lib().grapes_gcn_long_items_capacity(e)
        self.long_items = torch.empty(4 * self.item_cap, dtype=_i32, device=dev)
        self.n_long = torch.zeros(4, dtype=_i32, device=dev)
        self.n_long[2] = e
        self.items_t, self.items_s = self.long_items[: 2 * self.item_cap], self.long_items[2 * self.item_cap:]
        self.n_items_t, self.n_items_s = self.n_long[0:1], self.n_long[1:2]
        _lib.check(lib().grapes_gcn_prepare_from_csr(_p(self.rowptr_t), n, _p(self.dinv), _p(self.items_t),
                                                     _p(self.n_items_t), self.item_cap, _stream()), "gcn_prepare_from_csr")
        if rowptr_s32 is None:      # symmetric: the by-source items are the by-target items
            self.items_s, self.n_items_s = self.items_t, self.n_items_t
        else:
            tmp = torch.empty_like(self.dinv)
            _lib.check(lib().grapes_gcn_prepare_from_csr(_p(self.rowptr_s), n, _p(tmp), _p(self.items_s),
                                                         _p(self.n_items_s), self.item_cap, _stream()), "gcn_prepare_from_csr")
        return self

    @property
    def num_edges_no_loops(self) -> torch.Tensor:
        """1-element device tensor: number of aggregated (non-self-loop) edges (also valid for capacity-padded
        graphs whose true sizes live on the device)."""
        return self.n_long[2:3]


def linear_fwd(x, w, d_n=None, out=None):
    _chk(x, _f32, "x"); _chk(w, _f32, "w")
    n, fi = x.shape
    fo = w.shape[0]
    if w.shape[1] != fi:
        raise ValueError("weight / input width mismatch")
    if out is None:
        out = torch.empty((n, fo), dtype=_f32, device=x.device)
    _lib.check(lib().grapes_linear_fwd(_p(x), _p(w), _p(out), n, _p(d_n), fi, fo, _stream()), "linear_fwd")
    return out


def eval_predict(logits, node_map, targets, status=None, want_rows=True):
    """eval.py:154-155: (argmax of the targets' logit rows [B] int64, the rows [B, C] or None) in one launch."""
    _chk(logits, _f32, "logits"); _chk(node_map, _i32, "node_map"); _chk(targets, _i32, "targets"); _chk(status, _i32, "status", True)
    n, c = logits.shape
    b = targets.numel()
    pred = torch.empty(b, dtype=_i64, device=logits.device)
    rows = torch.empty((b, c), dtype=_f32, device=logits.device) if want_rows else None
    _lib.check(lib().grapes_eval_predict(_p(logits), n, c, _p(node_map), _p(targets), b, _p(pred), _p(rows), _p(status), _stream()),
               "eval_predict")
    return pred, rows


def linear_fwd_row_scaled(x, w, row_scale, d_n=None, out=None):
    """diag(row_scale) · x wᵀ in one launch (the full-batch inference transform: rows leave the GEMM scaled by dinv) — the same bits
    as scale_rows(linear_fwd(x, w), row_scale)."""
    _chk(x, _f32, "x"); _chk(w, _f32, "w"); _chk(row_scale, _f32, "row_scale")
    n, fi = x.shape
    fo = w.shape[0]
    if w.shape[1] != fi or row_scale.numel() < n:
        raise ValueError("weight / input width or scale length mismatch")
    if out is None:
        out = torch.empty((n, fo), dtype=_f32, device=x.device)
    _lib.check(lib().grapes_linear_fwd_row_scaled(_p(x), _p(w), _p(row_scale), _p(out), n, _p(d_n), fi, fo, _stream()),
               "linear_fwd_row_scaled")
    return out


def linear_bwd_weight(dh, x, d_n=None, out=None, accumulate=False, defer=None):
    _chk(dh, _f32, "dh"); _chk(x, _f32, "x")
    n, fi = x.shape
    fo = dh.shape[1]
    if out is None:
        out = torch.empty((fo, fi), dtype=_f32, device=x.device)
        accumulate = False
    if defer is not None and fo > 1 and defer.try_add(dh, None, x, d_n, out, None, accumulate):
        return out
    ws = _ws(lib().grapes_linear_bwd_weight_workspace_bytes(n, fi, fo), x.device)
    _lib.check(lib().grapes_linear_bwd_weight(_p(dh), _p(x), _p(out), n, _p(d_n), fi, fo, 1 if accumulate else 0, _p(ws),
                                              _stream()), "linear_bwd_weight")
    return out


def linear_bwd_weight_and_input(dh, x, w, d_n=None, out=None, accumulate=False, defer=None):
    """(dW = dhᵀ x, dx = dh w) of one linear map (modules/gcn.py:32,36 backward).  With defer (a DeferredSlabs) and shapes of the
    two few-row kernels both run as ONE launch; otherwise the two separate entry points.  -> dx"""
    _chk(dh, _f32, "dh"); _chk(x, _f32, "x"); _chk(w, _f32, "w")
    n, fi = x.shape
    fo = dh.shape[1]
    if defer is not None and fo > 1 and out is not None:
        dx = torch.empty((n, fi), dtype=_f32, device=dh.device)
        if defer.try_add(dh, None, x, d_n, out, None, accumulate, w=w, dx=dx):
            return dx
    linear_bwd_weight(dh, x, d_n=d_n, out=out, accumulate=accumulate, defer=defer)
    return linear_bwd_input(dh, w, d_n=d_n)


def linear_bias_act_fwd(x, w, bias=None, relu=False, d_n=None, out=None):
    """act(x Wᵀ + b) in one GEMM (aggregate-first layers)."""
    _chk(x, _f32, "x"); _chk(w, _f32, "w"); _chk(bias, _f32, "bias", True)
    n, fi = x.shape
    fo = w.shape[0]
    if out is None:
        out = torch.empty((n, fo), dtype=_f32, device=x.device)
    _lib.check(lib().grapes_linear_bias_act_fwd(_p(x), _p(w), _p(bias), 1 if relu else 0, _p(out), n, _p(d_n), fi, fo,
                                                _stream()), "linear_bias_act_fwd")
    return out


def linear_bias_act_head_fwd(x, w, bias, relu, head_w, d_n=None):
    """(act(x Wᵀ + b), its product with the 1-wide head weight head_w [1, F_out] or [F_out]) — one launch where the
    bf16x3 GEMM applies."""
    _chk(x, _f32, "x"); _chk(w, _f32, "w"); _chk(bias, _f32, "bias", True); _chk(head_w, _f32, "head_w")
    n, fi = x.shape
    fo = w.shape[0]
    if head_w.numel() != fo:
        raise ValueError("linear_bias_act_head_fwd: head_w must have F_out elements")
    out = torch.empty((n, fo), dtype=_f32, device=x.device)
    head = torch.empty((n, 1), dtype=_f32, device=x.device)
    _lib.check(lib().grapes_linear_bias_act_head_fwd(_p(x), _p(w), _p(bias), 1 if relu else 0, _p(out), _p(head_w), _p(head),
                                                     n, _p(d_n), fi, fo, _stream()), "linear_bias_act_head_fwd")
    return out, head


def split_gemm_available(n, f_in, f_out) -> bool:
    """True where the bf16x3 forward / dW kernels (and with them the strided-input forms below) apply."""
    return bool(lib().grapes_split_gemm_available(int(n), int(f_in), int(f_out)))


def _row_strided(x, f_in, name):
    """x: fp32 [n, >= f_in] whose rows may be a column-slice view of a wider contiguous matrix."""
    if x.dtype != _f32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] != f_in:
        raise _lib.GrapesHipError(f"{name}: expected a CUDA fp32 [n, {f_in}] matrix with unit column stride")
    return int(x.stride(0))


def linear_relu_head_fwd_bits_pair(x, w, bias, head_w, x_b, w_b, bias_b, head_w_b, d_n=None):
    """Two linear_relu_head_fwd_bits over the SAME rows in one launch (the sampler net's and the log-Z net's first layers at hop 0):
    -> (GateBits, head, GateBits_b, head_b), or None where the pair kernel does not take the shapes (call them separately)."""
    for t, nm in ((w, "w"), (bias, "bias"), (head_w, "head_w"), (w_b, "w_b"), (bias_b, "bias_b"), (head_w_b, "head_w_b")):
        _chk(t, _f32, nm)
    n, fi = x.shape
    fib = x_b.shape[1]
    fo = w.shape[0]
    if x_b.shape[0] != n or w_b.shape[0] != fo:
        return None
    ldx, ldxb = _row_strided(x, fi, "linear_relu_head_fwd_bits_pair"), _row_strided(x_b, fib, "linear_relu_head_fwd_bits_pair")
    nw = (fo + 31) // 32
    words = torch.empty((n, nw), dtype=torch.int32, device=x.device); head = torch.empty((n, 1), dtype=_f32, device=x.device)
    words_b = torch.empty((n, nw), dtype=torch.int32, device=x.device); head_b = torch.empty((n, 1), dtype=_f32, device=x.device)
    rc = lib().grapes_linear_relu_head_fwd_bits_pair(x.data_ptr(), ldx, _p(w), _p(bias), _p(head_w), _p(words), _p(head),
                                                     x_b.data_ptr(), ldxb, _p(w_b), _p(bias_b), _p(head_w_b), _p(words_b), _p(head_b),
                                                     fib, n, _p(d_n), fi, fo, _stream())
    if rc == -1:
        return None
    _lib.check(rc, "linear_relu_head_fwd_bits_pair")
    return GateBits(words, n, fo), head, GateBits(words_b, n, fo), head_b


def linear_bias_act_head_fwd_strided(x, w, bias, relu, head_w, d_n=None):
    """linear_bias_act_head_fwd for an x whose rows are x.stride(0) floats apart (a leading-columns view of a wider
    matrix).  Only where split_gemm_available(...)."""
    _chk(w, _f32, "w"); _chk(bias, _f32, "bias", True); _chk(head_w, _f32, "head_w", True)
    n, fi = x.shape
    fo = w.shape[0]
    ldx = _row_strided(x, fi, "linear_bias_act_head_fwd_strided")
    out = torch.empty((n, fo), dtype=_f32, device=x.device)
    head = torch.empty((n, 1), dtype=_f32, device=x.device) if head_w is not None else None
    _lib.check(lib().grapes_linear_bias_act_head_fwd_strided(x.data_ptr(), ldx, _p(w), _p(bias), 1 if relu else 0, _p(out),
                                                             _p(head_w), _p(head), n, _p(d_n), fi, fo, _stream()),
               "linear_bias_act_head_fwd_strided")
    return out, head


def linear_bwd_weight_gated_strided(x, gate, row_scale, col_vec, dw, dbias=None, dw_head=None, d_n=None, accumulate=False):
    """Rank-1 gated dW (see linear_bwd_weight_gated) for a row-strided x."""
    _chk(gate, _f32, "gate"); _chk(row_scale, _f32, "row_scale"); _chk(col_vec, _f32, "col_vec"); _chk(dw, _f32, "dw")
    _chk(dbias, _f32, "dbias", True); _chk(dw_head, _f32, "dw_head", True)
    n, fi = x.shape
    fo = gate.shape[1]
    ldx = _row_strided(x, fi, "linear_bwd_weight_gated_strided")
    ws = _ws(lib().grapes_linear_bwd_weight_gated_workspace_bytes(n, fi, fo), x.device)
    _lib.check(lib().grapes_linear_bwd_weight_gated_strided(_p(gate), x.data_ptr(), ldx, _p(row_scale), n, _p(d_n), _p(col_vec),
                                                            _p(dw), _p(dbias), _p(dw_head), fi, fo, 1 if accumulate else 0,
                                                            _p(ws), _stream()), "linear_bwd_weight_gated_strided")


def linear_bwd_weight_gated(dout, x, gate=None, d_n=None, dw=None, dbias=None, accumulate=False, want_bias=True,
                            row_scale=None, col_vec=None, dw_head=None, defer=None):
    """dW (+)= (dout ⊙ [gate>0])ᵀ x and dbias (+)= colsum(dout ⊙ [gate>0]) in one split-K GEMM.
    dw_head (rank-1 mode): also dw_head (+)= row_scaleᵀ·gate, the 1-wide head's weight gradient."""
    _chk(dw_head, _f32, "dw_head", True)
    _chk(dout, _f32, "dout", row_scale is not None); _chk(x, _f32, "x"); _chk(gate, _f32, "gate", True)
    _chk(row_scale, _f32, "row_scale", True); _chk(col_vec, _f32, "col_vec", True)
    n, fi = x.shape
    fo = dout.shape[1] if dout is not None else gate.shape[1]
    dev = x.device
    if dw is None:
        dw = torch.empty((fo, fi), dtype=_f32, device=dev)
        accumulate = False
    if want_bias and dbias is None:
        dbias = torch.empty(fo, dtype=_f32, device=dev)
    if (defer is not None and row_scale is None and dout is not None and fo > 1 and
            defer.try_add(dout, gate, x, d_n, dw, dbias if want_bias else None, accumulate)):
        return dw, dbias
    ws = _ws(lib().grapes_linear_bwd_weight_gated_workspace_bytes(n, fi, fo), dev)
    _lib.check(lib().grapes_linear_bwd_weight_gated(_p(dout), _p(gate), _p(x), _p(dw), _p(dbias) if want_bias else None, n,
                                                    _p(d_n), fi, fo, 1 if accumulate else 0, _p(row_scale), _p(col_vec),
                                                    _p(dw_head), _p(ws), _stream()),
               "linear_bwd_weight_gated")
    return dw, dbias


def linear_bwd_weight_gated_multi(gates, xs, row_scales, d_ns, col_vec, dw, dbias=None, dw_head=None, accumulate=False):
    """The rank-1 gated dW of SEVERAL hops that share the weights in one split-K GEMM + one slab reduction:
    dw (+)= Σ_h ((row_scales[h] ⊗ col_vec) ⊙ [gates[h] > 0])ᵀ xs[h], dbias (+)= its column sums,
    dw_head (+)= Σ_h row_scales[h]ᵀ gates[h]."""
    import ctypes as C
    nseg = len(gates)
    if not (1 <= nseg <= 4 and len(xs) == nseg and len(row_scales) == nseg and len(d_ns) == nseg):
        raise ValueError("1..4 hops with matching operand lists")
    for t in list(gates) + list(xs) + list(row_scales) + [col_vec, dw]:
        _chk(t, _f32, "operand")
    fo, fi = gates[0].shape[1], xs[0].shape[1]
    arr = lambda ts: (C.c_void_p * nseg)(*[t.data_ptr() for t in ts])
    caps = (C.c_int32 * nseg)(*[x.shape[0] for x in xs])
    ws = _ws(lib().grapes_linear_bwd_weight_gated_workspace_bytes(1, fi, fo), dw.device)
    _lib.check(lib().grapes_linear_bwd_weight_gated_multi(nseg, arr(gates), arr(xs), arr(row_scales), arr(d_ns), caps,
                                                          _p(col_vec), _p(dw), _p(dbias), _p(dw_head), fi, fo,
                                                          1 if accumulate else 0, _p(ws), _stream()),
               "linear_bwd_weight_gated_multi")
    return dw


class DeferredSlabs:
    """Few-row weight gradients of several layers, summed by ONE launch: linear_bwd_weight / linear_bwd_weight_gated called
    with defer=<this> only launch their partial products (when the shape is one of the few-row kernel; otherwise they run
    as usual) and flush() sums all of them.  All deferred calls must be over the same row count (n, d_n)."""

    def __init__(self):
        self.sets, self.n, self.d_n, self.acc = [], None, None, None

    def try_add(self, dout, gate, x, d_n, dw, dbias, accumulate, w=None, dx=None):
        """with (w, dx): the layer's input gradient dx = dout w is computed by the same launch (two independent few-row GEMMs
        side by side) — or nothing is launched and False is returned when either shape is outside its kernel"""
        n, fi = x.shape
        fo = dout.shape[1]
        if len(self.sets) + (2 if dbias is not None else 1) > 8:
            self.flush()
        if self.sets and (self.n != n or (self.d_n is None) != (d_n is None) or
                          (d_n is not None and self.d_n.data_ptr() != d_n.data_ptr()) or self.acc != bool(accumulate)):
            self.flush()
        ws = _ws(lib().grapes_linear_bwd_weight_slabs_bytes(n, fi, fo), x.device)
        if dx is not None:
            rc = lib().grapes_linear_bwd_weight_slabs_and_input(_p(dout), _p(gate), _p(x), _p(w), _p(dx), n, _p(d_n), fi, fo,
                                                                1 if dbias is not None else 0, _p(ws), _stream())
        else:
            rc = lib().grapes_linear_bwd_weight_slabs(_p(dout), _p(gate), _p(x), n, _p(d_n), fi, fo, 1 if dbias is not None else 0,
                                                      _p(ws), _stream())
        if rc != 0:
            return False
        ns = (n + 127) // 128
        self.n, self.d_n, self.acc = n, d_n, bool(accumulate)
        self.sets.append((ws, ws.data_ptr(), dw, fo * fi))
        if dbias is not None:
            self.sets.append((ws, ws.data_ptr() + ns * fo * fi * 4, dbias, fo))
        return True

    def try_add_multi(self, problems):
        """problems: 1..4 tuples (dout, gate, x, dw, dbias, d_n) over the same rows (n, d_n), not accumulating: their slab launches
        as ONE launch (grapes_linear_bwd_weight_slabs_multi), their sets registered in the order given — or nothing is launched
        and False is returned when a shape is outside the few-row kernel."""
        import ctypes as C
        k = len(problems)
        n, d_n = problems[0][2].shape[0], problems[0][5]
        nsets = sum(2 if p[4] is not None else 1 for p in problems)
        if not (1 <= k <= 4) or any(p[2].shape[0] != n or p[5] is not d_n for p in problems):
            return False
        if len(self.sets) + nsets > 8:
            self.flush()
        if self.sets and (self.n != n or (self.d_n is None) != (d_n is None) or
                          (d_n is not None and self.d_n.data_ptr() != d_n.data_ptr()) or self.acc):
            self.flush()
        fis, fos = [p[2].shape[1] for p in problems], [p[0].shape[1] for p in problems]
        wss = [_ws(lib().grapes_linear_bwd_weight_slabs_bytes(n, fi, fo), problems[0][2].device) for fi, fo in zip(fis, fos)]
        arr = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
        ints = lambda vs: (C.c_int32 * k)(*vs)
        rc = lib().grapes_linear_bwd_weight_slabs_multi(k, arr([p[0] for p in problems]), arr([p[1] for p in problems]),
                                                        arr([p[2] for p in problems]), n, _p(d_n), ints(fis), ints(fos),
                                                        ints([1 if p[4] is not None else 0 for p in problems]), arr(wss), _stream())
        if rc != 0:
            return False
        ns = (n + 127) // 128
        self.n, self.d_n, self.acc = n, d_n, False
        for (dout, gate, x, dw, dbias, _), ws, fi, fo in zip(problems, wss, fis, fos):
            self.sets.append((ws, ws.data_ptr(), dw, fo * fi))
            if dbias is not None:
                self.sets.append((ws, ws.data_ptr() + ns * fo * fi * 4, dbias, fo))
        return True

    def flush(self):
        if not self.sets:
            return
        import ctypes as C
        k = len(self.sets)
        slabs = (C.c_void_p * k)(*[s[1] for s in self.sets])
        outs = (C.c_void_p * k)(*[s[2].data_ptr() for s in self.sets])
        counts = (C.c_int64 * k)(*[s[3] for s in self.sets])
        _lib.check(lib().grapes_slab_reduce_sets(k, slabs, outs, counts, self.n, _p(self.d_n), 1 if self.acc else 0, _stream()),
                   "slab_reduce_sets")
        self.sets = []


class GateBits:
    """What linear_relu_head_fwd_bits keeps of a hidden layer for the backward pass: one word of ReLU gate bits per row and
    32 output columns (include/grapes_hip.h) instead of the [n, f_out] activations."""
    __slots__ = ("words", "n", "f_out")

    def __init__(self, words, n, f_out):
        self.words, self.n, self.f_out = words, n, f_out


def linear_relu_head_fwd_bits(x, w, bias, head_w, d_n=None):
    """head = relu(x wᵀ + bias) head_wᵀ  [n, 1]  WITHOUT writing the activations: -> (GateBits, head).  x may be a
    leading-columns view of a wider matrix.  Only where split_gemm_available(n, f_in, f_out)."""
    _chk(w, _f32, "w"); _chk(bias, _f32, "bias", True); _chk(head_w, _f32, "head_w")
    n, fi = x.shape
    fo = w.shape[0]
    ldx = _row_strided(x, fi, "linear_relu_head_fwd_bits")
    words = torch.empty((n, (fo + 31) // 32), dtype=torch.int32, device=x.device)
    head = torch.empty((n, 1), dtype=_f32, device=x.device)
    _lib.check(lib().grapes_linear_relu_head_fwd_bits(x.data_ptr(), ldx, _p(w), _p(bias), _p(head_w), _p(words), _p(head), n,
                                                      _p(d_n), fi, fo, _stream()), "linear_relu_head_fwd_bits")
    return GateBits(words, n, fo), head


def _dw_cols(dw, fo, fi, what):
    """dw is the padded [f_out, f_in] buffer or the parameter's own [f_out, K] gradient, f_in = K rounded up to a multiple of 4"""
    if dw.dim() != 2 or dw.shape[0] != fo or not dw.is_contiguous() or not (fi - 3 <= dw.shape[1] <= fi):
        raise ValueError(f"{what}: dw must be a dense [f_out, f_in] matrix (or [f_out, K], f_in = K rounded up to a multiple of 4)")
    return int(dw.shape[1])


def linear_bwd_weight_bits_multi(bits, xs, row_scales, d_ns, col_vec, w1, b1, dw, dbias=None, dw_head=None, accumulate=False):
    """Backward of linear_relu_head_fwd_bits for 1..4 row sets that share the weights, given d head = row_scales[h] and the
    head's weight col_vec:  dw (+)= dW1, dbias (+)= db1, dw_head (+)= dW2 (include/grapes_hip.h).  One split-K GEMM + one
    slab reduction; no activation is read."""
    import ctypes as C
    nseg = len(bits)
    if not (1 <= nseg <= 4 and len(xs) == nseg and len(row_scales) == nseg and len(d_ns) == nseg):
        raise ValueError("1..4 row sets with matching operand lists")
    for t in list(row_scales) + [col_vec, dw, w1, b1]:
        _chk(t, _f32, "operand")
    fo, fi = bits[0].f_out, xs[0].shape[1]
    if tuple(w1.shape) != (fo, fi) or not w1.is_contiguous() or b1.numel() != fo:
        raise ValueError("linear_bwd_weight_bits_multi: w1 must be a dense [f_out, f_in] matrix and b1 [f_out]")
    dw_cols = _dw_cols(dw, fo, fi, "linear_bwd_weight_bits_multi")
    strides = (C.c_int32 * nseg)(*[_row_strided(x, fi, "linear_bwd_weight_bits_multi") for x in xs])
    arr = lambda ts: (C.c_void_p * nseg)(*[t.data_ptr() for t in ts])
    caps = (C.c_int32 * nseg)(*[x.shape[0] for x in xs])
    ws = _ws(lib().grapes_linear_bwd_weight_gated_workspace_bytes(1, fi, fo), dw.device)
    _lib.check(lib().grapes_linear_bwd_weight_bits_multi_cols(nseg, arr([b.words for b in bits]), arr(xs), strides, arr(row_scales),
                                                              arr(d_ns), caps, _p(col_vec), _p(w1), _p(b1), _p(dw), dw_cols,
                                                              _p(dbias), _p(dw_head), fi, fo, 1 if accumulate else 0, _p(ws),
                                                              _stream()),
               "linear_bwd_weight_bits_multi")
    return dw


def linear_bwd_weight_bits_pair(bits, xs, row_scales, d_ns, col_vec, w1, b1, dw, dbias, dw_head,
                                bits_b, x_b, row_scale_b, d_n_b, col_vec_b, w1_b, b1_b, dw_b, dbias_b, dw_head_b, accumulate=False):
    """linear_bwd_weight_bits_multi of layer a's 1..3 row sets AND of one row set of a second layer b (same f_out, f_in_b <= f_in_a,
    its own parameters and gradient buffers) in one GEMM launch + one slab reduction."""
    import ctypes as C
    nseg = len(bits)
    if not (1 <= nseg <= 3 and len(xs) == nseg and len(row_scales) == nseg and len(d_ns) == nseg):
        raise ValueError("1..3 row sets of layer a with matching operand lists")
    for t in list(row_scales) + [row_scale_b, col_vec, col_vec_b, dw, dw_b, w1, b1, w1_b, b1_b]:
        _chk(t, _f32, "operand")
    fo, fi, fib = bits[0].f_out, xs[0].shape[1], x_b.shape[1]
    if (bits_b.f_out != fo or tuple(w1.shape) != (fo, fi) or tuple(w1_b.shape) != (fo, fib) or not w1.is_contiguous() or
            not w1_b.is_contiguous()):
        raise ValueError("linear_bwd_weight_bits_pair: dense [f_out, f_in] weights of one f_out")
    allx = list(xs) + [x_b]
    strides = (C.c_int32 * (nseg + 1))(*[_row_strided(x, fi if i < nseg else fib, "linear_bwd_weight_bits_pair") for i, x in enumerate(allx)])
    arr = lambda ts: (C.c_void_p * (nseg + 1))(*[t.data_ptr() for t in ts])
    caps = (C.c_int32 * (nseg + 1))(*[x.shape[0] for x in allx])
    ws = _ws(lib().grapes_linear_bwd_weight_gated_workspace_bytes(1, fi, fo), dw.device)
    dw_cols = _dw_cols(dw, fo, fi, "linear_bwd_weight_bits_pair")
    _lib.check(lib().grapes_linear_bwd_weight_bits_pair_cols(
        nseg, arr([b.words for b in bits] + [bits_b.words]), arr(allx), strides, arr(list(row_scales) + [row_scale_b]),
        arr(list(d_ns) + [d_n_b]), caps, _p(col_vec), _p(w1), _p(b1), _p(dw), dw_cols, _p(dbias), _p(dw_head), fi,
        _p(col_vec_b), _p(w1_b), _p(b1_b), _p(dw_b), _p(dbias_b), _p(dw_head_b), fib, fo, 1 if accumulate else 0, _p(ws),
        _stream()), "linear_bwd_weight_bits_pair")
    return dw, dw_b


def pad_features(X):
    """The resident feature matrix with rows padded to a multiple of 4 floats (16-byte aligned rows for the dwordx4 gathers):
    X itself when its width already is one, else a zero-padded copy (made once, outside the step).  Returns (Xp, F)."""
    F = X.shape[1]
    if F % 4 == 0:
        return X.contiguous(), F
    Xp = torch.zeros((X.shape[0], (F + 3) // 4 * 4), dtype=X.dtype, device=X.device)
    Xp[:, :F] = X
    return Xp, F


class FeaturePlanes:
    """The resident (row-padded) feature matrix split ONCE into its three bf16 planes and registered with the library: the
    gathered-operand bf16x3 GEMMs (linear_fwd_gathered(w_image=...), linear_bwd_weight_gathered(split=True)) then read the planes of
    the rows they gather instead of splitting them in their K loops (X is a run-long constant: main.py:66).  +1.5 x the bytes of X.
    MEASURED SLOWER (Reddit 1.418 against 1.366 ms/step: the kernels are bound by their MFMAs, and the planes are 1.5 x the bytes to
    gather in 8-byte pieces): diagnostic build only, off by default (GRAPES_FEATURE_PLANES=1).
    Keep the object alive as long as X is used; close() (or deletion) forgets the registration."""

    def __init__(self, Xp: torch.Tensor):
        _chk(Xp, _f32, "X")
        if lib().grapes_build_flavor() != b"diag":
            raise _lib.GrapesHipError("FeaturePlanes is an A/B form of the diagnostic build (GRAPES_DIAG=1): it measured slower")
        if Xp.shape[1] % 4 != 0 or Xp.stride(0) != Xp.shape[1]:
            raise ValueError("FeaturePlanes: rows padded to a multiple of 4 floats (ops.pad_features)")
        self.X = Xp
        n, ld = Xp.shape
        self.planes = torch.empty(int(lib().grapes_feature_planes_bytes(n, ld)), dtype=torch.uint8, device=Xp.device)
        _lib.check(lib().grapes_feature_split_planes(_p(Xp), n, ld, _p(self.planes), _stream()), "feature_split_planes")
        _lib.check(lib().grapes_feature_planes_register(_p(Xp), ld, _p(self.planes)), "feature_planes_register")
        self._registered = True

    def close(self):
        if getattr(self, "_registered", False):
            lib().grapes_feature_planes_register(_p(self.X), self.X.shape[1], None)
            self._registered = False

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001  (interpreter shutdown)
            pass


def gcn_aggregate_gather(X, ids, prep, ind_code=None, epoch=0, num_ind=0, d_epoch=None, out=None, F=None):
    """Â · [X[ids] | indicators(ids) | 0-padding] without materialising the gathered features: [n, ceil4(F + num_ind)].
    F: logical feature width when X is a padded matrix (pad_features); default X.shape[1]."""
    peers = X if hasattr(X, "c_table") else None          # peer.PeerFeatures: rows read in place from the GPUs that own them
    if peers is not None:
        _chk(ids, _i32, "ids"); _chk(ind_code, _i32, "ind_code", True)
        n, ldx, F = ids.numel(), peers.pitch, peers.F
        kp = (F + num_ind + 3) // 4 * 4
        if out is None:
            out = torch.empty((n, kp), dtype=_f32, device=ids.device)
        if prep.row_head is None or prep.head_ids is not ids:
            raise ValueError("gcn_aggregate_gather over peer shards needs the graph's head records built on these ids")
        bases, bounds, P = peers.c_table()
        _lib.check(lib().grapes_gcn_aggregate_gather_fwd_peers(bases, bounds, P, F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch),
                                                               num_ind, _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv),
                                                               _p(prep.row_head), _p(out), n, _p(prep.d_n), _stream()),
                   "gcn_aggregate_gather_fwd_peers")
        return out
    _chk(X, _f32, "X"); _chk(ids, _i32, "ids"); _chk(ind_code, _i32, "ind_code", True)
    n, ldx = ids.numel(), X.shape[1]
    F = ldx if F is None else int(F)
    if ldx % 4 != 0 or not (ldx - 3 <= F <= ldx):
        raise ValueError("gcn_aggregate_gather: X rows must be padded to a multiple of 4 floats (ops.pad_features)")
    kp = (F + num_ind + 3) // 4 * 4
    if out is None:
        out = torch.empty((n, kp), dtype=_f32, device=X.device)
    head = prep.row_head if (prep.row_head is not None and prep.head_ids is ids) else None     # heads hold THESE ids
    _lib.check(lib().grapes_gcn_aggregate_gather_fwd(_p(X), F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch), num_ind,
                                                     _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv), _p(head), _p(out),
                                                     n, _p(prep.d_n), _stream()), "gcn_aggregate_gather_fwd")
    return out


def split_gathered_available(f_out) -> bool:
    return bool(lib().grapes_split_gathered_available(int(f_out)))


def weight_split_image(w, image=None, w_pad=None):
    """bf16x3 image of a weight [f_out, K] (any row stride) for linear_fwd_gathered(w_image=...): one launch per step.
    w_pad [f_out, Kp >= K]: also refreshed as the zero-padded fp32 copy of w by the same launch."""
    _chk(w, _f32, "w") if w.is_contiguous() else None
    fo, k = w.shape
    nbytes = int(lib().grapes_weight_split_image_bytes(k))
    if image is None:
        image = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    if w_pad is not None:
        _chk(w_pad, _f32, "w_pad")
        _lib.check(lib().grapes_weight_split_image_padded(w.data_ptr(), int(w.stride(0)), fo, k, image.data_ptr(), _p(w_pad),
                                                          int(w_pad.shape[1]), _stream()), "weight_split_image_padded")
        return image
    _lib.check(lib().grapes_weight_split_image(w.data_ptr(), int(w.stride(0)), fo, k, image.data_ptr(), _stream()), "weight_split_image")
    return image


def weight_split_images(ws, images, w_pads=None):
    """weight_split_image of up to four weights in ONE launch (images preallocated; w_pads: per weight a padded copy or None)."""
    import ctypes as C
    k = len(ws)
    if not (1 <= k <= 4) or len(images) != k or (w_pads is not None and len(w_pads) != k):
        raise ValueError("weight_split_images: 1..4 weights, as many images")
    pads = list(w_pads) if w_pads is not None else [None] * k
    for w, im, wp in zip(ws, images, pads):
        if w.dtype != _f32 or not w.is_cuda or w.dim() != 2 or w.stride(1) != 1:
            raise _lib.GrapesHipError("weight_split_images: weights must be cuda float32 [f_out, K] with unit column stride")
        if im.numel() * im.element_size() < int(lib().grapes_weight_split_image_bytes(int(w.shape[1]))):
            raise ValueError("weight_split_images: image too small")
        _chk(wp, _f32, "w_pad", True)
    i32s = lambda vs: (C.c_int32 * k)(*[int(v) for v in vs])
    ptrs = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
    _lib.check(lib().grapes_weight_split_images(
        k, ptrs(ws), i32s([w.stride(0) for w in ws]), i32s([w.shape[0] for w in ws]), i32s([w.shape[1] for w in ws]),
        ptrs(images), ptrs(pads), i32s([0 if wp is None else wp.shape[1] for wp in pads]), _stream()), "weight_split_images")
    return images


def linear_fwd_gathered(X, F, ids, w_pad, ind_code=None, epoch=0, num_ind=0, d_epoch=None, d_n=None, out=None, w_image=None):
    """H = [X[ids, :F] | indicators(ids) | 0] · w_padᵀ  — the XW step of a first layer in the reference order, reading the
    frontier rows through the id list.  X: row-padded resident matrix (pad_features); w_pad [f_out, ceil4(F + num_ind)]."""
    _chk(X, _f32, "X"); _chk(ids, _i32, "ids"); _chk(w_pad, _f32, "w_pad"); _chk(ind_code, _i32, "ind_code", True)
    n, ldx, fo = ids.numel(), X.shape[1], w_pad.shape[0]
    kp = (F + num_ind + 3) // 4 * 4
    if w_pad.shape[1] != kp:
        raise ValueError(f"linear_fwd_gathered: weight image must be [f_out, {kp}]")
    if out is None:
        out = torch.empty((n, fo), dtype=_f32, device=X.device)
    if w_image is not None and n >= 8192 and fo % 4 == 0 and _sw("GRAPES_TSPLIT_FWD_TAIL", "1") != "0":
        # bf16x3 on the bf16 matrix pipe, the tiles of the last (partial) round cut along K (A/B: GRAPES_TSPLIT_FWD_TAIL=0)
        ws = _ws(lib().grapes_linear_fwd_gathered_split_tail_workspace_bytes(fo), X.device)
        import ctypes as C
        one = lambda v: (C.c_void_p * 1)(v)
        _lib.check(lib().grapes_linear_fwd_gathered_split_tail(_p(X), F, ldx, _p(ids), 1, one(_p(ind_code) if num_ind else None), epoch,
                                                               _p(d_epoch), (C.c_int32 * 1)(num_ind), one(w_image.data_ptr()),
                                                               one(out.data_ptr()), n, _p(d_n), fo, _p(ws), _stream()),
                   "linear_fwd_gathered_split_tail")
        return out
    if w_image is not None and n >= 8192:   # bf16x3 on the bf16 matrix pipe (w_image = weight_split_image of the same weight);
        # with few rows (the classifier's <= B + hops K, a small graph) a handful of 128-row tiles would walk K alone: the
        # fp32 kernel's split-K form is faster there (Cora, 2.7k rows x K = 1436: 56 us against 107)
        _lib.check(lib().grapes_linear_fwd_gathered_split(_p(X), F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch), num_ind,
                                                          w_image.data_ptr(), _p(out), n, _p(d_n), fo, _stream()),
                   "linear_fwd_gathered_split")
        return out
    if w_image is not None and n >= 128 and _sw("GRAPES_TSPLIT_FWD_SPLITK", "1") != "0":
        # few rows: the same bf16x3 kernel split along K into slabs + their sum (instead of the fp32-MFMA split-K kernel)
        ws = _ws(lib().grapes_linear_fwd_gathered_split_k_workspace_bytes(n, kp, fo), X.device)
        _lib.check(lib().grapes_linear_fwd_gathered_split_k(_p(X), F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch), num_ind,
                                                            w_image.data_ptr(), _p(out), n, _p(d_n), fo, _p(ws), _stream()),
                   "linear_fwd_gathered_split_k")
        return out
    ws = _ws(lib().grapes_linear_gathered_workspace_bytes(n, kp, fo), X.device)
    _lib.check(lib().grapes_linear_fwd_gathered(_p(X), F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch), num_ind, _p(w_pad),
                                                _p(out), n, _p(d_n), fo, _p(ws), _stream()), "linear_fwd_gathered")
    return out


def linear_fwd_gathered_tail(X, F, ids, w_images, f_out, ind_codes, num_inds, epoch=0, d_epoch=None, d_n=None):
    """H_q = [X[ids, :F] | indicators_q(ids) | 0] · W_qᵀ for one or two nets over the SAME gathered rows, on the bf16 matrix pipe
    with a split tail (include/grapes_hip.h: grapes_linear_fwd_gathered_split_tail).  w_images: weight_split_image of each net's
    [f_out, F + num_ind_q] weight.  Returns the list of outputs [n, f_out]."""
    import ctypes as C
    k = len(w_images)
    _chk(X, _f32, "X"); _chk(ids, _i32, "ids")
    for c in ind_codes:
        _chk(c, _i32, "ind_code", True)
    n, ldx = ids.numel(), X.shape[1]
    outs = [torch.empty((n, f_out), dtype=_f32, device=X.device) for _ in range(k)]
    ws = _ws(lib().grapes_linear_fwd_gathered_split_tail_workspace_bytes(f_out), X.device)
    arr = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
    _lib.check(lib().grapes_linear_fwd_gathered_split_tail(_p(X), F, ldx, _p(ids), k, arr(ind_codes), epoch, _p(d_epoch),
                                                           (C.c_int32 * k)(*[int(v) for v in num_inds]), arr(w_images), arr(outs), n,
                                                           _p(d_n), f_out, _p(ws), _stream()), "linear_fwd_gathered_split_tail")
    return outs


def linear_bwd_weight_gathered_multi_ok(F, probs) -> bool:
    """True when linear_bwd_weight_gathered_multi takes these problems (dicts as below): 2..4 of them on the bf16 pipe, f_out and
    padded widths of the tile shape that launch has (include/grapes_hip.h: grapes_linear_bwd_weight_gathered_split_multi)."""
    if not 2 <= len(probs) <= 4:
        return False
    fo = probs[0]["dh"].shape[1]
    for q in probs:
        kp = (F + q.get("num_ind", 0) + 3) // 4 * 4
        if q["dh"].shape[1] != fo or q["dh"].shape[0] != q["ids"].numel() or not q.get("split", True):
            return False
        if tuple(q["dw"].shape) not in ((fo, kp), (fo, F + q.get("num_ind", 0))):
            return False
        if not lib().grapes_linear_bwd_weight_gathered_split_multi_available(fo, kp):
            return False
    return True


def linear_bwd_weight_gathered_multi(X, F, probs, epoch=0, d_epoch=None):
    """Several  dw_q (+)= dh_qᵀ · [X[ids_q, :F] | indicators_q(ids_q) | 0]  in ONE launch and one slab sum (the sampler net's first
    layer at every hop and the log-Z net's at hop 0: main.py:271-283's backward).  probs: dicts with dh, ids, dw and optionally
    ind_code, num_ind, d_n, accumulate, ind_mask — the arguments of linear_bwd_weight_gathered(split=True); problems that name the
    same dw tensor are summed into it together (accumulate: the first one's)."""
    import ctypes as C
    k = len(probs)
    _chk(X, _f32, "X")
    for q in probs:
        _chk(q["dh"], _f32, "dh"); _chk(q["ids"], _i32, "ids"); _chk(q["dw"], _f32, "dw"); _chk(q.get("ind_code"), _i32, "ind_code", True)
    fo, ldx = probs[0]["dh"].shape[1], X.shape[1]
    kps = [(F + q.get("num_ind", 0) + 3) // 4 * 4 for q in probs]
    lds = [0 if tuple(q["dw"].shape) == (fo, kp) else F + q.get("num_ind", 0) for q, kp in zip(probs, kps)]
    n_out = len({q["dw"].data_ptr() for q in probs})
    ws = _ws(lib().grapes_linear_bwd_weight_gathered_split_multi_workspace_bytes(n_out, max(kps), fo), X.device)
    ptrs = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
    i32s = lambda vs: (C.c_int32 * k)(*[int(v) for v in vs])
    _lib.check(lib().grapes_linear_bwd_weight_gathered_split_multi(
        k, ptrs([q["dh"] for q in probs]), _p(X), F, ldx, ptrs([q["ids"] for q in probs]),
        ptrs([q.get("ind_code") if q.get("num_ind", 0) else None for q in probs]), epoch, _p(d_epoch),
        i32s([q.get("num_ind", 0) for q in probs]), (C.c_uint32 * k)(*[int(q.get("ind_mask", 0)) for q in probs]),
        ptrs([q["dw"] for q in probs]), i32s(lds), i32s([q["ids"].numel() for q in probs]), ptrs([q.get("d_n") for q in probs]),
        fo, i32s([1 if q.get("accumulate") else 0 for q in probs]), _p(ws), _stream()), "linear_bwd_weight_gathered_split_multi")


def linear_bwd_weight_gathered(dh, X, F, ids, dw_pad, ind_code=None, epoch=0, num_ind=0, d_epoch=None, d_n=None,
                               accumulate=False, ind_mask=0, split=False):
    """dw_pad [f_out, ceil4(F + num_ind)] (+)= dhᵀ · [X[ids, :F] | indicators(ids) | 0].  ind_mask: the indicator bits the
    forward pass of this layer saw (0 = all) — later hops of the same batch add bits to the shared table."""
    _chk(dh, _f32, "dh"); _chk(X, _f32, "X"); _chk(ids, _i32, "ids"); _chk(dw_pad, _f32, "dw_pad")
    _chk(ind_code, _i32, "ind_code", True)
    n, ldx, fo = ids.numel(), X.shape[1], dh.shape[1]
    kp = (F + num_ind + 3) // 4 * 4
    if split and tuple(dw_pad.shape) == (fo, F + num_ind) and dh.shape[0] == n and F + num_ind != kp:
        # the parameter's own [f_out, F + num_ind] gradient: the slab sum writes it directly (no padded buffer + strided copy)
        ws = _ws(lib().grapes_linear_bwd_weight_gathered_split_workspace_bytes(kp, fo), X.device)
        _lib.check(lib().grapes_linear_bwd_weight_gathered_split_ld(_p(dh), _p(X), F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch),
                                                                    num_ind, int(ind_mask), _p(dw_pad), F + num_ind, n, _p(d_n), fo,
                                                                    1 if accumulate else 0, _p(ws), _stream()),
                   "linear_bwd_weight_gathered_split_ld")
        return dw_pad
    if tuple(dw_pad.shape) != (fo, kp) or dh.shape[0] != n:
        raise ValueError("linear_bwd_weight_gathered: shape mismatch")
    if split:                          # bf16x3 on the bf16 matrix pipe
        ws = _ws(lib().grapes_linear_bwd_weight_gathered_split_workspace_bytes(kp, fo), X.device)
        _lib.check(lib().grapes_linear_bwd_weight_gathered_split(_p(dh), _p(X), F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch),
                                                                 num_ind, int(ind_mask), _p(dw_pad), n, _p(d_n), fo,
                                                                 1 if accumulate else 0, _p(ws), _stream()),
                   "linear_bwd_weight_gathered_split")
        return dw_pad
    ws = _ws(lib().grapes_linear_gathered_workspace_bytes(n, kp, fo), X.device)
    _lib.check(lib().grapes_linear_bwd_weight_gathered(_p(dh), _p(X), F, ldx, _p(ids), _p(ind_code), epoch, _p(d_epoch), num_ind,
                                                       int(ind_mask), _p(dw_pad), n, _p(d_n), fo, 1 if accumulate else 0, _p(ws), _stream()),
               "linear_bwd_weight_gathered")
    return dw_pad


def linear_bwd_input(dh, w, d_n=None, out=None):
    _chk(dh, _f32, "dh"); _chk(w, _f32, "w")
    n, fo = dh.shape
    fi = w.shape[1]
    if out is None:
        out = torch.empty((n, fi), dtype=_f32, device=dh.device)
    _lib.check(lib().grapes_linear_bwd_input(_p(dh), _p(w), _p(out), n, _p(d_n), fi, fo, _stream()), "linear_bwd_input")
    return out


def _rec_form(prep, n, f) -> bool:
    return (getattr(prep, "head_local", False) and prep.row_head is not None and not prep.items_fwd and 16 < f <= 256 and f % 4 == 0
            and prep.row_head.shape[0] >= n and _sw("GRAPES_AGG_REC", "1") != "0")


def gcn_aggregate_fwd(h, prep: PreparedGraph, bias=None, relu=False, out=None):
    _chk(h, _f32, "h"); _chk(bias, _f32, "bias", True)
    n, f = h.shape
    if out is None:
        out = torch.empty_like(h)
    if _rec_form(prep, n, f) and (bias is None or bias.data_ptr() % 16 == 0):
        # the hop graph carries head records over local ids: one dependent trip per row (grapes_gcn_aggregate_fwd_rec)
        _lib.check(lib().grapes_gcn_aggregate_fwd_rec(_p(h), _p(prep.row_head), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv),
                                                      _p(bias), _p(out), n, _p(prep.d_n), f, 1 if relu else 0, None, None, None,
                                                      _stream()), "gcn_aggregate_fwd_rec")
        return out
    use_items = prep.items_fwd and f > 16 and prep.n > _SMALL_GRAPH
    ws = _ws(lib().grapes_gcn_aggregate_workspace_bytes(prep.item_cap, f), h.device) if use_items else None
    _lib.check(lib().grapes_gcn_aggregate_fwd(_p(h), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv), _p(bias), _p(out),
                                              n, _p(prep.d_n), f, 1 if relu else 0,
                                              _p(prep.items_t) if use_items else None,
                                              _p(prep.n_items_t) if use_items else None,
                                              prep.item_cap if use_items else 0, _p(ws), _stream()), "gcn_aggregate_fwd")
    return out


def gcn_aggregate_fwd_head(h, prep: PreparedGraph, bias, relu, head_w, want_bits=False):
    """(Â h + bias [ReLU], its product with head_w [f][, gate bits]) in one launch — the aggregation of a transform-first layer
    and the X W step of the 1-wide layer behind it (main.py:210).  want_bits (ReLU, f <= 256): also int32 [n, 8], the ReLU gates
    of the output for gcn_aggregate_bwd_rank1(gate_bits=...).  None when the shape is not covered (the caller runs the two
    launches)."""
    _chk(h, _f32, "h"); _chk(bias, _f32, "bias", True); _chk(head_w, _f32, "head_w")
    n, f = h.shape
    if f <= 16 or f % 4 or head_w.numel() != f or (prep.items_fwd and prep.n > _SMALL_GRAPH):
        return None
    out = torch.empty_like(h)
    hw = torch.empty((n, 1), dtype=_f32, device=h.device)
    bits = torch.empty((n, 8), dtype=_i32, device=h.device) if (want_bits and relu and f <= 256) else None
    if _rec_form(prep, n, f) and (bias is None or bias.data_ptr() % 16 == 0):
        _lib.check(lib().grapes_gcn_aggregate_fwd_rec(_p(h), _p(prep.row_head), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv),
                                                      _p(bias), _p(out), n, _p(prep.d_n), f, 1 if relu else 0, _p(head_w), _p(hw),
                                                      _p(bits), _stream()), "gcn_aggregate_fwd_rec")
        return (out, hw, bits) if want_bits else (out, hw)
    _lib.check(lib().grapes_gcn_aggregate_fwd_head(_p(h), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv), _p(bias), _p(out),
                                                   n, _p(prep.d_n), f, 1 if relu else 0, _p(head_w), _p(hw), _p(bits), _stream()),
               "gcn_aggregate_fwd_head")
    return (out, hw, bits) if want_bits else (out, hw)


def gcn_aggregate_bwd_rank1(act, dh2, w2, prep: PreparedGraph, dw_head=None, dbias=None, accumulate=False, gate_bits=None):
    """Backward of (transform-first GCNConv -> ReLU -> 1-wide GCNConv) from dh2 = Âᵀ d(head output): returns
    dh = Âᵀ ((dh2 ⊗ w2) ⊙ [act > 0]) [n, f]; dw_head (+)= dh2ᵀ act, dbias (+)= the first layer's bias gradient.  No n x f
    temporary is written (include/grapes_hip.h: grapes_gcn_aggregate_bwd_rank1)."""
    _chk(act, _f32, "act"); _chk(dh2, _f32, "dh2"); _chk(w2, _f32, "w2"); _chk(dw_head, _f32, "dw_head", True); _chk(dbias, _f32, "dbias", True)
    n, f = act.shape
    if dh2.numel() != n or w2.numel() != f:
        raise ValueError("gcn_aggregate_bwd_rank1: dh2 [n], w2 [f]")
    dh = torch.empty_like(act)
    use_items = prep.n > _SMALL_GRAPH
    ws = _ws(lib().grapes_gcn_aggregate_bwd_rank1_workspace_bytes(prep.item_cap, f), act.device)
    if gate_bits is not None:     # the gates of the aggregation from 32 bytes of bits per row (gcn_aggregate_fwd_head)
        if gate_bits.dtype != _i32 or tuple(gate_bits.shape) != (n, 8) or not gate_bits.is_contiguous() or f > 256:
            raise ValueError("gcn_aggregate_bwd_rank1: gate_bits int32 [n, 8], f <= 256")
        _lib.check(lib().grapes_gcn_aggregate_bwd_rank1_bits(
            _p(act), _p(gate_bits), _p(dh2), _p(w2), _p(prep.rowptr_s), _p(prep.csr_dst), _p(prep.dinv), _p(dh), _p(dw_head),
            _p(dbias), 1 if accumulate else 0, n, _p(prep.d_n), f, _p(prep.items_s) if use_items else None,
            _p(prep.n_items_s) if use_items else None, prep.item_cap if use_items else 0, _p(ws), _stream()),
            "gcn_aggregate_bwd_rank1_bits")
        return dh
    _lib.check(lib().grapes_gcn_aggregate_bwd_rank1(_p(act), _p(dh2), _p(w2), _p(prep.rowptr_s), _p(prep.csr_dst), _p(prep.dinv),
                                                    _p(dh), _p(dw_head), _p(dbias), 1 if accumulate else 0, n, _p(prep.d_n), f,
                                                    _p(prep.items_s) if use_items else None,
                                                    _p(prep.n_items_s) if use_items else None,
                                                    prep.item_cap if use_items else 0, _p(ws), _stream()),
               "gcn_aggregate_bwd_rank1")
    return dh


def gcn_aggregate_bwd_rank1_multi(problems):
    """gcn_aggregate_bwd_rank1 (gate-bit form) for up to three independent problems in the same five launches.  problems: dicts
    with act, dh2, w2, prep, gate_bits and optionally dw_head, dbias, accumulate.  Returns the list of dh.  Equal bit for bit to
    the calls one after the other, in order (problems that name the same dw_head / dbias are added in that order)."""
    import ctypes as C
    k = len(problems)
    if not (1 <= k <= 3):
        raise ValueError("gcn_aggregate_bwd_rank1_multi: 1..3 problems")
    f = problems[0]["act"].shape[1]
    dev = problems[0]["act"].device
    dhs, wss, ns, caps, items, nitems, accs = [], [], [], [], [], [], []
    for pr in problems:
        act, dh2, w2, prep, bits = pr["act"], pr["dh2"], pr["w2"], pr["prep"], pr["gate_bits"]
        _chk(act, _f32, "act"); _chk(dh2, _f32, "dh2"); _chk(w2, _f32, "w2")
        _chk(pr.get("dw_head"), _f32, "dw_head", True); _chk(pr.get("dbias"), _f32, "dbias", True)
        n = act.shape[0]
        if act.shape[1] != f or dh2.numel() != n or w2.numel() != f or f > 256:
            raise ValueError("gcn_aggregate_bwd_rank1_multi: one width f <= 256; dh2 [n], w2 [f]")
        if bits is None or bits.dtype != _i32 or tuple(bits.shape) != (n, 8) or not bits.is_contiguous():
            raise ValueError("gcn_aggregate_bwd_rank1_multi: gate_bits int32 [n, 8]")
        use_items = prep.n > _SMALL_GRAPH
        dhs.append(torch.empty_like(act))
        wss.append(_ws(lib().grapes_gcn_aggregate_bwd_rank1_workspace_bytes(prep.item_cap, f), dev))
        ns.append(n); caps.append(prep.item_cap if use_items else 0)
        items.append(prep.items_s if use_items else None); nitems.append(prep.n_items_s if use_items else None)
        accs.append(1 if pr.get("accumulate") else 0)
    arr = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
    ints = lambda vs: (C.c_int32 * k)(*vs)
    _lib.check(lib().grapes_gcn_aggregate_bwd_rank1_bits_multi(
        k, arr([p["act"] for p in problems]), arr([p["gate_bits"] for p in problems]), arr([p["dh2"] for p in problems]),
        arr([p["w2"] for p in problems]), arr([p["prep"].rowptr_s for p in problems]), arr([p["prep"].csr_dst for p in problems]),
        arr([p["prep"].dinv for p in problems]), arr(dhs), arr([p.get("dw_head") for p in problems]),
        arr([p.get("dbias") for p in problems]), ints(accs), ints(ns), arr([p["prep"].d_n for p in problems]), f, arr(items),
        arr(nitems), ints(caps), arr(wss), _stream()), "gcn_aggregate_bwd_rank1_bits_multi")
    return dhs


def scale_rows(h, dinv, out=None):
    """hs[r, :] = dinv[r] * h[r, :] (out may be h): the pre-scaled operand of gcn_aggregate_fwd(..., prescaled=True)."""
    _chk(h, _f32, "h"); _chk(dinv, _f32, "dinv")
    n, f = h.shape
    if out is None:
        out = torch.empty_like(h)
    _lib.check(lib().grapes_scale_rows(_p(h), _p(dinv), _p(out), n, f, _stream()), "scale_rows")
    return out


def gcn_aggregate_fwd_prescaled(hs, prep: PreparedGraph, bias=None, relu=False, out=None):
    """Â h + bias from hs = scale_rows(h, prep.dinv): out[c] = dinv[c] (sum hs[s] + hs[c]) + b — the full-batch inference form
    (no gather of dinv[source] per aggregated edge)."""
    _chk(hs, _f32, "hs"); _chk(bias, _f32, "bias", True)
    n, f = hs.shape
    if out is None:
        out = torch.empty_like(hs)
    use_items = prep.items_fwd and prep.n > _SMALL_GRAPH
    ws = _ws(lib().grapes_gcn_aggregate_workspace_bytes(prep.item_cap, f), hs.device) if use_items else None
    _lib.check(lib().grapes_gcn_aggregate_fwd_prescaled(_p(hs), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv), _p(bias),
                                                        _p(out), n, _p(prep.d_n), f, 1 if relu else 0,
                                                        _p(prep.items_t) if use_items else None,
                                                        _p(prep.n_items_t) if use_items else None,
                                                        prep.item_cap if use_items else 0, _p(ws), _stream()),
               "gcn_aggregate_fwd_prescaled")
    return out


def gcn_aggregate_narrow_pair(h_a, h_b, prep: PreparedGraph, bias_a=None, bias_b=None):
    """(Â h_a + bias_a, Â h_b + bias_b) for two [n, 1] vectors over the same prepared graph in one launch."""
    _chk(h_a, _f32, "h_a"); _chk(h_b, _f32, "h_b"); _chk(bias_a, _f32, "bias_a", True); _chk(bias_b, _f32, "bias_b", True)
    if h_a.numel() != h_b.numel():
        raise ValueError("gcn_aggregate_narrow_pair: two vectors of one length")
    out_a, out_b = torch.empty_like(h_a), torch.empty_like(h_b)
    _lib.check(lib().grapes_gcn_aggregate_narrow_pair(_p(h_a), _p(h_b), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv),
                                                      _p(bias_a), _p(bias_b), _p(out_a), _p(out_b), h_a.numel(), _p(prep.d_n),
                                                      _stream()), "gcn_aggregate_narrow_pair")
    return out_a, out_b


_BWD_HOSTS: List = []     # launches waiting to carry a few-row backward aggregation (carry_backward_aggregations)
_BWD_ALONE = [0]          # recorded gcn_aggregate_bwd_input launches a host did NOT carry (issued on their own): tests read it


def carry_backward_aggregations(hosts):
    """hosts: callables, each issuing ONE launch that can carry a recorded few-row backward aggregation as extra workgroups
    (SamplerHeadBwdMulti.launch(1) / (2)) and that neither reads what the next gcn_aggregate_bwd calls write nor writes what
    they read.  Each of the next gcn_aggregate_bwd calls then RECORDS its launch and issues the next host with the record
    attached: the pair takes the time of the longer one (both are dependent round trips on a mostly idle chip).  Order on the
    stream: host launch (with the aggregation inside), then whatever the caller issues next.  flush_backward_hosts() issues the
    hosts nobody used.  Not while another rider program is attached."""
    _BWD_HOSTS[:] = list(hosts)


def flush_backward_hosts():
    while _BWD_HOSTS:
        _BWD_HOSTS.pop(0)()


def gcn_aggregate_bwd(dout, prep: PreparedGraph, relu_out=None, want_bias=True, dbias=None, accumulate_bias=False):
    """Returns (dh, dbias).  dout is not modified."""
    _chk(dout, _f32, "dout"); _chk(relu_out, _f32, "relu_out", True)
    n, f = dout.shape
    dev = dout.device
    dpre = torch.empty_like(dout) if relu_out is not None else dout
    dh = torch.empty_like(dout)
    if want_bias and dbias is None:
        dbias = torch.empty(f, dtype=_f32, device=dev)
        accumulate_bias = False
    ws = _ws(lib().grapes_gcn_aggregate_bwd_workspace_bytes(prep.item_cap, f), dev)
    use_items = prep.n > _SMALL_GRAPH          # small graphs: one launch, every row by one wavefront whatever its length
    L = lib()
    host = _BWD_HOSTS.pop(0) if (_BWD_HOSTS and not use_items) else None
    if host is not None:
        _lib.check(L.grapes_rider_record_begin(), "rider_record_begin")
    prog = -1
    try:
        rc = L.grapes_gcn_aggregate_bwd(_p(dout), _p(relu_out), _p(prep.rowptr_s), _p(prep.csr_dst), _p(prep.dinv),
                                        _p(dpre), _p(dh), _p(dbias) if want_bias else None,
                                        1 if accumulate_bias else 0, n, _p(prep.d_n), f,
                                        _p(prep.items_s) if use_items else None,
                                        _p(prep.n_items_s) if use_items else None,
                                        prep.item_cap if use_items else 0, _p(ws), _p(_ticket(dev)[16:32]), _stream())
    finally:
        if host is not None:
            prog = int(L.grapes_rider_record_end())
    _lib.check(rc, "gcn_aggregate_bwd")
    if host is not None:        # (a call that took another form launched at once and recorded nothing: the host then runs on its own)
        _lib.check(L.grapes_rider_attach(prog, 0, _stream()), "rider_attach")
        try:
            host()
        finally:
            alone = L.grapes_rider_detach(_stream(), None)
            L.grapes_rider_free(prog)
        if alone < 0:
            raise _lib.GrapesHipError(f"rider_detach failed ({alone})")
    return dh, dbias


def gcn_aggregate_bwd_input(dout, prep: PreparedGraph, w, relu_out=None, dbias=None, accumulate_bias=False, dt=None, dx=None):
    """gcn_aggregate_bwd and linear_bwd_input on its output as ONE launch (include/grapes_hip.h: grapes_gcn_aggregate_bwd_input):
    -> (dt, dx) with dt = Âᵀ(dout ⊙ [relu_out > 0]) and dx = dt w, bit for bit what the two calls give, dbias (+)= the gated
    column sums — or None where that launch does not take the shape (nothing is launched then).  Carried by a waiting host
    launch like gcn_aggregate_bwd (carry_backward_aggregations)."""
    _chk(dout, _f32, "dout"); _chk(relu_out, _f32, "relu_out", True); _chk(w, _f32, "w"); _chk(dbias, _f32, "dbias", True)
    n, f = dout.shape
    fi = w.shape[1]
    dev = dout.device
    if w.shape[0] != f or prep.n > _SMALL_GRAPH:
        return None
    _chk(dt, _f32, "dt", True); _chk(dx, _f32, "dx", True)
    if dt is None:
        dt = torch.empty_like(dout)
    L = lib()
    if not L.grapes_gcn_aggregate_bwd_input_available(_p(dout), _p(relu_out), _p(dt), n, f, fi):
        return None
    if dx is None:
        dx = torch.empty((n, fi), dtype=_f32, device=dev)
    if tuple(dt.shape) != (n, f) or tuple(dx.shape) != (n, fi):
        raise ValueError("gcn_aggregate_bwd_input: dt [n, f], dx [n, f_in]")
    ws = _ws(L.grapes_gcn_aggregate_bwd_workspace_bytes(0, f), dev)
    host = _BWD_HOSTS.pop(0) if _BWD_HOSTS else None
    if host is not None:
        _lib.check(L.grapes_rider_record_begin(), "rider_record_begin")
    prog = -1
    try:
        rc = L.grapes_gcn_aggregate_bwd_input(_p(dout), _p(relu_out), _p(prep.rowptr_s), _p(prep.csr_dst), _p(prep.dinv), _p(w),
                                              _p(dt), _p(dx), _p(dbias), 1 if accumulate_bias else 0, n, _p(prep.d_n), f, fi,
                                              _p(ws), _p(_ticket(dev)[16:32]), _stream())
    finally:
        if host is not None:
            prog = int(L.grapes_rider_record_end())
    _lib.check(rc, "gcn_aggregate_bwd_input")
    if host is not None:
        _lib.check(L.grapes_rider_attach(prog, 0, _stream()), "rider_attach")
        try:
            host()
        finally:
            alone = L.grapes_rider_detach(_stream(), None)
            L.grapes_rider_free(prog)
        if alone < 0:
            raise _lib.GrapesHipError(f"rider_detach failed ({alone})")
        _BWD_ALONE[0] += alone
    return dt, dx


# ------------------------------------------------------------------------------- GATConv aggregation (modules/gcn.py:45-72)
def gather_width_ok(f: int, wide_scalar: bool = False) -> bool:
    """The widths the row-gather kernels are built for (csrc/row_gather.h, ROW_LAUNCH): float4 columns up to 1024, scalar columns up
    to 256 — or, where the wide scalar form is built too (wide_scalar: GCN2), any width up to 1024."""
    return 1 <= f <= 1024 and (wide_scalar or f <= 256 or f % 4 == 0)


def _gather_width(f: int, who: str, wide_scalar: bool = False):
    if not gather_width_ok(f, wide_scalar):
        built = "any width up to 1024" if wide_scalar else "any width up to 256, multiples of 4 up to 1024"
        raise ValueError(f"{who}: width {f} is not built ({built})")


def _long_items(prep, by_target: bool, forward: bool, long_rows: Optional[bool] = None):
    """(items, n_items, cap) as the row-gather entry points take them: prep's long-row work items by target or by source, or
    (None, None, 0) where every row runs in the rows kernel — a forward over a graph prepared without them, or a graph that counts
    as small.  long_rows None: up to _SMALL_GRAPH nodes is small.  True: no graph is (GATv2: one head's score costs a whole row of
    arithmetic per edge, so a hub row is worth its own workgroups on a small graph too).  False: every graph is.  Tests force
    either form."""
    small = prep.n <= _SMALL_GRAPH if long_rows is None else not long_rows
    if small or (forward and not prep.items_fwd):
        return None, None, 0
    items, n_items = (prep.items_t, prep.n_items_t) if by_target else (prep.items_s, prep.n_items_s)
    return _p(items), _p(n_items), prep.item_cap


def gat_scores(h, a_src, a_dst, d_n=None):
    """(s_src, s_dst) = (H a_src, H a_dst): the per-node halves of GATConv's attention logits, one read of H."""
    _chk(h, _f32, "h"); _chk(a_src, _f32, "a_src"); _chk(a_dst, _f32, "a_dst")
    n, f = h.shape
    _gather_width(f, "GAT aggregation")
    if a_src.numel() != f or a_dst.numel() != f:
        raise ValueError("a_src / a_dst must hold one value per column of h")
    s_src = torch.empty(max(n, 1), dtype=_f32, device=h.device)
    s_dst = torch.empty(max(n, 1), dtype=_f32, device=h.device)
    _lib.check(lib().grapes_gat_scores(_p(h), _p(a_src), _p(a_dst), _p(s_src), _p(s_dst), n, _p(d_n), f, _stream()), "gat_scores")
    return s_src, s_dst


def gat_aggregate_fwd(h, s_src, s_dst, prep: PreparedGraph, bias=None, relu=False, out=None):
    """(out, row_ms): out_i = sum_j softmax_j(LeakyReLU(s_src[j] + s_dst[i])) H_j + bias (+ReLU) over prep's by-target CSR plus
    one unit self-loop per node; row_ms [n, 2] = (row maximum, log of the softmax sum), what gat_aggregate_bwd recomputes the
    attention weights from."""
    _chk(h, _f32, "h"); _chk(s_src, _f32, "s_src"); _chk(s_dst, _f32, "s_dst"); _chk(bias, _f32, "bias", True)
    n, f = h.shape
    _gather_width(f, "GAT aggregation")
    if n != prep.n or s_src.numel() < n or s_dst.numel() < n:
        raise ValueError("h, s_src and s_dst need one row per node of the prepared graph")
    if out is None:
        out = torch.empty_like(h)
    row_ms = torch.empty((max(n, 1), 2), dtype=_f32, device=h.device)
    items, n_items, cap = _long_items(prep, by_target=True, forward=True)
    ws = _ws(lib().grapes_gat_aggregate_workspace_bytes(cap, f), h.device) if cap else None
    _lib.check(lib().grapes_gat_aggregate_fwd(_p(h), _p(s_src), _p(s_dst), _p(prep.rowptr_t), _p(prep.csr_src), _p(bias), _p(out),
                                              _p(row_ms), n, _p(prep.d_n), f, 1 if relu else 0, items, n_items, cap, _p(ws),
                                              _p(prep.status), _stream()), "gat_aggregate_fwd")
    return out, row_ms


def gat_aggregate_bwd(dout, out, h, s_src, s_dst, row_ms, a_src, a_dst, prep: PreparedGraph, bias=None, relu=False):
    """Returns (dh, da_src, da_dst, dbias) for gat_aggregate_fwd + gat_scores (dh includes the scores' share, ds_src a_src +
    ds_dst a_dst).  `out` is the forward's output; dout is not modified."""
    for t, name in ((dout, "dout"), (out, "out"), (h, "h"), (s_src, "s_src"), (s_dst, "s_dst"), (row_ms, "row_ms"),
                    (a_src, "a_src"), (a_dst, "a_dst")):
        _chk(t, _f32, name)
    _chk(bias, _f32, "bias", True)
    n, f = dout.shape
    _gather_width(f, "GAT aggregation")
    if n != prep.n or out.shape != dout.shape or h.shape != dout.shape:
        raise ValueError("dout, out and h must be [n, f] over the prepared graph's nodes")
    dev = dout.device
    dh = torch.empty_like(dout)
    da_src = torch.empty(f, dtype=_f32, device=dev); da_dst = torch.empty(f, dtype=_f32, device=dev)
    dbias = torch.empty(f, dtype=_f32, device=dev)
    items_t, n_items_t, cap = _long_items(prep, by_target=True, forward=False)
    items_s, n_items_s, _ = _long_items(prep, by_target=False, forward=False)
    ws = _ws(lib().grapes_gat_aggregate_bwd_workspace_bytes(n, cap, f), dev)
    _lib.check(lib().grapes_gat_aggregate_bwd(_p(dout), _p(out), _p(bias), 1 if relu else 0, _p(h), _p(s_src), _p(s_dst), _p(row_ms),
                                              _p(a_src), _p(a_dst), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.rowptr_s),
                                              _p(prep.csr_dst), _p(dh), _p(da_src), _p(da_dst), _p(dbias), n, _p(prep.d_n), f,
                                              items_t, n_items_t, items_s, n_items_s, cap, _p(ws), _p(prep.status), _stream()),
               "gat_aggregate_bwd")
    return dh, da_src, da_dst, dbias


# ------------------------------------------------------------------------------- GATv2Conv aggregation (PyG GATv2Conv)
def _gatv2_shape(heads: int, c: int):
    """The shapes csrc/gatv2_kernels.hip is built for: 1..16 heads of c channels, f = heads c up to 256, or up to 1024 with c % 4 == 0."""
    if not 1 <= heads <= 16:
        raise ValueError(f"GATv2 aggregation: heads = {heads} is not built (1 <= heads <= 16)")
    f = heads * c
    if c < 1 or f > 1024 or (f > 256 and c % 4):
        raise ValueError(f"GATv2 aggregation: heads x out_channels = {heads} x {c} is not built (heads * out_channels up to 256, "
                         "or up to 1024 with out_channels % 4 == 0)")


def _gatv2_slope(negative_slope: float) -> float:
    if not 0.0 <= negative_slope < 1.0:
        raise ValueError(f"GATv2 aggregation: negative_slope = {negative_slope} is outside [0, 1)")
    return float(negative_slope)


def gatv2_aggregate_fwd(x_l, x_r, att, prep: PreparedGraph, heads: int, concat=True, negative_slope=0.2, bias=None, relu=False):
    """(out, agg, row_ms) of GATv2Conv's propagate over prep's by-target CSR plus one unit self-loop per node: per head h,
    e_ij = att[h] . LeakyReLU(x_l[j, h] + x_r[i, h]), alpha = softmax_j e_ij, agg_i[h] = sum_j alpha_ij x_l[j, h]; out = the heads
    side by side [n, f] (concat) or their mean [n, c], + bias (+ReLU).  agg [n, f] is the per-head aggregate when concat is false
    (else None: it is out - bias); row_ms [n, heads, 2] = (maximum, log of the softmax sum), what gatv2_aggregate_bwd recomputes
    the attention weights from."""
    _chk(x_l, _f32, "x_l"); _chk(x_r, _f32, "x_r"); _chk(att, _f32, "att"); _chk(bias, _f32, "bias", True)
    n, f = x_l.shape
    if heads < 1 or f % heads:
        raise ValueError(f"GATv2 aggregation: width {f} is not a multiple of heads = {heads}")
    c = f // heads
    _gatv2_shape(heads, c)
    slope = _gatv2_slope(negative_slope)
    if n != prep.n or x_r.shape != x_l.shape or att.numel() != f:
        raise ValueError("x_l and x_r must be [n, heads * c] over the prepared graph's nodes and att must hold heads * c values")
    if bias is not None and bias.numel() != (f if concat else c):
        raise ValueError("bias must hold heads * c values (concat) or c values (head mean)")
    dev = x_l.device
    out = torch.empty((n, f if concat else c), dtype=_f32, device=dev)
    agg = None if concat else torch.empty((n, f), dtype=_f32, device=dev)
    row_ms = torch.empty((max(n, 1), heads, 2), dtype=_f32, device=dev)
    items, n_items, cap = _long_items(prep, by_target=True, forward=True, long_rows=True)
    ws = _ws(lib().grapes_gatv2_aggregate_workspace_bytes(cap, f, heads), dev) if cap else None
    _lib.check(lib().grapes_gatv2_aggregate_fwd(_p(x_l), _p(x_r), _p(att), _p(prep.rowptr_t), _p(prep.csr_src), _p(bias), _p(out),
                                                _p(agg), _p(row_ms), n, _p(prep.d_n), heads, c, 1 if concat else 0, slope,
                                                1 if relu else 0, items, n_items, cap, _p(ws), _p(prep.status), _stream()),
               "gatv2_aggregate_fwd")
    return out, agg, row_ms


def gatv2_aggregate_bwd(dout, out, agg, x_l, x_r, att, row_ms, prep: PreparedGraph, heads: int, concat=True, negative_slope=0.2,
                        bias=None, relu=False):
    """Returns (dx_l, dx_r, datt, dbias) for gatv2_aggregate_fwd.  `out`, `agg` and `row_ms` are the forward's; dout is not
    modified."""
    for t, name in ((dout, "dout"), (out, "out"), (x_l, "x_l"), (x_r, "x_r"), (att, "att"), (row_ms, "row_ms")):
        _chk(t, _f32, name)
    _chk(bias, _f32, "bias", True); _chk(agg, _f32, "agg", concat)
    n, f = x_l.shape
    if heads < 1 or f % heads:
        raise ValueError(f"GATv2 aggregation: width {f} is not a multiple of heads = {heads}")
    c = f // heads
    _gatv2_shape(heads, c)
    slope = _gatv2_slope(negative_slope)
    w = f if concat else c
    if n != prep.n or x_r.shape != x_l.shape or tuple(dout.shape) != (n, w) or out.shape != dout.shape or att.numel() != f:
        raise ValueError("x_l and x_r must be [n, heads * c] over the prepared graph's nodes, dout and out [n, heads * c] (concat) "
                         "or [n, c]")
    if not concat and tuple(agg.shape) != (n, f):
        raise ValueError("agg must be the forward's [n, heads * c] per-head aggregate")
    if row_ms.numel() < n * heads * 2:
        raise ValueError("row_ms must be the forward's [n, heads, 2]")
    dev = dout.device
    dx_l, dx_r = torch.empty_like(x_l), torch.empty_like(x_l)
    datt = torch.empty(f, dtype=_f32, device=dev)
    dbias = torch.empty(w, dtype=_f32, device=dev)
    items_t, n_items_t, cap = _long_items(prep, by_target=True, forward=False, long_rows=True)
    items_s, n_items_s, _ = _long_items(prep, by_target=False, forward=False, long_rows=True)
    ws = _ws(lib().grapes_gatv2_aggregate_bwd_workspace_bytes(n, cap, f, heads), dev)
    _lib.check(lib().grapes_gatv2_aggregate_bwd(_p(dout), _p(out), _p(agg), _p(bias), 1 if relu else 0, _p(x_l), _p(x_r), _p(att),
                                                _p(row_ms), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.rowptr_s), _p(prep.csr_dst),
                                                _p(dx_l), _p(dx_r), _p(datt), _p(dbias), n, _p(prep.d_n), heads, c,
                                                1 if concat else 0, slope, items_t, n_items_t, items_s, n_items_s, cap, _p(ws),
                                                _p(prep.status), _stream()), "gatv2_aggregate_bwd")
    return dx_l, dx_r, datt, dbias


# ------------------------------------------------------------------------------- GCN2Conv propagation (modules/gcn.py:76-117)
def gcn2_loop_counts(edge_src, edge_dst, n, d_n=None, d_e=None, node_map=None):
    """int32[n]: loops[i] = number of stored edges (i, i) of the edge list a PreparedGraph is built from (the build drops them;
    GCN2Conv(normalize=False) counts them like any edge)."""
    _chk(edge_src, _i32, "edge_src"); _chk(edge_dst, _i32, "edge_dst"); _chk(node_map, _i32, "node_map", True)
    loops = torch.empty(max(n, 1), dtype=_i32, device=edge_src.device)
    _lib.check(lib().grapes_gcn2_loop_counts(_p(edge_src), _p(edge_dst), edge_src.numel(), _p(d_e), _p(node_map), n, _p(d_n),
                                             _p(loops), _stream()), "gcn2_loop_counts")
    return loops


def gcn2_loop_counts_csr(rowptr, col, n):
    """The same from a DeviceGraph's CSR (int64 row pointers): 0 or 1 per node when the rows are de-duplicated."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col")
    loops = torch.empty(max(n, 1), dtype=_i32, device=col.device)
    _lib.check(lib().grapes_gcn2_loop_counts_csr(_p(rowptr), _p(col), n, _p(loops), _stream()), "gcn2_loop_counts_csr")
    return loops


def gcn2_attach_loops(prep: "PreparedGraph", edge_src, edge_dst, node_map=None) -> "PreparedGraph":
    """Counts the stored self-loops of the edge list `prep` was built from and keeps them beside it (prep.loops)."""
    prep.loops = gcn2_loop_counts(edge_src, edge_dst, prep.n, d_n=prep.d_n, d_e=prep.d_e, node_map=node_map)
    return prep


def gcn2_loops(prep: "PreparedGraph") -> torch.Tensor:
    loops = getattr(prep, "loops", None)
    if loops is None:
        raise _lib.GrapesHipError("GCN2 propagation: this PreparedGraph carries no stored-self-loop counts (the build drops the "
                                  "loops GCN2Conv counts): call ops.gcn2_attach_loops(prep, edge_src, edge_dst) with its edge list")
    return loops


def gcn2_propagate_fwd(x, x0, prep: PreparedGraph, alpha: float, want_p: bool = False):
    """(S, P'): S = (1 - alpha) (A x + loops * x) + alpha x0 over prep's by-target CSR, P' = S's first term (want_p)."""
    _chk(x, _f32, "x"); _chk(x0, _f32, "x0")
    n, f = x.shape
    _gather_width(f, "GCN2 propagation", wide_scalar=True)
    if n != prep.n or tuple(x0.shape) != (n, f):
        raise ValueError("x and x0 must be [n, f] over the prepared graph's nodes")
    loops = gcn2_loops(prep)
    s_out = torch.empty_like(x)
    p_out = torch.empty_like(x) if want_p else None
    items, n_items, cap = _long_items(prep, by_target=True, forward=True)
    ws = _ws(lib().grapes_gcn2_propagate_workspace_bytes(0, cap, f), x.device) if cap else None
    _lib.check(lib().grapes_gcn2_propagate_fwd(_p(x), _p(x0), _p(loops), _p(prep.rowptr_t), _p(prep.csr_src), float(alpha), _p(s_out),
                                               _p(p_out), n, _p(prep.d_n), f, items, n_items, cap, _p(ws), _p(prep.status),
                                               _stream()), "gcn2_propagate_fwd")
    return s_out, p_out


def gcn2_propagate_bwd(ds, prep: PreparedGraph, alpha: float, ds_add=None, add_is_p: bool = False, dx0_add=None, dx0=None,
                       want_x0: bool = True):
    """(dx, dx0) of gcn2_propagate_fwd from ds = d S (+ ds_add: a second share of d S, or d P' when add_is_p; + dx0_add: a gradient
    that reaches x0 directly).  A dx0 tensor passed in is accumulated into."""
    _chk(ds, _f32, "ds"); _chk(ds_add, _f32, "ds_add", True); _chk(dx0_add, _f32, "dx0_add", True); _chk(dx0, _f32, "dx0", True)
    n, f = ds.shape
    _gather_width(f, "GCN2 propagation", wide_scalar=True)
    if n != prep.n:
        raise ValueError("ds must be [n, f] over the prepared graph's nodes")
    loops = gcn2_loops(prep)
    dx = torch.empty_like(ds)
    accumulate = dx0 is not None
    if dx0 is None and want_x0:
        dx0 = torch.empty_like(ds)
    items, n_items, cap = _long_items(prep, by_target=False, forward=False)
    two = ds_add is not None or dx0_add is not None
    ws = _ws(lib().grapes_gcn2_propagate_workspace_bytes(n if two else 0, cap, f), ds.device) if (two or cap) else None
    _lib.check(lib().grapes_gcn2_propagate_bwd(_p(ds), _p(ds_add), 1 if add_is_p else 0, _p(dx0_add), _p(loops), _p(prep.rowptr_s),
                                               _p(prep.csr_dst), float(alpha), _p(dx), _p(dx0), 1 if accumulate else 0, n,
                                               _p(prep.d_n), f, items, n_items, cap, _p(ws), _p(prep.status), _stream()),
               "gcn2_propagate_bwd")
    return dx, dx0


def gcn2_mix_fwd(s, t1, c0: float, c1: float, t2=None, c2: float = 0.0, relu: bool = False, d_n=None):
    """act(c0 s + c1 t1 [+ c2 t2]): GCN2Conv's identity-mapping blend (+ the ReLU behind it) in one launch."""
    _chk(s, _f32, "s"); _chk(t1, _f32, "t1"); _chk(t2, _f32, "t2", True)
    n, f = s.shape
    if t1.shape != s.shape or (t2 is not None and t2.shape != s.shape):
        raise ValueError("gcn2_mix_fwd: operands of one shape")
    out = torch.empty_like(s)
    _lib.check(lib().grapes_gcn2_mix_fwd(_p(s), _p(t1), _p(t2), float(c0), float(c1), float(c2), 1 if relu else 0, _p(out), n,
                                         _p(d_n), f, _stream()), "gcn2_mix_fwd")
    return out


def gcn2_mix_bwd(dout, out, relu: bool, c0: float, c1=None, c2=None, d_n=None):
    """(c0 g, c1 g, c2 g) with g = dout gated by out > 0 (relu): one read of dout and out; a coefficient None gives no output."""
    _chk(dout, _f32, "dout"); _chk(out, _f32, "out", not relu)
    n, f = dout.shape
    g0 = torch.empty_like(dout)
    g1 = torch.empty_like(dout) if c1 is not None else None
    g2 = torch.empty_like(dout) if c2 is not None else None
    _lib.check(lib().grapes_gcn2_mix_bwd(_p(dout), _p(out) if relu else None, 1 if relu else 0, float(c0), float(c1 or 0.0),
                                         float(c2 or 0.0), _p(g0), _p(g1), _p(g2), n, _p(d_n), f, _stream()), "gcn2_mix_bwd")
    return g0, g1, g2


# ------------------------------------------------------------------------------- PNAConv aggregation (modules/gcn.py:120-149)
PNA_AGGREGATORS = ("mean", "min", "max", "std", "var", "sum")                       # the kernels' aggregator codes, by position
PNA_SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")
PNA_NSTAT = 6                                                                       # mean, min, max, var, ties_min, ties_max


class PNAConfig:
    """The aggregator / scaler lists of a PNAConv as the kernels take them (3-bit codes, the first entry in the low bits) and the
    two averages of the degree histogram."""

    __slots__ = ("aggregators", "scalers", "n_agg", "agg_code", "n_scal", "scal_code", "avg_log", "avg_lin")

    def __init__(self, aggregators, scalers, avg_log: float, avg_lin: float):
        self.aggregators, self.scalers = tuple(aggregators), tuple(scalers)
        for name in self.aggregators:
            if name not in PNA_AGGREGATORS:
                raise NotImplementedError(f"PNA aggregator {name!r} is not built (built: {', '.join(PNA_AGGREGATORS)})")
        for name in self.scalers:
            if name not in PNA_SCALERS:
                raise NotImplementedError(f"PNA scaler {name!r} is not built (built: {', '.join(PNA_SCALERS)})")
        if not (1 <= len(self.aggregators) <= 6) or not (1 <= len(self.scalers) <= 5):
            raise ValueError("PNA: 1..6 aggregators and 1..5 scalers")
        self.n_agg, self.n_scal = len(self.aggregators), len(self.scalers)
        self.agg_code = sum(PNA_AGGREGATORS.index(a) << (3 * k) for k, a in enumerate(self.aggregators))
        self.scal_code = sum(PNA_SCALERS.index(s) << (3 * k) for k, s in enumerate(self.scalers))
        self.avg_log, self.avg_lin = float(avg_log), float(avg_lin)

    @property
    def blocks(self) -> int:
        return 1 + self.n_agg * self.n_scal


def pna_aggregate_fwd(x, ab, prep: PreparedGraph, cfg: PNAConfig):
    """(z, stats): z[i] = [x_i | scaler_1(aggs) | scaler_2(aggs) | ...] ([n, cfg.blocks * f], post_nn's operand) of the messages
    m_ij = a_i + b_j over prep's by-target CSR (+ its stored loops), ab = [a | b] ([n, 2 f]); stats [n, 6, f] for the backward."""
    _chk(x, _f32, "x"); _chk(ab, _f32, "ab")
    n, f = x.shape
    if n != prep.n or tuple(ab.shape) != (n, 2 * f):
        raise ValueError("x must be [n, f] and ab [n, 2 f] over the prepared graph's nodes")
    loops = gcn2_loops(prep)
    z = torch.empty((n, cfg.blocks * f), dtype=_f32, device=x.device)
    stats = torch.empty((n, PNA_NSTAT, f), dtype=_f32, device=x.device)
    items, n_items, cap = _long_items(prep, by_target=True, forward=True)
    ws = _ws(lib().grapes_pna_aggregate_fwd_workspace_bytes(cap, f), x.device) if cap else None
    _lib.check(lib().grapes_pna_aggregate_fwd(_p(x), _p(ab), ab.data_ptr() + 4 * f, 2 * f, _p(loops), _p(prep.rowptr_t),
                                              _p(prep.csr_src), cfg.n_agg, cfg.agg_code, cfg.n_scal, cfg.scal_code, cfg.avg_log,
                                              cfg.avg_lin, _p(z), _p(stats), n, _p(prep.d_n), f, items, n_items, cap, _p(ws),
                                              _p(prep.status), _stream()), "pna_aggregate_fwd")
    return z, stats


def pna_aggregate_bwd(dz, ab, stats, prep: PreparedGraph, cfg: PNAConfig):
    """dab = [da | db] ([n, 2 f]) of pna_aggregate_fwd from dz = d z (its first f columns, the gradient of the copy of x, are not
    read: pna_add_input_grad)."""
    _chk(dz, _f32, "dz"); _chk(ab, _f32, "ab"); _chk(stats, _f32, "stats")
    n, f2 = ab.shape
    f = f2 // 2
    if n != prep.n or tuple(dz.shape) != (n, cfg.blocks * f) or tuple(stats.shape) != (n, PNA_NSTAT, f):
        raise ValueError("dz must be [n, blocks * f] and stats [n, 6, f] over the prepared graph's nodes")
    loops = gcn2_loops(prep)
    dab = torch.empty_like(ab)
    items, n_items, cap = _long_items(prep, by_target=False, forward=False)
    ws = _ws(lib().grapes_pna_aggregate_bwd_workspace_bytes(n, cap, f), dz.device)
    _lib.check(lib().grapes_pna_aggregate_bwd(_p(dz), ab.data_ptr() + 4 * f, 2 * f, _p(stats), _p(loops), _p(prep.rowptr_t),
                                              _p(prep.rowptr_s), _p(prep.csr_dst), cfg.n_agg, cfg.agg_code, cfg.n_scal,
                                              cfg.scal_code, cfg.avg_log, cfg.avg_lin, _p(dab), dab.data_ptr() + 4 * f, 2 * f, n,
                                              _p(prep.d_n), f, items, n_items, cap, _p(ws), _p(prep.status), _stream()),
               "pna_aggregate_bwd")
    return dab


def pna_add_input_grad(dx, dz, d_n=None):
    """dx += dz[:, :f] in place (the gradient that reaches x through its copy in post_nn's operand)."""
    _chk(dx, _f32, "dx"); _chk(dz, _f32, "dz")
    n, f = dx.shape
    if dz.shape[0] != n or dz.shape[1] < f:
        raise ValueError("dz must be [n, >= f]")
    _lib.check(lib().grapes_pna_add_input_grad(_p(dx), _p(dz), dz.shape[1], n, _p(d_n), f, _stream()), "pna_add_input_grad")
    return dx


# ------------------------------------------------------------------------------- GCNConv with edge weights (PyG GCNConv.forward)
WGCN_LOOP_FILL, WGCN_LOOP_SUM, WGCN_UNNORMALIZED = 0, 1, 2      # GRAPES_WGCN_* of grapes_hip.h: the rule for lw, and whether dinv exists


class WeightedStructure:
    """Where every entry of an edge list sits in the two CSRs of the PreparedGraph built from it: pos_t / pos_s [e] (slot by target
    / by source, -1 for a stored loop or a dropped entry), their inverses inv_t / inv_s, and loop_src [n] (the input index of the
    stored loop that sets a node's loop weight — the last one in input order — or -1).  Built once per edge list; the weights
    themselves go through wgcn_weights on every call.  Duplicates of one (r, c) take adjacent slots in input order.
    loops(): (loop_ptr [n + 1], loop_idx) — every node's stored loops as a list in input order, for the modes that sum them; built
    on first use."""

    __slots__ = ("prep", "edge_src", "edge_dst", "n", "e", "pos_t", "pos_s", "inv_t", "inv_s", "loop_src", "_loops")

    def __init__(self, prep: PreparedGraph, edge_src, edge_dst):
        _chk(edge_src, _i32, "edge_src"); _chk(edge_dst, _i32, "edge_dst")
        e = edge_src.numel()
        if edge_dst.numel() != e or e != prep.e:
            raise ValueError("WeightedStructure: edge_src / edge_dst must be the list the PreparedGraph was built from")
        dev = edge_src.device
        self.prep, self.edge_src, self.edge_dst, self.n, self.e = prep, edge_src, edge_dst, prep.n, e
        self._loops = None
        self.pos_t = torch.empty(max(e, 1), dtype=_i32, device=dev); self.pos_s = torch.empty(max(e, 1), dtype=_i32, device=dev)
        self.inv_t = torch.empty(max(e, 1), dtype=_i32, device=dev); self.inv_s = torch.empty(max(e, 1), dtype=_i32, device=dev)
        self.loop_src = torch.empty(max(prep.n, 1), dtype=_i32, device=dev)
        ws = _ws(lib().grapes_wgcn_structure_workspace_bytes(e), dev)
        _lib.check(lib().grapes_wgcn_structure(_p(edge_src), _p(edge_dst), e, _p(prep.d_e), prep.n, _p(prep.d_n), _p(prep.rowptr_t),
                                               _p(prep.csr_src), _p(prep.rowptr_s), _p(prep.csr_dst), _p(self.pos_t), _p(self.pos_s),
                                               _p(self.inv_t), _p(self.inv_s), _p(self.loop_src), _p(ws), _p(prep.status), _stream()),
                   "wgcn_structure")

    def loops(self):
        if self._loops is None:
            dev, prep = self.edge_src.device, self.prep
            loop_ptr = torch.empty(self.n + 1, dtype=_i32, device=dev)
            loop_idx = torch.empty(max(self.e, 1), dtype=_i32, device=dev)
            ws = _ws(lib().grapes_wgcn_loops_workspace_bytes(self.n, self.e), dev)
            _lib.check(lib().grapes_wgcn_loops(_p(self.edge_src), _p(self.edge_dst), self.e, _p(prep.d_e), self.n, _p(prep.d_n),
                                               _p(loop_ptr), _p(loop_idx), _p(ws), _stream()), "wgcn_loops")
            self._loops = (loop_ptr, loop_idx)
        return self._loops


class WeightedValues:
    """What wgcn_weights makes of one weight vector: val_t / val_s (the weights in both CSR orders), lw (the loop weights) and
    dinv = (lw + the weighted in-degree)^-1/2 (inf -> 0; a negative degree gives NaN, as in PyG); mode: the rule they were made
    by (WGCN_UNNORMALIZED: dinv is None)."""

    __slots__ = ("val_t", "val_s", "lw", "dinv", "mode")


def wgcn_weights(ws: WeightedStructure, edge_weight, mode: int = WGCN_LOOP_FILL, fill: float = 1.0) -> WeightedValues:
    """mode / fill: the rule for lw (grapes_hip.h: GRAPES_WGCN_*).  edge_weight None (any mode but the default one): every weight
    is 1 — no ones vector is formed."""
    _chk(edge_weight, _f32, "edge_weight", mode != WGCN_LOOP_FILL or fill != 1.0)
    if mode not in (WGCN_LOOP_FILL, WGCN_LOOP_SUM, WGCN_UNNORMALIZED):
        raise ValueError(f"wgcn_weights: mode {mode}")
    if edge_weight is not None and edge_weight.numel() != ws.e:
        raise ValueError(f"edge_weight holds {edge_weight.numel()} values for {ws.e} entries")
    dev, prep = ws.edge_src.device, ws.prep
    v = WeightedValues()
    v.mode = mode
    v.val_t = torch.empty(max(ws.e, 1), dtype=_f32, device=dev); v.val_s = torch.empty(max(ws.e, 1), dtype=_f32, device=dev)
    v.lw = torch.empty(max(ws.n, 1), dtype=_f32, device=dev)
    v.dinv = torch.empty(max(ws.n, 1), dtype=_f32, device=dev) if mode != WGCN_UNNORMALIZED else None
    loop_ptr, loop_idx = (None, None) if mode == WGCN_LOOP_FILL else ws.loops()
    _lib.check(lib().grapes_wgcn_weights(_p(edge_weight), ws.e, _p(ws.inv_t), _p(ws.inv_s), _p(ws.loop_src), _p(loop_ptr), _p(loop_idx),
                                         _p(prep.rowptr_t), _p(prep.rowptr_s), ws.n, _p(prep.d_n), mode, float(fill), _p(v.val_t),
                                         _p(v.val_s), _p(v.lw), _p(v.dinv), _stream()), "wgcn_weights")
    return v


def wgcn_aggregate_fwd(h, ws: WeightedStructure, vals: WeightedValues, bias=None, relu=False, out=None):
    """out[c] = dinv[c] sum_{e: r -> c} w_e dinv[r] h[r] + dinv[c]^2 lw[c] h[c] + bias (+ReLU) over the first ws.n rows of h (h and
    out may hold more rows, which are left alone); with vals of WGCN_UNNORMALIZED out[c] = sum_e w_e h[r] + lw[c] h[c] + bias."""
    _chk(h, _f32, "h"); _chk(bias, _f32, "bias", True); _chk(out, _f32, "out", True)
    prep, (rows, f) = ws.prep, h.shape
    _gather_width(f, "weighted GCN aggregation")
    if out is None:
        out = torch.empty_like(h)
    if rows < ws.n or out.shape[0] < ws.n or out.shape[1] != f or (bias is not None and bias.numel() != f):
        raise ValueError("h and out need one row of the same width per node of the structure's graph, bias one value per column")
    items, n_items, cap = _long_items(prep, by_target=True, forward=True)
    wsp = _ws(lib().grapes_wgcn_aggregate_workspace_bytes(cap, f), h.device) if cap else None
    _lib.check(lib().grapes_wgcn_aggregate_fwd(_p(h), _p(prep.rowptr_t), _p(prep.csr_src), _p(vals.val_t), _p(vals.dinv), _p(vals.lw),
                                               _p(bias), _p(out), ws.n, _p(prep.d_n), f, 1 if relu else 0, vals.mode, items, n_items,
                                               cap, _p(wsp), _p(prep.status), _stream()), "wgcn_aggregate_fwd")
    return out


def wgcn_aggregate_bwd(dout, ws: WeightedStructure, vals: WeightedValues, h=None, relu_out=None, want_dh=True, want_dw=False,
                       want_bias=True):
    """(dh, dbias, dw) of wgcn_aggregate_fwd + wgcn_weights: dout gated by relu_out > 0 when given; dw (the gradient of the edge
    weights, in input order, through the normalisation too — by the rule of vals.mode) needs h, the forward's input.  dout is not
    modified."""
    _chk(dout, _f32, "dout"); _chk(relu_out, _f32, "relu_out", True); _chk(h, _f32, "h", True)
    prep, (rows, f) = ws.prep, dout.shape
    _gather_width(f, "weighted GCN aggregation")
    if rows < ws.n or (relu_out is not None and relu_out.shape != dout.shape) or (h is not None and h.shape != dout.shape):
        raise ValueError("dout, relu_out and h must be [>= n, f] over the structure's nodes")
    if want_dw and h is None:
        raise ValueError("the edge-weight gradient needs h, the aggregation's input")
    if not (want_dh or want_dw or want_bias):
        return None, None, None
    dev = dout.device
    dh = torch.empty_like(dout) if want_dh else None
    dbias = torch.empty(f, dtype=_f32, device=dev) if want_bias else None
    dw = torch.empty(max(ws.e, 1), dtype=_f32, device=dev)[: ws.e] if want_dw else None
    items_t, n_items_t, cap = _long_items(prep, by_target=True, forward=False)
    items_s, n_items_s, _ = _long_items(prep, by_target=False, forward=False)
    wsp = _ws(lib().grapes_wgcn_aggregate_bwd_workspace_bytes(ws.n, ws.e, cap, f), dev)
    _lib.check(lib().grapes_wgcn_aggregate_bwd(_p(dout), _p(relu_out), _p(h) if want_dw else None, _p(ws.edge_src), _p(ws.edge_dst),
                                               ws.e, _p(prep.d_e), _p(ws.pos_t), _p(ws.loop_src), _p(prep.rowptr_t), _p(prep.csr_src),
                                               _p(vals.val_t), _p(prep.rowptr_s), _p(prep.csr_dst), _p(vals.val_s), _p(vals.dinv),
                                               _p(vals.lw), _p(dh), _p(dbias), _p(dw), ws.n, _p(prep.d_n), f, vals.mode, items_t,
                                               n_items_t, items_s, n_items_s, cap, _p(wsp), _p(prep.status), _stream()),
               "wgcn_aggregate_bwd")
    return dh, dbias, dw


# ------------------------------------------------------------------------------- sampler
def gumbel_topk(logits, k, uniforms=None, logit_index=None, candidate_ids=None, n=None, d_n=None, mode=0,
                philox_seed=0, philox_offset=0, d_philox_offset=None, want_log_prob=True, want_keys=False,
                want_stats=True, prefix_ids=None, stats_out=None, agg=None, defer_finish=False, ext=None):
    """Sampler draw (two launches).  Returns dict(mask, kept_pos, kept_ids, kept_count, log_prob, keys, stats);
    defer_finish: the draw's last launch has no tail — res["finish"] must be handed to the NEXT frontier_expand_fused(finish=...)
    on the stream, whose extra workgroup forms stats[4] (the log-prob sum) and zeroes the draw-wide histogram; until then stats[4]
    is not valid and no other draw may start on the device.
    with prefix_ids also union_ids = [prefix_ids | kept ids] and union_count (main.py:236-238).
    agg = (head_in [n_rows] or [n_rows, 1], prep, bias [1], cand_pos): `logits` is None and the logits are produced on the way,
    logits[r] = (Â head_in)[r] + bias over the prepared hop graph (the sampler net's 1-wide last layer), fused with the key
    computation; logit_index is then required (nb_local).  The result carries them as res["logits"] ([n_rows, 1])."""
    if agg is not None:
        head_in, prep, bias, cand_pos = agg
        _chk(head_in, _f32, "head_in"); _chk(bias, _f32, "bias", True); _chk(cand_pos, _i32, "cand_pos")
        if logits is not None or logit_index is None:
            raise ValueError("gumbel_topk(agg=...): logits must be None and logit_index given")
        n_rows = head_in.numel()
        logits = torch.empty(n_rows, dtype=_f32, device=head_in.device)
    _chk(logits, _f32, "logits"); _chk(uniforms, _f32, "uniforms", True)
    _chk(logit_index, _i32, "logit_index", True); _chk(candidate_ids, _i32, "candidate_ids", True)
    _chk(prefix_ids, _i32, "prefix_ids", True)
    dev = logits.device
    if n is None:
        n = logit_index.numel() if logit_index is not None else logits.numel()
    if uniforms is not None and uniforms.numel() < n:
        raise ValueError("uniforms shorter than the candidate list")
    if prefix_ids is not None and candidate_ids is None:
        raise ValueError("prefix_ids needs candidate_ids")
    kk = min(k, n) if n > 0 else 0
    mask = torch.empty(n, dtype=_f32, device=dev)
    kept_pos = torch.empty(max(kk, 1), dtype=_i32, device=dev)
    kept_ids = torch.empty(max(kk, 1), dtype=_i32, device=dev) if candidate_ids is not None else None
    cnt = torch.empty(1, dtype=_i32, device=dev)
    log_prob = torch.empty(n, dtype=_f32, device=dev) if want_log_prob else None
    keys = torch.empty(n, dtype=_f32, device=dev) if want_keys else None
    stats = (stats_out if stats_out is not None else torch.empty(6, dtype=_f32, device=dev)) if want_stats else None
    _chk(stats, _f32, "stats", True)
    npre = prefix_ids.numel() if prefix_ids is not None else 0
    union = torch.empty(npre + max(kk, 1), dtype=_i32, device=dev) if prefix_ids is not None else None
    ucnt = torch.empty(1, dtype=_i32, device=dev) if prefix_ids is not None else None
    ws = _ws(lib().grapes_sampler_workspace_bytes(n), dev)
    finish = None
    if agg is not None:
        _lib.check(lib().grapes_gumbel_topk_from_aggregate(
            _p(head_in), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv), _p(bias), _p(logits), n_rows, _p(prep.d_n),
            _p(cand_pos), _p(logit_index), _p(uniforms), philox_seed, philox_offset, _p(d_philox_offset), n, _p(d_n), k, mode,
            _p(candidate_ids), _p(mask), _p(kept_pos), _p(kept_ids), _p(cnt), _p(log_prob), _p(keys), _p(stats),
            _p(prefix_ids), npre, _p(union), _p(ucnt), _p(ws), _stream()), "gumbel_topk_from_aggregate")
    elif _SAMPLER_GHIST and defer_finish and n > 0:
        import ctypes as C
        fin = _DrawFinishArgs()
        e_rowptr = e_prefix = union_ext = None
        if ext is not None:       # ext = (rowptr of the graph expanded next, prefix ids' extents int64[2 npre]): res["union_ext"]
            e_rowptr, e_prefix = ext
            _chk(e_rowptr, _i64, "ext rowptr"); _chk(e_prefix, _i64, "ext prefix", npre == 0)
            if prefix_ids is None or (npre and e_prefix.numel() < 2 * npre):
                raise ValueError("gumbel_topk(ext=...): needs prefix_ids and two int64 per prefix id")
            union_ext = torch.empty(2 * (npre + max(kk, 1)), dtype=torch.int64, device=dev)
        _lib.check(lib().grapes_gumbel_topk_deferred_ext(_p(logits), _p(logit_index), _p(uniforms), philox_seed, philox_offset,
                                                         _p(d_philox_offset), n, _p(d_n), k, mode, _p(candidate_ids), _p(mask),
                                                         _p(kept_pos), _p(kept_ids), _p(cnt), _p(log_prob), _p(keys), _p(stats),
                                                         _p(prefix_ids), npre, _p(union), _p(ucnt), _p(ws), _p(_sampler_hist(dev)),
                                                         C.byref(fin), _p(e_rowptr), _p(e_prefix), _p(union_ext), _stream()),
                   "gumbel_topk_deferred_ext")
        finish = (fin, ws, stats)             # (the workspace must outlive the launch that finishes the draw)
    elif _SAMPLER_GHIST:
        _lib.check(lib().grapes_gumbel_topk_hist(_p(logits), _p(logit_index), _p(uniforms), philox_seed, philox_offset,
                                                 _p(d_philox_offset), n, _p(d_n), k, mode, _p(candidate_ids), _p(mask),
                                                 _p(kept_pos), _p(kept_ids), _p(cnt), _p(log_prob), _p(keys), _p(stats),
                                                 _p(prefix_ids), npre, _p(union), _p(ucnt), _p(ws), _p(_sampler_hist(dev)), _stream()),
                   "gumbel_topk_hist")
    else:
        _lib.check(lib().grapes_gumbel_topk(_p(logits), _p(logit_index), _p(uniforms), philox_seed, philox_offset,
                                            _p(d_philox_offset), n, _p(d_n), k, mode, _p(candidate_ids), _p(mask),
                                            _p(kept_pos), _p(kept_ids), _p(cnt), _p(log_prob), _p(keys), _p(stats),
                                            _p(prefix_ids), npre, _p(union), _p(ucnt), _p(ws), _stream()), "gumbel_topk")
    out = dict(mask=mask, kept_pos=kept_pos[:kk], kept_ids=None if kept_ids is None else kept_ids[:kk], kept_count=cnt,
               log_prob=log_prob, keys=keys, stats=stats)
    if prefix_ids is not None:
        out["union_ids"], out["union_count"] = union[:npre + kk], ucnt
    if agg is not None:
        out["logits"] = logits.view(-1, 1)
    if finish is not None:
        out["finish"] = finish
        if ext is not None:
            out["union_ext"] = union_ext
    return out


_TICKETS = {}
_SAMPLER_HIST = {}
_SAMPLER_GHIST = _sw("GRAPES_SAMPLER_GHIST", "1") != "0"     # A/B: one 12-bit histogram per draw instead of per-workgroup 8-bit rows


def _sampler_hist(dev) -> torch.Tensor:
    """The per-device, zero-at-rest histogram of grapes_gumbel_topk_hist (draws on one device are stream-ordered)."""
    t = _SAMPLER_HIST.get(dev)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("sampler histogram: first use inside a stream capture; run one eager draw first")
        t = torch.zeros(int(lib().grapes_sampler_hist_words()), dtype=_i32, device=dev)
        _SAMPLER_HIST[dev] = t
    return t


def _ticket(dev) -> torch.Tensor:
    """A persistent zero word per device for the last-workgroup tickets (kernels leave it zero)."""
    t = _TICKETS.get(dev)
    if t is None:
        t = torch.zeros(64, dtype=_i32, device=dev)     # [0] sums, [1] sampler head bwd, [8] step losses, [16:32] column sums
        _TICKETS[dev] = t
    return t


def bernoulli_logprob_bwd(logits, mask, grad_vec=None, d_grad_scale=None, logit_index=None, out=None, d_n=None,
                          sum_out=None, accumulate_sum=False):
    """sum_out: float32[1] that receives (+)= the sum of the gradients written (bias gradient of a 1-wide head)."""
    _chk(logits, _f32, "logits"); _chk(mask, _f32, "mask"); _chk(sum_out, _f32, "sum_out", True)
    n = mask.numel()
    if out is None:
        out = torch.zeros_like(logits) if logit_index is not None else torch.empty_like(logits)
    partials = torch.empty(2048, dtype=_f32, device=logits.device) if sum_out is not None else None
    ticket = _ticket(logits.device) if sum_out is not None else None
    _lib.check(lib().grapes_bernoulli_logprob_bwd(_p(logits), _p(logit_index), _p(mask), _p(grad_vec), _p(d_grad_scale),
                                                  _p(out), n, _p(d_n), _p(sum_out), 1 if accumulate_sum else 0,
                                                  _p(partials), _p(ticket), _stream()), "bernoulli_logprob_bwd")
    return out


class SamplerHeadBwdMulti:
    """Backward of the sampler net's 1-wide head for up to four hops in two launches: per hop the dense d log_prob / d logit
    (zero on non-candidate rows; cand_pos from frontier_compact(want_cand_pos=True)) and its by-source aggregation
    Âᵀ dlogits; sum_out (+)= the sum of all dlogits.  A hop whose mask is None is a MEAN head (the log-Z net): d logits =
    scale / n on its live rows, their sum goes to mean_sum_out.  Results: .dlog, .dh ([count, n_cap] each) once launch(0), or
    launch(1) and launch(2), have been issued — between the two the caller may issue launches of its own, and each of them
    carries a pending recorded few-row backward aggregation (carry_backward_aggregations)."""

    def __init__(self, logits, masks, cand_pos, preps, d_grad_scale=None, sum_out=None, accumulate_sum=False, mean_sum_out=None):
        k = len(logits)
        if not (1 <= k <= 4) or len(masks) != k or len(cand_pos) != k or len(preps) != k:
            raise ValueError("sampler_head_bwd_multi: 1..4 hops")
        dev = logits[0].device
        for l, m, c in zip(logits, masks, cand_pos):
            _chk(l, _f32, "logits"); _chk(m, _f32, "mask", True); _chk(c, _i32, "cand_pos", m is None)
        _chk(mean_sum_out, _f32, "mean_sum_out", True)
        _chk(sum_out, _f32, "sum_out", True); _chk(d_grad_scale, _f32, "d_grad_scale", True)
        self.k, self.dev = k, dev
        self.caps = [int(l.numel()) for l in logits]
        ncap = max(self.caps)
        self.dlog = torch.empty((k, ncap), dtype=_f32, device=dev)
        self.dh = torch.empty((k, ncap), dtype=_f32, device=dev)
        self.ws = _ws(lib().grapes_sampler_head_bwd_multi_workspace_bytes(), dev)
        self._hold = (list(logits), list(masks), list(cand_pos), list(preps), d_grad_scale, sum_out, mean_sum_out)
        self.accumulate_sum = accumulate_sum

    def launch(self, phase: int = 0):
        import ctypes as C
        logits, masks, cand_pos, preps, d_grad_scale, sum_out, mean_sum_out = self._hold
        k, dlog, dh = self.k, self.dlog, self.dh
        arr = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
        _lib.check(lib().grapes_sampler_head_bwd_multi_phase(
            k, arr(logits), arr(masks), arr(cand_pos), (C.c_int32 * k)(*self.caps), arr([p.d_n for p in preps]), _p(d_grad_scale),
            arr([p.rowptr_s for p in preps]), arr([p.csr_dst for p in preps]), arr([p.dinv for p in preps]),
            arr([dlog[q] for q in range(k)]), arr([dh[q] for q in range(k)]), _p(sum_out), 1 if self.accumulate_sum else 0,
            _p(mean_sum_out), _p(self.ws), _p(_ticket(self.dev)[1:2]), int(phase), _stream()), "sampler_head_bwd_multi")


def sampler_head_bwd_multi(logits, masks, cand_pos, preps, d_grad_scale=None, sum_out=None, accumulate_sum=False,
                           mean_sum_out=None):
    """SamplerHeadBwdMulti in one call.  Returns (dlogits [count, n_cap], dh [count, n_cap])."""
    hb = SamplerHeadBwdMulti(logits, masks, cand_pos, preps, d_grad_scale=d_grad_scale, sum_out=sum_out,
                             accumulate_sum=accumulate_sum, mean_sum_out=mean_sum_out)
    hb.launch(0)
    return hb.dlog, hb.dh


def philox_uniform(n, seed, offset, device):
    out = torch.empty(n, dtype=_f32, device=device)
    _lib.check(lib().grapes_philox_uniform(_p(out), n, seed, offset, _stream()), "philox_uniform")
    return out


def fill(x, value=0.0, d_n=None, d_value=None, scale_by_inv_n=0.0, sum_out=None, accumulate_sum=False):
    """x[i] = value (or *d_value, optionally times scale_by_inv_n / n) for i < n; sum_out (+)= n * that value."""
    _chk(x, _f32, "x"); _chk(sum_out, _f32, "sum_out", True)
    _lib.check(lib().grapes_fill(_p(x), x.numel(), _p(d_n), float(value), _p(d_value), float(scale_by_inv_n), _p(sum_out),
                                 1 if accumulate_sum else 0, _stream()), "fill")
    return x


def reduce_sum(x, mean=False, d_n=None):
    _chk(x, _f32, "x")
    out = torch.empty(1, dtype=_f32, device=x.device)
    _lib.check(lib().grapes_reduce_sum(_p(x), x.numel(), _p(d_n), 1 if mean else 0, _p(out), _stream()), "reduce_sum")
    return out


# ------------------------------------------------------------------------------- ingest (§8f N3)
def csr_build(edge_index, num_nodes, status=None):
    """(rowptr int64[N+1], col int32[nnz]) of sp.csr_matrix((ones(E, bool), edge_index), (N, N)) — main.py:134-136 —
    from a device int64 edge_index [2, E].  One host read (nnz) to trim the column array."""
    if not edge_index.is_cuda or edge_index.dtype != _i64:
        raise _lib.GrapesHipError("csr_build: edge_index must be a cuda int64 tensor (torch.long, as the reference's data.edge_index)")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must be [2, E]")
    dev, E, N = edge_index.device, int(edge_index.shape[1]), int(num_nodes)
    src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()
    rowptr = torch.empty(N + 1, dtype=_i64, device=dev)
    col = torch.empty(max(E, 1), dtype=_i32, device=dev)
    nnz = torch.zeros(1, dtype=_i64, device=dev)
    own = status is None
    if own:
        status = torch.zeros(1, dtype=_i32, device=dev)
    ws = torch.empty(int(lib().grapes_csr_build_workspace_bytes(E, N)) + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    _lib.check(lib().grapes_csr_build(_p(src), _p(dst), E, N, _p(rowptr), _p(col), _p(nnz), ws.data_ptr() + off, _p(status),
                                      _stream()), "csr_build")
    k = int(nnz.item())
    if own and int(status.item()):
        raise _lib.GrapesHipError("csr_build: edge_index holds node ids outside [0, num_nodes)")
    del ws
    return rowptr, col[:k].clone() if k < col.numel() // 2 else col[:k]


# ------------------------------------------------------------------------------- full graph above 2^31 entries (N1)
def _aligned_ws(nbytes: int, device) -> "tuple[torch.Tensor, int]":
    ws = _tmp(torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device))
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


def csr_symmetric_check(rowptr, col, n) -> int:
    """Device flag of grapes_csr_symmetric_check: 0 = every (r, c), r != c, has (c, r); bit 1 = not symmetric; bit 2 = a bad id.
    One host read."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col")
    flag = torch.empty(1, dtype=_i32, device=rowptr.device)
    _lib.check(lib().grapes_csr_symmetric_check(_p(rowptr), _p(col), int(n), _p(flag), _stream()), "csr_symmetric_check")
    return int(flag.item())


def csr_transpose_bytes(nnz: int, n: int) -> int:
    """HBM the transpose allocates: its rowptr + col and the build's workspace."""
    return 8 * (n + 1) + 4 * max(nnz, 1) + int(lib().grapes_csr_build_workspace_bytes(nnz, n)) + 256


def csr_transpose(rowptr, col, n, status=None):
    """(rowptr_t int64[N+1], col_t int32[nnz]): the CSR of (c, r) for every stored (r, c), rows ascending."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(status, _i32, "status", True)
    dev, nnz = rowptr.device, col.numel()
    rowptr_t = torch.empty(n + 1, dtype=_i64, device=dev)
    col_t = torch.empty(max(nnz, 1), dtype=_i32, device=dev)
    ws, base = _aligned_ws(lib().grapes_csr_build_workspace_bytes(nnz, n), dev)
    _lib.check(lib().grapes_csr_transpose(_p(rowptr), _p(col), nnz, int(n), _p(rowptr_t), _p(col_t), base, _p(status), _stream()),
               "csr_transpose")
    del ws
    return rowptr_t, col_t


class LargeGraphPlan:
    """The by-target CSR, dinv and hub-item count of a whole graph for full-batch message passing with 64-bit offsets
    (DeviceGraph.full_graph_plan): rowptr_t / col_t are the graph's own arrays when it is symmetric, else its transpose."""

    __slots__ = ("n", "rowptr_t", "col_t", "dinv", "chunk", "item_cap", "symmetric")

    def __init__(self, rowptr_t, col_t, n, symmetric, chunk=1024):
        """chunk: rows with more entries are cut into work items of this many entries (a multiple of 64)."""
        _chk(rowptr_t, _i64, "rowptr_t"); _chk(col_t, _i32, "col_t")
        self.n, self.rowptr_t, self.col_t, self.symmetric, self.chunk = int(n), rowptr_t, col_t, bool(symmetric), int(chunk)
        self.dinv = torch.empty(max(self.n, 1), dtype=_f32, device=rowptr_t.device)
        d_items = torch.empty(1, dtype=_i64, device=rowptr_t.device)
        _lib.check(lib().grapes_gcn_large_prepare(_p(rowptr_t), _p(col_t), self.n, self.chunk, _p(self.dinv), _p(d_items), _stream()),
                   "gcn_large_prepare")
        self.item_cap = int(d_items.item())
        if self.item_cap >= 2 ** 31:
            raise ValueError("full_graph_plan: more than 2^31 hub-row work items")


def gcn_large_aggregate_workspace_bytes(plan: LargeGraphPlan, m: int, f: int) -> int:
    return int(lib().grapes_gcn_large_aggregate_workspace_bytes(int(m), plan.item_cap, int(f))) + 256


def gcn_large_aggregate(h, plan: LargeGraphPlan, prescaled: bool, r0=0, m=None, rows=None, bias=None, relu=False, out=None,
                        status=None):
    """out[i] = Â h [row i] + bias (+ReLU) for the rows r0 .. r0+m-1, or for rows[i] (int32): the gather-SpMM with 64-bit row
    offsets.  h [N, ldh] with ldh % 4 == 0 (the width f = h.shape[1] must be a multiple of 4: callers pad), out [m, f]."""
    _chk(h, _f32, "h"); _chk(bias, _f32, "bias", True); _chk(rows, _i32, "rows", True); _chk(status, _i32, "status", True)
    n, f = h.shape
    if n != plan.n:
        raise ValueError("gcn_large_aggregate: h must hold every node's row")
    if rows is not None:
        m = rows.numel()
    elif m is None or r0 < 0 or r0 + m > n:
        raise ValueError("gcn_large_aggregate: row range outside the graph")
    if out is None:
        out = torch.empty((m, f), dtype=_f32, device=h.device)
    elif out.shape[0] < m or out.shape[1] != f or out.stride(1) != 1:
        raise ValueError("gcn_large_aggregate: out must be [m, f] with unit column stride")
    ws, base = _aligned_ws(lib().grapes_gcn_large_aggregate_workspace_bytes(m, plan.item_cap, f), h.device)
    _lib.check(lib().grapes_gcn_large_aggregate(_p(h), h.stride(0), _p(plan.rowptr_t), _p(plan.col_t), _p(plan.dinv),
                                                1 if prescaled else 0, int(r0), _p(rows), int(m), int(f), _p(bias),
                                                1 if relu else 0, _p(out), out.stride(0), plan.chunk, plan.item_cap, base, _p(status),
                                                _stream()), "gcn_large_aggregate")
    del ws
    return out


# ------------------------------------------------------------------------------- 1-D partition exchange (§8e)
def exchange_pack_query(ids32, d_n, cap, query):
    """query[cap + 1] <- [ids | padding | live count] in one launch."""
    _chk(ids32, _i32, "ids"); _chk(query, _i32, "query"); _chk(d_n, _i32, "d_n", True)
    if query.numel() != cap + 1:
        raise ValueError("exchange_pack_query: query must hold cap + 1 words")
    _lib.check(lib().grapes_exchange_pack_query(_p(ids32), ids32.numel(), _p(d_n), cap, _p(query), _stream()),
               "exchange_pack_query")


def exchange_serve_rows(rowptr_local, col_local, req, n_peers, cap, lo, hi, reply, reply_stride, e_slot, status=None):
    """Owner side of the adjacency-row exchange: fills the per-peer reply slots [len | off | columns]."""
    _chk(rowptr_local, _i64, "rowptr_local"); _chk(col_local, _i32, "col_local"); _chk(req, _i32, "req")
    _chk(reply, _i32, "reply")
    if req.numel() != n_peers * (cap + 1) or reply.numel() != n_peers * reply_stride:
        raise ValueError("exchange_serve_rows: req / reply do not match (n_peers, cap, reply_stride)")
    eoff = torch.empty(n_peers * cap + 1, dtype=_i32, device=req.device)
    if col_local.numel() == 0 and hi > lo:     # a shard of nodes without any edge: every length is 0 and no column is read,
        col_local = eoff                       # but the call takes no NULL there (an empty tensor has no address)
    _lib.check(lib().grapes_exchange_serve_rows(_p(rowptr_local), _p(col_local), _p(req), n_peers, cap, lo, hi, _p(reply),
                                                reply_stride, e_slot, _p(eoff), _p(status), _stream()),
               "exchange_serve_rows")


def exchange_recv_rows(back, reply_stride, nodes, bounds, n_peers, e_cap, d_m=None, status=None):
    """Requester side: (src, dst, d_e, eoff) with the contract of frontier_offsets + frontier_expand."""
    _chk(back, _i32, "back"); _chk(nodes, _i32, "nodes"); _chk(bounds, _i32, "bounds")
    cap, dev = nodes.numel(), nodes.device
    if back.numel() != n_peers * reply_stride or bounds.numel() != n_peers + 1:
        raise ValueError("exchange_recv_rows: back / bounds do not match (n_peers, reply_stride)")
    eoff = torch.empty(cap + 1, dtype=_i32, device=dev)
    rowstart = torch.empty(cap, dtype=_i32, device=dev)
    src = torch.empty(e_cap, dtype=_i32, device=dev)
    dst = torch.empty(e_cap, dtype=_i32, device=dev)
    d_e = torch.empty(1, dtype=_i32, device=dev)
    _lib.check(lib().grapes_exchange_recv_rows(_p(back), reply_stride, _p(nodes), cap, _p(d_m), _p(bounds), n_peers, e_cap,
                                               _p(eoff), _p(rowstart), _p(src), _p(dst), _p(d_e), _p(status), _stream()),
               "exchange_recv_rows")
    return src, dst, d_e, eoff


def exchange_serve_features(X_local, req, n_peers, cap, lo, hi, reply, n_slot, status=None):
    _chk(X_local, _f32, "X_local"); _chk(req, _i32, "req"); _chk(reply, _f32, "reply")
    F = X_local.shape[1]
    if req.numel() != n_peers * (cap + 1) or reply.numel() != n_peers * n_slot * F:
        raise ValueError("exchange_serve_features: req / reply do not match (n_peers, cap, n_slot, F)")
    _lib.check(lib().grapes_exchange_serve_features(_p(X_local), F, _p(req), n_peers, cap, lo, hi, _p(reply), n_slot,
                                                    _p(status), _stream()), "exchange_serve_features")


def exchange_assemble_features(back, F, n_slot, ids, bounds, n_peers, d_n=None, ind_code=None, epoch=0, d_epoch=None,
                               num_ind=0, out=None):
    _chk(back, _f32, "back"); _chk(ids, _i32, "ids"); _chk(bounds, _i32, "bounds"); _chk(ind_code, _i32, "ind_code", True)
    n = ids.numel()
    if back.numel() != n_peers * n_slot * F or bounds.numel() != n_peers + 1:
        raise ValueError("exchange_assemble_features: back / bounds do not match (n_peers, n_slot, F)")
    if out is None:
        out = torch.empty((n, F + num_ind), dtype=_f32, device=ids.device)
    _lib.check(lib().grapes_exchange_assemble_features(_p(back), F, n_slot, _p(ids), n, _p(d_n), _p(bounds), n_peers,
                                                       _p(ind_code), epoch, _p(d_epoch), num_ind, _p(out), _stream()),
               "exchange_assemble_features")
    return out


def exchange_halo_positions(ids, bounds, n_peers, n_slot, d_n=None, ind_code=None, pos=None, code_pos=None):
    """(pos int32[len(ids)], code_pos int32[n_peers * n_slot] | None): where the rows of `ids` sit inside the exchanged buffer
    back[n_peers * n_slot, F], and their indicator words at those positions (see include/grapes_hip.h)."""
    _chk(ids, _i32, "ids"); _chk(bounds, _i32, "bounds"); _chk(ind_code, _i32, "ind_code", True)
    n = ids.numel()
    if pos is None:
        pos = torch.empty(n, dtype=_i32, device=ids.device)
    if ind_code is not None and code_pos is None:
        code_pos = torch.zeros(n_peers * n_slot, dtype=_i32, device=ids.device)
    _lib.check(lib().grapes_exchange_halo_positions(_p(ids), n, _p(d_n), _p(bounds), n_peers, n_slot, _p(ind_code), _p(pos),
                                                    _p(code_pos) if ind_code is not None else None, _stream()), "exchange_halo_positions")
    return pos, (code_pos if ind_code is not None else None)


def exchange_note_rows(loc, ids, pos, base, d_n=None, node_map=None, batch=None, d_n_batch=None, idx_a=None, idx_b=None):
    """loc[ids[i]] = base + pos[row(i)] with row(i) = node_map[ids[i]] (ids that are rows of `batch` only) or idx_b[idx_a[i]]
    (include/grapes_hip.h: grapes_exchange_note_rows) — where a node's feature row sits among the rows already received."""
    _chk(loc, _i32, "loc"); _chk(ids, _i32, "ids"); _chk(pos, _i32, "pos"); _chk(node_map, _i32, "node_map", True)
    _chk(batch, _i32, "batch", True); _chk(idx_a, _i32, "idx_a", True); _chk(idx_b, _i32, "idx_b", True)
    _lib.check(lib().grapes_exchange_note_rows(_p(loc), _p(ids), ids.numel(), _p(d_n), _p(node_map), _p(batch),
                                               batch.numel() if batch is not None else 0, _p(d_n_batch), _p(idx_a), _p(idx_b),
                                               _p(pos), int(base), _stream()), "exchange_note_rows")


# ------------------------------------------------------------------------------- losses + Adam (§8f N2)
# ------------------------------------------------------------------------------- full-batch training above 2^31 entries
def rowlist_transpose_bytes(plan: LargeGraphPlan, e_cap: int) -> int:
    """HBM grapes_rowlist_transpose allocates: its outputs (srcs, src_off, pos, counts) and its workspace."""
    n = plan.n
    return (4 * n + 8 * (n + 1) + 4 * max(int(e_cap), 1) + 64 +
            int(lib().grapes_rowlist_transpose_workspace_bytes(int(e_cap), n)) + 256)


def rowlist_entries_cap(plan: LargeGraphPlan, rows) -> int:
    """Upper bound of the row-list transpose's entries: sum over rows of (row length + 1).  One host read."""
    rp = plan.rowptr_t
    r = rows.long()
    return int((rp[r + 1] - rp[r]).sum().item()) + rows.numel()


def rowlist_transpose(plan: LargeGraphPlan, rows, e_cap: int, status=None):
    """(srcs int32[n_src], src_off int64[n_src + 1], pos int32[entries]) of grapes_rowlist_transpose over the plan's CSR by
    target and the ascending, distinct int32 `rows`.  One host read (the two counts)."""
    _chk(rows, _i32, "rows"); _chk(status, _i32, "status", True)
    dev, n, m = rows.device, plan.n, rows.numel()
    srcs = torch.empty(max(n, 1), dtype=_i32, device=dev)
    src_off = torch.empty(n + 1, dtype=_i64, device=dev)
    pos = torch.empty(max(int(e_cap), 1), dtype=_i32, device=dev)
    counts = torch.zeros(2, dtype=_i64, device=dev)
    ws, base = _aligned_ws(lib().grapes_rowlist_transpose_workspace_bytes(int(e_cap), n), dev)
    _lib.check(lib().grapes_rowlist_transpose(_p(plan.rowptr_t), _p(plan.col_t), n, _p(rows), m, int(e_cap), _p(srcs), _p(src_off),
                                              _p(pos), _p(counts), base, _p(status), _stream()), "rowlist_transpose")
    del ws
    n_src, entries = (int(v) for v in counts.tolist())
    return srcs[:n_src], src_off[:n_src + 1], pos[:entries]


def rowlist_gather_t_item_cap(entries: int, chunk: int) -> int:
    return 2 * int(entries) // int(chunk) + 1


def rowlist_gather_t_workspace_bytes(n_src: int, item_cap: int, f: int) -> int:
    return int(lib().grapes_rowlist_gather_t_workspace_bytes(int(n_src), int(item_cap), int(f))) + 256


def rowlist_gather_t(g, srcs, src_off, pos, dinv, chunk: int, out=None, status=None):
    """out[j] = dinv[srcs[j]] * sum of g[pos[k]] over source j's entries (grapes_rowlist_gather_t).  g [M, f], f % 4 == 0; g may be
    a column slice of a wider matrix (unit column stride, the row pitch a multiple of 4)."""
    _chk(srcs, _i32, "srcs"); _chk(src_off, _i64, "src_off"); _chk(pos, _i32, "pos"); _chk(dinv, _f32, "dinv")
    _chk(status, _i32, "status", True)
    if g.dtype != _f32 or not g.is_cuda or g.dim() != 2 or g.stride(1) != 1:
        raise _lib.GrapesHipError("rowlist_gather_t: expected a CUDA fp32 matrix with unit column stride")
    n_src, f = srcs.numel(), g.shape[1]
    if out is None:
        out = torch.empty((n_src, f), dtype=_f32, device=g.device)
    elif out.shape[0] < n_src or out.shape[1] != f or out.stride(1) != 1:
        raise ValueError("rowlist_gather_t: out must be [n_src, f] with unit column stride")
    cap = rowlist_gather_t_item_cap(pos.numel(), chunk)
    if cap >= 2 ** 31:
        raise ValueError("rowlist_gather_t: more than 2^31 work items")
    ws, base = _aligned_ws(lib().grapes_rowlist_gather_t_workspace_bytes(n_src, cap, f), g.device)
    _lib.check(lib().grapes_rowlist_gather_t(_p(g), g.stride(0), _p(srcs), _p(src_off), _p(pos), _p(dinv), n_src, f, _p(out),
                                             out.stride(0), int(chunk), cap, base, _p(status), _stream()), "rowlist_gather_t")
    del ws
    return out


def dropout_rows(x, width: int, p: float, seed: int, offset: int, r0: int = 0, rows=None, f=None, out=None):
    """Dropout of rows r0.. (or rows[i]) of an N x width matrix with the mask grapes_dropout_fwd draws on the whole matrix
    (element r * width + c of the stream (seed, offset)); columns f.. untouched.  out may be x (in place)."""
    _chk(rows, _i32, "rows", True)
    if x.dtype != _f32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise _lib.GrapesHipError("dropout_rows: expected a CUDA fp32 matrix with unit column stride")
    m = x.shape[0]
    f = int(width if f is None else f)
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib().grapes_dropout_rows(_p(x), x.stride(0), _p(out), out.stride(0), int(r0), _p(rows), m, f, int(width), float(p),
                                         int(seed), int(offset), _stream()), "dropout_rows")
    return out


def rowlist_loss(z, C: int, rows, labels, dinv, p: float = 0.0, seed: int = 0, offset: int = 0, g=None, status=None):
    """(loss [1], g [M, ldg_cols] = dinv[rows] ⊙ dloss/dZ, dcol [ldg_cols] = column sums of dloss/dZ) of grapes_rowlist_loss over
    the pre-dropout logits z [M, >= C] of `rows`.  labels: int64 [N] (CrossEntropy) or fp32 [N, C] (BCEWithLogits).  g may be z."""
    _chk(rows, _i32, "rows"); _chk(dinv, _f32, "dinv"); _chk(status, _i32, "status", True)
    if z.dtype != _f32 or not z.is_cuda or z.dim() != 2 or z.stride(1) != 1:
        raise _lib.GrapesHipError("rowlist_loss: expected a CUDA fp32 matrix with unit column stride")
    multi = labels.dim() == 2
    _chk(labels, _f32 if multi else _i64, "labels")
    M, cols = z.shape
    if g is None:
        g = torch.empty((M, cols), dtype=_f32, device=z.device)
    dcol = torch.empty(cols, dtype=_f32, device=z.device)
    loss = torch.empty(1, dtype=_f32, device=z.device)
    ws, base = _aligned_ws(lib().grapes_rowlist_loss_workspace_bytes(M, cols), z.device)
    _lib.check(lib().grapes_rowlist_loss(_p(z), z.stride(0), int(C), _p(rows), M, None if multi else _p(labels),
                                         _p(labels) if multi else None, _p(dinv), float(p), int(seed), int(offset), _p(g),
                                         g.stride(0), cols, _p(dcol), _p(loss), base, _p(status), _stream()), "rowlist_loss")
    del ws
    return loss, g, dcol


# ------------------------------------------------------------------------------- GraphSAINT random walks (graphsaint.py:104)
SAINT_MAX_IDS = 16384     # B (L + 1) of one batch: its node set is sorted in one workgroup's LDS


def saint_walk_nodes(rowptr, col, num_nodes: int, batch_size: int, walk_length: int, roots=None, uniforms=None,
                     philox_seed: int = 0, philox_offset: int = 0, d_philox_offset=None, node_map=None, status=None, out=None):
    """(walks int32 [B, L + 1], node_idx int32 [B (L + 1)], count int32 [1]) of grapes_saint_walk_nodes: B random walks of L steps
    and their ascending duplicate-free node set (the first *count entries of node_idx); node_map[node_idx[i]] = i.  roots int32 [B]
    / uniforms fp32 [B L] replace the Philox draws.  out: the three tensors to write (captured steps)."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(roots, _i32, "roots", True); _chk(uniforms, _f32, "uniforms", True)
    _chk(d_philox_offset, _i64, "d_philox_offset", True); _chk(node_map, _i32, "node_map"); _chk(status, _i32, "status", True)
    B, L = int(batch_size), int(walk_length)
    if B <= 0 or L < 0 or B * (L + 1) > SAINT_MAX_IDS:
        raise ValueError(f"saint_walk_nodes: batch_size * (walk_length + 1) must be in 1 .. {SAINT_MAX_IDS}")
    if roots is not None and roots.numel() < B:
        raise ValueError("roots shorter than batch_size")
    if uniforms is not None and uniforms.numel() < B * L:
        raise ValueError("uniforms shorter than batch_size * walk_length")
    dev = rowptr.device
    if roots is not None and status is None:
        status = torch.zeros(1, dtype=_i32, device=dev)
    if out is None:
        out = (torch.empty((B, L + 1), dtype=_i32, device=dev), torch.empty(B * (L + 1), dtype=_i32, device=dev),
               torch.empty(1, dtype=_i32, device=dev))
    walks, node_idx, count = out
    _lib.check(lib().grapes_saint_walk_nodes(_p(rowptr), _p(col), int(num_nodes), B, L, _p(roots), _p(uniforms),
                                             int(philox_seed) & (2 ** 64 - 1), int(philox_offset), _p(d_philox_offset), _p(walks),
                                             _p(node_idx), _p(count), _p(node_map), _p(status), _stream()), "saint_walk_nodes")
    return walks, node_idx, count


def saint_edge_weights(rowptr, col, num_nodes: int, status=None):
    """(colcount int32 [N], blockw int64 [(nnz >> 6) + N], roww int64 [N + 1]) of grapes_saint_edge_weights: the one-time weight
    table of GraphSAINTEdgeSampler.  Entry (r, c) weighs colcount[r] + rowcount[c]; row r's 64-entry blocks keep their inclusive
    weight prefix in blockw from slot (rowptr[r] >> 6) + r on (slots no row owns stay 0); roww is the exclusive prefix over rows,
    roww[N] the total weight.  No host read."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(status, _i32, "status", True)
    N, nnz, dev = int(num_nodes), col.numel(), rowptr.device
    if nnz >= 2 ** 31:
        raise ValueError("saint_edge_weights: the edge sampler's weights are 32-bit: fewer than 2^31 stored entries")
    colcount = torch.empty(N, dtype=_i32, device=dev)
    blockw = torch.zeros((nnz >> 6) + N, dtype=_i64, device=dev)
    roww = torch.empty(N + 1, dtype=_i64, device=dev)
    _lib.check(lib().grapes_saint_edge_weights(_p(rowptr), _p(col), N, nnz, _p(colcount), _p(blockw), _p(roww), _p(status),
                                               _stream()), "saint_edge_weights")
    return colcount, blockw, roww


def saint_draw_nodes(rowptr, col, num_nodes: int, batch_size: int, weights=None, draws=None, philox_seed: int = 0,
                     philox_offset: int = 0, d_philox_offset=None, node_map=None, status=None, out=None):
    """(ids int32 [B or 2 B], node_idx int32 [the same size], count int32 [1], entries int64 [B]) of grapes_saint_draw_nodes: B
    draws of a stored entry — uniform (weights None: the node sampler; ids = the entries' rows) or by the table of
    saint_edge_weights (the edge sampler; ids = row and column of every entry) — and the ascending duplicate-free set of the ids
    as saint_walk_nodes returns it.  draws int64 [B] replace the Philox draws (values t in [0, total)).  out: the four tensors
    to write (captured steps)."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(draws, _i64, "draws", True)
    _chk(d_philox_offset, _i64, "d_philox_offset", True); _chk(node_map, _i32, "node_map"); _chk(status, _i32, "status", True)
    B = int(batch_size)
    M = B if weights is None else 2 * B
    if B <= 0 or M > SAINT_MAX_IDS:
        raise ValueError(f"saint_draw_nodes: {'2 * ' if weights is not None else ''}batch_size must be in 1 .. {SAINT_MAX_IDS}")
    if draws is not None and draws.numel() < B:
        raise ValueError("draws shorter than batch_size")
    colcount, blockw, roww = weights if weights is not None else (None, None, None)
    _chk(colcount, _i32, "colcount", True); _chk(blockw, _i64, "blockw", True); _chk(roww, _i64, "roww", True)
    dev = rowptr.device
    if draws is not None and status is None:
        status = torch.zeros(1, dtype=_i32, device=dev)
    if out is None:
        out = (torch.empty(M, dtype=_i32, device=dev), torch.empty(M, dtype=_i32, device=dev), torch.empty(1, dtype=_i32, device=dev),
               torch.empty(B, dtype=_i64, device=dev))
    ids, node_idx, count, entries = out
    _lib.check(lib().grapes_saint_draw_nodes(_p(rowptr), _p(col), int(num_nodes), B, _p(colcount), _p(blockw), _p(roww), _p(draws),
                                             int(philox_seed) & (2 ** 64 - 1), int(philox_offset), _p(d_philox_offset), _p(ids),
                                             _p(entries), _p(node_idx), _p(count), _p(node_map), _p(status), _stream()),
               "saint_draw_nodes")
    return ids, node_idx, count, entries


def saint_subgraph(rowptr, col, node_idx, count, node_map, e_cap: int, edge_norm=None, ids=False, status=None, out=None):
    """(edge_src, edge_dst int32 [e_cap], e_count int32 [1], rowptr_l int32 [n_cap + 1]) of grapes_saint_subgraph: the subgraph
    induced by the first *count ids of node_idx, relabelled to local ids, in CSR order.  Overflow of e_cap sets a status bit.
    ids=True or a table edge_norm (fp32 [nnz]) also tells which stored entry every edge is — two more results: edge_id int64
    [e_cap], the position in col of edge p, and edge_norm_b fp32 [e_cap] = edge_norm[edge_id[p]] (None without a table).
    out: the four (or six) tensors to write."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(node_idx, _i32, "node_idx"); _chk(count, _i32, "count")
    _chk(node_map, _i32, "node_map"); _chk(status, _i32, "status", True); _chk(edge_norm, _f32, "edge_norm", True)
    if edge_norm is not None and edge_norm.numel() < col.numel():
        raise ValueError("saint_subgraph: edge_norm holds one value per stored entry")
    ids = ids or edge_norm is not None
    n_cap, dev, ec = node_idx.numel(), node_idx.device, max(int(e_cap), 1)
    if out is None:
        out = (torch.empty(ec, dtype=_i32, device=dev), torch.empty(ec, dtype=_i32, device=dev),
               torch.empty(1, dtype=_i32, device=dev), torch.empty(n_cap + 1, dtype=_i32, device=dev))
        if ids:
            out += (torch.empty(ec, dtype=_i64, device=dev), torch.empty(ec, dtype=_f32, device=dev) if edge_norm is not None else None)
    src, dst, d_e, rowptr_l, edge_id, edge_norm_b = out if ids else (*out, None, None)
    if ids:
        _chk(edge_id, _i64, "edge_id"); _chk(edge_norm_b, _f32, "edge_norm_b", edge_norm is None)
        if min(src.numel(), dst.numel(), edge_id.numel()) < int(e_cap) or (edge_norm_b is not None and edge_norm_b.numel() < int(e_cap)):
            raise ValueError("saint_subgraph: the edge buffers hold e_cap values each")
        if edge_norm is None:
            edge_norm_b = None
    ws = _ws(lib().grapes_saint_subgraph_workspace_bytes(n_cap), dev)
    _lib.check(lib().grapes_saint_subgraph(_p(rowptr), _p(col), _p(node_idx), _p(count), _p(node_map), n_cap, int(e_cap),
                                           _p(rowptr_l), _p(src), _p(dst), _p(d_e), _p(edge_id), _p(edge_norm), _p(edge_norm_b),
                                           _p(ws), _p(status), _stream()), "saint_subgraph")
    return (src, dst, d_e, rowptr_l, edge_id, edge_norm_b) if ids else (src, dst, d_e, rowptr_l)


def saint_masked_loss(z, C: int, node_idx, count, train_mask, labels, node_norm=None, g=None, loss=None, d_train=None, status=None):
    """(loss [1], g = d loss / d z [n_cap, C]) of grapes_saint_masked_loss over the batch rows whose node is a training node: mean
    CrossEntropy (labels int64 [N]) or BCEWithLogits (fp32 [N, C]); no training row: loss NaN, g = 0.  With node_norm (fp32 [N],
    read through node_idx) the SUM of node_norm[node] * row loss (CrossEntropy, or the mean over the columns of BCEWithLogits); no
    training row: loss 0, g = 0."""
    _chk(node_idx, _i32, "node_idx"); _chk(count, _i32, "count", True); _chk(d_train, _i32, "d_train", True)
    _chk(status, _i32, "status", True); _chk(node_norm, _f32, "node_norm", True)
    if z.dtype != _f32 or not z.is_cuda or z.dim() != 2 or z.stride(1) != 1:
        raise _lib.GrapesHipError("saint_masked_loss: expected a CUDA fp32 matrix with unit column stride")
    if not train_mask.is_cuda or train_mask.dtype not in (torch.bool, torch.uint8):
        raise _lib.GrapesHipError("saint_masked_loss: train_mask must be a cuda bool / uint8 vector")
    multi = labels.dim() == 2
    _chk(labels, _f32 if multi else _i64, "labels")
    if node_norm is not None and node_norm.numel() != train_mask.numel():
        raise ValueError("saint_masked_loss: node_norm holds one value per node, like train_mask")
    n_cap = z.shape[0]
    if g is None:
        g = torch.empty((n_cap, int(C)), dtype=_f32, device=z.device)
    if loss is None:
        loss = torch.empty(1, dtype=_f32, device=z.device)
    _lib.check(lib().grapes_saint_masked_loss(_p(z), z.stride(0), int(C), _p(node_idx), _p(count), n_cap, _p(train_mask),
                                              _p(node_norm), None if multi else _p(labels), _p(labels) if multi else None, _p(g),
                                              g.stride(0), _p(loss), _p(d_train), _p(status), _stream()), "saint_masked_loss")
    return loss, g


# ------------------------------------------------------------------------------- GraphSAINT normalisation (sample_coverage > 0)
# [PyG-recall: GraphSAINTSampler._compute_norm / __collate__].  node_count / edge_count are int32 tensors that hold the kernels'
# uint32 counts (torch's uint32 supports too few operations); a count reaches 2^31 only after 2^31 batches.
def saint_coverage_count(rowptr, col, num_nodes: int, node_idx, count, node_map, out=None):
    """(node_count int32 [N], edge_count int32 [nnz], total int64 [1]) of grapes_saint_coverage_count: one drawn batch's share of
    the coverage counts — node_count[v] += 1 over the node set, edge_count[j] += 1 over the stored entries with both ends in it,
    total += the set's size.  out: the three tensors to add into (None: fresh zeros).  No host read."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(node_idx, _i32, "node_idx"); _chk(count, _i32, "count")
    _chk(node_map, _i32, "node_map")
    N, dev = int(num_nodes), rowptr.device
    if out is None:
        out = (torch.zeros(N, dtype=_i32, device=dev), torch.zeros(max(col.numel(), 1), dtype=_i32, device=dev),
               torch.zeros(1, dtype=_i64, device=dev))
    node_count, edge_count, total = out
    _chk(node_count, _i32, "node_count"); _chk(edge_count, _i32, "edge_count"); _chk(total, _i64, "total")
    if node_count.numel() < N or edge_count.numel() < col.numel() or rowptr.numel() != N + 1 or node_map.numel() < N:
        raise ValueError("saint_coverage_count: node_count / node_map hold one value per node, edge_count one per stored entry")
    _lib.check(lib().grapes_saint_coverage_count(_p(rowptr), _p(col), N, _p(node_idx), _p(count), _p(node_map), node_idx.numel(),
                                                 _p(node_count), _p(edge_count), _p(total), _stream()), "saint_coverage_count")
    return node_count, edge_count, total


def saint_norms(rowptr, num_nodes: int, node_count, edge_count, num_samples: int, out=None):
    """(edge_norm fp32 [nnz], node_norm fp32 [N]) of grapes_saint_norms from the counts of num_samples batches:
    edge_norm[j] = node_count[row(j)] / edge_count[j] clamped to [0, 1e4] (0 / 0 -> 0.1), node_norm[v] = num_samples /
    node_count[v] / N (a count of 0 taken as 0.1), all in fp32.  out: the two tensors to write."""
    _chk(rowptr, _i64, "rowptr"); _chk(node_count, _i32, "node_count"); _chk(edge_count, _i32, "edge_count")
    N, dev = int(num_nodes), rowptr.device
    if rowptr.numel() != N + 1 or node_count.numel() < N:
        raise ValueError("saint_norms: rowptr holds N + 1 values, node_count one per node")
    if out is None:
        out = (torch.empty(edge_count.numel(), dtype=_f32, device=dev), torch.empty(N, dtype=_f32, device=dev))
    edge_norm, node_norm = out
    _chk(edge_norm, _f32, "edge_norm"); _chk(node_norm, _f32, "node_norm")
    if edge_norm.numel() < edge_count.numel() or node_norm.numel() < N:
        raise ValueError("saint_norms: edge_norm holds one value per stored entry, node_norm one per node")
    _lib.check(lib().grapes_saint_norms(_p(rowptr), N, _p(node_count), _p(edge_count), int(num_samples), _p(edge_norm),
                                        _p(node_norm), _stream()), "saint_norms")
    return edge_norm, node_norm


# ------------------------------------------------------------------------------- what the samplers' layer calls share
def _list_rows(who, rowptr, col, num_nodes, rows, d_m, status, bad=False, says="rowptr holds N + 1 values and rows is not empty"):
    """The checks of every call over a list of rows of the CSR -> (N, m).  bad: the caller's further conditions under the same
    message `says`."""
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(rows, _i32, "rows"); _chk(d_m, _i32, "d_m", True)
    _chk(status, _i32, "status", True)
    N, m = int(num_nodes), rows.numel()
    if rowptr.numel() != N + 1 or m < 1 or bad:
        raise ValueError(f"{who}: {says}")
    return N, m


def _edge_buffers(who, ec, dev, out, pos=None, weight=None, weight_name="edge_weight"):
    """A layer's edge buffers (edge_src, edge_dst[, edge_pos][, the weights], e_count): allocated for e_cap = ec entries, or out's,
    checked.  pos / weight: None — the call has no such buffer; else whether to allocate it (a buffer not wanted is None)."""
    opt = [(want, dt, name) for want, dt, name in ((pos, _i64, "edge_pos"), (weight, _f32, weight_name)) if want is not None]
    if out is None:
        out = (torch.empty(ec, dtype=_i32, device=dev), torch.empty(ec, dtype=_i32, device=dev),
               *(torch.empty(ec, dtype=dt, device=dev) if want else None for want, dt, _ in opt),
               torch.empty(1, dtype=_i32, device=dev))
    src, dst, *rest, d_e = out
    _chk(src, _i32, "edge_src"); _chk(dst, _i32, "edge_dst")
    for t, (_, dt, name) in zip(rest, opt):
        _chk(t, dt, name, True)
    _chk(d_e, _i32, "e_count")
    if any(t is not None and t.numel() < ec for t in (src, dst, *rest)):
        raise ValueError(f"{who}: the edge buffers hold e_cap values each")
    return out


def _key_words(who, keys) -> int:
    """The number of 32-bit words in a caller's key tensor (0 for None), after its type check."""
    if keys is None:
        return 0
    if not keys.is_cuda or keys.dtype not in (_i32, getattr(torch, "uint32", _i32)) or not keys.is_contiguous():
        raise TypeError(f"{who}: keys must be a contiguous cuda tensor of 32-bit words (int32 bit patterns or uint32)")
    return keys.numel()


def _candidate_set(who, rowptr, rowptr_t, col_t, num_nodes, ids, n, d_n, prev_bits, m, d_m, status):
    """The candidate-set arguments of the layer-wise importances -> (N, n, m): n defaults to ids' length or N, m to N — a bitmap comes
    with its m."""
    _chk(rowptr, _i64, "rowptr"); _chk(rowptr_t, _i64, "rowptr_t"); _chk(col_t, _i32, "col_t"); _chk(ids, _i32, "ids", True)
    _chk(d_n, _i32, "d_n", True); _chk(prev_bits, _i64, "prev_bits", True); _chk(d_m, _i32, "d_m", True)
    _chk(status, _i32, "status", True)
    N = int(num_nodes)
    if n is None:
        n = ids.numel() if ids is not None else N
    if m is None:
        if prev_bits is not None:
            raise ValueError(f"{who}: a bitmap comes with m, the number of rows it holds")
        m = N
    n, m = int(n), int(m)
    if rowptr.numel() != N + 1 or rowptr_t.numel() != N + 1 or n < 1 or m < 1 or (ids is not None and ids.numel() < n):
        raise ValueError(f"{who}: rowptr / rowptr_t hold N + 1 values, ids at least n >= 1 ids, and m >= 1")
    return N, n, m


# ------------------------------------------------------------------------------- LADIES / FastGCN layer-wise samplers
# [LADIES-recall: acbull/LADIES pytorch_ladies.py, ladies_sampler / fastgcn_sampler]  V = A + I, P = D^-1 V (grapes_hip.h).
def ladies_importance(rowptr, rowptr_t, col_t, num_nodes: int, ids=None, n=None, d_n=None, prev_bits=None, m=None, d_m=None,
                      pi_table=None, status=None, out=None):
    """(pi fp32 [n], logit fp32 [n]) of grapes_ladies_importance: pi[k] = sum over the rows i of the set of P_ij^2 for j = ids[k]
    (ids None: j = k, n defaults to N), logit = logf(pi) - (20 + logf(float(m))).  The set: the bitmap prev_bits of m rows, or every
    row (prev_bits None: m defaults to N).  rowptr_t / col_t: the CSR of the transpose (the graph's own arrays when symmetric).
    pi_table (fp32 [N]): also pi_table[ids[k]] = pi[k].  out: the two tensors to write; entries past *d_n stay as they are."""
    _chk(pi_table, _f32, "pi_table", True)
    N, n, m = _candidate_set("ladies_importance", rowptr, rowptr_t, col_t, num_nodes, ids, n, d_n, prev_bits, m, d_m, status)
    dev = rowptr.device
    if (prev_bits is not None and prev_bits.numel() < (N + 63) // 64) or (pi_table is not None and pi_table.numel() < N):
        raise ValueError("ladies_importance: prev_bits holds ceil(N / 64) words, pi_table one value per node")
    if out is None:
        out = (torch.empty(n, dtype=_f32, device=dev), torch.empty(n, dtype=_f32, device=dev))
    pi, logit = out
    _chk(pi, _f32, "pi"); _chk(logit, _f32, "logit")
    if pi.numel() < n or logit.numel() < n:
        raise ValueError("ladies_importance: pi and logit hold n values each")
    _lib.check(lib().grapes_ladies_importance(_p(rowptr), _p(rowptr_t), _p(col_t), N, _p(ids), n, _p(d_n), _p(prev_bits), m, _p(d_m),
                                              _p(pi), _p(logit), _p(pi_table), _p(status), _stream()), "ladies_importance")
    return pi, logit


def ladies_layer(rowptr, col, num_nodes: int, rows, keep_bits, pi_table, e_cap: int, d_m=None, status=None, out=None):
    """(edge_src, edge_dst int32 [e_cap], weight fp32 [e_cap], e_count int32 [1]) of grapes_ladies_layer: for the rows i = rows[r]
    in order and ascending j, every (i, j) of V = A + I with j in the bitmap keep_bits — source j, target i, global ids — with
    weight (v_ij / pi_table[j]) / the row's sum of them.  More than e_cap entries set the overflow status bit.
    out: the four tensors to write."""
    _chk(keep_bits, _i64, "keep_bits"); _chk(pi_table, _f32, "pi_table")
    dev, ec = rows.device, int(e_cap)
    N, m = _list_rows("ladies_layer", rowptr, col, num_nodes, rows, d_m, status,
                      keep_bits.numel() < (int(num_nodes) + 63) // 64 or pi_table.numel() < int(num_nodes) or ec < 1,
                      "rowptr holds N + 1 values, keep_bits ceil(N / 64) words, pi_table N values; rows and e_cap are not empty")
    src, dst, w, d_e = _edge_buffers("ladies_layer", ec, dev, out, weight=True, weight_name="weight")
    _chk(w, _f32, "weight")
    ws = _ws(lib().grapes_ladies_layer_workspace_bytes(m), dev)
    _lib.check(lib().grapes_ladies_layer(_p(rowptr), _p(col), N, _p(rows), m, _p(d_m), _p(keep_bits), _p(pi_table), ec, _p(src),
                                         _p(dst), _p(w), _p(d_e), _p(ws), _p(status), _stream()), "ladies_layer")
    return src, dst, w, d_e


# ------------------------------------------------------------------------------- AS-GCN adaptive layer-wise sampler
# [AS-GCN-recall: Huang et al., NeurIPS 2018, the layer-wise sampler with g(x(u_j))] on the LADIES conventions (grapes_hip.h).
def asgcn_importance(rowptr, rowptr_t, col_t, num_nodes: int, x, w_g, b_g, ids=None, n=None, d_n=None, prev_bits=None, m=None,
                     d_m=None, q_table=None, a_table=None, status=None, out=None):
    """(c, a, q, logq, logit), fp32 [n] each, of grapes_asgcn_importance for j = ids[k] (ids None: j = k, n defaults to N):
    c = sum over the rows i of the set of P_ij, a = <x[j], w_g> + b_g, q = c (max(a, 0) + 1), logq = logf(q),
    logit = (logq - max logq) - 20.  x fp32 [N, F] (rows may be strided), w_g fp32 [F], b_g fp32 [1].  The set: the bitmap prev_bits
    of m rows, or every row (prev_bits None).  q_table / a_table (fp32 [N]): also written at the candidates.  out: the five tensors
    to write; entries past *d_n stay as they are."""
    _chk(q_table, _f32, "q_table", True); _chk(a_table, _f32, "a_table", True); _chk(w_g, _f32, "w_g"); _chk(b_g, _f32, "b_g")
    if x.dim() != 2:
        raise ValueError("asgcn_importance: x is a matrix of one feature row per node")
    F = int(x.shape[1])
    ldx = _row_strided(x, F, "asgcn_importance: x")
    N, n, m = _candidate_set("asgcn_importance", rowptr, rowptr_t, col_t, num_nodes, ids, n, d_n, prev_bits, m, d_m, status)
    dev = rowptr.device
    if x.shape[0] < N or F < 1 or w_g.numel() != F or b_g.numel() != 1:
        raise ValueError("asgcn_importance: x holds one row of F >= 1 features per node, w_g F values, b_g one")
    if (prev_bits is not None and prev_bits.numel() < (N + 63) // 64) or any(t is not None and t.numel() < N for t in (q_table, a_table)):
        raise ValueError("asgcn_importance: prev_bits holds ceil(N / 64) words, q_table and a_table one value per node")
    if out is None:
        out = tuple(torch.empty(n, dtype=_f32, device=dev) for _ in range(5))
    for t, name in zip(out, ("c", "a", "q", "logq", "logit")):
        _chk(t, _f32, name)
        if t.numel() < n:
            raise ValueError("asgcn_importance: c, a, q, logq and logit hold n values each")
    c, a, q, logq, logit = out
    _lib.check(lib().grapes_asgcn_importance(_p(rowptr), _p(rowptr_t), _p(col_t), N, _p(ids), n, _p(d_n), _p(prev_bits), m, _p(d_m),
                                             _p(x), ldx, F, _p(w_g), _p(b_g), _p(c), _p(a), _p(q), _p(logq), _p(logit), _p(q_table),
                                             _p(a_table), _p(status), _stream()), "asgcn_importance")
    return c, a, q, logq, logit


def _asgcn_entries(who, edge_src, edge_dst, weight, rows, n_local):
    """The checks the two calls over a layer's entry list share -> (e, m, workspace)."""
    _chk(edge_src, _i32, "edge_src"); _chk(edge_dst, _i32, "edge_dst"); _chk(weight, _f32, "weight"); _chk(rows, _i32, "rows")
    e, m = edge_src.numel(), rows.numel()
    if e < 1 or m < 1 or int(n_local) < 1 or edge_dst.numel() != e or weight.numel() != e:
        raise ValueError(f"{who}: edge_src, edge_dst and weight hold the same e >= 1 entries, rows m >= 1 ids below n_local >= 1")
    return e, m, _ws(lib().grapes_asgcn_rows_workspace_bytes(m, int(n_local)), edge_src.device)


def asgcn_variance(edge_src, edge_dst, weight, rows, h, status=None):
    """(V fp32 [m], L_var fp32 [1], dw fp32 [e]) of grapes_asgcn_variance over one layer's entry list in ladies_layer's order with
    LOCAL ids (row-contiguous, rows in `rows` order): with mu_i = sum_j w_ij h[j] and s_i the row's entries,
    V_i = s_i sum_j w_ij^2 |h_j|^2 - |mu_i|^2, L_var = mean V, dw = d L_var / d w = (2 / m)(s_i w_ij |h_j|^2 - <mu_i, h_j>).
    h fp32 [n_local, C] is a constant of the term."""
    _chk(h, _f32, "h"); _chk(status, _i32, "status", True)
    n_local, C = h.shape
    _gather_width(C, "weighted GCN aggregation")
    e, m, ws = _asgcn_entries("asgcn_variance", edge_src, edge_dst, weight, rows, n_local)
    dev = h.device
    V, lvar, dw = torch.empty(m, dtype=_f32, device=dev), torch.empty(1, dtype=_f32, device=dev), torch.empty(e, dtype=_f32, device=dev)
    _lib.check(lib().grapes_asgcn_variance(_p(edge_src), _p(edge_dst), _p(weight), e, _p(rows), m, _p(h), n_local, C, _p(V), _p(lvar),
                                           _p(dw), _p(ws), _p(status), _stream()), "asgcn_variance")
    return V, lvar, dw


def asgcn_logq_bwd(edge_src, edge_dst, weight, grad_weight, rows, n_local: int, out=None, status=None):
    """T fp32 [n_local] of grapes_asgcn_logq_bwd: T[j] += sum_i w_ij (G_ij - sum_j' G_ij' w_ij') over one layer's entry list (LOCAL
    ids, ladies_layer's order, a row's sources ascending), G = grad_weight = d L / d w; d L / d logq_j = -T[j].  out: the array
    to accumulate into (None: zeros)."""
    _chk(grad_weight, _f32, "grad_weight"); _chk(status, _i32, "status", True)
    e, m, ws = _asgcn_entries("asgcn_logq_bwd", edge_src, edge_dst, weight, rows, n_local)
    if grad_weight.numel() != e:
        raise ValueError("asgcn_logq_bwd: grad_weight holds one value per entry")
    if out is None:
        out = torch.zeros(int(n_local), dtype=_f32, device=edge_src.device)
    _chk(out, _f32, "out")
    if out.numel() < int(n_local):
        raise ValueError("asgcn_logq_bwd: out holds one value per batch node")
    _lib.check(lib().grapes_asgcn_logq_bwd(_p(edge_src), _p(edge_dst), _p(weight), _p(grad_weight), e, _p(rows), m, int(n_local),
                                           _p(out), _p(ws), _p(status), _stream()), "asgcn_logq_bwd")
    return out


# ------------------------------------------------------------------------------- GraphSAGE: node-wise sampler, SAGEConv aggregation
# [Hamilton et al., NeurIPS 2017; PyG-recall: torch_geometric 2.5.2 SAGEConv, NeighborLoader] (grapes_hip.h, csrc/sage_kernels.hip)
SAGE_MAX_FANOUT = 64
SAGE_AGGRS = ("mean", "sum")


def sage_sample_layer(rowptr, col, num_nodes: int, rows, fanout: int, e_cap: Optional[int] = None, keys=None, philox_seed: int = 0,
                      philox_offset: int = 0, d_philox_offset=None, d_m=None, deg_sum: Optional[int] = None, want_pos: bool = True,
                      status=None, out=None):
    """(edge_src, edge_dst int32 [e_cap], edge_pos int64 [e_cap] or None, e_count int32 [1]) of grapes_sage_sample_layer: for the rows
    i = rows[r] in order keep min(deg_i, fanout) entries of CSR row i, uniformly without replacement — those with the smallest
    (key << 32) | t, key = keys[p] or raw word p of the Philox stream (philox_seed, offset) at the stream position p = (entries of
    the list rows before r) + t — written for r ascending and within a row for t ascending: source = the neighbour, target = the row,
    global ids; edge_pos = the entry's position in col.  1 <= fanout <= 64.  e_cap defaults to rows.numel() * fanout, which cannot
    overflow; more entries than e_cap set the overflow status bit.  keys: int32 (or uint32) bit patterns, one per stream position.
    deg_sum: the rows' entry count when the caller knows it — 2^31 or more is refused here, and keys must hold that many.
    d_philox_offset: int64 [1] device stream offset, used instead of philox_offset and advanced by ceil(deg_sum / 4).
    out: the four tensors to write (edge_pos may be None)."""
    _chk(d_philox_offset, _i64, "d_philox_offset", True)
    dev, k = rows.device, int(fanout)
    if not 1 <= k <= SAGE_MAX_FANOUT:
        raise ValueError(f"sage_sample_layer: fanout = {fanout} is not built (1 <= fanout <= {SAGE_MAX_FANOUT})")
    ec = rows.numel() * k if e_cap is None else int(e_cap)
    N, m = _list_rows("sage_sample_layer", rowptr, col, num_nodes, rows, d_m, status, ec < 1,
                      "rowptr holds N + 1 values; rows and e_cap are not empty")
    if deg_sum is not None and int(deg_sum) >= 2 ** 31:
        raise ValueError("sage_sample_layer: rows with 2^31 or more entries in all are not built")
    n_keys = _key_words("sage_sample_layer", keys)
    if keys is not None and deg_sum is not None and n_keys < int(deg_sum):
        raise ValueError("sage_sample_layer: keys holds one word per entry of the listed rows")
    src, dst, pos, d_e = _edge_buffers("sage_sample_layer", ec, dev, out, pos=bool(want_pos))
    ws = _ws(lib().grapes_sage_sample_layer_workspace_bytes(m), dev)
    _lib.check(lib().grapes_sage_sample_layer(_p(rowptr), _p(col), N, _p(rows), m, _p(d_m), k, _p(keys), n_keys,
                                              int(philox_seed) & (2 ** 64 - 1), int(philox_offset) & (2 ** 64 - 1),
                                              _p(d_philox_offset), ec, _p(src), _p(dst), _p(pos), _p(d_e), _p(ws), _p(status),
                                              _stream()), "sage_sample_layer")
    return src, dst, pos, d_e


def _strided_rows(t, name: str, n: int, f: int, allow_none: bool = False):
    """The leading dimension of a row-major [n, f] matrix that may be a column block of a wider one."""
    if t is None:
        if allow_none:
            return 0
        raise TypeError(f"{name} is required")
    if not t.is_cuda:
        raise _lib.GrapesHipError(f"{name} must live in HBM (cuda tensor); grapes_amd has no CPU path")
    if t.dtype != _f32:
        raise TypeError(f"{name}: expected {_f32}, got {t.dtype}")
    if t.dim() != 2 or tuple(t.shape) != (n, f):
        raise ValueError(f"{name} must be [{n}, {f}], got {tuple(t.shape)}")
    if f > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} must have contiguous rows")
    ld = t.stride(0) if n > 1 else max(f, t.stride(0))
    if ld < f:
        raise ValueError(f"{name}: rows overlap")
    return ld


ROOTSUM_SCALE_NONE, ROOTSUM_SCALE_MEAN, ROOTSUM_SCALE_MEAN_PLUS_ONE = 0, 1, 2          # GRAPES_ROOTSUM_SCALE_*
_ROOTSUM_LAYERS = {"sage": "SAGE aggregation", "cluster": "Cluster-GCN aggregation"}  # who -> the layer's name in a width refusal


def _sage_aggr(aggr: str) -> int:
    if aggr not in SAGE_AGGRS:
        raise NotImplementedError(f"SAGE aggregation {aggr!r} is not built (built: {', '.join(SAGE_AGGRS)})")
    return ROOTSUM_SCALE_MEAN if aggr == "mean" else ROOTSUM_SCALE_NONE


def _rootsum_fwd(who: str, scale: int, self_weight: float, self_term: bool, loops, src, prep: PreparedGraph, add, bias, relu, out,
                 copy_out, long_rows):
    """grapes_rootsum_aggregate_fwd for {who}_aggregate_fwd, who = "sage" or "cluster" (the name a refusal carries):
    out[i] = act(s_i (sum_{j -> i} src[j] + (loops[i] + [self_term] self_weight) src[i]) + add[i] + bias), s_i by `scale`."""
    n, f = src.shape
    _gather_width(f, _ROOTSUM_LAYERS[who])
    if n != prep.n:
        raise ValueError("src must be [n, f] over the prepared graph's nodes")
    _chk(bias, _f32, "bias", True)
    if bias is not None and bias.numel() != f:
        raise ValueError("bias must hold f values")
    if out is None:
        out = torch.empty((n, f), dtype=_f32, device=src.device)
    ld_src, ld_add = _strided_rows(src, "src", n, f), _strided_rows(add, "add", n, f, True)
    ld_out, ld_copy = _strided_rows(out, "out", n, f), _strided_rows(copy_out, "copy_out", n, f, True)
    items, n_items, cap = _long_items(prep, True, True, long_rows)
    ws = _ws(lib().grapes_rootsum_aggregate_workspace_bytes(0, cap, f), src.device) if cap else None
    _lib.check(lib().grapes_rootsum_aggregate_fwd(_p(src), ld_src, _p(add), ld_add, _p(bias), _p(loops), _p(prep.rowptr_t),
                                                  _p(prep.csr_src), float(self_weight), 1 if self_term else 0, scale, 1 if relu else 0,
                                                  _p(out), ld_out, _p(copy_out), ld_copy, n, _p(prep.d_n), f, items, n_items, cap, _p(ws),
                                                  _p(prep.status), _stream()), who + "_aggregate_fwd")
    return out


def _rootsum_bwd(who: str, scale: int, self_weight: float, self_term: bool, loops, dout, prep: PreparedGraph, relu_out, add, want_src,
                 want_add, want_bias, dsrc, dadd, long_rows):
    """(dsrc, dadd, dbias) of grapes_rootsum_aggregate_bwd for {who}_aggregate_bwd."""
    n, f = dout.shape
    _gather_width(f, _ROOTSUM_LAYERS[who])
    if n != prep.n:
        raise ValueError("dout must be [n, f] over the prepared graph's nodes")
    dev = dout.device
    if dsrc is None and want_src:
        dsrc = torch.empty((n, f), dtype=_f32, device=dev)
    if dadd is None and want_add:
        dadd = torch.empty((n, f), dtype=_f32, device=dev)
    dbias = torch.empty(f, dtype=_f32, device=dev) if want_bias else None
    ld_dout, ld_relu = _strided_rows(dout, "dout", n, f), _strided_rows(relu_out, "relu_out", n, f, True)
    ld_add, ld_dsrc = _strided_rows(add, "add", n, f, True), _strided_rows(dsrc, "dsrc", n, f, True)
    ld_dadd = _strided_rows(dadd, "dadd", n, f, True)
    items, n_items, cap = _long_items(prep, False, False, long_rows) if dsrc is not None else (None, None, 0)
    ws = _ws(lib().grapes_rootsum_aggregate_workspace_bytes(n, cap, f), dev)
    _lib.check(lib().grapes_rootsum_aggregate_bwd(_p(dout), ld_dout, _p(relu_out), ld_relu, _p(loops), _p(prep.rowptr_t),
                                                  _p(prep.rowptr_s), _p(prep.csr_dst), float(self_weight), 1 if self_term else 0, scale,
                                                  _p(add), ld_add, _p(dsrc), ld_dsrc, _p(dadd), ld_dadd, _p(dbias), n, _p(prep.d_n), f,
                                                  items, n_items, cap, _p(ws), _p(prep.status), _stream()), who + "_aggregate_bwd")
    return dsrc, dadd, dbias


def sage_aggregate_fwd(src, prep: PreparedGraph, aggr: str = "mean", add=None, bias=None, relu: bool = False, out=None, copy_out=None,
                       long_rows: Optional[bool] = None):
    """out[i] = act(s_i (sum_{j -> i} src[j] + loops[i] src[i]) + add[i] + bias) over prep's by-target CSR and its stored loops,
    s_i = 1 / deg_i (mean; an empty row gives 0) or 1 (sum).  src, add, out and copy_out ([n, f]) may be column blocks of wider
    matrices (rows contiguous); copy_out[i] = src[i].  long_rows: see _long_items (tests force either form)."""
    return _rootsum_fwd("sage", _sage_aggr(aggr), 0.0, False, gcn2_loops(prep), src, prep, add, bias, relu, out, copy_out, long_rows)


def sage_aggregate_bwd(dout, prep: PreparedGraph, aggr: str = "mean", relu_out=None, add=None, want_src: bool = True,
                       want_add: bool = False, want_bias: bool = False, dsrc=None, dadd=None, long_rows: Optional[bool] = None):
    """(dsrc, dadd, dbias) of sage_aggregate_fwd from dout = d out: g = dout gated by relu_out > 0 (the forward's output, when the
    ReLU was fused); dsrc[j] = sum_{i <- j} s_i g_i + loops[j] s_j g_j (+ add[j]) over the by-source CSR; dadd = g; dbias = the
    column sums of g.  dsrc / dadd: tensors (column blocks allowed) to write; want_*: allocate them.  Fixed order, no atomics."""
    return _rootsum_bwd("sage", _sage_aggr(aggr), 0.0, False, gcn2_loops(prep), dout, prep, relu_out, add, want_src, want_add,
                        want_bias, dsrc, dadd, long_rows)


# ------------------------------------------------------------------------------- VR-GCN: control variates on historical activations
# [Chen, Zhu and Song, ICML 2018] (grapes_hip.h, csrc/vrgcn_kernels.hip)
VRGCN_LONG_ROW = 64          # grapes_vrgcn_long_row(): rows with more entries are cut into chunks of this many (1 GRAPES_LONG_ROW)
VRGCN_ITEM_CAP_MAX = 1 << 20


def _vrgcn_ids(t, name: str, n: Optional[int] = None):
    _chk(t, _i32, name)
    if t.dim() != 1 or (n is not None and t.numel() != n):
        raise ValueError(f"{name} must be a flat int32 tensor" + (f" of {n} values" if n is not None else ""))


def vrgcn_item_cap(rowptr, rows_g) -> int:
    """The chunks of the listed rows with more than VRGCN_LONG_ROW entries (one host read)."""
    deg = rowptr[rows_g.long() + 1] - rowptr[rows_g.long()]
    nc = torch.where(deg > VRGCN_LONG_ROW, (deg + (VRGCN_LONG_ROW - 1)) // VRGCN_LONG_ROW, torch.zeros_like(deg))
    return int(nc.sum().item())


def vrgcn_aggregate_fwd(h, node_idx, hbar, dinv, rowptr, col, rows_g, rows_l, prep: PreparedGraph, item_cap: Optional[int] = None,
                        want_coef: bool = True, out=None, status=None):
    """(A [m, f], coef [m] or None) of grapes_vrgcn_aggregate_fwd: for the listed rows u = rows_g[r] (local id rows_l[r])
      A[r] = dinv_u (dinv_u h[loc u] + (d_u / k_u) sum_{kept v} dinv_v (h[loc v] - hbar[v]) + sum_{every entry v of row u} dinv_v hbar[v])
    over the loop-free global CSR (rowptr int64 [N + 1], col int32; d_u = row u's entries, dinv fp32 [N] = (d + 1)^-1/2), the layer's
    input h [n_local, f] on the batch's local rows (node_idx int32 [n_local] = their global ids), its history hbar [N, f] on global
    rows, and the kept entries as prep's by-target CSR over local ids (prep.n = n_local).  coef[r] = (d_u / k_u) dinv_u is what
    vrgcn_aggregate_bwd takes.  item_cap: the chunks of the listed rows longer than VRGCN_LONG_ROW (None: counted here, one host
    read; 0: every row by one group of lanes).  status defaults to prep.status."""
    for t, name in ((h, "h"), (hbar, "hbar"), (dinv, "dinv")):
        _chk(t, _f32, name)
    _chk(rowptr, _i64, "rowptr"); _chk(col, _i32, "col"); _chk(status, _i32, "status", True)
    _vrgcn_ids(node_idx, "node_idx"); _vrgcn_ids(rows_g, "rows_g"); _vrgcn_ids(rows_l, "rows_l", rows_g.numel())
    if h.dim() != 2 or hbar.dim() != 2 or h.shape[1] != hbar.shape[1]:
        raise ValueError("h is [n_local, f] and hbar [N, f]")
    n_local, f = h.shape
    N, m = hbar.shape[0], rows_g.numel()
    _gather_width(f, "VR-GCN aggregation")
    if node_idx.numel() != n_local or prep.n != n_local or n_local < 1:
        raise ValueError("node_idx and the prepared kept entries cover h's n_local rows")
    if rowptr.numel() != N + 1 or dinv.numel() != N or N < 1:
        raise ValueError("rowptr holds N + 1 values and dinv N, N = hbar's rows")
    if col.numel() >= 2 ** 31:
        raise ValueError("VR-GCN aggregation over a graph with 2^31 or more entries is not built")
    if item_cap is None:
        item_cap = vrgcn_item_cap(rowptr, rows_g) if m else 0
    item_cap = int(item_cap)
    if not 0 <= item_cap <= VRGCN_ITEM_CAP_MAX:
        raise ValueError(f"item_cap is 0 .. {VRGCN_ITEM_CAP_MAX}")
    dev = h.device
    if out is None:
        out = torch.empty((m, f), dtype=_f32, device=dev)
    ld_out = _strided_rows(out, "out", m, f)
    coef = torch.empty(max(m, 1), dtype=_f32, device=dev) if want_coef else None
    ws = _ws(lib().grapes_vrgcn_aggregate_workspace_bytes(m, item_cap, f), dev) if item_cap else None
    st = status if status is not None else prep.status
    _lib.check(lib().grapes_vrgcn_aggregate_fwd(_p(h), f, _p(node_idx), n_local, _p(hbar), f, _p(dinv), _p(rowptr), _p(col), N,
                                                _p(rows_g), _p(rows_l), m, _p(prep.rowptr_t), _p(prep.csr_src), _p(out), ld_out,
                                                _p(coef), f, item_cap, _p(ws), _p(st), _stream()), "vrgcn_aggregate_fwd")
    return out, (coef[:m] if coef is not None else None)


def vrgcn_aggregate_bwd(da, coef, pos, node_idx, dinv, prep: PreparedGraph, out=None, status=None):
    """dh [n_local, f] of grapes_vrgcn_aggregate_bwd from da = d A [m, f]:
      dh[loc v] = dinv_v sum_{kept (u, v)} coef[pos[loc u]] da[pos[loc u]] + dinv_v^2 da[pos[loc v]]   (the self term for listed v)
    over prep's by-source CSR; pos int32 [n_local] = a local node's position among the listed rows, or -1.  hbar is a constant and has
    no gradient.  Fixed order, no atomics."""
    _chk(da, _f32, "da"); _chk(coef, _f32, "coef"); _chk(dinv, _f32, "dinv"); _chk(status, _i32, "status", True)
    _vrgcn_ids(node_idx, "node_idx"); _vrgcn_ids(pos, "pos", node_idx.numel())
    if da.dim() != 2 or da.shape[0] < 1 or coef.numel() != da.shape[0]:
        raise ValueError("da is [m, f] with m >= 1 and coef holds m values")
    m, f = da.shape
    n_local = node_idx.numel()
    _gather_width(f, "VR-GCN aggregation")
    if prep.n != n_local or n_local < 1:
        raise ValueError("the prepared kept entries cover node_idx's n_local rows")
    if out is None:
        out = torch.empty((n_local, f), dtype=_f32, device=da.device)
    ld_out = _strided_rows(out, "dh", n_local, f)
    st = status if status is not None else prep.status
    _lib.check(lib().grapes_vrgcn_aggregate_bwd(_p(da), f, _p(coef), _p(pos), _p(node_idx), _p(dinv), dinv.numel(), _p(prep.rowptr_s),
                                                _p(prep.csr_dst), _p(out), ld_out, n_local, m, f, _p(st), _stream()),
               "vrgcn_aggregate_bwd")
    return out


# ------------------------------------------------------------------------------- GNNAutoScale: cluster batches over histories
# [Fey, Lenssen, Weichert and Leskovec, ICML 2021; pyg_autoscale-recall] (grapes_hip.h, csrc/gas_kernels.hip)
GAS_CHUNK = 64               # GRAPES_LONG_ROW: the entries of one work item of the resolve
GAS_ITEM_CAP_MAX = 1 << 24
GAS_BAD_CODE = 2 ** 31 - 1   # the code of an entry the resolve had to drop (a bad column or `where` entry)


def gas_resolve(rowptr, col, num_nodes: int, node_idx, n: int, where, stamp, serial: int, e_cap: int, item_cap: Optional[int] = None,
                status=None, out=None):
    """(rowptr_h int32 [n + 1], code int32 [e_cap], counts int64 [2]) of grapes_gas_resolve, after cluster_batch with the same stamp
    and serial: for the first n rows of node_idx (the batch's rows) the WHOLE global neighbourhood of each, entry by entry in the
    CSR's order, as code = the local row of an in-batch neighbour, -1 - v for an out-of-batch neighbour v.  rowptr_h = the prefix sum
    of the rows' global degrees; rowptr_h[n] is the true total even when it exceeds e_cap (status then carries the edge-overflow bit
    and nothing is written at or past e_cap).  counts = (in-batch entries, out-of-batch entries).  item_cap: the work items (64
    entries of one row) the call has room for — default n + nnz / 64 + 1, which cannot overflow but launches 64 threads per item of
    room: pass the partition's bound, as GasLoader does.  out: the three tensors to write."""
    _chk(rowptr, _i64, "rowptr")
    for t, name in ((col, "col"), (node_idx, "node_idx"), (where, "where"), (stamp, "stamp")):
        _chk(t, _i32, name)
    _chk(status, _i32, "status", True)
    N, n, ec, dev = int(num_nodes), int(n), int(e_cap), node_idx.device
    if rowptr.numel() != N + 1 or N < 1 or tuple(where.shape) != (N, 2) or stamp.dim() != 2 or stamp.shape[1] != 2 or stamp.shape[0] < 1:
        raise ValueError("gas_resolve: rowptr holds N + 1 values, where is [N, 2] and stamp [P, 2]")
    if node_idx.dim() != 1 or not 1 <= n <= node_idx.numel():
        raise ValueError("gas_resolve: node_idx is a flat int32 tensor of at least n >= 1 values")
    if col.numel() >= 2 ** 31:
        raise ValueError("gas_resolve: a graph with 2^31 or more entries is not built")
    if not 1 <= int(serial) <= CLUSTER_MAX_SERIAL:
        raise ValueError(f"gas_resolve: serial is 1 .. {CLUSTER_MAX_SERIAL}")
    ic = min(n + col.numel() // GAS_CHUNK + 1, GAS_ITEM_CAP_MAX) if item_cap is None else int(item_cap)
    if not 1 <= ec <= 2 ** 31 - 1 or not 1 <= ic <= GAS_ITEM_CAP_MAX:
        raise ValueError(f"gas_resolve: e_cap is 1 .. 2^31 - 1, item_cap 1 .. {GAS_ITEM_CAP_MAX}")
    if out is None:
        out = (torch.empty(n + 1, dtype=_i32, device=dev), torch.empty(ec, dtype=_i32, device=dev),
               torch.empty(2, dtype=_i64, device=dev))
    rowptr_h, code, counts = out
    _chk(rowptr_h, _i32, "rowptr_h"); _chk(code, _i32, "code"); _chk(counts, _i64, "counts")
    if rowptr_h.numel() < n + 1 or code.numel() < ec or counts.numel() < 2:
        raise ValueError("gas_resolve: rowptr_h holds n + 1 values, code e_cap and counts 2")
    ws = _ws(lib().grapes_gas_resolve_workspace_bytes(n), dev)
    if col.numel() == 0:
        col = ws                                                     # (a graph without an entry: any address, never read)
    _lib.check(lib().grapes_gas_resolve(_p(rowptr), _p(col), N, _p(node_idx), n, _p(where), _p(stamp), stamp.shape[0], int(serial), ec,
                                        ic, _p(rowptr_h), _p(code), _p(counts), _p(ws), _p(status), _stream()), "gas_resolve")
    return rowptr_h, code, counts


def gas_item_cap(rowptr_h) -> int:
    """The chunks of the batch rows with more than VRGCN_LONG_ROW codes (one host read)."""
    deg = rowptr_h[1:] - rowptr_h[:-1]
    nc = torch.where(deg > VRGCN_LONG_ROW, (deg + (VRGCN_LONG_ROW - 1)) // VRGCN_LONG_ROW, torch.zeros_like(deg))
    return int(nc.sum().item())


def gas_aggregate_fwd(h, hbar, dinv, node_idx, rowptr_h, code, item_cap: Optional[int] = None, out=None, status=None):
    """A [n, f] of grapes_gas_aggregate_fwd: for every batch row i, u = node_idx[i],
      A[i] = dinv_u (dinv_u h[i] + sum_{t in row i of rowptr_h} dinv_{v_t} (code_t >= 0 ? h[code_t] : hbar[-1 - code_t]))
    with h [n, f] the layer's input on the batch's local rows, hbar [N, f] its history on global rows — both read in place — dinv fp32
    [N] = (d + 1)^-1/2 and (rowptr_h, code) as gas_resolve wrote them (code may be the whole e_cap buffer: the offsets say what is
    read).  item_cap: the chunks of the rows longer than VRGCN_LONG_ROW (None: counted here, one host read; 0: every row by one
    group of lanes).  h, hbar and out may be column blocks of wider matrices."""
    _chk(dinv, _f32, "dinv"); _chk(status, _i32, "status", True)
    _vrgcn_ids(node_idx, "node_idx"); _vrgcn_ids(rowptr_h, "rowptr_h"); _vrgcn_ids(code, "code")
    if h.dim() != 2 or hbar.dim() != 2 or h.shape[1] != hbar.shape[1] or h.shape[0] < 1:
        raise ValueError("h is [n, f] with n >= 1 and hbar [N, f]")
    n, f = h.shape
    N = hbar.shape[0]
    _gather_width(f, "GAS aggregation")
    ld_h, ld_hbar = _strided_rows(h, "h", n, f), _strided_rows(hbar, "hbar", N, f)
    if node_idx.numel() < n or rowptr_h.numel() != n + 1 or dinv.numel() != N or N < 1:
        raise ValueError("node_idx holds h's n rows, rowptr_h n + 1 values and dinv N, N = hbar's rows")
    if item_cap is None:
        item_cap = gas_item_cap(rowptr_h)
    item_cap = int(item_cap)
    if not 0 <= item_cap <= VRGCN_ITEM_CAP_MAX:
        raise ValueError(f"item_cap is 0 .. {VRGCN_ITEM_CAP_MAX}")
    dev = h.device
    if out is None:
        out = torch.empty((n, f), dtype=_f32, device=dev)
    ld_out = _strided_rows(out, "out", n, f)
    ws = _ws(lib().grapes_gas_aggregate_workspace_bytes(n, item_cap, f), dev) if item_cap else None
    if code.numel() == 0:
        code = rowptr_h                                              # (no entry: any address, never read)
        e = 0
    else:
        e = code.numel()
    _lib.check(lib().grapes_gas_aggregate_fwd(_p(h), ld_h, _p(hbar), ld_hbar, _p(dinv), N, _p(node_idx), n, _p(rowptr_h), _p(code), e,
                                              _p(out), ld_out, f, item_cap, _p(ws), _p(status), _stream()), "gas_aggregate_fwd")
    return out


def gas_aggregate_bwd(da, node_idx, dinv, prep, out=None, status=None):
    """dh [n, f] of grapes_gas_aggregate_bwd from da = d A [n, f]:
      dh[j] = dinv_{v_j} (dinv_{v_j} da[j] + sum_{i in by-source row j} dinv_{u_i} da[i]),  v_j = node_idx[j]
    over prep's by-source CSR of the batch's induced entries (prep.rowptr_s, prep.csr_dst; prep.n = n).  hbar is a constant and has
    no gradient.  Fixed order, no atomics."""
    _chk(dinv, _f32, "dinv"); _chk(status, _i32, "status", True)
    _vrgcn_ids(node_idx, "node_idx")
    if da.dim() != 2 or da.shape[0] < 1:
        raise ValueError("da is [n, f] with n >= 1")
    n, f = da.shape
    _gather_width(f, "GAS aggregation")
    ld_da = _strided_rows(da, "da", n, f)
    if prep.n != n or node_idx.numel() < n:
        raise ValueError("the prepared induced entries and node_idx cover da's n rows")
    if out is None:
        out = torch.empty((n, f), dtype=_f32, device=da.device)
    ld_out = _strided_rows(out, "dh", n, f)
    st = status if status is not None else prep.status
    _lib.check(lib().grapes_gas_aggregate_bwd(_p(da), ld_da, _p(node_idx), _p(dinv), dinv.numel(), _p(prep.rowptr_s), _p(prep.csr_dst),
                                              _p(out), ld_out, n, f, _p(st), _stream()), "gas_aggregate_bwd")
    return out


# ------------------------------------------------------------------------------- LABOR: the layer-neighbour sampler
# [Balin and Catalyurek, NeurIPS 2023; LABOR-recall: DGL's LaborSampler] (grapes_hip.h, csrc/labor_kernels.hip)
LABOR_CHUNK = 64             # GRAPES_LONG_ROW: the entries of one work item; a longer row is cut over several wavefronts
LABOR_MAX_ITERS = 8
LABOR_ITEM_CAP_MAX = 1 << 24


def labor_item_cap(m: int, deg_sum: int) -> int:
    """An upper bound of the work items of m rows with deg_sum entries in all: sum of ceil(deg / LABOR_CHUNK) <= m + deg_sum // 64,
    and no item is empty."""
    return max(1, min(int(m) + int(deg_sum) // LABOR_CHUNK, int(deg_sum)))


def labor_sample_layer(rowptr, col, num_nodes: int, rows, fanout: int, e_cap: Optional[int] = None, keys=None, philox_seed: int = 0,
                       philox_base: int = 0, c=None, pi=None, d_m=None, deg_sum: Optional[int] = None, item_cap: Optional[int] = None,
                       want_pos: bool = True, want_weight: bool = True, status=None, out=None):
    """(edge_src, edge_dst int32 [e_cap], edge_pos int64 [e_cap] or None, edge_weight fp32 [e_cap] or None, e_count int32 [1]) of
    grapes_labor_sample_layer [LABOR-recall]: for the rows s = rows[r] in order, d_s = deg(s), every stored entry t (a global id) of
    row s is kept with the variate r_t of NODE t — keys[t], or word t & 3 of philox4x32_10(philox_base + (t >> 2), philox_seed) —
    shared by every row that sees t:  d_s <= fanout keeps everything;  c, pi None (LABOR-0): kept iff r_t d_s < fanout << 32 in 64-bit
    integers;  c fp32 [m], pi fp32 [N] (ops.labor_importance): kept iff (r_t >> 8) 2^-24 < fminf(1, c[r] pi[t]).  edge_weight: the
    Hajek weights (1 / p) / (the row's sum of 1 / p over its kept entries).  Entries come for r ascending and within a row in CSR
    order: source = the neighbour, target = the row.  fanout >= 1 (no upper limit: a fanout past every degree is the expansion with
    weights 1 / d_s).  keys: int32 (or uint32) bit patterns, one per NODE.  deg_sum: the rows' entry count when the caller knows it
    (2^31 or more is refused); it sets the defaults e_cap = deg_sum — which cannot overflow — and item_cap
    (ops.labor_item_cap); without it both e_cap and item_cap are required.  More kept entries than e_cap, or more work items than
    item_cap, set the overflow status bit.  out: the five tensors to write (edge_pos and edge_weight may be None)."""
    N, m = _list_rows("labor_sample_layer", rowptr, col, num_nodes, rows, d_m, status, int(num_nodes) < 1)
    _chk(c, _f32, "c", True); _chk(pi, _f32, "pi", True)
    k, dev = int(fanout), rows.device
    if not 1 <= k < 2 ** 31:
        raise ValueError(f"labor_sample_layer: fanout = {fanout} is not built (1 <= fanout < 2^31)")
    if (c is None) != (pi is None) or (c is not None and (c.numel() != m or pi.numel() != N)):
        raise ValueError("labor_sample_layer: c holds one value per listed row and pi one per node; both or neither")
    if deg_sum is None and (e_cap is None or item_cap is None):
        raise ValueError("labor_sample_layer: give deg_sum, the rows' entry count, or both e_cap and item_cap")
    if deg_sum is not None and int(deg_sum) >= 2 ** 31:
        raise ValueError("labor_sample_layer: rows with 2^31 or more entries in all are not built")
    ec = max(int(deg_sum), 1) if e_cap is None else int(e_cap)
    ic = labor_item_cap(m, deg_sum) if item_cap is None else int(item_cap)
    if ec < 1 or not 1 <= ic <= LABOR_ITEM_CAP_MAX:
        raise ValueError(f"labor_sample_layer: e_cap is at least 1 and item_cap is 1 .. {LABOR_ITEM_CAP_MAX}")
    if keys is not None and _key_words("labor_sample_layer", keys) != N:
        raise ValueError("labor_sample_layer: keys holds one word per node")
    src, dst, pos, w, d_e = _edge_buffers("labor_sample_layer", ec, dev, out, pos=bool(want_pos), weight=bool(want_weight))
    ws = _ws(lib().grapes_labor_sample_layer_workspace_bytes(m, ic), dev)
    _lib.check(lib().grapes_labor_sample_layer(_p(rowptr), _p(col), N, _p(rows), m, _p(d_m), k, _p(keys),
                                               int(philox_seed) & (2 ** 64 - 1), int(philox_base) & (2 ** 64 - 1), _p(c), _p(pi), ic, ec,
                                               _p(src), _p(dst), _p(pos), _p(w), _p(d_e), _p(ws), _p(status), _stream()),
               "labor_sample_layer")
    return src, dst, pos, w, d_e


def labor_scratch(num_nodes: int, device) -> torch.Tensor:
    """The N-sized table of grapes_labor_importance: zero at rest, left zero by every call."""
    return torch.zeros(lib().grapes_labor_importance_workspace_bytes(int(num_nodes)) // 4, dtype=_i32, device=device)


def labor_importance(rowptr, col, num_nodes: int, rows, fanout: int, iters: int, scratch, pi=None, d_m=None, status=None):
    """(c fp32 [m], pi fp32 [N]) of grapes_labor_importance [LABOR-recall]: `iters` (0 .. 8) iterations pi_t <- pi_t max_s c_s(pi) from
    pi = 1, over the listed rows with more than `fanout` entries, then c_s(pi) once more; c_s solves sum_t 1 / min(1, c pi_t) =
    d_s^2 / fanout (0 is written for a row with d_s <= fanout, whose p is 1).  pi: the table to write (only the columns the rows touch
    are written, and only they mean anything).  scratch: ops.labor_scratch(N, device) — zero on entry, zero again on return."""
    N, m = _list_rows("labor_importance", rowptr, col, num_nodes, rows, d_m, status, int(num_nodes) < 1)
    _chk(scratch, _i32, "scratch"); _chk(pi, _f32, "pi", True)
    k, it = int(fanout), int(iters)
    if not 1 <= k < 2 ** 31 or not 0 <= it <= LABOR_MAX_ITERS:
        raise ValueError(f"labor_importance: fanout >= 1 and 0 <= iters <= {LABOR_MAX_ITERS}, not {fanout} and {iters}")
    if scratch.numel() * 4 < lib().grapes_labor_importance_workspace_bytes(N) or (pi is not None and pi.numel() != N):
        raise ValueError("labor_importance: scratch is ops.labor_scratch(num_nodes, device) and pi holds one value per node")
    dev = rows.device
    if pi is None:
        pi = torch.empty(N, dtype=_f32, device=dev)
    c = torch.empty(m, dtype=_f32, device=dev)
    _lib.check(lib().grapes_labor_importance(_p(rowptr), _p(col), N, _p(rows), m, _p(d_m), k, it, _p(c), _p(pi), _p(scratch),
                                             _p(status), _stream()), "labor_importance")
    return c, pi


# ------------------------------------------------------------------------------- ShaDow-GNN: the per-root ego-net sampler
# [Zeng et al., NeurIPS 2021; PyG-recall: ShaDowKHopSampler] (grapes_hip.h, csrc/shadow_kernels.hip)
SHADOW_MAX_NODES = 1024      # the ego-net cap: 1 + k + ... + k^depth nodes of one root sit in one workgroup's LDS
SHADOW_MAX_ROOTS = 4096
SHADOW_MAX_FANOUT = 64
SEGMENT_MEAN_MAX_WIDTH = 1024


def shadow_cap(depth: int, fanout: int) -> int:
    """C = 1 + k + k^2 + ... + k^depth, the most nodes one ego-net can hold.  ValueError unless depth >= 1, 1 <= k <=
    SHADOW_MAX_FANOUT (-1, every neighbour, is refused: the ego-net would be unbounded) and C <= SHADOW_MAX_NODES."""
    depth, k = int(depth), int(fanout)
    if depth < 1:
        raise ValueError(f"shadow_sample: depth = {depth} is not built (depth >= 1)")
    if not 1 <= k <= SHADOW_MAX_FANOUT:
        raise ValueError(f"shadow_sample: num_neighbors = {k} is not built (1 .. {SHADOW_MAX_FANOUT}; -1, every neighbour, would leave "
                         "the ego-net unbounded)")
    C = 1
    for h in range(1, depth + 1):
        C += k ** h
        if C > SHADOW_MAX_NODES:
            raise ValueError(f"shadow_sample: depth {depth} with num_neighbors {k} exceeds the ego-net cap: 1 + k + ... + k^depth "
                             f"must be at most {SHADOW_MAX_NODES}")
    return C


def shadow_sample(rowptr, col, num_nodes: int, roots, depth: int, fanout: int, n_cap: Optional[int] = None, e_cap: Optional[int] = None,
                  words=None, philox_seed: int = 0, philox_offset: int = 0, d_philox_offset=None, d_m=None, want_e_id: bool = True,
                  status=None, out=None):
    """(n_id int32 [n_cap], ptr int32 [B + 1], batch int32 [n_cap], root_n_id int32 [B], edge_index int32 [2, e_cap], e_id int64 [e_cap] or
    None, n_count int32 [1], e_count int32 [1]) of grapes_shadow_sample: one sampled ego-net per root — depth hops, at most fanout
    entries per expanded row chosen by Floyd's algorithm on Philox words, then the subgraph induced on the reached set — concatenated
    in root order; the rule is in grapes_hip.h.  edge_index[0] holds the sources (the neighbours), edge_index[1] the targets (the
    rows), batch-local ids.  n_cap defaults to B * C, which cannot overflow; e_cap is required (an ego-net's induced entries are not
    bounded by its nodes where the graph stores duplicates).  words: int32 (or uint32) bit patterns [B, depth, fanout] replacing the
    Philox words (tests).  d_philox_offset: int64 [1] device stream offset, used instead of philox_offset and advanced by B * depth.
    out: the eight tensors to write (e_id may be None)."""
    _chk(d_philox_offset, _i64, "d_philox_offset", True)
    C = shadow_cap(depth, fanout)
    N, B = _list_rows("shadow_sample", rowptr, col, num_nodes, roots, d_m, status, int(num_nodes) < 1 or e_cap is None,
                      "rowptr holds N + 1 values, roots is not empty and e_cap is given")
    if B > SHADOW_MAX_ROOTS:
        raise ValueError(f"shadow_sample: at most {SHADOW_MAX_ROOTS} roots per call")
    if col.numel() >= 2 ** 31:
        raise ValueError("shadow_sample: a graph with 2^31 or more entries is not built")
    nc, ec, dev = B * C if n_cap is None else int(n_cap), int(e_cap), roots.device
    if nc < 1 or ec < 1:
        raise ValueError("shadow_sample: n_cap and e_cap are at least 1")
    if words is not None and _key_words("shadow_sample", words) != B * int(depth) * int(fanout):
        raise ValueError("shadow_sample: words holds one word per (root, hop, step): [B, depth, fanout]")
    if out is None:
        out = (torch.empty(nc, dtype=_i32, device=dev), torch.empty(B + 1, dtype=_i32, device=dev), torch.empty(nc, dtype=_i32, device=dev),
               torch.empty(B, dtype=_i32, device=dev), torch.empty((2, ec), dtype=_i32, device=dev),
               torch.empty(ec, dtype=_i64, device=dev) if want_e_id else None, torch.empty(1, dtype=_i32, device=dev),
               torch.empty(1, dtype=_i32, device=dev))
    n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e = out
    for t, name in ((n_id, "n_id"), (ptr, "ptr"), (batch, "batch"), (root_n_id, "root_n_id"), (ei, "edge_index"), (d_n, "n_count"),
                    (d_e, "e_count")):
        _chk(t, _i32, name)
    _chk(e_id, _i64, "e_id", True)
    if (n_id.numel() < nc or batch.numel() < nc or ptr.numel() < B + 1 or root_n_id.numel() < B or ei.dim() != 2 or ei.shape[0] != 2 or
            ei.shape[1] < ec or (e_id is not None and e_id.numel() < ec)):
        raise ValueError("shadow_sample: n_id and batch hold n_cap values, ptr B + 1, root_n_id B, edge_index [2, e_cap], e_id e_cap")
    ws = _ws(lib().grapes_shadow_sample_workspace_bytes(B, int(depth), int(fanout)), dev)
    if col.numel() == 0:
        col = ws                                                     # (a graph without an entry: any address, never read)
    _lib.check(lib().grapes_shadow_sample(_p(rowptr), _p(col), N, _p(roots), B, _p(d_m), int(depth), int(fanout), _p(words),
                                          int(philox_seed) & (2 ** 64 - 1), int(philox_offset) & (2 ** 64 - 1), _p(d_philox_offset),
                                          nc, ec, _p(n_id), _p(ptr), _p(batch), _p(root_n_id), ei[0].data_ptr(), ei[1].data_ptr(),
                                          _p(e_id), _p(d_n), _p(d_e), _p(ws), _p(status), _stream()), "shadow_sample")
    return n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e


SHADOW_PPR_TOUCHED = 4096    # T, the touched-set capacity of the PPR push: part of the rule, not a tuning knob
SHADOW_PPR_ONE = 1 << 30     # the unit of mass
SHADOW_PPR_MAX_K = SHADOW_MAX_NODES - 1
SHADOW_PPR_MAX_ROUNDS = 1024


def shadow_ppr_args(k: int, alpha_q: int, thr: int, max_rounds: int) -> int:
    """C = k + 1, the most nodes of one PPR ego-net.  ValueError unless 1 <= k <= SHADOW_PPR_MAX_K, 1 <= alpha_q <= 65535,
    1 <= thr <= 2^30 and 1 <= max_rounds <= SHADOW_PPR_MAX_ROUNDS."""
    k, alpha_q, thr, max_rounds = int(k), int(alpha_q), int(thr), int(max_rounds)
    if not 1 <= k <= SHADOW_PPR_MAX_K:
        raise ValueError(f"shadow_ppr_sample: k = {k} is not built (1 .. {SHADOW_PPR_MAX_K}: the root and k nodes sit in one ego-net)")
    if not 1 <= alpha_q <= 65535:
        raise ValueError(f"shadow_ppr_sample: alpha_q = {alpha_q} is outside 1 .. 65535 (the teleport probability in units of 2^-16)")
    if not 1 <= thr <= SHADOW_PPR_ONE:
        raise ValueError(f"shadow_ppr_sample: thr = {thr} is outside 1 .. 2^30 (the push threshold per entry in units of 2^-30)")
    if not 1 <= max_rounds <= SHADOW_PPR_MAX_ROUNDS:
        raise ValueError(f"shadow_ppr_sample: max_rounds = {max_rounds} is outside 1 .. {SHADOW_PPR_MAX_ROUNDS}")
    return k + 1


def shadow_ppr_sample(rowptr, col, num_nodes: int, roots, k: int, alpha_q: int, thr: int, max_rounds: int, n_cap: Optional[int] = None,
                      e_cap: Optional[int] = None, d_m=None, want_e_id: bool = True, status=None, out=None):
    """(n_id int32 [n_cap], ptr int32 [B + 1], batch int32 [n_cap], root_n_id int32 [B], edge_index int32 [2, e_cap], e_id int64 [e_cap] or
    None, n_count int32 [1], e_count int32 [1], score int32 [n_cap], rounds int32 [B], stop int32 [B]) of grapes_shadow_ppr_sample: one
    PPR ego-net per root — fixed-point forward push from the root (teleport alpha_q / 2^16, threshold thr / 2^30 per stored entry, at
    most max_rounds synchronous rounds over at most SHADOW_PPR_TOUCHED touched nodes), the root and the k best-scoring nodes, the
    induced subgraph — concatenated in root order; the rule is in grapes_hip.h.  The first eight are shadow_sample's, with the ego-net
    cap C = k + 1; score holds each row's fixed-point score in units of 2^-30 (at most 2^30, so int32 holds it), rounds and stop the
    rounds run and the stop code (0 no node left to push, 1 max_rounds, 2 the next round could overflow the touched set) of each
    root.  n_cap defaults to B * C, which cannot overflow; e_cap is required.  No random numbers.  out: the eleven tensors to write
    (e_id may be None)."""
    C = shadow_ppr_args(k, alpha_q, thr, max_rounds)
    N, B = _list_rows("shadow_ppr_sample", rowptr, col, num_nodes, roots, d_m, status, int(num_nodes) < 1 or e_cap is None,
                      "rowptr holds N + 1 values, roots is not empty and e_cap is given")
    if B > SHADOW_MAX_ROOTS:
        raise ValueError(f"shadow_ppr_sample: at most {SHADOW_MAX_ROOTS} roots per call")
    if col.numel() >= 2 ** 31:
        raise ValueError("shadow_ppr_sample: a graph with 2^31 or more entries is not built")
    nc, ec, dev = B * C if n_cap is None else int(n_cap), int(e_cap), roots.device
    if nc < 1 or ec < 1:
        raise ValueError("shadow_ppr_sample: n_cap and e_cap are at least 1")
    if out is None:
        i32 = lambda *shape: torch.empty(shape, dtype=_i32, device=dev)
        out = (i32(nc), i32(B + 1), i32(nc), i32(B), i32(2, ec), torch.empty(ec, dtype=_i64, device=dev) if want_e_id else None, i32(1),
               i32(1), i32(nc), i32(B), i32(B))
    n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e, score, rounds, stop = out
    for t, name in ((n_id, "n_id"), (ptr, "ptr"), (batch, "batch"), (root_n_id, "root_n_id"), (ei, "edge_index"), (d_n, "n_count"),
                    (d_e, "e_count"), (score, "score"), (rounds, "rounds"), (stop, "stop")):
        _chk(t, _i32, name)
    _chk(e_id, _i64, "e_id", True)
    if (n_id.numel() < nc or batch.numel() < nc or score.numel() < nc or ptr.numel() < B + 1 or root_n_id.numel() < B or
            rounds.numel() < B or stop.numel() < B or ei.dim() != 2 or ei.shape[0] != 2 or ei.shape[1] < ec or
            (e_id is not None and e_id.numel() < ec)):
        raise ValueError("shadow_ppr_sample: n_id, batch and score hold n_cap values, ptr B + 1, root_n_id, rounds and stop B, "
                         "edge_index [2, e_cap], e_id e_cap")
    ws = _ws(lib().grapes_shadow_ppr_sample_workspace_bytes(B, int(k)), dev)
    if col.numel() == 0:
        col = ws                                                     # (a graph without an entry: any address, never read)
    _lib.check(lib().grapes_shadow_ppr_sample(_p(rowptr), _p(col), N, _p(roots), B, _p(d_m), int(k), int(alpha_q), int(thr),
                                              int(max_rounds), nc, ec, _p(n_id), _p(ptr), _p(batch), _p(root_n_id), ei[0].data_ptr(),
                                              ei[1].data_ptr(), _p(e_id), _p(score), _p(rounds), _p(stop), _p(d_n), _p(d_e), _p(ws),
                                              _p(status), _stream()), "shadow_ppr_sample")
    return n_id, ptr, batch, root_n_id, ei, e_id, d_n, d_e, score, rounds, stop


def _segments(who, x, ptr, status):
    """The checks of the two segment-mean calls -> (num_segments, n_rows, f)."""
    _chk(x, _f32, who + ": the matrix"); _chk(ptr, _i32, "ptr"); _chk(status, _i32, "status", True)
    if x.dim() != 2 or ptr.dim() != 1 or ptr.numel() < 2 or not 1 <= x.shape[1] <= SEGMENT_MEAN_MAX_WIDTH:
        raise ValueError(f"{who}: a matrix of 1 .. {SEGMENT_MEAN_MAX_WIDTH} columns and ptr with one more entry than there are segments")
    return ptr.numel() - 1, int(x.shape[0]), int(x.shape[1])


def segment_mean_fwd(h, ptr, status=None, out=None):
    """out fp32 [B, f]: out[b] = the mean of the rows h[ptr[b] : ptr[b + 1]] (0 for an empty segment), ptr int32 [B + 1] ascending
    inside [0, h's rows]; f <= 1024.  The rows are added in row order and divided once: a fixed order, no atomics."""
    B, _, f = _segments("segment_mean_fwd", h, ptr, status)
    if out is None:
        out = torch.empty((B, f), dtype=_f32, device=h.device)
    _chk(out, _f32, "out")
    if tuple(out.shape) != (B, f):
        raise ValueError("segment_mean_fwd: out is [B, f]")
    _lib.check(lib().grapes_segment_mean_fwd(_p(h), _p(ptr), B, int(h.shape[0]), f, _p(out), _p(status), _stream()), "segment_mean_fwd")
    return out


def segment_mean_bwd(g, ptr, n_rows: int, status=None, out=None):
    """dh fp32 [n_rows, f] of segment_mean_fwd from g = d out [B, f]: dh[r] = g[b] / n_b for the rows of segment b, 0 for a row of no
    segment."""
    _chk(g, _f32, "g"); _chk(ptr, _i32, "ptr"); _chk(status, _i32, "status", True)
    if g.dim() != 2 or ptr.dim() != 1 or ptr.numel() != g.shape[0] + 1 or not 1 <= g.shape[1] <= SEGMENT_MEAN_MAX_WIDTH or int(n_rows) < 0:
        raise ValueError(f"segment_mean_bwd: g is [B, f] with f in 1 .. {SEGMENT_MEAN_MAX_WIDTH}, ptr holds B + 1 entries")
    B, f = g.shape
    if out is None:
        out = torch.empty((int(n_rows), f), dtype=_f32, device=g.device)
    _chk(out, _f32, "dh")
    if tuple(out.shape) != (int(n_rows), f):
        raise ValueError("segment_mean_bwd: dh is [n_rows, f]")
    _lib.check(lib().grapes_segment_mean_bwd(_p(g), _p(ptr), B, int(n_rows), f, _p(out), _p(status), _stream()), "segment_mean_bwd")
    return out


# ------------------------------------------------------------------------------- PPRGo: top-k PPR slot tables and the weighted gathers
# [Bojchevski et al., KDD 2020 — recalled] (grapes_hip.h, csrc/shadow_kernels.hip for the push, csrc/pprgo_kernels.hip)
PPRGO_MAX_ROOTS = SHADOW_MAX_ROOTS
PPRGO_MAX_SLOTS = SHADOW_PPR_MAX_K + 1       # K = k + 1
PPRGO_ITEM_CAP_MAX = 1 << 22


def pprgo_topk(rowptr, col, num_nodes: int, roots, k: int, alpha_q: int, thr: int, max_rounds: int, d_m=None, status=None, out=None):
    """(nbr int32 [B, K], score int32 [B, K], cnt int32 [B], rounds int32 [B], stop int32 [B]) of grapes_pprgo_topk, K = k + 1: the push
    and the selection of shadow_ppr_sample without the ego-net, in fixed slots — slot 0 the root, then the best nodes by score
    descending, id ascending; slots at or past cnt[b] hold (root, 0).  score is the fixed-point score in units of 2^-30 (at most 2^30,
    so int32 holds the library's uint32).  One launch, no workspace, no random numbers.  out: the five tensors to write."""
    K = shadow_ppr_args(k, alpha_q, thr, max_rounds)
    N, B = _list_rows("pprgo_topk", rowptr, col, num_nodes, roots, d_m, status, int(num_nodes) < 1)
    if B > PPRGO_MAX_ROOTS:
        raise ValueError(f"pprgo_topk: at most {PPRGO_MAX_ROOTS} roots per call")
    if col.numel() >= 2 ** 31:
        raise ValueError("pprgo_topk: a graph with 2^31 or more entries is not built")
    dev = roots.device
    if out is None:
        i32 = lambda *shape: torch.empty(shape, dtype=_i32, device=dev)
        out = (i32(B, K), i32(B, K), i32(B), i32(B), i32(B))
    nbr, score, cnt, rounds, stop = out
    for t, name in ((nbr, "nbr"), (score, "score"), (cnt, "cnt"), (rounds, "rounds"), (stop, "stop")):
        _chk(t, _i32, name)
    if nbr.numel() < B * K or score.numel() < B * K or cnt.numel() < B or rounds.numel() < B or stop.numel() < B:
        raise ValueError("pprgo_topk: nbr and score hold B * (k + 1) values, cnt, rounds and stop B")
    if col.numel() == 0:
        col = _ws(16, dev)                                           # (a graph without an entry: any address, never read)
    _lib.check(lib().grapes_pprgo_topk(_p(rowptr), _p(col), N, _p(roots), B, _p(d_m), int(k), int(alpha_q), int(thr), int(max_rounds),
                                       _p(nbr), _p(score), _p(cnt), _p(rounds), _p(stop), _p(status), _stream()), "pprgo_topk")
    return nbr, score, cnt, rounds, stop


def pprgo_scratch(num_nodes: int, device):
    """(bits int64 [ceil(N / 64)] zeroed, node_map int32 [N]): pprgo_batch's scratch, made once per graph.  bits is zero at rest —
    every call returns it so; node_map may hold anything."""
    N = int(num_nodes)
    return torch.zeros((N + 63) // 64, dtype=_i64, device=device), torch.empty(N, dtype=_i32, device=device)


def _pprgo_slots(who, nbr_like, cnt, names):
    _chk(cnt, _i32, "cnt")
    if nbr_like.dim() != 2 or cnt.numel() != nbr_like.shape[0] or not 1 <= nbr_like.shape[0] <= PPRGO_MAX_ROOTS or \
            not 2 <= nbr_like.shape[1] <= PPRGO_MAX_SLOTS:
        raise ValueError(f"{who}: {names} is [m, K] with 1 <= m <= {PPRGO_MAX_ROOTS}, 2 <= K <= {PPRGO_MAX_SLOTS}, and cnt holds m values")
    return int(nbr_like.shape[0]), int(nbr_like.shape[1])


def pprgo_batch(nbr, cnt, num_nodes: int, scratch, n_cap: Optional[int] = None, e_cap: Optional[int] = None, status=None, out=None):
    """(node_idx int32 [n_cap], loc int32 [m, K], tptr int32 [n_cap + 1], tslot int32 [e_cap], counts int32 [3]) of grapes_pprgo_batch
    over the slot tables nbr / cnt: the ascending union of the live slots' ids, each slot's rank in it (a dead slot repeats slot
    0's), and the by-source inverted index with ascending flat slot indices; counts = (n, E, the longest segment), one host read;
    the rule is in grapes_hip.h.  scratch: ops.pprgo_scratch(N, device), returned as it must be on entry.  n_cap and e_cap default to
    m * K, which cannot overflow.  out: the five tensors to write."""
    _chk(nbr, _i32, "nbr"); _chk(status, _i32, "status", True)
    m, K = _pprgo_slots("pprgo_batch", nbr, cnt, "nbr")
    bits, node_map = scratch
    _chk(bits, _i64, "scratch bits"); _chk(node_map, _i32, "scratch node_map")
    N, dev = int(num_nodes), nbr.device
    if N < 1 or bits.numel() < (N + 63) // 64 or node_map.numel() < N:
        raise ValueError("pprgo_batch: scratch is ops.pprgo_scratch(num_nodes, device)")
    nc, ec = (m * K if n_cap is None else int(n_cap)), (m * K if e_cap is None else int(e_cap))
    if nc < 1 or ec < 1:
        raise ValueError("pprgo_batch: n_cap and e_cap are at least 1")
    if out is None:
        i32 = lambda *shape: torch.empty(shape, dtype=_i32, device=dev)
        out = (i32(nc), i32(m, K), i32(nc + 1), i32(ec), i32(3))
    node_idx, loc, tptr, tslot, counts = out
    for t, name in ((node_idx, "node_idx"), (loc, "loc"), (tptr, "tptr"), (tslot, "tslot"), (counts, "counts")):
        _chk(t, _i32, name)
    if node_idx.numel() < nc or loc.numel() < m * K or tptr.numel() < nc + 1 or tslot.numel() < ec or counts.numel() < 3:
        raise ValueError("pprgo_batch: node_idx holds n_cap values, loc m * K, tptr n_cap + 1, tslot e_cap, counts 3")
    ws = _ws(lib().grapes_pprgo_batch_workspace_bytes(nc, N), dev)
    _lib.check(lib().grapes_pprgo_batch(_p(nbr), _p(cnt), m, K, N, _p(bits), _p(node_map), nc, ec, _p(node_idx), _p(loc), _p(tptr),
                                        _p(tslot), counts.data_ptr(), counts.data_ptr() + 4, counts.data_ptr() + 8, _p(ws), _p(status),
                                        _stream()), "pprgo_batch")
    return node_idx, loc, tptr, tslot, counts


def pprgo_aggregate_fwd(z, w, loc, cnt, status=None, out=None):
    """out fp32 [m, f]: out[b] = sum_{t < cnt[b]} w[b, t] z[loc[b, t]] — PPRGo's readout over z fp32 [n, f], w fp32 [m, K], loc int32
    [m, K].  Slots at or past cnt[b] are never read.  A fixed order of additions, no atomics."""
    _chk(z, _f32, "z"); _chk(w, _f32, "w"); _chk(loc, _i32, "loc"); _chk(status, _i32, "status", True)
    m, K = _pprgo_slots("pprgo_aggregate_fwd", w, cnt, "w")
    if z.dim() != 2 or z.shape[0] < 1 or tuple(loc.shape) != (m, K):
        raise ValueError("pprgo_aggregate_fwd: z is [n, f] with n >= 1 and loc is [m, K] like w")
    n, f = int(z.shape[0]), int(z.shape[1])
    _gather_width(f, "pprgo_aggregate_fwd")
    if out is None:
        out = torch.empty((m, f), dtype=_f32, device=z.device)
    _chk(out, _f32, "out")
    if tuple(out.shape) != (m, f):
        raise ValueError("pprgo_aggregate_fwd: out is [m, f]")
    ws = _ws(lib().grapes_pprgo_aggregate_fwd_workspace_bytes(m, K, f), z.device)
    _lib.check(lib().grapes_pprgo_aggregate_fwd(_p(z), n, _p(w), _p(loc), _p(cnt), m, K, f, _p(out), _p(ws), _p(status), _stream()),
               "pprgo_aggregate_fwd")
    return out


def pprgo_item_cap(e: int, seg_max: Optional[int] = None) -> int:
    """A bound on the chunks behind the first of the segments longer than VRGCN_LONG_ROW among e entries: such a segment of L entries
    has ceil(L / 64) - 1 <= L / 64 of them.  seg_max: the longest segment where the caller knows it (pprgo_batch's third count) —
    0 chunks when none is long, and the backward is then one launch."""
    if seg_max is not None and int(seg_max) <= VRGCN_LONG_ROW:
        return 0
    return min(int(e) // VRGCN_LONG_ROW, PPRGO_ITEM_CAP_MAX)


def pprgo_aggregate_bwd(g, w, tptr, tslot, n: int, e: int, item_cap: Optional[int] = None, status=None, out=None):
    """dz fp32 [n, f] of pprgo_aggregate_fwd from g = d out [m, f]: dz[u] = sum of w[s] g[s // K] over the slots s of
    tslot[tptr[u] : tptr[u + 1]] in ascending s, every row u < n written; n and e = tptr[n] are host values (the batch's one read).
    item_cap: the room for long segments' chunks, default ops.pprgo_item_cap(e), which cannot overflow.  No float atomics."""
    _chk(g, _f32, "g"); _chk(w, _f32, "w"); _chk(tptr, _i32, "tptr"); _chk(tslot, _i32, "tslot"); _chk(status, _i32, "status", True)
    n, e = int(n), int(e)
    if g.dim() != 2 or w.dim() != 2 or w.shape[0] != g.shape[0] or not 1 <= w.shape[0] <= PPRGO_MAX_ROOTS or \
            not 2 <= w.shape[1] <= PPRGO_MAX_SLOTS or n < 1 or e < 0 or tptr.numel() < n + 1 or tslot.numel() < e:
        raise ValueError(f"pprgo_aggregate_bwd: g is [m, f], w [m, K] (m <= {PPRGO_MAX_ROOTS}, 2 <= K <= {PPRGO_MAX_SLOTS}), tptr holds "
                         "n + 1 values and tslot e")
    m, K, f = int(w.shape[0]), int(w.shape[1]), int(g.shape[1])
    _gather_width(f, "pprgo_aggregate_bwd")
    ic = pprgo_item_cap(e) if item_cap is None else int(item_cap)
    if not 0 <= ic <= PPRGO_ITEM_CAP_MAX:
        raise ValueError(f"pprgo_aggregate_bwd: item_cap is 0 .. {PPRGO_ITEM_CAP_MAX}")
    if out is None:
        out = torch.empty((n, f), dtype=_f32, device=g.device)
    _chk(out, _f32, "dz")
    if tuple(out.shape) != (n, f):
        raise ValueError("pprgo_aggregate_bwd: dz is [n, f]")
    ws = _ws(lib().grapes_pprgo_aggregate_bwd_workspace_bytes(n, ic, f), g.device)
    _lib.check(lib().grapes_pprgo_aggregate_bwd(_p(g), m, _p(w), K, _p(tptr), _p(tslot), n, e, f, _p(out), ic, _p(ws), _p(status),
                                                _stream()), "pprgo_aggregate_bwd")
    return out


# ------------------------------------------------------------------------------- LINKX: the adjacency embedding bag
# [Lim et al., NeurIPS 2021; PyG-recall: LINKX, SparseLinear] (grapes_hip.h, csrc/bag_kernels.hip)
BAG_MAX_ROWS = 4096
BAG_ITEM_CAP_MAX = 1 << 22


def _bag_graph(who, rowptr, col, num_nodes, rows, status):
    N, m = _list_rows(who, rowptr, col, num_nodes, rows, None, status, int(num_nodes) < 1)
    if m > BAG_MAX_ROWS:
        raise ValueError(f"{who}: at most {BAG_MAX_ROWS} rows per call")
    if col.numel() >= 2 ** 31:
        raise ValueError(f"{who}: a graph with 2^31 or more entries is not built")
    if col.numel() == 0:
        col = _ws(16, rows.device)                                   # (a graph without an entry: any address, never read)
    return N, m, col


def bag_batch(rowptr, col, num_nodes: int, rows, scratch, u_cap: int, e_cap: int, status=None, out=None):
    """(bptr int32 [m + 1], uniq int32 [u_cap], tptr int32 [u_cap + 1], trow int32 [e_cap], counts int32 [4]) of grapes_bag_batch over
    the rows `rows` of the CSR: the prefix of their stored lengths, the ascending distinct column ids, and per column the batch rows
    that store it, ascending; counts = (n_u, e, the longest segment, the longest row) — the TRUE totals also past a capacity, which
    raises the status bits and leaves the tables incomplete: the caller retries with them (modules.linkx.BagBatcher).  scratch:
    ops.pprgo_scratch(N, device) (or a DeviceGraph's bits and node_map): the bitmap zero on entry and on return.  The rule is in
    grapes_hip.h.  out: the five tensors to write."""
    N, m, col = _bag_graph("bag_batch", rowptr, col, num_nodes, rows, status)
    bits, node_map = scratch
    _chk(bits, _i64, "scratch bits"); _chk(node_map, _i32, "scratch node_map")
    if bits.numel() < (N + 63) // 64 or node_map.numel() < N:
        raise ValueError("bag_batch: scratch is ops.pprgo_scratch(num_nodes, device)")
    uc, ec, dev = int(u_cap), int(e_cap), rows.device
    if uc < 1 or ec < 1:
        raise ValueError("bag_batch: u_cap and e_cap are at least 1")
    if out is None:
        i32 = lambda *shape: torch.empty(shape, dtype=_i32, device=dev)
        out = (i32(m + 1), i32(uc), i32(uc + 1), i32(ec), i32(4))
    bptr, uniq, tptr, trow, counts = out
    for t, name in ((bptr, "bptr"), (uniq, "uniq"), (tptr, "tptr"), (trow, "trow"), (counts, "counts")):
        _chk(t, _i32, name)
    if bptr.numel() < m + 1 or uniq.numel() < uc or tptr.numel() < uc + 1 or trow.numel() < ec or counts.numel() < 4:
        raise ValueError("bag_batch: bptr holds m + 1 values, uniq u_cap, tptr u_cap + 1, trow e_cap, counts 4")
    ws = _ws(lib().grapes_bag_batch_workspace_bytes(m, uc, N), dev)
    _lib.check(lib().grapes_bag_batch(_p(rowptr), _p(col), N, _p(rows), m, _p(bits), _p(node_map), uc, ec, _p(bptr), _p(uniq), _p(tptr),
                                      _p(trow), _p(counts), _p(ws), _p(status), _stream()), "bag_batch")
    return bptr, uniq, tptr, trow, counts


def bag_fwd_item_cap(e: int, row_max: Optional[int] = None) -> int:
    """A bound on the chunks behind the first of the rows longer than VRGCN_LONG_ROW among e entries (such a row of L entries has
    ceil(L / 64) - 1 <= L / 64); 0 where the longest row, if known, is no long row."""
    if row_max is not None and int(row_max) <= VRGCN_LONG_ROW:
        return 0
    return min(int(e) // VRGCN_LONG_ROW, BAG_ITEM_CAP_MAX)


def bag_bwd_item_cap(e: int, seg_max: Optional[int] = None) -> int:
    """A bound on the chunks of the segments longer than VRGCN_LONG_ROW among e entries, the first chunk included (such a segment of
    L >= 65 entries has ceil(L / 64) <= L / 32); 0 where the longest segment, if known, is not long."""
    if seg_max is not None and int(seg_max) <= VRGCN_LONG_ROW:
        return 0
    return min(int(e) // (VRGCN_LONG_ROW // 2), BAG_ITEM_CAP_MAX)


def bag_fwd(rowptr, col, num_nodes: int, rows, weight, bias=None, item_cap: Optional[int] = None, status=None, out=None):
    """out fp32 [m, H]: out[b] = bias + sum of weight[col[t]] over the stored entries of row rows[b], in stored order — LINKX's
    adjacency embedding (grapes_bag_fwd).  weight fp32 [N, H], rows any leading dimension apart; an empty row gives bias.  item_cap:
    the room for the long rows' chunks; the default reads the rows' entry count from the device (one host read) — a caller who
    knows the batch's entries and longest row passes ops.bag_fwd_item_cap of them.  A fixed order of additions, no atomics."""
    N, m, col = _bag_graph("bag_fwd", rowptr, col, num_nodes, rows, status)
    if weight is None or weight.dim() != 2 or weight.shape[0] != N:
        raise ValueError("bag_fwd: weight is [N, H]")
    H = int(weight.shape[1])
    ld_w = _strided_rows(weight, "weight", N, H)
    _gather_width(H, "bag_fwd")
    if bias is not None:
        _chk(bias, _f32, "bias")
        if bias.numel() != H:
            raise ValueError("bag_fwd: bias holds H values")
    if out is None:
        out = torch.empty((m, H), dtype=_f32, device=rows.device)
    ld_out = _strided_rows(out, "out", m, H)
    if item_cap is None:                                             # (one host read: the rows' entries)
        r = rows.long().clamp(0, N - 1)
        item_cap = bag_fwd_item_cap(int((rowptr[r + 1] - rowptr[r]).sum()))
    ic = int(item_cap)
    if not 0 <= ic <= BAG_ITEM_CAP_MAX:
        raise ValueError(f"bag_fwd: item_cap is 0 .. {BAG_ITEM_CAP_MAX}")
    ws = _ws(lib().grapes_bag_fwd_workspace_bytes(m, ic, H), rows.device)
    _lib.check(lib().grapes_bag_fwd(_p(rowptr), _p(col), N, _p(rows), m, _p(weight), ld_w, _p(bias), H, _p(out), ld_out, ic, _p(ws),
                                    _p(status), _stream()), "bag_fwd")
    return out


def _bag_segments(who, g, tptr, trow, n_u, e, item_cap, status):
    _chk(tptr, _i32, "tptr"); _chk(trow, _i32, "trow"); _chk(status, _i32, "status", True)
    n_u, e = int(n_u), int(e)
    if g is None or g.dim() != 2 or not 1 <= g.shape[0] <= BAG_MAX_ROWS or n_u < 1 or e < 0 or tptr.numel() < n_u + 1 or trow.numel() < e:
        raise ValueError(f"{who}: g is [m, H] with 1 <= m <= {BAG_MAX_ROWS}, n_u >= 1, tptr holds n_u + 1 values and trow e")
    m, H = int(g.shape[0]), int(g.shape[1])
    ld_g = _strided_rows(g, "g", m, H)
    _gather_width(H, who)
    ic = bag_bwd_item_cap(e) if item_cap is None else int(item_cap)
    if not 0 <= ic <= BAG_ITEM_CAP_MAX:
        raise ValueError(f"{who}: item_cap is 0 .. {BAG_ITEM_CAP_MAX}")
    return n_u, e, m, H, ld_g, ic


def bag_bwd(g, tptr, trow, n_u: int, e: int, item_cap: Optional[int] = None, status=None, out=None):
    """values fp32 [n_u, H] of the row-sparse gradient of bag_fwd's weight from g = d out [m, H]: values[s] = the sum of g[trow[q]]
    over segment s in segment order; uniq[:n_u] are its indices (grapes_bag_bwd).  item_cap: the room for long segments' chunks,
    default ops.bag_bwd_item_cap(e), which cannot overflow.  No float atomics."""
    n_u, e, m, H, ld_g, ic = _bag_segments("bag_bwd", g, tptr, trow, n_u, e, item_cap, status)
    if out is None:
        out = torch.empty((n_u, H), dtype=_f32, device=g.device)
    ld_o = _strided_rows(out, "values", n_u, H)
    ws = _ws(lib().grapes_bag_bwd_workspace_bytes(n_u, ic, H), g.device)
    _lib.check(lib().grapes_bag_bwd(_p(g), ld_g, m, _p(tptr), _p(trow), n_u, e, H, _p(out), ld_o, ic, _p(ws), _p(status), _stream()),
               "bag_bwd")
    return out


def bag_adam_step_size(lr: float, beta1: float, beta2: float, t: int) -> float:
    """torch.optim.SparseAdam's step size at step t >= 1, in double: lr sqrt(1 - beta2^t) / (1 - beta1^t)."""
    import math
    return float(lr) * math.sqrt(1.0 - float(beta2) ** int(t)) / (1.0 - float(beta1) ** int(t))


def bag_bwd_adam(g, tptr, trow, uniq, n_u: int, e: int, weight, exp_avg, exp_avg_sq, lr: float, beta1: float, beta2: float, eps: float,
                 t: int, item_cap: Optional[int] = None, status=None):
    """The backward of bag_fwd and torch.optim.SparseAdam's update of the touched rows in one pass (grapes_bag_bwd_adam): no gradient
    is written; rows uniq[:n_u] of weight, exp_avg and exp_avg_sq [N, H] are updated in place with the segment sums, every other row
    is neither read nor written (lazy semantics).  t >= 1 is the number of this call, not of a row's touches.  Returns weight."""
    n_u, e, m, H, ld_g, ic = _bag_segments("bag_bwd_adam", g, tptr, trow, n_u, e, item_cap, status)
    _chk(uniq, _i32, "uniq")
    if weight is None or weight.dim() != 2 or weight.shape[1] != H or uniq.numel() < n_u or int(t) < 1:
        raise ValueError("bag_bwd_adam: weight is [N, H] like g's width, uniq holds n_u ids and t is at least 1")
    N = int(weight.shape[0])
    ld_w = _strided_rows(weight, "weight", N, H)
    ld_a, ld_b = _strided_rows(exp_avg, "exp_avg", N, H), _strided_rows(exp_avg_sq, "exp_avg_sq", N, H)
    if ld_a != ld_b:
        raise ValueError("bag_bwd_adam: exp_avg and exp_avg_sq share one leading dimension")
    ws = _ws(lib().grapes_bag_bwd_workspace_bytes(n_u, ic, H), g.device)
    _lib.check(lib().grapes_bag_bwd_adam(_p(g), ld_g, m, _p(tptr), _p(trow), _p(uniq), n_u, e, N, H, _p(weight), ld_w, _p(exp_avg),
                                         _p(exp_avg_sq), ld_a, 1.0 - float(beta1), 1.0 - float(beta2), float(eps),
                                         bag_adam_step_size(lr, beta1, beta2, t), ic, _p(ws), _p(status), _stream()), "bag_bwd_adam")
    return weight


# ------------------------------------------------------------------------------- PinSAGE: random-walk importance neighbourhoods
# [Ying et al., KDD 2018 — recalled; DGL-recall: RandomWalkNeighborSampler / PinSAGESampler] (grapes_hip.h, csrc/pinsage_kernels.hip)
PINSAGE_MAX_VISITS = 1024                    # V = R L, the visit slots of one root
PINSAGE_MAX_NEIGHBORS = PPRGO_MAX_SLOTS - 1  # T: K = T + 1 slots fit pprgo_batch


def pinsage_term_q(p: float) -> int:
    """The termination probability 0 <= p < 1 in units of 2^-32: min(2^32 - 1, round(p 2^32))."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"pinsage_neighbors: the termination probability {p} is outside [0, 1)")
    return min(2 ** 32 - 1, int(round(p * 2 ** 32)))


def pinsage_args(R: int, L: int, T: int) -> int:
    """K = T + 1, the slots of a root.  ValueError unless 1 <= R, 1 <= L, R L <= PINSAGE_MAX_VISITS and 1 <= T <=
    PINSAGE_MAX_NEIGHBORS."""
    R, L, T = int(R), int(L), int(T)
    if R < 1 or L < 1 or R * L > PINSAGE_MAX_VISITS:
        raise ValueError(f"pinsage_neighbors: {R} walks of {L} steps are not built (each at least 1, and R L <= {PINSAGE_MAX_VISITS}: "
                         "a root's visits sit in one workgroup's LDS)")
    if not 1 <= T <= PINSAGE_MAX_NEIGHBORS:
        raise ValueError(f"pinsage_neighbors: T = {T} neighbours are not built (1 .. {PINSAGE_MAX_NEIGHBORS})")
    return T + 1


def pinsage_neighbors(rowptr, col, num_nodes: int, roots, R: int, L: int, term_q: int, T: int, philox_seed: int = 0,
                      philox_offset: int = 0, d_philox_offset=None, d_m=None, status=None, out=None):
    """(nbr int32 [m, K], visits int32 [m, K], cnt int32 [m]) of grapes_pinsage_neighbors, K = T + 1: per root the T nodes that R
    restarting walks of at most L steps visit most often (term_q: ops.pinsage_term_q(p)), with their visit counts, in pprgo_topk's
    slot convention — slot 0 the root, then count descending, id ascending; slots at or past cnt[b] hold (root, 0).  visits is at
    most 1024, so int32 holds the library's uint32.  d_philox_offset: int64 [1] device stream offset, used instead of philox_offset
    and advanced by ceil(L / 2).  One launch (two with the device offset), no workspace.  out: the three tensors to write."""
    _chk(d_philox_offset, _i64, "d_philox_offset", True)
    K = pinsage_args(R, L, T)
    N, m = _list_rows("pinsage_neighbors", rowptr, col, num_nodes, roots, d_m, status, int(num_nodes) < 1)
    if col.numel() >= 2 ** 31 or m * K >= 2 ** 31:
        raise ValueError("pinsage_neighbors: a graph, or slot tables, with 2^31 or more entries are not built")
    if not 0 <= int(term_q) <= 2 ** 32 - 1:
        raise ValueError("pinsage_neighbors: term_q is a uint32 (ops.pinsage_term_q)")
    dev = roots.device
    if out is None:
        out = (torch.empty((m, K), dtype=_i32, device=dev), torch.empty((m, K), dtype=_i32, device=dev),
               torch.empty(m, dtype=_i32, device=dev))
    nbr, visits, cnt = out
    for t, name in ((nbr, "nbr"), (visits, "visits"), (cnt, "cnt")):
        _chk(t, _i32, name)
    if nbr.numel() < m * K or visits.numel() < m * K or cnt.numel() < m:
        raise ValueError("pinsage_neighbors: nbr and visits hold m * (T + 1) values, cnt m")
    if col.numel() == 0:
        col = _ws(16, dev)                                           # (a graph without an entry: any address, never read)
    _lib.check(lib().grapes_pinsage_neighbors(_p(rowptr), _p(col), N, _p(roots), m, _p(d_m), int(R), int(L), int(term_q), int(T),
                                              int(philox_seed) & (2 ** 64 - 1), int(philox_offset) & (2 ** 64 - 1),
                                              _p(d_philox_offset), _p(nbr), _p(visits), _p(cnt), _p(status), _stream()),
               "pinsage_neighbors")
    return nbr, visits, cnt


def _row_matrix(t, name, m=None, f=None):
    """A float32 device matrix with unit column stride (a column block of a wider one is fine) -> its row stride."""
    if t is None or not t.is_cuda:
        raise _lib.GrapesHipError(f"{name} must live in HBM (cuda tensor); grapes_amd has no CPU path")
    if t.dtype != _f32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or (t.shape[1] > 1 and t.stride(1) != 1) or \
            (m is not None and tuple(t.shape) != (m, f)):
        raise ValueError(f"{name}: a float32 matrix [m, f] with unit column stride" + ("" if m is None else f", here [{m}, {f}]"))
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def relu_l2norm_fwd(s, eps: float = 1e-12, out=None):
    """(out fp32 [m, f], nrm fp32 [m]) of grapes_relu_l2norm_fwd: z = max(s, 0), nrm[b] = |z[b]|_2, out = z / max(nrm, eps) — PinSAGE's
    layer epilogue in one launch; f as the row gathers take it."""
    ld_s = _row_matrix(s, "s")
    m, f = int(s.shape[0]), int(s.shape[1])
    _gather_width(f, "relu_l2norm_fwd")
    if not float(eps) > 0.0:
        raise ValueError("relu_l2norm_fwd: eps is positive")
    if out is None:
        out = (torch.empty((m, f), dtype=_f32, device=s.device), torch.empty(m, dtype=_f32, device=s.device))
    o, nrm = out
    ld_o = _row_matrix(o, "out", m, f)
    _chk(nrm, _f32, "nrm")
    if nrm.numel() < m:
        raise ValueError("relu_l2norm_fwd: nrm holds m values")
    _lib.check(lib().grapes_relu_l2norm_fwd(_p(s), ld_s, m, f, float(eps), _p(o), ld_o, _p(nrm), _stream()), "relu_l2norm_fwd")
    return o, nrm


def relu_l2norm_bwd(g, out, nrm, s, eps: float = 1e-12, ds=None):
    """ds fp32 [m, f] of relu_l2norm_fwd from g = d out: ds = [s > 0] (g - out <g, out> [nrm >= eps]) / max(nrm, eps); out and nrm as
    the forward returned them."""
    ld_g = _row_matrix(g, "g")
    m, f = int(g.shape[0]), int(g.shape[1])
    _gather_width(f, "relu_l2norm_bwd")
    ld_o, ld_s = _row_matrix(out, "out", m, f), _row_matrix(s, "s", m, f)
    _chk(nrm, _f32, "nrm")
    if nrm.numel() < m or not float(eps) > 0.0:
        raise ValueError("relu_l2norm_bwd: nrm holds m values and eps is positive")
    if ds is None:
        ds = torch.empty((m, f), dtype=_f32, device=g.device)
    ld_d = _row_matrix(ds, "ds", m, f)
    _lib.check(lib().grapes_relu_l2norm_bwd(_p(g), ld_g, _p(out), ld_o, _p(nrm), _p(s), ld_s, m, f, float(eps), _p(ds), ld_d, _stream()),
               "relu_l2norm_bwd")
    return ds


# ------------------------------------------------------------------------------- Cluster-GCN: cluster-union batches, ClusterGCNConv
# [Chiang et al., KDD 2019; PyG-recall: ClusterData, ClusterLoader, ClusterGCNConv] (grapes_hip.h, csrc/cluster_kernels.hip)
CLUSTER_MAX_BATCH_PARTS = 1 << 20        # clusters of one batch
CLUSTER_CHUNK = 64                       # GRAPES_LONG_ROW: the entries of one work item; a longer row is cut over several wavefronts
CLUSTER_ITEM_CAP_MAX = 1 << 24
CLUSTER_MAX_SERIAL = 2 ** 31 - 1


def cluster_batch(rowptr, col, num_nodes: int, perm, partptr, where, clusters, stamp, serial: int, n_cap: int, e_cap: int,
                  item_cap: Optional[int] = None, want_e_id: bool = True, status=None, out=None):
    """(cptr int32 [q + 1], node_idx int32 [n_cap], rowptr_l int32 [n_cap + 1], edge_index int32 [2, e_cap], e_id int64 [e_cap] or None,
    n_count int32 [1], e_count int32 [1]) of grapes_cluster_batch: the subgraph induced on the union of the chosen clusters, taken in
    the given order; the rule is in grapes_hip.h.  perm int32 [N], partptr int32 [P + 1] and where int32 [N, 2] are the partition
    tables (modules.cluster.ClusterData builds them); stamp int32 [P, 2] is the caller's membership table, zeroed once, and serial
    (1 .. 2^31 - 1) a value no call has passed since.  edge_index[0] holds the neighbours, edge_index[1] the target rows, batch-local
    ids; rowptr_l[i] = the edge count for every slot from n to n_cap.  item_cap: the work items (64 entries of one row) the call has
    room for — default n_cap + nnz / 64, which cannot overflow but launches 64 threads per item of room: pass the partition's bound, as
    ClusterLoader does.  out: the seven tensors to write (e_id may be None)."""
    _chk(rowptr, _i64, "rowptr")
    for t, name in ((col, "col"), (perm, "perm"), (partptr, "partptr"), (where, "where"), (clusters, "clusters"), (stamp, "stamp")):
        _chk(t, _i32, name)
    _chk(status, _i32, "status", True)
    N, P, q, dev = int(num_nodes), partptr.numel() - 1, clusters.numel(), clusters.device
    if (rowptr.numel() != N + 1 or N < 1 or P < 1 or perm.numel() != N or tuple(where.shape) != (N, 2) or tuple(stamp.shape) != (P, 2)):
        raise ValueError("cluster_batch: rowptr holds N + 1 values, perm N, partptr P + 1, where is [N, 2] and stamp [P, 2]")
    if not 1 <= q <= CLUSTER_MAX_BATCH_PARTS:
        raise ValueError(f"cluster_batch: 1 .. {CLUSTER_MAX_BATCH_PARTS} clusters per batch")
    if col.numel() >= 2 ** 31:
        raise ValueError("cluster_batch: a graph with 2^31 or more entries is not built")
    if not 1 <= int(serial) <= CLUSTER_MAX_SERIAL:
        raise ValueError(f"cluster_batch: serial is 1 .. {CLUSTER_MAX_SERIAL}")
    nc, ec = int(n_cap), int(e_cap)
    ic = min(nc + col.numel() // CLUSTER_CHUNK + 1, CLUSTER_ITEM_CAP_MAX) if item_cap is None else int(item_cap)
    if not 1 <= nc <= 2 ** 31 - 2 or ec < 1 or not 1 <= ic <= CLUSTER_ITEM_CAP_MAX:
        raise ValueError(f"cluster_batch: n_cap is 1 .. 2^31 - 2, e_cap at least 1, item_cap 1 .. {CLUSTER_ITEM_CAP_MAX}")
    if out is None:
        out = (torch.empty(q + 1, dtype=_i32, device=dev), torch.empty(nc, dtype=_i32, device=dev),
               torch.empty(nc + 1, dtype=_i32, device=dev), torch.empty((2, ec), dtype=_i32, device=dev),
               torch.empty(ec, dtype=_i64, device=dev) if want_e_id else None, torch.empty(1, dtype=_i32, device=dev),
               torch.empty(1, dtype=_i32, device=dev))
    cptr, node_idx, rowptr_l, ei, e_id, d_n, d_e = out
    for t, name in ((cptr, "cptr"), (node_idx, "node_idx"), (rowptr_l, "rowptr_l"), (ei, "edge_index"), (d_n, "n_count"), (d_e, "e_count")):
        _chk(t, _i32, name)
    _chk(e_id, _i64, "e_id", True)
    if (cptr.numel() < q + 1 or node_idx.numel() < nc or rowptr_l.numel() < nc + 1 or ei.dim() != 2 or ei.shape[0] != 2 or
            ei.shape[1] < ec or (e_id is not None and e_id.numel() < ec)):
        raise ValueError("cluster_batch: cptr holds q + 1 values, node_idx n_cap, rowptr_l n_cap + 1, edge_index [2, e_cap], e_id e_cap")
    ws = _ws(lib().grapes_cluster_batch_workspace_bytes(nc, ic), dev)
    if col.numel() == 0:
        col = ws                                                     # (a graph without an entry: any address, never read)
    _lib.check(lib().grapes_cluster_batch(_p(rowptr), _p(col), N, _p(perm), _p(partptr), _p(where), P, _p(clusters), q, _p(stamp),
                                          int(serial), nc, ic, ec, _p(cptr), _p(node_idx), _p(rowptr_l), ei[0].data_ptr(),
                                          ei[1].data_ptr(), _p(e_id), _p(d_n), _p(d_e), _p(ws), _p(status), _stream()), "cluster_batch")
    return cptr, node_idx, rowptr_l, ei, e_id, d_n, d_e


# the graph partitioner: size-constrained synchronous label propagation (grapes_hip.h, csrc/partition_kernels.hip)
PARTITION_LDS_ROW = 2048                 # rows of 65 .. this many entries count in an LDS table; longer ones in slabs of the workspace


def _partition_graph(rowptr, col, num_nodes: int, part, num_parts: int, status, who: str):
    _chk(rowptr, _i64, "rowptr")
    _chk(col, _i32, "col")
    _chk(part, _i32, "part")
    _chk(status, _i32, "status", True)
    N, P = int(num_nodes), int(num_parts)
    if N < 1 or not 1 <= P <= N or rowptr.numel() != N + 1 or part.numel() != N:
        raise ValueError(f"{who}: rowptr holds N + 1 values, part N, and num_parts is 1 .. N")
    if col.numel() >= 2 ** 31:
        raise ValueError(f"{who}: a graph with 2^31 or more entries is not built")
    return N, P


def partition_propose(rowptr, col, num_nodes: int, part, num_parts: int, status=None, out=None):
    """(want int32 [N], gain int32 [N]) of grapes_partition_propose: the proposal of every node under the label-propagation rule of
    grapes_hip.h from part int32 [N] — want[v] = -1 and gain[v] = 0 for a node that stays.  out: the two tensors to write."""
    N, P = _partition_graph(rowptr, col, num_nodes, part, num_parts, status, "partition_propose")
    dev = part.device
    want, gain = out if out is not None else (torch.empty(N, dtype=_i32, device=dev), torch.empty(N, dtype=_i32, device=dev))
    _chk(want, _i32, "want")
    _chk(gain, _i32, "gain")
    if want.numel() != N or gain.numel() != N:
        raise ValueError("partition_propose: want and gain hold N values")
    ws = _ws(lib().grapes_partition_propose_workspace_bytes(N, P), dev)
    if col.numel() == 0:
        col = ws                                                     # (a graph without an entry: any address, never read)
    _lib.check(lib().grapes_partition_propose(_p(rowptr), _p(col), N, _p(part), P, _p(want), _p(gain), _p(ws), _p(status), _stream()),
               "partition_propose")
    return want, gain


def partition_admit(want, gain, part, size, cap: int, status=None, moved=None):
    """grapes_partition_admit: admits, per destination, the cap - size proposers with the smallest keys and moves them — part int32 [N]
    and size int32 [P] are updated in place.  Returns moved int32 [1]."""
    for t, name in ((want, "want"), (gain, "gain"), (part, "part"), (size, "size")):
        _chk(t, _i32, name)
    _chk(status, _i32, "status", True)
    N, P, dev = part.numel(), size.numel(), part.device
    if N < 1 or not 1 <= P <= N or want.numel() != N or gain.numel() != N or not 0 <= int(cap) < 2 ** 31:
        raise ValueError("partition_admit: want, gain and part hold N values, size 1 .. N, and cap is 0 .. 2^31 - 1")
    moved = torch.empty(1, dtype=_i32, device=dev) if moved is None else moved
    _chk(moved, _i32, "moved")
    ws = _ws(lib().grapes_partition_admit_workspace_bytes(N, P), dev)
    _lib.check(lib().grapes_partition_admit(_p(want), _p(gain), N, P, _p(part), _p(size), int(cap), _p(moved), _p(ws), _p(status),
                                            _stream()), "partition_admit")
    return moved


def partition_cut(rowptr, col, num_nodes: int, part, num_parts: int, status=None, out=None):
    """int64 [1]: the stored entries (v, u) with u != v and part[v] != part[u] (grapes_partition_cut)."""
    N, P = _partition_graph(rowptr, col, num_nodes, part, num_parts, status, "partition_cut")
    dev = part.device
    cut = torch.empty(1, dtype=_i64, device=dev) if out is None else out
    _chk(cut, _i64, "cut")
    ws = _ws(lib().grapes_partition_cut_workspace_bytes(N), dev)
    if col.numel() == 0:
        col = ws
    _lib.check(lib().grapes_partition_cut(_p(rowptr), _p(col), N, _p(part), P, _p(cut), _p(ws), _p(status), _stream()), "partition_cut")
    return cut


def _cluster_self_weight(diag_lambda: float) -> float:
    """1 + diag_lambda as fp32 adds them (diag_lambda rounded to fp32 first; the sum of two fp32 values rounds once through fp64)."""
    return 1.0 + _C.c_float(float(diag_lambda)).value


def cluster_aggregate_fwd(src, prep: PreparedGraph, diag_lambda: float = 0.0, add=None, bias=None, relu: bool = False, out=None,
                          copy_out=None, long_rows: Optional[bool] = None):
    """out[i] = act(s_i (sum_{j -> i} src[j] + (1 + diag_lambda) src[i]) + add[i] + bias) over prep's loop-free by-target CSR,
    s_i = 1 / (1 + deg_i): ClusterGCNConv's propagation.  src, add, out and copy_out ([n, f]) may be column blocks of wider matrices
    (rows contiguous); copy_out[i] = src[i].  long_rows: see _long_items (tests force either form)."""
    if not src.is_cuda:
        raise _lib.GrapesHipError("cluster_aggregate_fwd: src must live in HBM (cuda tensor); grapes_amd has no CPU path")
    return _rootsum_fwd("cluster", ROOTSUM_SCALE_MEAN_PLUS_ONE, _cluster_self_weight(diag_lambda), True, None, src, prep, add, bias,
                        relu, out, copy_out, long_rows)


def cluster_aggregate_bwd(dout, prep: PreparedGraph, diag_lambda: float = 0.0, relu_out=None, add=None, want_src: bool = True,
                          want_add: bool = False, want_bias: bool = False, dsrc=None, dadd=None, long_rows: Optional[bool] = None):
    """(dsrc, dadd, dbias) of cluster_aggregate_fwd from dout = d out: g = dout gated by relu_out > 0 (the forward's output, when the
    ReLU was fused); dsrc[j] = sum_{i <- j} s_i g_i + (1 + diag_lambda) s_j g_j (+ add[j]) over the by-source CSR; dadd = g; dbias =
    the column sums of g.  dsrc / dadd: tensors (column blocks allowed) to write; want_*: allocate them.  Fixed order, no atomics."""
    if not dout.is_cuda:
        raise _lib.GrapesHipError("cluster_aggregate_bwd: dout must live in HBM (cuda tensor); grapes_amd has no CPU path")
    return _rootsum_bwd("cluster", ROOTSUM_SCALE_MEAN_PLUS_ONE, _cluster_self_weight(diag_lambda), True, None, dout, prep, relu_out,
                        add, want_src, want_add, want_bias, dsrc, dadd, long_rows)


def classifier_loss(logits, local_rows, target_ids, labels, out_grad=None):
    """(loss_c [1], d loss_c / d logits [n_rows, C]) — main.py:260,267.  labels: int64 [N] or fp32 [N, C]."""
    _chk(logits, _f32, "logits"); _chk(local_rows, _i32, "local_rows"); _chk(target_ids, _i32, "target_ids")
    n_rows, C = logits.shape
    multi = labels.dim() == 2
    _chk(labels, _f32 if multi else _i64, "labels")
    if out_grad is None:
        out_grad = torch.empty_like(logits)
    loss = torch.empty(1, dtype=_f32, device=logits.device)
    _lib.check(lib().grapes_classifier_loss(_p(logits), n_rows, C, _p(local_rows), _p(target_ids),
                                            None if multi else _p(labels), _p(labels) if multi else None,
                                            local_rows.numel(), _p(out_grad), _p(loss), _stream()), "classifier_loss")
    return loss, out_grad


def gflownet_loss(hop_stats, loss_c, loss_coef, log_z_raw=None, log_z_init=0.0, reinforce=False):
    """out4 = [loss_gfn, grad scale, log_z, sum log-probs] — main.py:272-282."""
    _chk(hop_stats, _f32, "hop_stats"); _chk(loss_c, _f32, "loss_c"); _chk(log_z_raw, _f32, "log_z_raw", True)
    hops, stride = hop_stats.shape
    out = torch.empty(4, dtype=_f32, device=hop_stats.device)
    _lib.check(lib().grapes_gflownet_loss(_p(log_z_raw), float(log_z_init), _p(hop_stats), hops, stride, _p(loss_c),
                                          float(loss_coef), 1 if reinforce else 0, _p(out), _stream()), "gflownet_loss")
    return out


def dropout_fwd(x, p, philox_seed=0, philox_offset=0, d_philox_offset=None, d_n=None):
    """F.dropout(x, p, training=True) on the Philox stream (include/grapes_hip.h): -> (y, keep bytes).  With d_philox_offset the
    device counter is used and advanced."""
    _chk(x, _f32, "x")
    n, f = x.shape
    y = torch.empty_like(x)
    keep = torch.empty((n, f), dtype=torch.uint8, device=x.device)
    _lib.check(lib().grapes_dropout_fwd(_p(x), _p(y), _p(keep), n, _p(d_n), f, float(p), int(philox_seed), int(philox_offset),
                                        _p(d_philox_offset), _stream()), "dropout_fwd")
    return y, keep


def dropout_bwd(dy, keep, p, d_n=None):
    _chk(dy, _f32, "dy")
    n, f = dy.shape
    dx = torch.empty_like(dy)
    _lib.check(lib().grapes_dropout_bwd(_p(dy), _p(keep), _p(dx), n, _p(d_n), f, float(p), _stream()), "dropout_bwd")
    return dx


def logit_var_reg(logits, reg, d_n=None, dlogits=None):
    """reg * sum_r var(logits[r, :]) (main.py:260-261).  Without dlogits: returns the term ([1], for step_losses(loss_extra=));
    with dlogits: adds its gradient to them in place."""
    _chk(logits, _f32, "logits"); _chk(dlogits, _f32, "dlogits", True)
    n, C = logits.shape
    out = torch.empty(1, dtype=_f32, device=logits.device) if dlogits is None else None
    _lib.check(lib().grapes_logit_var_reg(_p(logits), n, _p(d_n), C, float(reg), _p(out), _p(dlogits), _stream()), "logit_var_reg")
    return out if dlogits is None else dlogits


def step_losses(logits, node_map, target_ids, labels, hop_stats, loss_coef, z_out=None, d_nz=None, log_z_init=0.0,
                reinforce=False, many_workgroups=True, loss_extra=None):
    """classifier_loss (target rows = node_map[target_ids]) + mean of z_out + gflownet_loss in one launch
    (main.py:259-282).  Returns (loss_c [1], d loss_c / d logits, out4)."""
    _chk(logits, _f32, "logits"); _chk(node_map, _i32, "node_map"); _chk(target_ids, _i32, "target_ids")
    _chk(hop_stats, _f32, "hop_stats"); _chk(z_out, _f32, "z_out", True)
    n_rows, C = logits.shape
    multi = labels.dim() == 2
    _chk(labels, _f32 if multi else _i64, "labels")
    hops, stride = hop_stats.shape
    dlogits = torch.empty_like(logits)
    loss = torch.empty(1, dtype=_f32, device=logits.device)
    out4 = torch.empty(4, dtype=_f32, device=logits.device)
    ws = _ws(lib().grapes_step_losses_workspace_bytes(target_ids.numel()), logits.device) if many_workgroups else None
    ticket = _ticket(logits.device)[8:9] if many_workgroups else None
    _lib.check(lib().grapes_step_losses(_p(logits), n_rows, C, _p(node_map), _p(target_ids),
                                        None if multi else _p(labels), _p(labels) if multi else None, target_ids.numel(),
                                        _p(dlogits), _p(loss), _p(z_out), 0 if z_out is None else z_out.numel(), _p(d_nz),
                                        float(log_z_init), _p(hop_stats), hops, stride, float(loss_coef),
                                        1 if reinforce else 0, _p(out4), _p(loss_extra), _p(ws), _p(ticket), _stream()), "step_losses")
    return loss, dlogits, out4


def gcn_aggregate_fwd_losses(h, prep: PreparedGraph, bias, node_map, target_ids, labels, hop_stats, loss_coef, z_out=None,
                             d_nz=None, log_z_init=0.0, reinforce=False):
    """gcn_aggregate_fwd(h, prep, bias) = the logits, and step_losses on them, in ONE launch (main.py:256-282): the wavefront that
    forms a row runs its loss.  Returns (logits, loss_c [1], d loss_c / d logits, out4), bit-identical to the two calls — or
    None when the shape is not covered (the caller runs the two launches): it covers the row-per-wavefront aggregation with one
    float per lane (f > 16, f % 4 != 0 or an unaligned base), n <= 65536 rows, no long-row items."""
    _chk(h, _f32, "h"); _chk(bias, _f32, "bias", True); _chk(node_map, _i32, "node_map"); _chk(target_ids, _i32, "target_ids")
    _chk(hop_stats, _f32, "hop_stats"); _chk(z_out, _f32, "z_out", True)
    n, f = h.shape
    multi = labels.dim() == 2
    _chk(labels, _f32 if multi else _i64, "labels")
    B = target_ids.numel()
    if (prep.items_fwd and prep.n > _SMALL_GRAPH) or _rec_form(prep, n, f) or not 0 < B <= 4096:
        return None
    out = torch.empty_like(h)
    if not lib().grapes_gcn_aggregate_fwd_losses_available(_p(h), _p(bias), _p(out), n, f):
        return None
    hops, stride = hop_stats.shape
    dlogits = torch.empty_like(h)
    loss = torch.empty(1, dtype=_f32, device=h.device)
    out4 = torch.empty(4, dtype=_f32, device=h.device)
    ws = _ws(lib().grapes_step_losses_workspace_bytes(B), h.device)
    ticket = _ticket(h.device)[8:9]
    _lib.check(lib().grapes_gcn_aggregate_fwd_losses(_p(h), _p(prep.rowptr_t), _p(prep.csr_src), _p(prep.dinv), _p(bias), _p(out),
                                                     n, _p(prep.d_n), f, _p(node_map), _p(target_ids),
                                                     None if multi else _p(labels), _p(labels) if multi else None, B,
                                                     _p(dlogits), _p(loss), _p(z_out), 0 if z_out is None else z_out.numel(),
                                                     _p(d_nz), float(log_z_init), _p(hop_stats), hops, stride, float(loss_coef),
                                                     1 if reinforce else 0, _p(out4), _p(ws), _p(ticket), _stream()),
               "gcn_aggregate_fwd_losses")
    return out, loss, dlogits, out4


class FusedAdam:
    """torch.optim.Adam updates of one or more optimisers in ONE launch (main.py:268,289).  Works on the optimisers'
    own state tensors (exp_avg, exp_avg_sq, step), so state_dict() / checkpoints stay those of torch.optim.Adam.
    Hyper-parameters are read when the descriptor is built; call refresh() after changing them (lr schedules)."""

    def __init__(self, optimizers, mirrors=None):
        """mirrors: {parameter: (w_pad | None, image | None)} — copies of a [rows, K] weight that the launch keeps current with the
        update: w_pad fp32 [rows, >= K] (its padding columns stay as they are) and / or the bf16x3 split image of
        weight_split_image (rows <= 256).  Both must hold the CURRENT weight when the first step runs."""
        self.optimizers = [o for o in optimizers if o is not None]
        self.mirrors = {id(p): (p, m) for p, m in (mirrors or {}).items()}
        self.refresh()

    def refresh(self):
        import struct
        recs, self._keep, dev, maxn = [], [], None, 1
        self._keep_mirrors = []
        for opt in self.optimizers:
            for gp in opt.param_groups:
                if gp.get("amsgrad", False):
                    raise ValueError("FusedAdam: amsgrad is not supported")
                b1, b2 = gp["betas"]
                for p in gp["params"]:
                    if not p.requires_grad:
                        continue
                    _chk(p.data, _f32, "param")
                    dev = p.device
                    if p.grad is None:
                        p.grad = torch.zeros_like(p)
                    st = opt.state[p]
                    if "step" not in st:                     # same lazy state torch creates (capturable layout)
                        st["step"] = torch.zeros((), dtype=_f32, device=dev)
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if not (st["step"].is_cuda and st["step"].dtype == _f32):
                        raise ValueError("FusedAdam needs device-resident step counters (Adam(capturable=True))")
                    self._keep.append((p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"]))
                    w_pad = img = None
                    K = ld_pad = 0
                    mir = self.mirrors.get(id(p))
                    if mir is not None:
                        w_pad, img = mir[1]
                        if p.dim() != 2 or not p.is_contiguous() or (img is not None and p.shape[0] > 256) or p.numel() >= 2 ** 31:
                            raise ValueError("FusedAdam: a mirrored weight is a contiguous [rows <= 256 for an image, K] matrix")
                        K = int(p.shape[1])
                        if w_pad is not None:
                            _chk(w_pad, _f32, "w_pad")
                            if w_pad.shape[0] != p.shape[0] or w_pad.shape[1] < K or w_pad.stride(1) != 1:
                                raise ValueError("FusedAdam: w_pad is fp32 [rows, >= K]")
                            ld_pad = int(w_pad.stride(0))
                        if img is not None and img.numel() < int(lib().grapes_weight_split_image_bytes(K)):
                            raise ValueError("FusedAdam: the image is smaller than grapes_weight_split_image_bytes(K)")
                        self._keep_mirrors.append((w_pad, img))
                    recs.append(struct.pack("PPPPPqdddddiiPPii", p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(),
                                            st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(), p.numel(), float(gp["lr"]),
                                            float(b1), float(b2), float(gp["eps"]), float(gp.get("weight_decay", 0.0)),
                                            1 if gp.get("maximize", False) else 0, 0,
                                            w_pad.data_ptr() if w_pad is not None else 0, img.data_ptr() if img is not None else 0,
                                            K, ld_pad))
                    maxn = max(maxn, p.numel())
        if not recs:
            raise ValueError("FusedAdam: no parameters")
        if len({k[4].data_ptr() for k in self._keep}) != len(self._keep):
            raise ValueError("FusedAdam: every parameter needs its own step counter (as torch.optim.Adam keeps them)")
        assert len(recs[0]) == lib().grapes_adam_desc_bytes()
        self.n, self.maxn = len(recs), maxn
        self.desc = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(dev)
        self.ticket = torch.zeros(self.n, dtype=_i32, device=dev)

    def step(self, slabs: "DeferredSlabs" = None):
        """slabs: deferred few-row weight-gradient slabs (DeferredSlabs, not flushed) whose sums are formed inside this launch;
        sets whose target is not a gradient of these optimisers (or not of its size) make the whole batch flush first."""
        for p, g, *_ in self._keep:
            if p.grad is not g:
                raise RuntimeError("FusedAdam: a .grad tensor was replaced; gradients must be written in place")
        if slabs is not None and slabs.sets:
            grads = {g.data_ptr(): g.numel() for _, g, *_ in self._keep}
            if len(slabs.sets) <= 8 and all(grads.get(s[2].data_ptr()) == s[3] for s in slabs.sets):
                import ctypes as C
                k = len(slabs.sets)
                sl = (C.c_void_p * k)(*[s[1] for s in slabs.sets])
                gr = (C.c_void_p * k)(*[s[2].data_ptr() for s in slabs.sets])
                _lib.check(lib().grapes_adam_step_slabs(_p(self.desc), self.n, self.maxn, _p(self.ticket), k, sl, gr, slabs.n,
                                                        _p(slabs.d_n), 1 if slabs.acc else 0, _stream()), "adam_step_slabs")
                slabs.sets = []
                return
            slabs.flush()
        _lib.check(lib().grapes_adam_step(_p(self.desc), self.n, self.maxn, _p(self.ticket), _stream()), "adam_step")
