"""Drop-in ``GCN`` (reference modules/gcn.py:9-42), ``GAT`` (modules/gcn.py:45-72), ``GCN2`` (modules/gcn.py:76-117) and ``PNA``
(modules/gcn.py:120-149) whose layers run the gfx950 kernels, and ``GATv2`` (PyG's GATv2Conv under GAT's routing; not in the reference).

state_dict keys match PyG's GCNConv inside the reference module: ``gcn_layers.{i}.lin.weight``
([out,in]) and ``gcn_layers.{i}.bias``; for GAT [PyG-recall: torch_geometric 2.5.2 GATConv] ``gat_layers.{i}.lin.weight``,
``.att_src`` / ``.att_dst`` ([1, 1, out]) and ``.bias``; for GCN2 [PyG-recall: GCN2Conv, Linear] ``lins.{0,1}.weight`` / ``.bias``
and ``conv.{i}.weight1`` (``.weight2`` with ``shared_weights=False``); for PNA [PyG-recall: PNAConv] ``conv.{i}.pre_nn`` / ``.post_nn`` /
``.lin`` ``.weight`` / ``.bias`` and ``lins.weight`` / ``.bias``; for GATv2 [PyG-recall: GATv2Conv] ``gat_layers.{i}.att`` ([1, heads, out]),
``.lin_l.weight`` / ``.bias``, ``.lin_r.weight`` / ``.bias`` (absent with ``share_weights``) and ``.bias``.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional, Union

import torch

from .._lib import diag_switch as _sw      # A/B switches: the default unless GRAPES_DIAG=1
import torch.nn as nn
import torch.nn.functional as F

from .. import full_graph, ops

_PREP_CACHE: "OrderedDict[int, tuple]" = OrderedDict()
_PREP_CACHE_SIZE = 16
# floats: full-batch inference pads a transform-first layer's output rows to a multiple of this (A/B: GRAPES_EVAL_ROW_PAD=4 is
# the default, 16-byte rows; 32 = whole 128-byte lines — measured no faster once the rows are pre-scaled: profiles/r03_bench_eval_fullbatch.json)
import os as _os
_EVAL_ROW_PAD = int(_sw("GRAPES_EVAL_ROW_PAD", "4"))            # inference: output rows padded to a multiple of this many floats (16 bytes)
_EVAL_PRESCALED = _sw("GRAPES_EVAL_PRESCALED", "1") != "0"     # A/B: 0 = per-edge dinv gather (round-2 form)


def prepare_edges(edge_index, n: int) -> ops.PreparedGraph:
    """gcn_norm + CSRs for one edge list, cached on the identity (and version) of the tensor so the
    two layers of gcn_gf and gcn_z (main.py:210,227) share one preparation."""
    if isinstance(edge_index, ops.PreparedGraph):
        return edge_index
    if hasattr(edge_index, "gcn_prepared"):        # graph.DeviceGraph: full-batch message passing (eval.py:50)
        return edge_index.gcn_prepared()
    key = id(edge_index)
    hit = _PREP_CACHE.get(key)
    if hit is not None and hit[0] is edge_index and hit[1] == edge_index._version and hit[2] == n:
        _PREP_CACHE.move_to_end(key)
        return hit[3]
    if not edge_index.is_cuda:
        raise ops._lib.GrapesHipError("edge_index must be a cuda tensor (grapes_amd has no CPU path)")
    ei = edge_index.to(torch.int32)
    prep = ops.PreparedGraph(ei[0].contiguous(), ei[1].contiguous(), n)
    _PREP_CACHE[key] = (edge_index, edge_index._version, n, prep)   # holds the tensor: its address cannot be reused
    while len(_PREP_CACHE) > _PREP_CACHE_SIZE:
        _PREP_CACHE.popitem(last=False)
    return prep


def _large(edge_index, large_graph: Optional[bool]) -> bool:
    """True when a whole-graph call goes through full_graph.py; with autograd on such a graph it raises."""
    if not hasattr(edge_index, "full_graph_plan") or not full_graph.use_large_path(edge_index, large_graph):
        return False
    if torch.is_grad_enabled():
        raise ValueError("full-graph training over a graph with 2^31 or more entries is not built into GCN.forward: the "
                         "full-graph pass there is inference only (call it under torch.no_grad() / torch.inference_mode()); "
                         "train with grapes_amd.full_graph.train_step")
    return True


def clear_prepare_cache():
    _PREP_CACHE.clear()


def weighted_structure(edge_index, n: int) -> ops.WeightedStructure:
    """The slots of every entry of an edge-index tensor in its PreparedGraph (ops.WeightedStructure), built once and cached
    beside the PreparedGraph, keyed on the tensor like it.  The weights are never cached."""
    prep = prepare_edges(edge_index, n)
    key = id(edge_index)
    hit = _PREP_CACHE.get(key)
    if hit is not None and hit[3] is prep and len(hit) > 4:
        return hit[4]
    ei = edge_index.to(torch.int32)
    ws = ops.WeightedStructure(prep, ei[0].contiguous(), ei[1].contiguous())
    if hit is not None and hit[3] is prep:
        _PREP_CACHE[key] = hit[:4] + (ws,)
    return ws


def _check_edge_weight(edge_index, edge_weight, large_graph, who: str):
    """ValueError unless edge_weight is one fp32 value per column of an edge-index TENSOR on the same device."""
    if not torch.is_tensor(edge_index) or large_graph:
        raise ValueError(f"{who}: edge_weight goes with an edge-index tensor [2, e]; the DeviceGraph / PreparedGraph / large-graph "
                         "paths are unweighted")
    if not torch.is_tensor(edge_weight):
        raise ValueError(f"{who}: edge_weight must be a tensor")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"{who}: edge_index must be [2, e]")
    if edge_weight.dim() != 1 or edge_weight.numel() != edge_index.shape[1]:
        raise ValueError(f"{who}: edge_weight {tuple(edge_weight.shape)} must hold one value per entry ({edge_index.shape[1]})")
    if edge_weight.dtype != torch.float32:
        raise ValueError(f"{who}: edge_weight must be float32, got {edge_weight.dtype}")
    if edge_weight.device != edge_index.device:
        raise ValueError(f"{who}: edge_weight is on {edge_weight.device}, edge_index on {edge_index.device}")


class _GCNConvFn(torch.autograd.Function):
    """out = Â (X Wᵀ) + b (PyG order).  When the input needs no gradient and F_in < F_out the same value is
    computed aggregate-first, act((Â X) Wᵀ + b): the SpMM runs on the narrow side, bias/ReLU ride in the GEMM
    epilogue and the backward is a single GEMM (no transposed SpMM) — equal up to fp32 rounding."""

    @staticmethod
    def forward(ctx, x, weight, bias, prep, relu):
        f_out, f_in = weight.shape
        ctx.prep, ctx.relu = prep, relu
        ctx.agg_first = (not ctx.needs_input_grad[0]) and f_in < f_out and f_out > 1
        if ctx.agg_first:
            ax = ops.gcn_aggregate_fwd(x, prep, None, False)               # Â X        (gather-SpMM, narrow rows)
            out = ops.linear_bias_act_fwd(ax, weight, bias, relu, d_n=prep.d_n)   # (ÂX) Wᵀ + b, ReLU  (MFMA)
            ctx.save_for_backward(ax, weight, out if relu else None)
            return out
        h = ops.linear_fwd(x, weight, d_n=prep.d_n)                        # H = X W^T   (MFMA fp32)
        out = ops.gcn_aggregate_fwd(h, prep, bias, relu)                   # gather-SpMM + bias (+ReLU)
        ctx.save_for_backward(x, weight, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, out = ctx.saved_tensors
        prep = ctx.prep
        if ctx.agg_first:
            dw, dbias = ops.linear_bwd_weight_gated(dout.contiguous(), x, gate=out if ctx.relu else None, d_n=prep.d_n)
            return None, dw, dbias if ctx.needs_input_grad[2] else None, None, None
        dh, dbias = ops.gcn_aggregate_bwd(dout.contiguous(), prep, relu_out=out if ctx.relu else None)
        dw = ops.linear_bwd_weight(dh, x, d_n=prep.d_n)
        dx = ops.linear_bwd_input(dh, weight, d_n=prep.d_n) if ctx.needs_input_grad[0] else None
        return dx, dw, dbias if ctx.needs_input_grad[2] else None, None, None


class _WeightedGCNConvFn(torch.autograd.Function):
    """_GCNConvFn with edge weights (PyG gcn_norm with edge_weight, ops.wgcn_*): the same transform-first / aggregate-first rule
    and the same GEMMs.  The edge-weight gradient (formed only when edge_weight needs one) is that of the aggregation
    out' = Â_w H with G = d out': transform-first H = X Wᵀ and G = the gated dout; aggregate-first H = X and
    G = linear_bwd_input(gated dout, W).
    mode / fill: the layer's rule for the loop weights and the normalisation (ops.WGCN_*: improved, add_self_loops=False,
    normalize=False); there edge_weight may be None (every weight 1, no weight gradient) and bias may be None."""

    @staticmethod
    def forward(ctx, x, weight, bias, edge_weight, ws, relu, mode, fill):
        f_out, f_in = weight.shape
        d_n = ws.prep.d_n
        vals = ops.wgcn_weights(ws, None if edge_weight is None else edge_weight.detach().contiguous(), mode, fill)
        ctx.ws, ctx.vals, ctx.relu = ws, vals, relu
        ctx.want_dw = ctx.needs_input_grad[3]
        ctx.agg_first = (not ctx.needs_input_grad[0]) and f_in < f_out and f_out > 1
        if ctx.agg_first:
            ax = ops.wgcn_aggregate_fwd(x, ws, vals)                             # Â_w X      (gather, narrow rows)
            out = ops.linear_bias_act_fwd(ax, weight, bias, relu, d_n=d_n)       # (Â_w X) Wᵀ + b, ReLU  (MFMA)
            ctx.save_for_backward(ax, weight, out if relu else None, x if ctx.want_dw else None)
            return out
        h = ops.linear_fwd(x, weight, d_n=d_n)                                   # H = X W^T   (MFMA fp32)
        out = ops.wgcn_aggregate_fwd(h, ws, vals, bias, relu)                    # weighted gather + bias (+ReLU)
        ctx.save_for_backward(x, weight, out if relu else None, h if ctx.want_dw else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        first, weight, out, h = ctx.saved_tensors
        ws, vals, d_n = ctx.ws, ctx.vals, ctx.ws.prep.d_n
        dout = dout.contiguous()
        if ctx.agg_first:
            dw = dbias = dew = None
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                dw, dbias = ops.linear_bwd_weight_gated(dout, first, gate=out if ctx.relu else None, d_n=d_n,
                                                        want_bias=ctx.needs_input_grad[2])
            if ctx.want_dw:
                g = ops.gcn2_mix_bwd(dout, out, True, 1.0, d_n=d_n)[0] if ctx.relu else dout
                dax = ops.linear_bwd_input(g, weight, d_n=d_n)
                dew = ops.wgcn_aggregate_bwd(dax, ws, vals, h=h, want_dh=False, want_dw=True, want_bias=False)[2]
            return None, dw, dbias, dew, None, None, None, None
        dh, dbias, dew = ops.wgcn_aggregate_bwd(dout, ws, vals, h=h, relu_out=out if ctx.relu else None,
                                                want_dh=ctx.needs_input_grad[0] or ctx.needs_input_grad[1], want_dw=ctx.want_dw,
                                                want_bias=ctx.needs_input_grad[2])
        dw = ops.linear_bwd_weight(dh, first, d_n=d_n) if ctx.needs_input_grad[1] else None
        dx = ops.linear_bwd_input(dh, weight, d_n=d_n) if ctx.needs_input_grad[0] else None
        return dx, dw, dbias, dew, None, None, None, None


class GCNConv(nn.Module):
    """out = D^-1/2 (A + I) D^-1/2 · X Wᵀ + b with PyG's conventions.  With edge_weight [e] (PyG's third
    argument): out = D^-1/2 (A_w + diag(lw)) D^-1/2 · X Wᵀ + b, where A_w sums the weights of the non-loop entries (duplicates each
    count), lw[i] = 1 or the weight of the LAST stored entry (i, i), and D = the weighted in-degree + lw.  A negative degree gives
    NaN, as in PyG; it is not checked.

    The constructor is PyG 2.5's [PyG-recall]: GCNConv(in_channels, out_channels, improved=False, cached=False, add_self_loops=None,
    normalize=True, bias=True); add_self_loops=None means "as normalize".
      improved=True           lw[i] = 2 where node i stores no loop (A + 2I);
      add_self_loops=False    nothing is added and a stored loop is an ordinary entry: out = D^-1/2 A_w D^-1/2 · X Wᵀ + b with every
                              occurrence counted in A_w and D (a node without an incoming entry outputs b); improved has no effect;
      normalize=False         out[c] = Σ_{e: r -> c} w_e (X Wᵀ)[r] + b, the weights (1 without edge_weight) as given;
      bias=False              no bias parameter.
    Anything but (improved=False, add_self_loops=True, normalize=True) takes an edge-index tensor [2, e] (ops.wgcn_* with a mode);
    cached=True is not built."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False,
                 add_self_loops: Optional[bool] = None, normalize: bool = True, bias: bool = True):
        super().__init__()
        if cached:
            raise NotImplementedError("GCNConv: cached=True is not built (the normalisation is recomputed on every call)")
        if add_self_loops is None:
            add_self_loops = normalize
        if add_self_loops and not normalize:
            raise ValueError("GCNConv: add_self_loops=True goes with normalize=True only (PyG refuses the pair too)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.add_self_loops, self.normalize = bool(improved), False, bool(add_self_loops), bool(normalize)
        if not self.normalize:
            self._mode, self._fill = ops.WGCN_UNNORMALIZED, 1.0
        elif not self.add_self_loops:
            self._mode, self._fill = ops.WGCN_LOOP_SUM, 1.0
        else:
            self._mode, self._fill = ops.WGCN_LOOP_FILL, (2.0 if self.improved else 1.0)
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))    # PyG glorot
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()

    def _default_mode(self) -> bool:
        return self._mode == ops.WGCN_LOOP_FILL and self._fill == 1.0

    def forward(self, x, edge_index, relu: bool = False, large_graph: Optional[bool] = None, edge_weight=None):
        if edge_weight is not None:
            _check_edge_weight(edge_index, edge_weight, large_graph, "GCNConv")
        elif not self._default_mode():
            if not torch.is_tensor(edge_index) or large_graph:
                raise ValueError("GCNConv: improved=True, add_self_loops=False and normalize=False go with an edge-index tensor "
                                 "[2, e]; the DeviceGraph / PreparedGraph / large-graph paths are the default layer's")
            if edge_index.dim() != 2 or edge_index.shape[0] != 2:
                raise ValueError("GCNConv: edge_index must be [2, e]")
        if not x.is_cuda:
            raise ops._lib.GrapesHipError("GCNConv input must be a cuda tensor (grapes_amd has no CPU path)")
        if edge_weight is not None or not self._default_mode():
            x = x.contiguous()
            if x.dtype != torch.float32:
                x = x.float()
            ws = weighted_structure(edge_index, x.shape[0])
            return _WeightedGCNConvFn.apply(x, self.lin.weight, self.bias, edge_weight, ws, relu, self._mode, self._fill)
        if _large(edge_index, large_graph):                    # a DeviceGraph with 2^31+ entries (or forced): full_graph.py
            return full_graph.conv_forward(self, x, edge_index, relu)
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        prep = prepare_edges(edge_index, x.shape[0])
        fo, fi = self.lin.weight.shape
        if self.bias is None:                                  # (the inference forms below pad the bias: the training form serves)
            return _GCNConvFn.apply(x, self.lin.weight, None, prep, relu)
        if (not torch.is_grad_enabled()) and _EVAL_PRESCALED and prep.n > ops._SMALL_GRAPH and prep.items_fwd and fo > 1:
            return self._forward_full_batch_inference(x, prep, relu)
        if ((not torch.is_grad_enabled()) and not _EVAL_PRESCALED and fo % _EVAL_ROW_PAD and fo > 16 and fi >= fo and
                prep.n > ops._SMALL_GRAPH and prep.items_fwd):
            # (A/B form of the diagnostic session only, GRAPES_EVAL_PRESCALED=0: the round-2 inference path — per-edge dinv
            # gather — with the output rows padded to a multiple of GRAPES_EVAL_ROW_PAD floats; the default path above does
            # the same padding inside _forward_full_batch_inference)
            fp = (fo + _EVAL_ROW_PAD - 1) // _EVAL_ROW_PAD * _EVAL_ROW_PAD
            wp = torch.zeros((fp, fi), dtype=x.dtype, device=x.device); wp[:fo] = self.lin.weight
            bp = torch.zeros(fp, dtype=x.dtype, device=x.device); bp[:fo] = self.bias
            h = ops.linear_fwd(x, wp, d_n=prep.d_n)
            return ops.gcn_aggregate_fwd(h, prep, bp, relu)[:, :fo]
        return _GCNConvFn.apply(x, self.lin.weight, self.bias, prep, relu)


def _full_batch_inference(self, x, prep, relu):
    """Full-batch message passing without autograd (eval.py:47-70: one pass over the whole adjacency; N1).  Two changes
    against the training form, both about memory requests per aggregated edge, neither about what is computed:
      * the aggregated rows are PRE-SCALED by their own dinv (ops.scale_rows — one streaming pass), so the gather-SpMM needs
        no random 4-byte gather of dinv[source] per edge;
      * a transform-first layer whose width is not a multiple of 4 floats computes on a weight / bias zero-padded to the next
        multiple of _EVAL_ROW_PAD = 4 (ogbn-products' 47 classes -> 48 columns, a 192-byte pitch): the gathered rows are
        16-byte aligned (dwordx4 loads instead of scalar ones) and the leading columns are returned as a view.  (Padding to
        whole 128-byte lines — 64 columns, GRAPES_EVAL_ROW_PAD=32 in a diagnostic session — measured the SAME time, 6.95 ms at
        F = 48: the pass is bound by requests per edge, not by the lines a row straddles; profiles/r03_bench_eval_fullbatch.json
        was measured with the default, 48 columns.)"""
    w, b = self.lin.weight, self.bias
    fo, fi = w.shape
    if fi < fo and fi % 4 == 0 and fi > 16:                                 # aggregate on the narrow side (as _GCNConvFn)
        ax = ops.gcn_aggregate_fwd_prescaled(ops.scale_rows(x, prep.dinv), prep, None, False)
        return ops.linear_bias_act_fwd(ax, w, b, relu, d_n=prep.d_n)
    fp = (fo + _EVAL_ROW_PAD - 1) // _EVAL_ROW_PAD * _EVAL_ROW_PAD if fo > 16 else fo
    if fp <= 16 or fp % 4:
        return _GCNConvFn.apply(x, w, b, prep, relu)
    if fp != fo:
        wp = torch.zeros((fp, fi), dtype=x.dtype, device=x.device); wp[:fo] = w
        bp = torch.zeros(fp, dtype=x.dtype, device=x.device); bp[:fo] = b
    else:
        wp, bp = w, b
    h = ops.linear_fwd_row_scaled(x, wp, prep.dinv, d_n=prep.d_n)       # dinv scaling in the GEMM's epilogue (no scale_rows pass)
    out = ops.gcn_aggregate_fwd_prescaled(h, prep, bp, relu)
    return out[:, :fo] if fp != fo else out


GCNConv._forward_full_batch_inference = _full_batch_inference


class _PhiloxDropoutFn(torch.autograd.Function):
    """F.dropout on the sampler's Philox stream (ops.dropout_fwd): the mask is a function of (seed, offset, element index), so
    a captured step and an eager step draw the same one."""

    @staticmethod
    def forward(ctx, x, p, seed, offset):
        y, keep = ops.dropout_fwd(x.contiguous(), p, philox_seed=seed, philox_offset=offset)
        ctx.save_for_backward(keep)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        (keep,) = ctx.saved_tensors
        return ops.dropout_bwd(dy.contiguous(), keep, ctx.p), None, None, None


def _memory_allocated_mb() -> float:
    """torch.cuda.memory_allocated() / 2^20 (gcn.py:40: the second element of GCN.forward's result) read from the allocator's
    nested statistics directly — torch.cuda.memory_allocated() flattens the whole statistics dictionary first (0.14 ms per call,
    five calls per training step: profiles/eager_profile.py)."""
    try:
        st = torch._C._cuda_memoryStats(torch._C._cuda_getDevice())
        return st["allocated_bytes"]["all"]["current"] / (1024 * 1024)
    except (AttributeError, KeyError, RuntimeError):
        return torch.cuda.memory_allocated() / (1024 * 1024)


class GCN(nn.Module):
    def __init__(self, in_features: int, hidden_dims: "list[int]", dropout: float = 0.):
        super(GCN, self).__init__()
        self.dropout = dropout
        # optional: a callable  n_elements -> (seed, offset)  that hands out Philox counters (step.GrapesTrainer sets it when it
        # was given a philox_seed); without it dropout draws from torch's generator exactly like the reference
        self.philox_dropout = None
        dims = [in_features] + hidden_dims
        gcn_layers = []
        for i in range(len(hidden_dims) - 1):
            gcn_layers.append(GCNConv(in_channels=dims[i], out_channels=dims[i + 1]))
        gcn_layers.append(GCNConv(in_channels=dims[-2], out_channels=dims[-1]))
        self.gcn_layers = nn.ModuleList(gcn_layers)

    def _drop(self, x):
        # (only under autograd, i.e. inside a training step: evaluate() runs under no_grad with the module still in training mode
        # — the reference never calls .eval() — and must not consume the training step's Philox counters)
        if (self.philox_dropout is not None and self.training and self.dropout > 0.0 and x.is_cuda and
                torch.is_grad_enabled()):
            seed, offset = self.philox_dropout(x.numel())
            return _PhiloxDropoutFn.apply(x, float(self.dropout), seed, offset)
        return F.dropout(x, p=self.dropout, training=self.training)

    def forward(self, x: torch.Tensor, edge_index: Union[torch.Tensor, "list[torch.Tensor]"], large_graph: Optional[bool] = None,
                edge_weight=None):
        """large_graph: None = automatic — a DeviceGraph with 2^31 or more entries runs the row-blocked 64-bit pass of
        full_graph.py (inference only); True forces that pass on any DeviceGraph.
        edge_weight: one fp32 vector for an edge-index tensor, or for a list of edge lists a list of equal length (entries may be
        None), indexed exactly as the edges are: [-i] for hidden layer i, [0] for the last."""
        if edge_weight is not None:
            if type(edge_index) == list:
                if type(edge_weight) != list or len(edge_weight) != len(edge_index):
                    raise ValueError("GCN: a list of edge lists takes a list of edge weights of equal length (entries may be None)")
                for ei, ew in zip(edge_index, edge_weight):
                    if ew is not None:
                        _check_edge_weight(ei, ew, large_graph, "GCN")
            elif type(edge_weight) == list:
                raise ValueError("GCN: a list of edge weights goes with a list of edge lists")
            else:
                _check_edge_weight(edge_index, edge_weight, large_graph, "GCN")
        if _large(edge_index, large_graph):                                   # eval.py:50 on papers100M-sized graphs
            return full_graph.gcn_forward(self, x, edge_index), _memory_allocated_mb()
        layerwise_adjacency = type(edge_index) == list
        # (the reference slices the ModuleList, gcn.py:31: a slice builds a NEW ModuleList on every call — add_module and its
        # hasattr probes, ~0.1 ms per layer of host time; iterate by index instead)
        n_layers = len(self.gcn_layers)
        for i in range(1, n_layers):
            layer = self.gcn_layers[i - 1]
            edges = edge_index[-i] if layerwise_adjacency else edge_index      # gcn.py:31
            w = edge_weight[-i] if (layerwise_adjacency and edge_weight is not None) else edge_weight
            x = layer(x, edges, relu=True, edge_weight=w)                      # gcn.py:32 (ReLU fused)
            x = self._drop(x)                                                  # gcn.py:33
        edges = edge_index[0] if layerwise_adjacency else edge_index           # gcn.py:35
        w = edge_weight[0] if (layerwise_adjacency and edge_weight is not None) else edge_weight
        logits = self.gcn_layers[n_layers - 1](x, edges, edge_weight=w)
        logits = self._drop(logits)                                            # gcn.py:37
        memory_alloc = _memory_allocated_mb()                                  # gcn.py:40
        return logits, memory_alloc


# ------------------------------------------------------------------------------------------------ GAT (modules/gcn.py:45-72)
class _GATConvFn(torch.autograd.Function):
    """out = softmax-weighted gather of H = X Wᵀ (+ b, ReLU): grapes_linear_fwd, grapes_gat_scores, grapes_gat_aggregate_fwd.
    The backward recomputes the attention weights from the saved scores and (row max, log sum): nothing is stored per edge."""

    @staticmethod
    def forward(ctx, x, weight, att_src, att_dst, bias, prep, relu):
        h = ops.linear_fwd(x, weight, d_n=prep.d_n)                           # H = X W^T   (MFMA fp32)
        a_src, a_dst = att_src.reshape(-1), att_dst.reshape(-1)
        s_src, s_dst = ops.gat_scores(h, a_src, a_dst, d_n=prep.d_n)
        out, row_ms = ops.gat_aggregate_fwd(h, s_src, s_dst, prep, bias, relu)
        ctx.prep, ctx.relu = prep, relu
        ctx.save_for_backward(x, weight, att_src, att_dst, bias, h, s_src, s_dst, row_ms, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, att_src, att_dst, bias, h, s_src, s_dst, row_ms, out = ctx.saved_tensors
        prep = ctx.prep
        dh, da_src, da_dst, dbias = ops.gat_aggregate_bwd(dout.contiguous(), out, h, s_src, s_dst, row_ms, att_src.reshape(-1),
                                                          att_dst.reshape(-1), prep, bias, ctx.relu)
        dw = ops.linear_bwd_weight(dh, x, d_n=prep.d_n)
        dx = ops.linear_bwd_input(dh, weight, d_n=prep.d_n) if ctx.needs_input_grad[0] else None
        return dx, dw, da_src.view_as(att_src), da_dst.view_as(att_dst), dbias, None, None


def _cuda_f32(x, who: str):
    """A layer's input as the kernels take it: on the device (there is no CPU path), contiguous, fp32."""
    if not x.is_cuda:
        raise ops._lib.GrapesHipError(f"{who} input must be a cuda tensor (grapes_amd has no CPU path)")
    x = x.contiguous()
    return x if x.dtype == torch.float32 else x.float()


def _refuse_large(edge_index, who: str):
    if hasattr(edge_index, "full_graph_plan") and full_graph.use_large_path(edge_index, None):
        raise ValueError(f"{who} over a graph with 2^31 or more entries is not built: the row-blocked 64-bit path of "
                         "full_graph.py is GCN only")


def _layer_graph(edge_index, n: int, who: str, loops: bool) -> ops.PreparedGraph:
    """The graph of layer `who`: a PreparedGraph, an edge-index tensor, or a DeviceGraph below 2^31 entries — with its stored-self-loop
    counts (_gcn2_graph) for the layers that aggregate the adjacency as stored (loops: PNAConv and SAGEConv, like GCN2Conv)."""
    _refuse_large(edge_index, who)
    return _gcn2_graph(edge_index, n) if loops else prepare_edges(edge_index, n)


class GATConv(nn.Module):
    """PyG GATConv(in_channels, out_channels) with every other argument at its default, as modules/gcn.py:53-57 builds it
    [PyG-recall]: one head, LeakyReLU slope 0.2, self-loops re-added, no attention dropout, bias."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, dropout: float = 0.0, edge_dim=None):
        super().__init__()
        if heads != 1:
            raise NotImplementedError("GATConv: only heads=1 is built (the reference passes no other value)")
        if dropout:
            raise NotImplementedError("GATConv: attention dropout is not built (the reference leaves it at 0)")
        if edge_dim is not None:
            raise NotImplementedError("GATConv: edge features (edge_dim) are not built")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, 1, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, 1, out_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))    # PyG glorot
        b = math.sqrt(6.0 / (1 + self.out_channels))                   # glorot on [1, 1, C]: fan = size(-2) + size(-1)
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)
            self.att_src.uniform_(-b, b)
            self.att_dst.uniform_(-b, b)
            self.bias.zero_()

    def forward(self, x, edge_index, relu: bool = False):
        x = _cuda_f32(x, "GATConv")
        prep = _layer_graph(edge_index, x.shape[0], "GAT", loops=False)
        return _GATConvFn.apply(x, self.lin.weight, self.att_src, self.att_dst, self.bias, prep, relu)


class GAT(nn.Module):
    """modules/gcn.py:45-72: the same layer-wise adjacency routing as GCN, no dropout, and logits ONLY (gcn.py:72)."""

    def __init__(self, in_features: int, hidden_dims: "list[int]"):
        super(GAT, self).__init__()
        dims = [in_features] + hidden_dims
        gat_layers = []
        for i in range(len(hidden_dims) - 1):
            gat_layers.append(GATConv(in_channels=dims[i], out_channels=dims[i + 1]))
        gat_layers.append(GATConv(in_channels=dims[-2], out_channels=dims[-1]))
        self.gat_layers = nn.ModuleList(gat_layers)

    def forward(self, x: torch.Tensor, edge_index: Union[torch.Tensor, "list[torch.Tensor]"]) -> torch.Tensor:
        if not x.is_cuda:
            raise ops._lib.GrapesHipError("GAT input must be a cuda tensor (grapes_amd has no CPU path)")
        layerwise_adjacency = type(edge_index) == list
        n_layers = len(self.gat_layers)
        for i in range(1, n_layers):
            edges = edge_index[-i] if layerwise_adjacency else edge_index      # gcn.py:65
            x = self.gat_layers[i - 1](x, edges, relu=True)                    # gcn.py:66-67 (ReLU fused)
        edges = edge_index[0] if layerwise_adjacency else edge_index           # gcn.py:69
        return self.gat_layers[n_layers - 1](x, edges)                         # gcn.py:70,72


# ------------------------------------------------------------------------------------------------ GATv2 (PyG GATv2Conv)
class _GATv2ConvFn(torch.autograd.Function):
    """out = per-head softmax-weighted gather of x_l = lin_l(x) with the scores att . LeakyReLU(x_l[j] + x_r[i]), x_r = lin_r(x):
    grapes_linear_bias_act_fwd (one GEMM when the weights are shared, else two), grapes_gatv2_aggregate_fwd.  The backward
    recomputes scores and attention weights from x_l, x_r and the per-head (row max, log sum): nothing is stored per edge."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, b_r, att, bias, prep, heads, concat, slope, relu):
        shared = w_r is None
        x_l = ops.linear_bias_act_fwd(x, w_l, b_l, d_n=prep.d_n)              # x Wᵀ + b in the GEMM's epilogue (MFMA fp32)
        x_r = x_l if shared else ops.linear_bias_act_fwd(x, w_r, b_r, d_n=prep.d_n)
        out, agg, row_ms = ops.gatv2_aggregate_fwd(x_l, x_r, att.reshape(-1), prep, heads, concat, slope, bias, relu)
        ctx.prep, ctx.cfg = prep, (heads, concat, slope, relu, shared)
        ctx.save_for_backward(x, w_l, w_r, att, bias, x_l, x_r, row_ms, out, agg)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w_l, w_r, att, bias, x_l, x_r, row_ms, out, agg = ctx.saved_tensors
        prep, (heads, concat, slope, relu, shared) = ctx.prep, ctx.cfg
        d_n = prep.d_n
        dx_l, dx_r, datt, dbias = ops.gatv2_aggregate_bwd(dout.contiguous(), out, agg, x_l, x_r, att.reshape(-1), row_ms, prep, heads,
                                                          concat, slope, bias, relu)
        if bias is None:
            dbias = None
        need_dx = ctx.needs_input_grad[0]
        if shared:                                                             # one weight: the two contributions add
            d = ops.pna_add_input_grad(dx_l, dx_r, d_n=d_n)                    # (dx_l += dx_r, in place)
            dw_l, db_l = ops.linear_bwd_weight_gated(d, x, d_n=d_n)            # dW and the bias gradient from one GEMM
            dx = ops.linear_bwd_input(d, w_l, d_n=d_n) if need_dx else None
            return dx, dw_l, db_l, None, None, datt.view_as(att), dbias, None, None, None, None, None
        dw_l, db_l = ops.linear_bwd_weight_gated(dx_l, x, d_n=d_n)
        dw_r, db_r = ops.linear_bwd_weight_gated(dx_r, x, d_n=d_n)
        dx = None
        if need_dx:
            dx = ops.pna_add_input_grad(ops.linear_bwd_input(dx_l, w_l, d_n=d_n), ops.linear_bwd_input(dx_r, w_r, d_n=d_n), d_n=d_n)
        return dx, dw_l, db_l, dw_r, db_r, datt.view_as(att), dbias, None, None, None, None, None


class GATv2Conv(nn.Module):
    """PyG GATv2Conv [PyG-recall: torch_geometric 2.5.2]: `heads` heads of dynamic attention,
    e_ij = att . LeakyReLU(lin_l(x_j) + lin_r(x_i)), softmax per head over the incoming edges and one re-added self-loop, the heads
    side by side (concat) or averaged, + bias.  State dict: att [1, H, C], lin_l.{weight,bias}, lin_r.{weight,bias} (absent with
    share_weights), bias.  Not built (NotImplementedError): attention dropout, edge features, add_self_loops=False, another
    fill_value."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True, edge_dim=None, fill_value="mean", bias: bool = True,
                 share_weights: bool = False):
        super().__init__()
        if dropout:
            raise NotImplementedError("GATv2Conv: attention dropout is not built (the two backward passes walk different CSRs and "
                                      "share no edge id to key a mask on)")
        if edge_dim is not None:
            raise NotImplementedError("GATv2Conv: edge features (edge_dim) are not built")
        if not add_self_loops:
            raise NotImplementedError("GATv2Conv: add_self_loops=False is not built (the kernels imply one unit self-loop per node)")
        if not (isinstance(fill_value, str) and fill_value == "mean"):
            raise NotImplementedError("GATv2Conv: fill_value other than the default is not built (it fills edge features only)")
        ops._gatv2_shape(heads, out_channels)
        ops._gatv2_slope(negative_slope)
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, bool(concat)
        self.negative_slope, self.share_weights = float(negative_slope), bool(share_weights)
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=True)
        if share_weights:                       # (the same module, not registered twice: the state dict has no lin_r.* keys)
            object.__setattr__(self, "lin_r", self.lin_l)
        else:
            self.lin_r = nn.Linear(in_channels, heads * out_channels, bias=True)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.heads * self.out_channels))    # PyG glorot
        b = math.sqrt(6.0 / (self.heads + self.out_channels))                       # glorot on [1, H, C]: fan = size(-2) + size(-1)
        with torch.no_grad():
            for lin in ((self.lin_l,) if self.share_weights else (self.lin_l, self.lin_r)):
                lin.weight.uniform_(-a, a)
                lin.bias.zero_()
            self.att.uniform_(-b, b)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index, relu: bool = False):
        x = _cuda_f32(x, "GATv2Conv")
        prep = _layer_graph(edge_index, x.shape[0], "GAT", loops=False)
        shared = self.share_weights
        return _GATv2ConvFn.apply(x, self.lin_l.weight, self.lin_l.bias, None if shared else self.lin_r.weight,
                                  None if shared else self.lin_r.bias, self.att, self.bias, prep, self.heads, self.concat,
                                  self.negative_slope, relu)


class GATv2(nn.Module):
    """GAT's routing (modules/gcn.py:45-72) over GATv2Conv layers with `heads` heads: hidden layers concatenate their heads (the
    next layer's input is hidden x heads wide) with the ReLU fused, the last layer averages them; logits ONLY."""

    def __init__(self, in_features: int, hidden_dims: "list[int]", heads: int = 1):
        super(GATv2, self).__init__()
        gat_layers, d_in = [], in_features
        for hidden in hidden_dims[:-1]:
            gat_layers.append(GATv2Conv(d_in, hidden, heads=heads))
            d_in = hidden * heads
        gat_layers.append(GATv2Conv(d_in, hidden_dims[-1], heads=heads, concat=False))
        self.gat_layers = nn.ModuleList(gat_layers)

    def forward(self, x: torch.Tensor, edge_index: Union[torch.Tensor, "list[torch.Tensor]"]) -> torch.Tensor:
        if not x.is_cuda:
            raise ops._lib.GrapesHipError("GATv2 input must be a cuda tensor (grapes_amd has no CPU path)")
        layerwise_adjacency = type(edge_index) == list
        n_layers = len(self.gat_layers)
        for i in range(1, n_layers):
            edges = edge_index[-i] if layerwise_adjacency else edge_index
            x = self.gat_layers[i - 1](x, edges, relu=True)
        edges = edge_index[0] if layerwise_adjacency else edge_index
        return self.gat_layers[n_layers - 1](x, edges)


# ------------------------------------------------------------------------------------------------ GCN2 (modules/gcn.py:76-117)
class _LinearFn(torch.autograd.Function):
    """act(x Wᵀ + b): one GEMM with the bias and the ReLU in its epilogue; the backward gates by the saved output."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        out = ops.linear_bias_act_fwd(x, weight, bias, relu)
        ctx.relu = relu
        ctx.save_for_backward(x, weight, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, out = ctx.saved_tensors
        dout = dout.contiguous()
        dw, dbias = ops.linear_bwd_weight_gated(dout, x, gate=out if ctx.relu else None)
        dx = None
        if ctx.needs_input_grad[0]:
            g = ops.gcn2_mix_bwd(dout, out, True, 1.0)[0] if ctx.relu else dout
            dx = ops.linear_bwd_input(g, weight)
        return dx, dw, dbias, None


class Linear(nn.Module):
    """PyG's Linear(in_channels, out_channels) as modules/gcn.py:84-85 builds it [PyG-recall: bias=True, the initial distribution of
    nn.Linear]: keys `weight` [out, in] and `bias`."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        if out_channels < 2:
            raise ValueError("Linear: out_channels >= 2 (the fused GEMM epilogue is not built for one column)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(self.in_channels) if self.in_channels > 0 else 0.0
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, relu: bool = False):
        return _LinearFn.apply(_cuda_f32(x, "Linear"), self.weight, self.bias, relu)


class _GCN2ConvFn(torch.autograd.Function):
    """out = act((1-β) S + β S W1) with S = (1-α)(A x) + α x0 (shared weights), or the two-weight form: grapes_gcn2_propagate_fwd,
    the GEMM entry points on the square weights as stored (S W = linear_bwd_input, G Wᵀ = linear_fwd, Sᵀ G = linear_bwd_weight)
    and grapes_gcn2_mix_fwd / _bwd.  Saved for the backward: S (or P' and x0) and, with ReLU, the output; nothing of size e."""

    @staticmethod
    def forward(ctx, x, x0, w1, w2, prep, alpha, beta, relu):
        d_n = prep.d_n
        s, p = ops.gcn2_propagate_fwd(x, x0, prep, alpha, want_p=w2 is not None)
        if w2 is None:
            t1 = ops.linear_bwd_input(s, w1, d_n=d_n)                               # S W1
            out = ops.gcn2_mix_fwd(s, t1, 1.0 - beta, beta, relu=relu, d_n=d_n)
            ctx.save_for_backward(s, w1, out if relu else None)
        else:
            t1 = ops.linear_bwd_input(p, w1, d_n=d_n)                               # (1-α) P W1
            t2 = ops.linear_bwd_input(x0, w2, d_n=d_n)                              # x0 W2
            out = ops.gcn2_mix_fwd(s, t1, 1.0 - beta, beta, t2=t2, c2=beta * alpha, relu=relu, d_n=d_n)
            ctx.save_for_backward(p, x0, w1, w2, out if relu else None)
        ctx.prep, ctx.alpha, ctx.beta, ctx.relu, ctx.shared = prep, alpha, beta, relu, w2 is None
        return out

    @staticmethod
    def backward(ctx, dout):
        prep, alpha, beta, d_n = ctx.prep, ctx.alpha, ctx.beta, ctx.prep.d_n
        dout = dout.contiguous()
        if ctx.shared:
            s, w1, out = ctx.saved_tensors
            g0, g1, _ = ops.gcn2_mix_bwd(dout, out, ctx.relu, 1.0 - beta, beta, d_n=d_n)
            dw1 = ops.linear_bwd_weight(s, g1, d_n=d_n)                             # Sᵀ (β dO')
            z = ops.linear_fwd(g1, w1, d_n=d_n)                                     # (β dO') W1ᵀ
            dx, dx0 = ops.gcn2_propagate_bwd(g0, prep, alpha, ds_add=z)
            return dx, dx0, dw1, None, None, None, None, None
        p, x0, w1, w2, out = ctx.saved_tensors
        g0, g1, g2 = ops.gcn2_mix_bwd(dout, out, ctx.relu, 1.0 - beta, beta, beta * alpha, d_n=d_n)
        dw1 = ops.linear_bwd_weight(p, g1, d_n=d_n)
        dw2 = ops.linear_bwd_weight(x0, g2, d_n=d_n)
        z1 = ops.linear_fwd(g1, w1, d_n=d_n)                                        # d P'
        z2 = ops.linear_fwd(g2, w2, d_n=d_n)                                        # the x0 W2 term's share of d x0
        dx, dx0 = ops.gcn2_propagate_bwd(g0, prep, alpha, ds_add=z1, add_is_p=True, dx0_add=z2)
        return dx, dx0, dw1, dw2, None, None, None, None


def _gcn2_graph(edge_index, n: int) -> ops.PreparedGraph:
    """The layer's graph WITH its stored-self-loop counts: a PreparedGraph that carries them (ops.gcn2_attach_loops), an
    edge-index tensor (counted once, cached beside the prepared graph) or a DeviceGraph below 2^31 entries (counted from its CSR)."""
    if hasattr(edge_index, "full_graph_plan"):                 # graph.DeviceGraph
        _refuse_large(edge_index, "GCN2")
        prep = edge_index.gcn_prepared()
        if getattr(prep, "loops", None) is None:
            prep.loops = ops.gcn2_loop_counts_csr(edge_index.rowptr, edge_index.col, edge_index.num_nodes)
        return prep
    prep = prepare_edges(edge_index, n)
    if getattr(prep, "loops", None) is None and torch.is_tensor(edge_index):
        ei = edge_index.to(torch.int32)
        ops.gcn2_attach_loops(prep, ei[0].contiguous(), ei[1].contiguous())
    return prep


class GCN2Conv(nn.Module):
    """PyG GCN2Conv(channels, alpha, theta, layer, shared_weights, normalize=False) as modules/gcn.py:91-92 builds it [PyG-recall]:
    beta = log(theta / layer + 1) (1.0 when both are None), weight1 [C, C] (glorot) and, unshared, weight2; no bias.  normalize=False
    means the adjacency is used as stored: every edge once per occurrence, stored self-loops included, no loop added."""

    def __init__(self, channels: int, alpha: float, theta: Optional[float] = None, layer: Optional[int] = None,
                 shared_weights: bool = True, cached: bool = False, add_self_loops: bool = True, normalize: bool = False):
        super().__init__()
        if normalize:
            raise NotImplementedError("GCN2Conv: normalize=True (gcn_norm) is not built (the reference passes normalize=False)")
        if cached:
            raise NotImplementedError("GCN2Conv: cached=True is not built (it only matters with normalize=True)")
        if not add_self_loops:
            raise NotImplementedError("GCN2Conv: add_self_loops=False is not built (the reference leaves the default, which "
                                      "normalize=False ignores)")
        self.channels, self.alpha = channels, float(alpha)
        self.beta = 1.0 if (theta is None or layer is None) else math.log(theta / layer + 1)
        self.weight1 = nn.Parameter(torch.empty(channels, channels))
        if shared_weights:
            self.register_parameter("weight2", None)
        else:
            self.weight2 = nn.Parameter(torch.empty(channels, channels))
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (2 * self.channels))                      # PyG glorot
        with torch.no_grad():
            self.weight1.uniform_(-a, a)
            if self.weight2 is not None:
                self.weight2.uniform_(-a, a)

    def forward(self, x, x_0, edge_index, relu: bool = False):
        if not x.is_cuda or not x_0.is_cuda:
            raise ops._lib.GrapesHipError("GCN2Conv inputs must be cuda tensors (grapes_amd has no CPU path)")
        if x.shape != x_0.shape:
            raise ValueError(f"GCN2Conv: x {tuple(x.shape)} and x_0 {tuple(x_0.shape)} must have the same rows and width "
                             "(the only case modules/gcn.py:104-113 produces)")
        if x.shape[1] != self.channels:
            raise ValueError(f"GCN2Conv: width {x.shape[1]} != channels {self.channels}")
        x, x_0 = _cuda_f32(x, "GCN2Conv"), _cuda_f32(x_0, "GCN2Conv")
        prep = _gcn2_graph(edge_index, x.shape[0])
        return _GCN2ConvFn.apply(x, x_0, self.weight1, self.weight2, prep, self.alpha, self.beta, relu)


class GCN2(nn.Module):
    """modules/gcn.py:76-117, line by line: lins[0] + ReLU gives x = x_0, len(hidden_dims) GCN2Conv layers of width hidden_dims[0]
    with the layer-wise adjacency routing of GCN, dropout in front of lins[0] and of every conv, lins[1], logits ONLY (gcn.py:117).
    Only hidden_dims[0], hidden_dims[1] and len(hidden_dims) are read (as in the reference)."""

    def __init__(self, in_features: int, hidden_dims: "list[int]", alpha: float, theta: float, shared_weights=True, dropout=0.0):
        super(GCN2, self).__init__()
        self.lins = nn.ModuleList([Linear(in_features, hidden_dims[0]), Linear(hidden_dims[0], hidden_dims[1])])   # gcn.py:83-86
        self.conv = nn.ModuleList([GCN2Conv(hidden_dims[0], alpha, theta, layer + 1, shared_weights, normalize=False)
                                   for layer in range(len(hidden_dims))])                                       # gcn.py:88-94
        self.dropout = dropout
        self.philox_dropout = None          # as GCN: a callable n_elements -> (seed, offset) set by step.GrapesTrainer

    _drop = GCN._drop

    def forward(self, x: torch.Tensor, edge_index: Union[torch.Tensor, "list[torch.Tensor]"]) -> torch.Tensor:
        if not x.is_cuda:
            raise ops._lib.GrapesHipError("GCN2 input must be a cuda tensor (grapes_amd has no CPU path)")
        layerwise_adjacency = type(edge_index) == list
        x = self._drop(x)                                                      # gcn.py:103
        x = x_0 = self.lins[0](x, relu=True)                                   # gcn.py:104
        n_conv = len(self.conv)
        for i in range(1, n_conv):
            edges = edge_index[-i] if layerwise_adjacency else edge_index      # gcn.py:107
            x = self._drop(x)                                                  # gcn.py:108
            x = self.conv[i - 1](x, x_0, edges, relu=True)                     # gcn.py:109 (ReLU fused)
        edges = edge_index[0] if layerwise_adjacency else edge_index           # gcn.py:111
        x = self._drop(x)                                                      # gcn.py:112
        x = self.conv[n_conv - 1](x, x_0, edges)                               # gcn.py:113
        return self.lins[1](x)                                                 # gcn.py:115-117


# ------------------------------------------------------------------------------------------------ PNA (modules/gcn.py:120-149)
def pna_degree_histogram(graph, num_nodes: Optional[int] = None) -> torch.Tensor:
    """int64[max in-degree + 1]: entry d = number of nodes whose in-degree is d — the `deg` argument of PNAConv, as PyG's
    PNAConv.get_degree_histogram builds it from a loader [PyG-recall].  graph: a graph.DeviceGraph (rows are sources, columns
    targets; stored loops count) or an edge index [2, e] (row 1 = targets; every occurrence counts)."""
    if hasattr(graph, "rowptr") and hasattr(graph, "col"):
        dst, n = graph.col.long(), int(graph.num_nodes)
    else:
        ei = torch.as_tensor(graph)
        dst = ei[1].long().reshape(-1)
        n = int(num_nodes) if num_nodes is not None else (int(ei.max().item()) + 1 if ei.numel() else 0)
    return torch.bincount(torch.bincount(dst, minlength=n)).to(torch.int64).cpu()


def pna_degree_averages(deg) -> "tuple[float, float]":
    """(avg_log, avg_lin) = (Σ_d log(d + 1) deg[d], Σ_d d deg[d]) / Σ_d deg[d] of a degree histogram [PyG-recall:
    DegreeScalerAggregation's avg_deg]."""
    deg = torch.as_tensor(deg).detach().cpu().to(torch.float64).reshape(-1)
    total = float(deg.sum())
    if total <= 0:
        raise ValueError("PNAConv: the degree histogram is empty")
    bins = torch.arange(deg.numel(), dtype=torch.float64)
    return float(((bins + 1).log() * deg).sum()) / total, float((bins * deg).sum()) / total


class _PNAConvFn(torch.autograd.Function):
    """out = act(lin(post_nn([x_i | scaled aggregates of pre_nn([x_i | x_j])]))).  pre_nn is linear, so the messages are a_i + b_j
    with [a | b] = x [W_i ; W_j]ᵀ + [bias | 0] — ONE GEMM; grapes_pna_aggregate_fwd writes post_nn's operand in one gather pass,
    then two GEMMs with the bias (and the ReLU) in their epilogues.  Saved: x, [a | b], post_nn's operand, the statistics of b
    ([n, 6, f]), post_nn's output and, with ReLU, the output; nothing of size e."""

    @staticmethod
    def forward(ctx, x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, prep, cfg, relu):
        d_n, f = prep.d_n, x.shape[1]
        w2 = torch.cat([w_pre[:, :f], w_pre[:, f:]], 0)                           # [W_i ; W_j]: [2f, f]
        bias2 = torch.cat([b_pre, torch.zeros_like(b_pre)])
        ab = ops.linear_bias_act_fwd(x, w2, bias2, False, d_n=d_n)                 # [a | b]
        z, stats = ops.pna_aggregate_fwd(x, ab, prep, cfg)
        h = ops.linear_bias_act_fwd(z, w_post, b_post, False, d_n=d_n)             # post_nn
        out = ops.linear_bias_act_fwd(h, w_lin, b_lin, relu, d_n=d_n)              # lin (+ the model's ReLU)
        ctx.prep, ctx.cfg, ctx.relu = prep, cfg, relu
        ctx.save_for_backward(x, w2, w_post, w_lin, ab, z, stats, h, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w2, w_post, w_lin, ab, z, stats, h, out = ctx.saved_tensors
        prep, cfg, d_n, f = ctx.prep, ctx.cfg, ctx.prep.d_n, x.shape[1]
        dout = dout.contiguous()
        dw_lin, db_lin = ops.linear_bwd_weight_gated(dout, h, gate=out if ctx.relu else None, d_n=d_n)
        g = ops.gcn2_mix_bwd(dout, out, True, 1.0, d_n=d_n)[0] if ctx.relu else dout
        dh = ops.linear_bwd_input(g, w_lin, d_n=d_n)
        dw_post, db_post = ops.linear_bwd_weight_gated(dh, z, d_n=d_n)
        dz = ops.linear_bwd_input(dh, w_post, d_n=d_n)
        dab = ops.pna_aggregate_bwd(dz, ab, stats, prep, cfg)                      # [da | db]
        dw2, db2 = ops.linear_bwd_weight_gated(dab, x, d_n=d_n)
        dw_pre = torch.cat([dw2[:f], dw2[f:]], 1)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.pna_add_input_grad(ops.linear_bwd_input(dab, w2, d_n=d_n), dz, d_n=d_n)
        return dx, dw_pre, db2[:f].contiguous(), dw_post, db_post, dw_lin, db_lin, None, None, None


class PNAConv(nn.Module):
    """PyG PNAConv(in_channels, out_channels, aggregators, scalers, deg) as modules/gcn.py:130-131 builds it, every other
    argument at its default [PyG-recall]: one tower, pre_nn = Linear(2 F, F) on [x_i | x_j] per stored edge (j -> i), the
    aggregators over the incoming messages, each scaler applied to all of them, post_nn = Linear((|agg| |scal| + 1) F, C) on
    [x_i | scaled aggregates], then lin = Linear(C, C).  Keys: pre_nn / post_nn / lin .weight / .bias (PyG nests the first two as
    pre_nns.0.0 / post_nns.0.0).  The adjacency is used as stored: duplicates by multiplicity, stored loops counted, none added."""

    def __init__(self, in_channels: int, out_channels: int, aggregators, scalers, deg, edge_dim=None, towers: int = 1,
                 pre_layers: int = 1, post_layers: int = 1, divide_input: bool = False, act="relu", act_kwargs=None,
                 train_norm: bool = False):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("PNAConv: edge features (edge_dim) are not built")
        if towers != 1 or divide_input:
            raise NotImplementedError("PNAConv: only towers=1, divide_input=False is built (the reference passes no other value)")
        if pre_layers != 1 or post_layers != 1:
            raise NotImplementedError("PNAConv: only pre_layers=1 and post_layers=1 are built (one Linear each, no activation)")
        if train_norm:
            raise NotImplementedError("PNAConv: train_norm=True (learned degree averages) is not built")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.aggregators, self.scalers = list(aggregators), list(scalers)
        avg_log, avg_lin = pna_degree_averages(deg)
        self.cfg = ops.PNAConfig(self.aggregators, self.scalers, avg_log, avg_lin)
        self.avg_deg = {"log": avg_log, "lin": avg_lin}
        self.pre_nn = Linear(2 * in_channels, in_channels)
        self.post_nn = Linear(self.cfg.blocks * in_channels, out_channels)
        self.lin = Linear(out_channels, out_channels)

    def reset_parameters(self):
        for m in (self.pre_nn, self.post_nn, self.lin):
            m.reset_parameters()

    def forward(self, x, edge_index, relu: bool = False):
        x = _cuda_f32(x, "PNAConv")
        if x.shape[1] != self.in_channels:
            raise ValueError(f"PNAConv: width {x.shape[1]} != in_channels {self.in_channels}")
        prep = _layer_graph(edge_index, x.shape[0], "PNA", loops=True)
        return _PNAConvFn.apply(x, self.pre_nn.weight, self.pre_nn.bias, self.post_nn.weight, self.post_nn.bias, self.lin.weight,
                                self.lin.bias, prep, self.cfg, relu)


class PNA(nn.Module):
    """modules/gcn.py:120-149 with its constructor signature, its `conv` ModuleList (PNAConv(dims[i], dims[i + 1], ...), gcn.py:127-132)
    and its `lins = Linear(in_features, hidden_dims[-1])` (gcn.py:134), so a state dict has the reference's names.  The reference's
    forward cannot run (self.drop_input, self.dropout and self.convs are never set; lins maps in_features -> hidden_dims[-1] in
    front of a conv that expects in_features), so forward has its evident intent: dropout on the input when drop_input, for all but
    the last layer relu(conv[i - 1](x, edge_index[-i])) then dropout, the last conv on edge_index[0] (the routing of GCN / GAT /
    GCN2), logits ONLY.  Deviations from the reference text:
      * `lins` is kept as a parameter but not applied;
      * drop_input and dropout are set from the constructor's arguments;
      * batch_norm=True and residual=True are refused (the reference accepts and ignores them);
      * dropout draws from the Philox stream when a trainer hands out counters, as GCN._drop."""

    def __init__(self, in_features: int, hidden_dims: "list[int]", aggregators: "list[str]", scalers: "list[str]", deg: torch.Tensor,
                 dropout: float = 0.0, drop_input: bool = True, batch_norm: bool = False, residual: bool = False, device=None):
        super(PNA, self).__init__()
        if batch_norm:
            raise NotImplementedError("PNA: batch_norm=True is not built (the reference accepts the flag and ignores it)")
        if residual:
            raise NotImplementedError("PNA: residual=True is not built (the reference accepts the flag and ignores it)")
        dims = [in_features] + list(hidden_dims)
        self.conv = nn.ModuleList([PNAConv(in_channels=dims[i], out_channels=dims[i + 1], aggregators=aggregators, scalers=scalers,
                                           deg=deg) for i in range(len(hidden_dims))])                     # gcn.py:127-132
        self.lins = Linear(in_features, hidden_dims[-1])                                                  # gcn.py:134 (not applied)
        self.dropout, self.drop_input = dropout, bool(drop_input)
        self.philox_dropout = None          # as GCN: a callable n_elements -> (seed, offset) set by step.GrapesTrainer
        if device is not None:
            self.to(device)

    _drop = GCN._drop

    def forward(self, x: torch.Tensor, edge_index: Union[torch.Tensor, "list[torch.Tensor]"], *args) -> torch.Tensor:
        if not x.is_cuda:
            raise ops._lib.GrapesHipError("PNA input must be a cuda tensor (grapes_amd has no CPU path)")
        layerwise_adjacency = type(edge_index) == list
        if self.drop_input:
            x = self._drop(x)                                                  # gcn.py:139-140
        n_conv = len(self.conv)
        for i in range(1, n_conv):
            edges = edge_index[-i] if layerwise_adjacency else edge_index      # gcn.py:143
            x = self.conv[i - 1](x, edges, relu=True)                          # gcn.py:145 (ReLU fused)
            x = self._drop(x)                                                  # gcn.py:146
        edges = edge_index[0] if layerwise_adjacency else edge_index           # (gcn.py:148 reads edge_index[-1]: see the docstring)
        return self.conv[n_conv - 1](x, edges)


# ------------------------------------------------------------------------- GraphSAGE and Cluster-GCN (PyG SAGEConv, ClusterGCNConv)
class _RootSumConvFn(torch.autograd.Function):
    """out = act(W_a (A^ x)_i + W_r x_i + b) for a row-scaled plain-sum aggregation A^ (ops.sage_aggregate_* or ops.cluster_aggregate_*,
    handed in as `agg` = (fwd, bwd, the layer's aggr / diag_lambda: their third argument)) — linear in x, so either operand form
    computes it:
      transform-first   H = x [W_a ; W_r]ᵀ in ONE GEMM ([n, 2 out]), then the aggregation gathers the left half with the right half,
                        the bias and the ReLU in its epilogue; backward: the gated gather of dout over the by-source CSR into the
                        left half of dH with g in its right half, then dW = dHᵀ x and dx = dH W, one GEMM each.
      aggregate-first   Z = [A^ x | x] from one gather of x itself ([n, 2 in]), then ONE GEMM act(Z [W_a | W_r]ᵀ + b);
                        backward: dW and db from one gated GEMM, dZ = g W, dx = the gather of dZ's left half plus its right half.
    W_r may be None (SAGEConv's root_weight=False): the right halves are then absent.  Saved: x or Z, the stacked weight and, with
    ReLU, the output; nothing of size e."""

    @staticmethod
    def forward(ctx, x, w_a, w_r, bias, prep, agg, relu, agg_first, long_rows):
        d_n, n = prep.d_n, x.shape[0]
        f_out, f_in = w_a.shape
        ctx.prep, ctx.agg, ctx.relu, ctx.agg_first, ctx.root, ctx.long_rows = prep, agg, relu, agg_first, w_r is not None, long_rows
        ctx.f_in, ctx.f_out = f_in, f_out
        if agg_first:
            if w_r is not None:
                z = torch.empty((n, 2 * f_in), dtype=torch.float32, device=x.device)
                agg[0](x, prep, agg[2], out=z[:, :f_in], copy_out=z[:, f_in:], long_rows=long_rows)
                w = torch.cat([w_a, w_r], 1)                                   # [W_a | W_r]: [out, 2 in]
            else:
                z, w = agg[0](x, prep, agg[2], long_rows=long_rows), w_a
            out = ops.linear_bias_act_fwd(z, w, bias, relu, d_n=d_n)
            ctx.save_for_backward(z, w, out if relu else None)
            return out
        w = torch.cat([w_a, w_r], 0) if w_r is not None else w_a               # [W_a ; W_r]: [2 out, in]
        h = ops.linear_fwd(x, w, d_n=d_n)
        out = agg[0](h[:, :f_out], prep, agg[2], add=h[:, f_out:] if w_r is not None else None, bias=bias, relu=relu,
                     long_rows=long_rows)
        ctx.save_for_backward(x, w, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, w, out = ctx.saved_tensors
        prep, d_n, f_in, f_out = ctx.prep, ctx.prep.d_n, ctx.f_in, ctx.f_out
        dout = dout.contiguous()
        want_b = ctx.needs_input_grad[3]
        if ctx.agg_first:
            dw, dbias = ops.linear_bwd_weight_gated(dout, a, gate=out if ctx.relu else None, d_n=d_n, want_bias=want_b)
            dx = None
            if ctx.needs_input_grad[0]:
                g = ops.gcn2_mix_bwd(dout, out, True, 1.0, d_n=d_n)[0] if ctx.relu else dout
                dz = ops.linear_bwd_input(g, w, d_n=d_n)
                dx = ctx.agg[1](dz[:, :f_in], prep, ctx.agg[2], add=dz[:, f_in:] if ctx.root else None, long_rows=ctx.long_rows)[0]
            dw_a, dw_r = (dw[:, :f_in].contiguous(), dw[:, f_in:].contiguous()) if ctx.root else (dw, None)
            return dx, dw_a, dw_r, dbias if want_b else None, None, None, None, None, None
        dh = torch.empty((dout.shape[0], w.shape[0]), dtype=torch.float32, device=dout.device)
        _, _, dbias = ctx.agg[1](dout, prep, ctx.agg[2], relu_out=out if ctx.relu else None, dsrc=dh[:, :f_out],
                                 dadd=dh[:, f_out:] if ctx.root else None, want_bias=want_b, long_rows=ctx.long_rows)
        dw = ops.linear_bwd_weight(dh, a, d_n=d_n)
        dx = ops.linear_bwd_input(dh, w, d_n=d_n) if ctx.needs_input_grad[0] else None
        dw_a, dw_r = (dw[:f_out], dw[f_out:]) if ctx.root else (dw, None)
        return dx, dw_a, dw_r, dbias, None, None, None, None, None


class _SAGELin(nn.Module):
    """The parameters of one of SAGEConv's two linear maps under PyG's names: `weight` [out, in] and, for lin_l, `bias`."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool):
        super().__init__()
        self.in_channels = in_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))                 # [PyG-recall: Linear's default, as nn.Linear]
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_channels) if self.in_channels > 0 else 0.0
            nn.init.uniform_(self.bias, -bound, bound)


class _RootSumConv(nn.Module):
    """What SAGEConv and ClusterGCNConv share: the widths and their refusals, the choice of the operand form, forward.  A layer
    supplies its two _SAGELin maps (_lins: the aggregate's, which carries the bias, and the root's, which may be None), the graph it
    asks _layer_graph for (_GRAPH, _LOOPS) and its aggregation (_aggregation: _RootSumConvFn's `agg`)."""
    _GRAPH, _LOOPS = None, None

    def _set_widths(self, in_channels: int, out_channels: int):
        who = type(self).__name__
        if int(in_channels) < 1 or int(out_channels) < 1:
            raise ValueError(f"{who}: in_channels and out_channels are at least 1")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        if not self.form_ok("transform") and not self.form_ok("aggregate"):
            raise ValueError(f"{who}: {in_channels} -> {out_channels} is not built: the gather takes any width up to 256 and "
                             "multiples of 4 up to 1024 (out_channels, or in_channels when it is the smaller)")

    def reset_parameters(self):
        for lin in self._lins():
            if lin is not None:
                lin.reset_parameters()

    def form_ok(self, form: str) -> bool:
        """Whether an operand form can run these widths (aggregate-first also needs two output columns for its fused GEMM)."""
        if form == "aggregate":
            return ops.gather_width_ok(self.in_channels) and self.out_channels >= 2
        return ops.gather_width_ok(self.out_channels)

    def default_form(self) -> str:
        if self.in_channels < self.out_channels and self.form_ok("aggregate"):
            return "aggregate"
        return "transform" if self.form_ok("transform") else "aggregate"

    def forward(self, x, edge_index, relu: bool = False, _form: Optional[str] = None, _long_rows: Optional[bool] = None):
        who = type(self).__name__
        x = _cuda_f32(x, who)
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError(f"{who}: width {tuple(x.shape)[-1]} != in_channels {self.in_channels}")
        form = self.default_form() if _form is None else _form
        if form not in ("transform", "aggregate") or not self.form_ok(form):
            raise ValueError(f"{who}: the {form!r} form is not built for {self.in_channels} -> {self.out_channels}")
        prep = _layer_graph(edge_index, x.shape[0], self._GRAPH, loops=self._LOOPS)
        lin_a, lin_r = self._lins()
        return _RootSumConvFn.apply(x, lin_a.weight, lin_r.weight if lin_r is not None else None, lin_a.bias, prep, self._aggregation(),
                                    relu, form == "aggregate", _long_rows)


class SAGEConv(_RootSumConv):
    """PyG SAGEConv(in_channels, out_channels, aggr="mean" | "sum", root_weight=True, bias=True) [PyG-recall: torch_geometric 2.5.2]:
    out_i = W_l aggr_{j -> i} x_j + W_r x_i + b, keys `lin_l.weight`, `lin_l.bias`, `lin_r.weight` (absent with root_weight=False).
    The adjacency is used as stored: duplicates by multiplicity, stored loops are ordinary neighbours, none added; a node without a
    neighbour aggregates 0.  Not built: aggr="max" / "lstm", project=True, normalize=True, the bipartite (x_src, x_dst) call.

    The operand form is chosen by width (both compute the same map, see _RootSumConvFn): aggregate-first when in_channels <
    out_channels and in_channels is a width the gather is built for (any up to 256, multiples of 4 up to 1024) — the gather then
    moves the narrower rows; transform-first otherwise, which needs out_channels to be such a width.  forward's private `_form`
    ("transform" / "aggregate") forces one; `_long_rows` is ops.sage_aggregate_fwd's long_rows."""
    _GRAPH, _LOOPS = "SAGE", True

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "mean", normalize: bool = False, root_weight: bool = True,
                 project: bool = False, bias: bool = True):
        super().__init__()
        if aggr not in ops.SAGE_AGGRS:
            raise NotImplementedError(f"SAGEConv: aggr={aggr!r} is not built (built: {', '.join(ops.SAGE_AGGRS)}; max is not linear "
                                      "and needs its own gather)")
        if normalize or project:
            raise NotImplementedError("SAGEConv: normalize=True and project=True are not built")
        self.aggr, self.root_weight = aggr, bool(root_weight)
        self._set_widths(in_channels, out_channels)
        self.lin_l = _SAGELin(self.in_channels, self.out_channels, bias)
        if root_weight:
            self.lin_r = _SAGELin(self.in_channels, self.out_channels, False)
        else:
            self.register_module("lin_r", None)

    def _lins(self):
        return self.lin_l, self.lin_r

    def _aggregation(self):
        return ops.sage_aggregate_fwd, ops.sage_aggregate_bwd, self.aggr


class ClusterGCNConv(_RootSumConv):
    """PyG ClusterGCNConv(in_channels, out_channels, diag_lambda=0., add_self_loops=True, bias=True) [PyG-recall]:
    out_i = W_out (A^ x)_i + b + W_root x_i with A^ = D⁻¹(A + I) + diag_lambda diag(D⁻¹), D the degrees of A + I; keys `lin_out.weight`,
    `lin_out.bias`, `lin_root.weight`.  Stored self-loops are dropped before the one loop per node is added and duplicates count by
    multiplicity (PyG's remove_self_loops, add_self_loops).  Not built: add_self_loops=False.

    The operand form is chosen by width as SAGEConv's.  forward's private `_form` ("transform" / "aggregate") forces one;
    `_long_rows` is ops.cluster_aggregate_fwd's."""
    _GRAPH, _LOOPS = "ClusterGCN", False

    def __init__(self, in_channels: int, out_channels: int, diag_lambda: float = 0., add_self_loops: bool = True, bias: bool = True):
        super().__init__()
        if not add_self_loops:
            raise NotImplementedError("ClusterGCNConv: add_self_loops=False is not built (the kernels' scale is 1 / (1 + deg))")
        self.diag_lambda = float(diag_lambda)
        self._set_widths(in_channels, out_channels)
        self.lin_out = _SAGELin(self.in_channels, self.out_channels, bias)
        self.lin_root = _SAGELin(self.in_channels, self.out_channels, False)

    def _lins(self):
        return self.lin_out, self.lin_root

    def _aggregation(self):
        return ops.cluster_aggregate_fwd, ops.cluster_aggregate_bwd, self.diag_lambda


class _RootSumNet(nn.Module):
    """GCN's routing over `convs`: ReLU (fused into the layer) and dropout between the layers, edge_index[-i] for hidden layer i and
    [0] for the last when a list is given, a single tensor / DeviceGraph for every layer otherwise; logits ONLY."""
    _drop = GCN._drop

    def forward(self, x: torch.Tensor, edge_index: Union[torch.Tensor, "list[torch.Tensor]"]) -> torch.Tensor:
        if not x.is_cuda:
            raise ops._lib.GrapesHipError(f"{type(self).__name__} input must be a cuda tensor (grapes_amd has no CPU path)")
        layerwise_adjacency = type(edge_index) == list
        n_conv = len(self.convs)
        for i in range(1, n_conv):
            edges = edge_index[-i] if layerwise_adjacency else edge_index
            x = self.convs[i - 1](x, edges, relu=True)
            x = self._drop(x)
        edges = edge_index[0] if layerwise_adjacency else edge_index
        return self.convs[n_conv - 1](x, edges)


class SAGE(_RootSumNet):
    """GraphSAGE(in_features, hidden_dims, dropout=0., aggr="mean") with GCN's routing (_RootSumNet): SAGEConv(dims[i], dims[i + 1])
    layers in `convs` [PyG-recall: GraphSAGE's name].  Every layer runs over the batch's node_idx rows (no bipartite trimming)."""

    def __init__(self, in_features: int, hidden_dims: "list[int]", dropout: float = 0., aggr: str = "mean"):
        super(SAGE, self).__init__()
        dims = [in_features] + list(hidden_dims)
        self.convs = nn.ModuleList([SAGEConv(dims[i], dims[i + 1], aggr=aggr) for i in range(len(hidden_dims))])
        self.dropout, self.aggr = dropout, aggr
        self.philox_dropout = None          # as GCN: a callable n_elements -> (seed, offset)


class ClusterGCN(_RootSumNet):
    """ClusterGCN(in_features, hidden_dims, dropout=0., diag_lambda=0.) with SAGE's routing (_RootSumNet): ClusterGCNConv(dims[i],
    dims[i + 1]) layers in `convs`."""

    def __init__(self, in_features: int, hidden_dims: "list[int]", dropout: float = 0., diag_lambda: float = 0.):
        super(ClusterGCN, self).__init__()
        dims = [in_features] + list(hidden_dims)
        self.convs = nn.ModuleList([ClusterGCNConv(dims[i], dims[i + 1], diag_lambda=diag_lambda) for i in range(len(hidden_dims))])
        self.dropout, self.diag_lambda = dropout, float(diag_lambda)
        self.philox_dropout = None          # as GCN: a callable n_elements -> (seed, offset)


def classifier_layers(model) -> nn.ModuleList:
    """The conv layers of a classifier: GCN (gcn_layers), GAT or GATv2 (gat_layers), GCN2 or PNA (conv), SAGE (convs)."""
    if isinstance(model, SAGE):
        return model.convs
    if isinstance(model, (GCN2, PNA)):
        return model.conv
    return model.gat_layers if isinstance(model, (GAT, GATv2)) else model.gcn_layers


def classifier_needs_loops(model) -> bool:
    """True when the classifier counts stored self-loops (GCN2Conv with normalize=False, PNAConv): its PreparedGraphs then need
    ops.gcn2_attach_loops (the graph build drops the loops).  SAGEConv counts them too."""
    return isinstance(model, (GCN2, PNA, SAGE))


def classifier_logits(model, x, edge_index):
    """(logits, allocated MiB): GCN.forward returns the pair (gcn.py:42), GAT.forward, GCN2.forward and PNA.forward the logits alone
    (gcn.py:72,117,149), and so do GATv2.forward and SAGE.forward."""
    if isinstance(model, (GAT, GATv2, GCN2, PNA, SAGE)):
        return model(x, edge_index), _memory_allocated_mb()
    return model(x, edge_index)
