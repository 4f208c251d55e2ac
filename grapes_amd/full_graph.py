"""Full-batch message passing over a graph with 2^31 or more CSR entries (eval.py:47-70 on ogbn-papers100M; N1).

The int32 path (DeviceGraph.gcn_prepared -> PreparedGraph) cannot hold such a graph, and the whole-graph inference form would
materialise an N x hidden activation next to N x C logits.  This path runs the classifier ROW-BLOCKED, LAYER BY LAYER, over the
graph's own int64 CSR (DeviceGraph.full_graph_plan: the CSR by target, dinv, the hub-row item count), and stores between two
layers only the operand the next aggregation reads — the rule of modules/gcn.py's aggregate-first form:

* layer l with F_in < F_out aggregates its input H_{l-1} as stored (layer 1: X itself, in place), then applies W_l in a GEMM;
* otherwise it aggregates T_l = dinv ⊙ (H_{l-1} W_lᵀ) (rows pre-scaled, as grapes_linear_fwd_row_scaled writes them), which is
  produced block by block while H_{l-1} is computed — H_{l-1} is never stored whole.

The last layer runs only over the rows the caller asks for (the evaluation mask) and each row block is reduced to predictions
at once: no N x C or |mask| x C fp32 array exists.  Widths are padded to a multiple of 4 floats (zero weight rows / columns and
zero bias), so any F and C <= 16 work.  Before anything is allocated the whole plan is compared with the free HBM
(torch.cuda.mem_get_info, after the caching allocator has returned its unused segments when the plan needs them); a plan that
does not fit raises MemoryError with the numbers instead of running out of memory halfway through.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import ops

LARGE_NNZ = 2 ** 31 - 1          # entry counts from here on need the 64-bit path (DeviceGraph.gcn_prepared refuses them)
DEFAULT_BLOCK_ROWS = 1 << 20
_I32_ELEMS = 2 ** 31 - 1         # the int32-n GEMM entry points: block_rows x width below this


def use_large_path(g, large_graph: Optional[bool]) -> bool:
    """large_graph None: automatic — the 64-bit path exactly where gcn_prepared() cannot serve the graph."""
    if large_graph is None:
        return g.nnz >= LARGE_NNZ
    return bool(large_graph)


def _pad4(f: int) -> int:
    return (f + 3) // 4 * 4


class _Layer:
    """One GCNConv with its weight / bias zero-padded to the stored widths."""

    def __init__(self, conv, relu: bool, in_stored: int):
        w, b = conv.lin.weight.detach(), conv.bias.detach()
        self.fo, self.fi = w.shape
        self.relu = relu
        self.fo_p = _pad4(self.fo)
        # aggregate-first needs a 16-byte row pitch of the stored input (X's own width for layer 1)
        self.agg_first = self.fi < self.fo and in_stored % 4 == 0
        self.in_stored = in_stored
        dev = w.device
        self.w = torch.zeros((self.fo_p, in_stored), dtype=torch.float32, device=dev)
        self.w[: self.fo, : self.fi] = w
        self.b = torch.zeros(self.fo_p, dtype=torch.float32, device=dev)
        self.b[: self.fo] = b
        # width of the operand this layer aggregates
        self.agg_width = in_stored if self.agg_first else self.fo_p


def _layers(convs: Sequence, relus: Sequence[bool], f_in: int) -> List[_Layer]:
    out, stored = [], f_in
    for conv, relu in zip(convs, relus):
        if conv.lin.weight.shape[1] != (f_in if not out else out[-1].fo):
            raise ValueError("layer widths do not chain")
        layer = _Layer(conv, relu, stored)
        out.append(layer)
        stored = layer.fo_p
    return out


def memory_plan(n: int, f_in: int, layers: List[_Layer], block_rows: int, item_cap: int, out_rows: int, out_cols: int,
                extra: int = 0) -> Tuple[int, dict]:
    """(peak bytes this pass allocates, per-part breakdown).  out_rows x out_cols: the caller's result (N x C logits of the
    module form; 0 for an evaluation, whose per-row results are counted in `extra`)."""
    stored = []                                                       # bytes of the operand each layer aggregates (0: X itself)
    for li, L in enumerate(layers):
        stored.append(0 if (li == 0 and L.agg_first) else 4 * n * L.agg_width)
    peak_operands = 0
    for li in range(len(layers)):
        nxt = stored[li + 1] if li + 1 < len(layers) else 0
        peak_operands = max(peak_operands, stored[li] + nxt)
    wmax = max([f_in] + [max(L.agg_width, L.fo_p, L.in_stored) for L in layers])
    m = min(block_rows, max(n, 1))
    agg_ws = int(ops.lib().grapes_gcn_large_aggregate_workspace_bytes(m, item_cap, wmax)) + 256
    working = 4 * 4 * m * wmax + agg_ws                               # aggregate, GEMM / dropout outputs, last block
    result = 4 * out_rows * out_cols
    parts = {"operands": peak_operands, "block_working_set": working, "result": result, "per_row_results": extra}
    return peak_operands + working + result + extra, parts


def free_bytes(device) -> int:
    """HBM the driver reports free.  Memory torch's caching allocator holds unused is not counted: its segments may be too
    fragmented for an N-row operand.  check_fits returns it to the driver first when the plan needs it."""
    free, _ = torch.cuda.mem_get_info(device)
    return int(free)


def check_fits(need: int, parts: dict, device, what: str):
    have = free_bytes(device)
    if need > have and torch.cuda.memory_reserved(device) > torch.cuda.memory_allocated(device):
        torch.cuda.empty_cache()                      # cached, unused segments back to the driver: then whole allocations
        have = free_bytes(device)
    if need > have:
        detail = ", ".join(f"{k} {v / 2**30:.2f} GiB" for k, v in parts.items())
        raise MemoryError(f"{what}: the row-blocked full-graph pass needs {need / 2**30:.2f} GiB of HBM ({detail}) but "
                          f"{have / 2**30:.2f} GiB are free; nothing was allocated")


def _block_rows(n: int, layers: List[_Layer], f_in: int, block_rows: Optional[int]) -> int:
    wmax = max([f_in] + [max(L.agg_width, L.fo_p, L.in_stored) for L in layers])
    cap = _I32_ELEMS // wmax
    # the gate-bit entry points refuse row sets of 4 GiB; the plain GEMMs used here take int32 element counts
    cap = min(cap, (4 << 30) // (4 * wmax) - 1)
    b = int(block_rows) if block_rows else DEFAULT_BLOCK_ROWS
    return max(1, min(b, cap, max(n, 1)))


def _layer_block(L: _Layer, S: torch.Tensor, plan, r0: int, m: int, rows: Optional[torch.Tensor], status) -> torch.Tensor:
    """Output rows (m x fo_p) of layer L for rows r0 .. r0+m-1 or rows[:]: aggregation (+ GEMM when aggregate-first)."""
    if L.agg_first:
        a = ops.gcn_large_aggregate(S, plan, False, r0=r0, m=m, rows=rows, status=status)
        return ops.linear_bias_act_fwd(a, L.w, L.b, L.relu)
    return ops.gcn_large_aggregate(S, plan, True, r0=r0, m=m, rows=rows, bias=L.b, relu=L.relu, status=status)


def _store_next(L_next: _Layer, h: torch.Tensor, S_next: torch.Tensor, plan, r0: int, m: int):
    """S_{l+1}[r0:r0+m] from this block's H_l: H_l itself (aggregate-first next layer) or dinv ⊙ (H_l W_{l+1}ᵀ)."""
    if L_next.agg_first:
        S_next[r0:r0 + m].copy_(h)
    else:
        ops.linear_fwd_row_scaled(h, L_next.w, plan.dinv[r0:r0 + m], out=S_next[r0:r0 + m])


def run(g, x: torch.Tensor, convs: Sequence, relus: Sequence[bool], drop: Callable, rows: Optional[torch.Tensor],
        consume: Callable, block_rows: Optional[int] = None, out_cols: int = 0, extra_bytes: int = 0,
        what: str = "full-graph pass") -> None:
    """The layer passes over the whole graph, then the last layer over `rows` (int32 ids, or None = every row in order), calling
    consume(i0, m, block) for every block of the last layer's output (m x C view, rows i0 .. i0+m-1 of the requested set)."""
    n, f_in = x.shape
    if n != g.num_nodes:
        raise ValueError("features must hold one row per node")
    if not x.is_cuda:
        raise ops._lib.GrapesHipError("full-graph pass: x must be a cuda tensor (grapes_amd has no CPU path)")
    layers = _layers(convs, relus, f_in)
    plan = g.full_graph_plan()
    B = _block_rows(n, layers, f_in, block_rows)
    convert = x.dtype != torch.float32 or not x.is_contiguous()          # (a float32 contiguous copy: part of the plan)
    need, parts = memory_plan(n, f_in, layers, B, plan.item_cap, n if out_cols else 0, out_cols,
                              extra_bytes + (4 * n * f_in if convert else 0))
    check_fits(need, parts, x.device, what)
    if convert:
        x = x.float().contiguous()
    dev = x.device
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L0 = layers[0]
    if L0.agg_first:
        S = x
    else:                                                                # T_1 = dinv ⊙ X W_1ᵀ, block by block
        S = torch.empty((n, L0.fo_p), dtype=torch.float32, device=dev)
        for r0 in range(0, n, B):
            m = min(B, n - r0)
            ops.linear_fwd_row_scaled(x[r0:r0 + m], L0.w, plan.dinv[r0:r0 + m], out=S[r0:r0 + m])
    for li in range(len(layers) - 1):                                    # hidden layers: whole graph, next operand only
        L, Ln = layers[li], layers[li + 1]
        S_next = torch.empty((n, Ln.agg_width), dtype=torch.float32, device=dev)
        for r0 in range(0, n, B):
            m = min(B, n - r0)
            h = drop(_layer_block(L, S, plan, r0, m, None, status))     # gcn.py:32-33
            _store_next(Ln, h, S_next, plan, r0, m)
            del h
        S = S_next
        del S_next
    L = layers[-1]
    total = n if rows is None else rows.numel()
    for i0 in range(0, total, B):                                        # last layer: the requested rows only
        m = min(B, total - i0)
        blk = _layer_block(L, S, plan, i0, m, None if rows is None else rows[i0:i0 + m], status)
        consume(i0, m, drop(blk[:, : L.fo]))
        del blk
    del S
    if int(status.item()):
        raise ops._lib.GrapesHipError(f"{what}: hub-row work items overflowed (a row list with repeated rows)")


def _whole(g, x, convs, relus, drop, block_rows, what) -> torch.Tensor:
    C = convs[-1].lin.weight.shape[0]
    out = {}

    def consume(i0, m, blk):
        if "t" not in out:                       # (allocated after run()'s up-front check, which counts it)
            out["t"] = torch.empty((g.num_nodes, C), dtype=torch.float32, device=x.device)
        out["t"][i0:i0 + m].copy_(blk)

    run(g, x, convs, relus, drop, None, consume, block_rows=block_rows, out_cols=C, what=what)
    return out.get("t", torch.empty((0, C), dtype=torch.float32, device=x.device))


def gcn_forward(gcn, x: torch.Tensor, g, block_rows: Optional[int] = None) -> torch.Tensor:
    """GCN.forward(x, g) on the whole graph through the row-blocked pass (inference only): the N x C logits (eval.py:50)."""
    convs = list(gcn.gcn_layers)
    return _whole(g, x, convs, [True] * (len(convs) - 1) + [False], gcn._drop, block_rows, "GCN.forward")


def conv_forward(conv, x: torch.Tensor, g, relu: bool, block_rows: Optional[int] = None) -> torch.Tensor:
    """GCNConv.forward(x, g) on the whole graph through the same kernels (inference only)."""
    return _whole(g, x, [conv], [relu], lambda t: t, block_rows, "GCNConv.forward")


def evaluate_rows(gcn, x: torch.Tensor, g, y: torch.Tensor, mask: torch.Tensor, return_predictions: bool,
                  block_rows: Optional[int] = None):
    """(accuracy, f1[, predictions]) of eval.py:47-70 with the last layer restricted to the mask rows and reduced block by block:
    argmax classes for single-label targets (accuracy = micro-F1), `logit > 0` TP / FP / FN for multi-label ones."""
    convs = list(gcn.gcn_layers)
    relus = [True] * (len(convs) - 1) + [False]
    C = convs[-1].lin.weight.shape[0]
    rows = torch.nonzero(mask, as_tuple=False).reshape(-1)
    M = rows.numel()
    multi = y.dim() != 1
    # per-row results kept: the row list (int32), the predictions (int64 classes, or the bool matrix if asked for); for one
    # label also the accuracy's temporaries after the pass (y of the mask rows, the comparison and its float32 copy)
    extra = 4 * M + (8 * M + 13 * M if not multi else (M * C if return_predictions else 0))
    acc = {"tp": 0, "fp": 0, "fn": 0}
    store = {}

    def consume(i0, m, blk):
        ids = rows[i0:i0 + m]
        if not multi:
            p = torch.argmax(blk, dim=1)                                          # eval.py:52
            if "pred" not in store:
                store["pred"] = torch.empty(M, dtype=torch.long, device=x.device)
            store["pred"][i0:i0 + m] = p
            return
        yp, yt = blk > 0, y[ids] > 0.5                                            # eval.py:58-59
        acc["tp"] += int((yt & yp).sum()); acc["fp"] += int((~yt & yp).sum()); acc["fn"] += int((yt & ~yp).sum())
        if return_predictions:
            if "pred" not in store:
                store["pred"] = torch.empty((M, C), dtype=torch.bool, device=x.device)
            store["pred"][i0:i0 + m] = yp

    rows32 = rows.to(torch.int32)
    run(g, x, convs, relus, gcn._drop, rows32, consume, block_rows=block_rows, extra_bytes=extra, what="evaluate(full_batch=True)")
    if not multi:                     # the float32 mean of eval._metrics (eval.py:54-55), on the same M predictions
        a = float((store["pred"] == y[rows]).float().mean().item()) if M else 0.0
        m_ = (a, a)
    else:
        tp, fp, fn = acc["tp"], acc["fp"], acc["fn"]
        try:
            precision, recall = tp / (tp + fp), tp / (tp + fn)
            f1 = 2 * (precision * recall) / (precision + recall)
        except ZeroDivisionError:
            f1 = 0.0
        m_ = (f1, f1)
    if return_predictions:
        pred = store.get("pred")
        if pred is None:
            pred = torch.empty((0,) if not multi else (0, C), dtype=torch.long if not multi else torch.bool, device=x.device)
        return m_ + (pred,)
    return m_
