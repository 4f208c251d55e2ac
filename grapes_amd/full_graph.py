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

train_step (full-batch.py:100-105) trains a two-layer GCN on such graphs with the same pieces: AX stored, T2 per block, the loss on
the train rows only, and a backward pass over the sources of the train rows' entries.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import ops
from .modules.sampling import draw_seed

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


# ---------------------------------------------------------------------------------------------- full-batch training
# measurement only (profiles/bench_fullbatch_train.py): a dict here receives the phase boundaries of the next train_step as
# device events ("phases": [(name, event)]) and the row-list sizes ("sources", "entries")
PROFILE: Optional[dict] = None


def _mark(name: str):
    if PROFILE is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        PROFILE.setdefault("phases", []).append((name, ev))


def _dropout_streams(gcn, n: int, h: int, c: int):
    """(p, (seed, offset) of the N x H mask, (seed, offset) of the N x C mask) of one training step, in the module's order.
    With gcn.philox_dropout set the counters come from it (the masks of the int32 autograd path under the same hook);
    otherwise the seed is drawn from torch's default generator, so torch.manual_seed makes a run reproducible."""
    p = float(gcn.dropout) if gcn.training else 0.0
    if p <= 0.0:
        return 0.0, (0, 0), (0, 0)
    if gcn.philox_dropout is not None:
        return p, gcn.philox_dropout(n * h), gcn.philox_dropout(n * c)
    seed = draw_seed(None)
    return p, (seed, 0), (seed, (n * h + 3) // 4)


def _row_ids(sel, n: int, dev) -> torch.Tensor:
    """Ascending int32 row ids of a bool mask, or an index tensor as given."""
    sel = sel.to(dev)
    if sel.dtype == torch.bool:
        if sel.numel() != n:
            raise ValueError("a row mask must hold one entry per node")
        sel = torch.nonzero(sel, as_tuple=False).reshape(-1)
    return sel.to(torch.int32).contiguous()


def train_memory_plan(n: int, f: int, h: int, c: int, m_train: int, m_eval: int, block_rows: int, item_cap: int,
                      transpose_bytes: int, entries_cap: int, chunk: int, convert_x: bool) -> Tuple[int, dict]:
    """(peak bytes train_step allocates, per-part breakdown).  Everything is counted as alive at once: the stored AX, T2 (whose
    storage then holds dU2), the loss rows' logits (then their gradient G), the evaluation rows' logits, the row-list
    transpose with its workspace, the transposed gather's and the aggregation's workspaces and one block's working set."""
    fp, hp, cp = _pad4(f), _pad4(h), _pad4(c)
    B = min(block_rows, max(n, 1))
    parts = {
        "x_padded": 4 * n * fp if convert_x else 0,
        "ax": 4 * n * fp,
        "t2": 4 * n * cp,
        "train_logits": 4 * m_train * cp + int(ops.lib().grapes_rowlist_loss_workspace_bytes(max(m_train, 1), cp)) + 512,
        "eval_logits": 4 * m_eval * cp,
        "row_list_transpose": transpose_bytes,
        "transposed_gather": ops.rowlist_gather_t_workspace_bytes(min(n, entries_cap),
                                                                  ops.rowlist_gather_t_item_cap(entries_cap, chunk), cp),
        "aggregate_workspace": int(ops.lib().grapes_gcn_large_aggregate_workspace_bytes(B, item_cap, max(fp, cp))) + 256,
        # gathered AX rows, H1, its dropout, dH1 (each B x width) and the GEMMs' split-K slabs
        "block_working_set": 4 * B * (fp + 3 * hp + cp) + (64 << 20),
        "gradients": 4 * (hp * fp + hp + cp * hp + cp) * 2,
    }
    return sum(parts.values()), parts


def _accumulate_grad(param: torch.Tensor, g: torch.Tensor):
    if param.grad is None:
        param.grad = g.detach().clone()
    else:
        param.grad.add_(g)


def _autograd_loss(logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    if y.dim() == 1:
        return torch.nn.functional.cross_entropy(logits, y)                   # full-batch.py:80 CrossEntropyLoss
    return torch.nn.functional.binary_cross_entropy_with_logits(logits, y.float())   # full-batch.py:82 BCEWithLogitsLoss


def train_step(gcn, x: torch.Tensor, g, y: torch.Tensor, train_mask: torch.Tensor, eval_rows: Optional[torch.Tensor] = None,
               block_rows: Optional[int] = None, large_graph: Optional[bool] = None):
    """One full-batch training step of a two-layer GCN over the whole DeviceGraph (full-batch.py:100-105): forward, the mean loss
    over the train rows and the backward pass, ACCUMULATED into p.grad of the module's parameters as loss.backward() would; the
    caller's optimiser then steps.  -> (loss, 0-d device tensor; logits of eval_rows [|eval_rows|, C] after dropout, or None).

    large_graph None: graphs with 2^31 or more CSR entries take the row-blocked 64-bit path below, smaller ones the int32
    autograd path (gcn(x, g), loss, backward); True forces the row-blocked path on any graph.  That path:
      forward   AX = Â X stored (layer 1 aggregate-first, X's columns padded to a multiple of 4), then per row block
                H1 = relu(AX W1ᵀ + b1), H1d = dropout(H1), T2 = dinv ⊙ (H1d W2ᵀ); Z = Â T2 + b2 on the train (and eval) rows only;
      loss      grapes_rowlist_loss: the loss, G = dinv ⊙ dZ (dropout's backward fused) and db2;
      backward  the row-list transpose gives the sources S of the train rows' entries; dU2 = dinv[S] ⊙ (Âᵀ-gather of G) is
                written over T2's storage; per block of S, H1[S] and its mask are recomputed from AX[S], then
                dW2 += dU2ᵀ H1d, dH1 = (dU2 W2) ⊙ mask / (1 - p), dW1 += (dH1 ⊙ [H1 > 0])ᵀ AX[S], db1 += its column sums.
    Rows outside S contribute exactly zero to every gradient, so no work is spent on them.  x needs no gradient."""
    convs = list(gcn.gcn_layers)
    n = g.num_nodes
    dev = x.device
    if not use_large_path(g, large_graph):
        logits, _ = gcn(x, g, large_graph=False)
        tr = _row_ids(train_mask, n, dev).long()
        loss = _autograd_loss(logits[tr], y.to(dev)[tr])
        loss.backward()
        ev = None if eval_rows is None else logits.detach()[_row_ids(eval_rows, n, dev).long()]
        return loss.detach(), ev
    if len(convs) != 2:
        raise ValueError(f"full-batch training on the row-blocked path takes a two-layer GCN (full-batch.py:72-74), got "
                         f"{len(convs)} layers")
    if not x.is_cuda:
        raise ops._lib.GrapesHipError("train_step: x must be a cuda tensor (grapes_amd has no CPU path)")
    if x.requires_grad:
        raise ValueError("train_step: x must not require a gradient (full-batch.py has no learned embeddings)")
    N, F = x.shape
    if N != n:
        raise ValueError("features must hold one row per node")
    c1, c2 = convs
    W1, b1, W2, b2 = c1.lin.weight, c1.bias, c2.lin.weight, c2.bias
    H, C = W1.shape[0], W2.shape[0]
    if W1.shape[1] != F or W2.shape[1] != H:
        raise ValueError("layer widths do not chain")
    Fp, Hp, Cp = _pad4(F), _pad4(H), _pad4(C)
    if Cp > 1024:
        raise ValueError("train_step: at most 1024 classes on the row-blocked path")
    multi = y.dim() != 1
    plan = g.full_graph_plan()
    R = _row_ids(train_mask, n, dev)
    E = None if eval_rows is None else _row_ids(eval_rows, n, dev)
    M, Me = R.numel(), (0 if E is None else E.numel())
    if M == 0:
        raise ValueError("train_step: the training split is empty")
    wmax = max(Fp, Hp, Cp)
    B = max(1, min(int(block_rows) if block_rows else DEFAULT_BLOCK_ROWS, _I32_ELEMS // wmax, (4 << 30) // (4 * wmax) - 1, n))
    e_cap = ops.rowlist_entries_cap(plan, R)
    convert = x.dtype != torch.float32 or not x.is_contiguous() or F != Fp
    need, parts = train_memory_plan(n, F, H, C, M, Me, B, plan.item_cap, ops.rowlist_transpose_bytes(plan, e_cap), e_cap,
                                   plan.chunk, convert)
    check_fits(need, parts, dev, "full_graph.train_step")
    p, (s1, o1), (s2, o2) = _dropout_streams(gcn, n, H, C)
    labels = y.to(dev)
    labels = labels.float().contiguous() if multi else labels.long().contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.no_grad():
        if convert:
            xs = torch.zeros((n, Fp), dtype=torch.float32, device=dev)
            xs[:, :F] = x
        else:
            xs = x
        w1 = torch.zeros((Hp, Fp), dtype=torch.float32, device=dev); w1[:H, :F] = W1
        bb1 = torch.zeros(Hp, dtype=torch.float32, device=dev); bb1[:H] = b1
        w2 = torch.zeros((Cp, Hp), dtype=torch.float32, device=dev); w2[:C, :H] = W2
        bb2 = torch.zeros(Cp, dtype=torch.float32, device=dev); bb2[:C] = b2
        # ---- forward: AX stored, T2 block by block
        _mark("start")
        AX = torch.empty((n, Fp), dtype=torch.float32, device=dev)
        for r0 in range(0, n, B):
            m = min(B, n - r0)
            ops.gcn_large_aggregate(xs, plan, False, r0=r0, m=m, out=AX[r0:r0 + m], status=status)
        if convert:
            del xs
        _mark("aggregate_x")
        T2 = torch.empty((n, Cp), dtype=torch.float32, device=dev)
        for r0 in range(0, n, B):
            m = min(B, n - r0)
            h1 = ops.linear_bias_act_fwd(AX[r0:r0 + m], w1, bb1, True)
            if p > 0.0:
                ops.dropout_rows(h1, H, p, s1, o1, r0=r0, out=h1)
            ops.linear_fwd_row_scaled(h1, w2, plan.dinv[r0:r0 + m], out=T2[r0:r0 + m])
            del h1
        _mark("layer1_t2")
        ev = None
        if E is not None:                                                  # full-batch.py:117: this epoch's logits
            Ze = torch.empty((Me, Cp), dtype=torch.float32, device=dev)
            for i0 in range(0, Me, B):
                m = min(B, Me - i0)
                ops.gcn_large_aggregate(T2, plan, True, rows=E[i0:i0 + m], bias=bb2, out=Ze[i0:i0 + m], status=status)
            if p > 0.0 and Me:
                ops.dropout_rows(Ze, C, p, s2, o2, rows=E, out=Ze)
            ev = Ze[:, :C]
        Z = torch.empty((M, Cp), dtype=torch.float32, device=dev)
        for i0 in range(0, M, B):
            m = min(B, M - i0)
            ops.gcn_large_aggregate(T2, plan, True, rows=R[i0:i0 + m], bias=bb2, out=Z[i0:i0 + m], status=status)
        loss, G, db2 = ops.rowlist_loss(Z, C, R, labels, plan.dinv, p, s2, o2, g=Z, status=status)
        _mark("layer2_rows_loss")
        # ---- backward: dU2 on the sources S over T2's storage
        srcs, src_off, pos = ops.rowlist_transpose(plan, R, e_cap, status=status)
        nS = srcs.numel()
        _mark("row_list_transpose")
        if PROFILE is not None:
            PROFILE["sources"], PROFILE["entries"] = nS, pos.numel()
        dU2 = T2.view(-1)[: nS * Cp].view(nS, Cp)
        ops.rowlist_gather_t(G, srcs, src_off, pos, plan.dinv, plan.chunk, out=dU2, status=status)
        _mark("transposed_gather")
        del Z, G, pos, src_off
        dW1 = torch.zeros((Hp, Fp), dtype=torch.float32, device=dev)
        db1 = torch.zeros(Hp, dtype=torch.float32, device=dev)
        dW2 = torch.zeros((Cp, Hp), dtype=torch.float32, device=dev)
        for j0 in range(0, nS, B):
            m = min(B, nS - j0)
            ids = srcs[j0:j0 + m]
            axs = ops.gather_rows(AX, ids)
            h1 = ops.linear_bias_act_fwd(axs, w1, bb1, True)                # H1[S] recomputed (not stored: N x H)
            h1d = ops.dropout_rows(h1, H, p, s1, o1, rows=ids) if p > 0.0 else h1
            du = dU2[j0:j0 + m]
            ops.linear_bwd_weight(du, h1d, out=dW2, accumulate=True)
            del h1d
            dh = ops.linear_bwd_input(du, w2)
            if p > 0.0:
                ops.dropout_rows(dh, H, p, s1, o1, rows=ids, out=dh)
            ops.linear_bwd_weight_gated(dh, axs, gate=h1, dw=dW1, dbias=db1, accumulate=True)
            del axs, h1, dh
        _mark("recompute_weight_grads")
        del dU2, T2, AX, srcs
        if int(status.item()):
            raise ops._lib.GrapesHipError(f"full_graph.train_step: status {int(status.item())} (a label outside [0, C), a bad row "
                                          "id or hub-row work items overflowed)")
        _accumulate_grad(W1, dW1[:H, :F]); _accumulate_grad(b1, db1[:H])
        _accumulate_grad(W2, dW2[:C, :H]); _accumulate_grad(b2, db2[:C])
    return loss.reshape(()), ev
