"""The layer-wise importance samplers LADIES and FastGCN [LADIES-recall: acbull/LADIES pytorch_ladies.py, ladies_sampler /
fastgcn_sampler], the other two baselines of the reference's analysis/significance.py that one GCN stack expresses, on the gfx950
kernels of csrc/ladies_kernels.hip and the project's exact-k draw.

A is the DeviceGraph CSR, V = A + I (a stored (i, i) makes v_ii = 2), P = D^-1 V, D_i = (rowptr[i + 1] - rowptr[i]) + 1.  Layers are
drawn from the targets inward: d = 0 is the layer next to the output, prev_0 = the targets as given.

LADIES, per layer d:
  1. candidates = the ascending union of prev_d and its neighbours (the columns of P[prev_d, :] that hold an entry);
  2. pi_j = sum_{i in prev_d} P_ij^2 (ops.ladies_importance), > 0 for every candidate;
  3. s = min(#candidates, samp_num) of them without replacement in proportion to pi: ops.gumbel_topk (mode 0) on the logits
     l_j = log pi_j - C, C = 20 + log |prev_d|.  pi_j <= |prev_d|, so l_j <= -20, where log sigmoid(l) = l in fp32: the draw's keys
     are log pi_j + Gumbel noise - C, and Gumbel-top-k on those is sequential sampling without replacement in proportion to pi —
     np.random.choice(p=p, replace=False).  The sampler kernels are untouched;
  4. after_d = the ascending union of the sampled nodes and the targets;
  5. the layer's entries (i in prev_d, j in after_d, v_ij > 0) with w_ij = (v_ij / pi_j) / sum_j' (v_ij' / pi_j') (ops.ladies_layer;
     D_i, sum pi and 1 / s cancel in the row normalisation); a row without a kept column has no entries;
  6. prev_{d + 1} = after_d.
FastGCN: pi_j = sum over ALL rows i of P_ij^2, computed once at construction; every layer draws min(N, samp_num) of all N nodes;
after_d = the ascending sampled set, not unioned with the targets; the same weights.

A batch: node_idx = the ascending union of the targets and every after_d; per layer a local edge list (source j, target i: the
direction of slice_adjacency) and its weight vector, in draw order — GCN's routing (edge_index[-i] for hidden layer i, [0] for the
last) applies as is.  Rows outside a layer's prev_d get the bias only; no later layer reads them.

Set work runs on the existing index kernels (frontier_offsets / frontier_expand, bitmap_mark_lists, frontier_compact, union_sorted,
the TensorMap).  Each layer reads three counts on the host (the expansion's size, the candidate count, the entry count): this is the
eager form.  The DeviceGraph's bitmaps are zero again when sample() returns; mult is not touched.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from .. import ops
from .sampling import _graph_of, as_targets, draw_seed, local_edge_lists, raise_on_status, union_of_lists

KINDS = ("ladies", "fastgcn")


class LayerWiseSampler:
    """LayerWiseSampler(data_or_graph, samp_num, num_layers, kind="ladies" | "fastgcn", seed=None, e_cap=None).
    data_or_graph: a DeviceGraph, or a data object as the GraphSAINT samplers take.  samp_num: nodes drawn per layer.  seed: the
    Philox key of the draws (None: from torch's generator); the stream position advances by ceil(n / 4) counters per draw of n
    candidates that is not keep-all.  e_cap: the entry capacity of a layer (None: sized per layer from the rows' degrees, which
    cannot overflow); more entries set a status bit that check() raises on."""

    def __init__(self, data_or_graph, samp_num: int, num_layers: int, kind: str = "ladies", seed: Optional[int] = None,
                 e_cap: Optional[int] = None):
        if kind not in KINDS:
            raise ValueError(f"sampler must be one of {', '.join(KINDS)}, not {kind!r}")
        if int(samp_num) < 1 or int(num_layers) < 1:
            raise ValueError("LayerWiseSampler: samp_num and num_layers are at least 1")
        self.kind, self.samp_num, self.num_layers = kind, int(samp_num), int(num_layers)
        self.graph, self.data = _graph_of(data_or_graph)
        g = self.graph
        if g.nnz >= 2 ** 31:
            raise ValueError("LADIES / FastGCN sampling over a graph with 2^31 or more entries is not built: the row degrees and the "
                             "layer's entry offsets are 32-bit")
        dev, N = g.device, g.num_nodes
        self.e_cap = None if e_cap is None else int(e_cap)
        self.seed, self.philox_offset = draw_seed(seed), 0
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        flag = ops.csr_symmetric_check(g.rowptr, g.col, N)
        if flag & 2:
            raise ops._lib.GrapesHipError("LayerWiseSampler: a column id is outside [0, num_nodes)")
        self.symmetric = flag == 0
        self.rowptr_t, self.col_t = (g.rowptr, g.col) if self.symmetric else ops.csr_transpose(g.rowptr, g.col, N, status=self.status)
        self.pi_table = torch.zeros(N, dtype=torch.float32, device=dev)
        self.global_pi = self.global_logit = None
        if kind == "fastgcn":
            self.global_pi, self.global_logit = ops.ladies_importance(g.rowptr, self.rowptr_t, self.col_t, N, pi_table=self.pi_table,
                                                                      status=self.status)

    # ------------------------------------------------------------------ set work
    def _union(self, lists):
        return union_of_lists(self.graph, lists, self.status)

    def _uniforms(self, n: int):
        u = ops.philox_uniform(n, self.seed, self.philox_offset, self.graph.device)
        self.philox_offset += (n + 3) // 4
        return u

    def _draw(self, logit, cand, n: int, uniforms):
        """The ascending ids of min(n, samp_num) candidates drawn in proportion to exp(logit) (cand None: position = id)."""
        if cand is None:
            cand = self._all_ids()
        if n <= self.samp_num:
            return cand[:n]
        u = uniforms if uniforms is not None else self._uniforms(n)
        res = ops.gumbel_topk(logit, self.samp_num, uniforms=u, candidate_ids=cand, n=n, mode=0, want_log_prob=False, want_stats=False)
        return res["kept_ids"]

    def _all_ids(self):
        if getattr(self, "_arange", None) is None:
            self._arange = torch.arange(self.graph.num_nodes, dtype=torch.int32, device=self.graph.device)
        return self._arange

    # ------------------------------------------------------------------ what a subclass with another importance replaces
    def _importance(self, cand, m: int):
        """(pi, logit, further per-layer fields) over the candidates of a layer whose m rows are marked in prev_bits; pi is also
        written to pi_table, which the layer's weights read."""
        g = self.graph
        pi, logit = ops.ladies_importance(g.rowptr, self.rowptr_t, self.col_t, g.num_nodes, ids=cand, prev_bits=g.prev_bits, m=m,
                                          pi_table=self.pi_table, status=self.status)
        return pi, logit, {}

    def _batch_fields(self, node_idx, layers) -> dict:
        """Further fields of the batch's namespace (node_map holds node_idx's ranks when this is called)."""
        return {}

    # ------------------------------------------------------------------ one batch
    def sample(self, targets, uniforms=None) -> SimpleNamespace:
        """targets: node ids (any integer tensor; taken in the given order).  uniforms: per layer one fp32 tensor with at least as
        many values as the layer has candidates (N for FastGCN), replacing the Philox draws (tests); None entries and layers past
        the list draw from the stream.  Returns a namespace: node_idx (int32, ascending), num_nodes, targets (int32), local_targets
        (the targets' rows in node_idx), edge_index (list of int32 [2, e_d], local ids, row 0 the sources), edge_weight (list of fp32
        [e_d]) and layers: per layer a namespace of prev, candidates (None for FastGCN: every node), pi, logit, sampled, after,
        edge_src, edge_dst (global ids) and weight."""
        g = self.graph
        dev, N = g.device, g.num_nodes
        targets = as_targets(targets, dev, "LayerWiseSampler")
        uniforms = list(uniforms) if uniforms is not None else []
        prev, layers = targets, []
        for d in range(self.num_layers):
            m = prev.numel()
            u = uniforms[d] if d < len(uniforms) else None
            eoff, d_e = ops.frontier_offsets(g.rowptr, prev)
            deg_sum = int(d_e.item())                                    # the rows' entry count (host read)
            if self.kind == "ladies":
                lists = [(prev, None)]
                if deg_sum > 0:
                    _, nbr, _ = ops.frontier_expand(g.rowptr, g.col, prev, eoff, deg_sum, status=self.status)
                    lists.append((nbr, None))
                ops.bitmap_mark_lists(g.bits, None, lists, N, status=self.status)
                cand_buf, _, _, counts = ops.frontier_compact(g.bits, None, None, N, min(m + deg_sum, N), status=self.status)
                n = int(counts[0].item())                                # the candidate count (host read)
                cand = cand_buf[:n]
                ops.bitmap_mark_lists(g.prev_bits, None, [(prev, None)], N, status=self.status)
                pi, logit, extra = self._importance(cand, m)
                ops.bitmap_clear(g.prev_bits, prev)
                sampled = self._draw(logit, cand, n, u)
                after = self._union([sampled, targets])
            else:
                cand, pi, logit, extra = None, self.global_pi, self.global_logit, {}
                sampled = self._draw(logit, None, N, u)
                after = sampled
            e_cap = self.e_cap if self.e_cap is not None else max(1, min(deg_sum + m, m * after.numel()))
            ops.bitmap_mark_lists(g.bits, None, [(after, None)], N, status=self.status)
            src, dst, w, d_l = ops.ladies_layer(g.rowptr, g.col, N, prev, g.bits, self.pi_table, e_cap, status=self.status)
            ops.bitmap_clear(g.bits, after)
            e = int(d_l.item())                                          # the layer's entry count (host read)
            layers.append(SimpleNamespace(prev=prev, candidates=cand, pi=pi, logit=logit, sampled=sampled, after=after,
                                          edge_src=src[:e], edge_dst=dst[:e], weight=w[:e], **extra))
            prev = after
        node_idx = self._union([targets] + [L.after for L in layers])     # (also node_map[id] = rank)
        edge_index = local_edge_lists(g, layers, dev)
        return SimpleNamespace(node_idx=node_idx, num_nodes=node_idx.numel(), targets=targets,
                               local_targets=ops.tensormap_map(g.node_map, targets), edge_index=edge_index,
                               edge_weight=[L.weight for L in layers], layers=layers, **self._batch_fields(node_idx, layers))

    def check(self):
        """Reads the status word (synchronises); raises GrapesHipError on an edge overflow or a bad id, and clears it (and, as
        DeviceGraph.check_status does, the bitmaps a truncated batch may have left marked)."""
        raise_on_status(self.status, f"{getattr(self, '_name', self.kind)} sampler", graph=self.graph,
                        hints={1: " (raise e_cap)"})
