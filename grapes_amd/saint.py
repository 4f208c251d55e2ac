"""GraphSAINT training of a two-layer GCN (reference graphsaint.py:22-43, 104-121), in two forms.

* EagerSaintTrainer — the readable form: batches of a modules.saint sampler, the GCN module with autograd and
  torch.optim.Adam, exactly the reference's loop body.  Two host reads per step (the batch's node and edge counts).
* GraphedSaintTrainer — the whole step as one captured hipGraph: the draw + node set, induced subgraph, feature-row
  gather, both GCN layers forward and backward, the masked loss, the embedding-row gradient (--embed_nodes) and FusedAdam.
  Buffers are sized for the sampler's n_cap nodes and e_cap edges; every kernel reads the live counts on the device, so a step
  reads nothing back.  The status word (edge overflow, bad ids) is read once per epoch by check().

sampler = "rw" (the reference's GraphSAINTRandomWalkSampler: n_cap = B (L + 1)), "node" (GraphSAINTNodeSampler: n_cap = B) or
"edge" (GraphSAINTEdgeSampler: n_cap = 2 B); walk_length is read by "rw" alone.

Both draw from the same Philox stream (seed, device offset), so from one seed they sample the same batches.

The loss of a batch without a training row is NaN with gradients exactly zero (torch's mean over an empty selection), and the
optimiser still steps — as in the reference.

use_normalization=True with sample_coverage=K > 0 (both trainers, any sampler) trains with GraphSAINT's bias correction [PyG-recall:
PyG 2.5 examples/graph_saint.py, whose flag the reference copied]: the loader's estimate_norm(K) runs at construction (it reads the
host once per pass, so before any capture), the model runs with edge_weight = the batch's edge_norm, and the loss is
sum over the training rows of node_norm * row loss — a sum, not a mean; a batch without a training row gives 0.  The defaults
(0, False) give the step described above, launch for launch.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .modules.gcn import GCN, _WeightedGCNConvFn
from .modules.saint import make_sampler
from .target_batch import _GatherX


class _MaskedLoss(torch.autograd.Function):
    """graphsaint.py:31-34 on the device count of training rows; with node_norm the normalised step's loss (ops.saint_masked_loss)."""

    @staticmethod
    def forward(ctx, z, node_idx, count, train_mask, y, node_norm, g, loss):
        loss, g = ops.saint_masked_loss(z.contiguous(), z.shape[1], node_idx, count, train_mask, y, node_norm=node_norm, g=g, loss=loss)
        ctx.g = g
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        return ctx.g * gl, None, None, None, None, None, None, None


def masked_loss(logits, node_idx, count, train_mask, y, node_norm=None, g=None, loss=None):
    """Over the rows of `logits` whose node (node_idx) is a training node: mean CE (1-D y) / BCEWithLogits (2-D y); with node_norm
    the sum of node_norm[node] * (CE, or the mean over the columns of BCEWithLogits)."""
    return _MaskedLoss.apply(logits, node_idx, count, train_mask, y, node_norm, g, loss)


def _normalised(loader, sample_coverage, use_normalization) -> bool:
    """Validates the two arguments; with both on runs the loader's estimate and returns True."""
    cov = int(sample_coverage)
    if cov < 0:
        raise ValueError(f"sample_coverage must not be negative, not {sample_coverage!r}")
    if use_normalization and cov == 0:
        raise ValueError("use_normalization needs the coverage estimate: pass sample_coverage > 0")
    if cov and not use_normalization:
        raise ValueError("sample_coverage > 0 estimates norms that only the normalised step reads: pass use_normalization=True")
    if not use_normalization:
        return False
    loader.estimate_norm(cov)
    return True


def _weighted_gcn(model: GCN, x, ws: "ops.WeightedStructure", edge_weight):
    """GCN.forward over a prepared weighted structure (GCNConv.forward refuses edge weights with a PreparedGraph, whose edge list
    it does not have): _WeightedGCNConvFn per layer, the ReLU fused on the hidden layers, dropout as GCN.forward."""
    n_layers = len(model.gcn_layers)
    for i, layer in enumerate(model.gcn_layers):
        last = i == n_layers - 1
        x = _WeightedGCNConvFn.apply(x, layer.lin.weight, layer.bias, edge_weight, ws, not last, layer._mode, layer._fill)
        x = model._drop(x)
    return x


class EagerSaintTrainer:
    def __init__(self, graph, x, y, train_mask, model: GCN, optimizer, batch_size=256, walk_length=2, num_steps=1, seed=None,
                 e_cap=None, sampler="rw", sample_coverage=0, use_normalization=False):
        self.loader = make_sampler(sampler, graph, batch_size, walk_length, num_steps=num_steps, seed=seed, e_cap=e_cap)
        self.x, self.y, self.train_mask, self.model, self.optimizer = x, y, train_mask, model, optimizer
        self.normalised = _normalised(self.loader, sample_coverage, use_normalization)

    def step(self, *inject, **kw):
        """One step (graphsaint.py:26-36); returns (loss tensor, batch).  inject: the sampler's injected draws (roots, uniforms
        for "rw"; draws for "node" / "edge")."""
        b = self.loader.batch(*inject, **kw)
        ids = b.node_idx.to(torch.int32)
        self.optimizer.zero_grad()                                                          # graphsaint.py:29
        x = _GatherX.apply(self.x, ids, None, None, False)                                  # batch.x (data.x gathered)
        out = self.model(x, b.edge_index, edge_weight=b.edge_norm if self.normalised else None)        # graphsaint.py:31
        loss = masked_loss(out[0], ids, None, self.train_mask, self.y, self.loader.node_norm)           # graphsaint.py:32-34
        loss.backward()                                                                     # graphsaint.py:36
        self.optimizer.step()                                                               # graphsaint.py:37
        return loss.detach(), b

    def epoch(self):
        """Mean of the epoch's step losses (graphsaint.py:39-41; every batch counts data.num_nodes)."""
        tot = 0.0
        for _ in range(self.loader.num_steps):
            loss, _ = self.step()
            tot += float(loss)
        return tot / self.loader.num_steps

    def check(self):
        self.loader.check()


class GraphedSaintTrainer:
    """The step of EagerSaintTrainer as one captured graph; the optimizer must be torch.optim.Adam(capturable=True) — its state
    is stepped by ops.FusedAdam."""

    def __init__(self, graph, x, y, train_mask, model: GCN, optimizer, batch_size=256, walk_length=2, num_steps=1, seed=None,
                 e_cap=None, sampler="rw", sample_coverage=0, use_normalization=False):
        self.loader = make_sampler(sampler, graph, batch_size, walk_length, num_steps=num_steps, seed=seed, e_cap=e_cap)
        L = self.loader
        self.normalised = _normalised(L, sample_coverage, use_normalization)     # (reads the host: before the capture)
        g = L.graph
        dev = g.device
        self.x, self.y, self.train_mask, self.model, self.optimizer = x, y, train_mask, model, optimizer
        self.n_cap, self.e_cap = L.n_cap, L.e_cap
        C = model.gcn_layers[-1].out_channels
        i32 = dict(dtype=torch.int32, device=dev)
        self.draw_out = L.draw_buffers()                 # "rw": (walks, node_idx, count); else (ids, node_idx, count, entries)
        self.walk_out = self.draw_out
        if sampler == "edge":
            L.weights()                                  # the one-time table (one host read) is built before the capture
        self.sub_out = (torch.zeros(self.e_cap, **i32), torch.zeros(self.e_cap, **i32), torch.zeros(1, **i32),
                        torch.zeros(self.n_cap + 1, **i32))
        if self.normalised:                              # the edges' entry positions and norms, beside src / dst
            self.sub_out = self.sub_out + (torch.zeros(self.e_cap, dtype=torch.int64, device=dev),
                                           torch.zeros(self.e_cap, dtype=torch.float32, device=dev))
        self.xbuf = torch.zeros((self.n_cap, x.shape[1]), dtype=torch.float32, device=dev)
        self.gbuf = torch.zeros((self.n_cap, C), dtype=torch.float32, device=dev)
        self.lossbuf = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_sum = torch.zeros(1, dtype=torch.float32, device=dev)
        self.embed = isinstance(x, torch.nn.Parameter) and x.requires_grad
        self.params = [p for p in model.parameters()] + ([x] if self.embed else [])
        self.fused = ops.FusedAdam([optimizer])          # creates .grad (zeros) and the Adam state in place
        self.graph = None

    def _body(self):
        L = self.loader
        g = L.graph
        d = L.draw(out=self.draw_out)
        node_idx, count = d["node_idx"], d["count"]
        sub = ops.saint_subgraph(g.rowptr, g.col, node_idx, count, g.node_map, self.e_cap, edge_norm=L.edge_norm, status=L.status,
                                 out=self.sub_out)
        src, dst, d_e = sub[:3]
        if self.normalised:
            # The graph is the general PreparedGraph at every n_cap: ops.WeightedStructure looks every entry up by binary search
            # in the CSRs of that preparation (ascending neighbour ids per row), which the small_batch form is not specified to
            # produce.
            prep = ops.WeightedStructure(ops.PreparedGraph(src, dst, self.n_cap, d_n=count, d_e=d_e, status=L.status,
                                                           src_grouped=True), src, dst)
        elif self.n_cap <= ops._SMALL_GRAPH:
            prep = ops.PreparedGraph.small_batch([(src, dst, d_e)], self.n_cap, d_n=count, status=L.status)[0]
        else:
            prep = ops.PreparedGraph(src, dst, self.n_cap, d_n=count, d_e=d_e, status=L.status, src_grouped=True)
        for p in self.params:
            p.grad.zero_()
        xb = _GatherX.apply(self.x, node_idx, count, self.xbuf, True)
        out = _weighted_gcn(self.model, xb, prep, sub[5]) if self.normalised else self.model(xb, prep)[0]    # sub[5]: the edges' norms
        loss = masked_loss(out, node_idx, count, self.train_mask, self.y, L.node_norm, g=self.gbuf, loss=self.lossbuf)
        loss.backward()
        self.fused.step()
        self.loss_sum.add_(self.lossbuf)

    def capture(self):
        """Captures the step.  One uncounted forward / backward runs first on a side stream (lazy initialisation); the weights,
        the optimiser state and the Philox offset are as before it."""
        L = self.loader
        off0 = L.philox_offset.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            saved = [p.detach().clone() for p in self.params]
            st = [(t.clone()) for p in self.params for t in self.optimizer.state[p].values()]
            self._body()
            for p, v in zip(self.params, saved):
                p.data.copy_(v)
            it = iter(st)
            for p in self.params:
                for t in self.optimizer.state[p].values():
                    t.copy_(next(it))
            L.philox_offset.copy_(off0)
            self.loss_sum.zero_()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body()
        return self

    def step(self):
        if self.graph is None:
            self.capture()
        self.graph.replay()

    def epoch(self):
        """num_steps replays; returns the mean step loss (one host read) after check()."""
        self.loss_sum.zero_()
        for _ in range(self.loader.num_steps):
            self.step()
        self.check()
        return float(self.loss_sum.item()) / self.loader.num_steps

    def check(self):
        self.loader.check()


def build_model(F: int, hidden_dim: int, C: int, device) -> GCN:
    return GCN(F, hidden_dims=[hidden_dim, C]).to(device)                                   # graphsaint.py:115


def make_trainer(engine: str, graph, x, y, train_mask, model, lr: float, embedding_params=(), **kw):
    """graphsaint.py:116: Adam(model.parameters() + embedding_params, lr)."""
    params = list(model.parameters()) + list(embedding_params)
    if engine == "graph":
        opt = torch.optim.Adam(params, lr=lr, capturable=True)
        return GraphedSaintTrainer(graph, x, y, train_mask, model, opt, **kw)
    if engine == "eager":
        opt = torch.optim.Adam(params, lr=lr)
        return EagerSaintTrainer(graph, x, y, train_mask, model, opt, **kw)
    raise ValueError(f"engine must be graph or eager, not {engine!r}")
