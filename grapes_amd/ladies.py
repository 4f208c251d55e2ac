"""LADIES / FastGCN baseline driver: layer-wise importance sampling [LADIES-recall: acbull/LADIES pytorch_ladies.py] training
the project's GCN, the two baselines of the reference's analysis/significance.py beside GraphSAINT that one GCN stack expresses.

    python -m grapes_amd.ladies --dataset cora --sampler ladies --max_epoch 50

* Per step (LadiesTrainer, eager): modules.ladies.LayerWiseSampler draws one weighted structure per layer for a batch of training
  nodes; GCN(F, [hidden_dim, ..., C]) runs over them with every layer in ops.WGCN_UNNORMALIZED mode — out[c] = sum_e w_e H[r] + b, the
  diagonal entries as ordinary entries (the pattern of saint._weighted_gcn, with one structure per layer); the loss is
  ops.classifier_loss over the targets' rows (CrossEntropy, or BCEWithLogits for 2-D labels); Adam.  The state dict is GCN's.
* evaluate(): one full-graph propagation with P = D^-1 (A + I) itself — the graph's entries plus one appended loop per node, weights
  v_ij / D_i, the same WGCN_UNNORMALIZED layers — so inference computes what training estimates; accuracy for 1-D labels, micro-F1
  for multi-label, as graphsaint.evaluate.
* Flags: --dataset, --sampler ladies|fastgcn, --samp_num 64, --batch_size 512, --hidden_dim 256, --lr 1e-3 and --max_epoch 100
  follow the LADIES script's defaults [LADIES-recall]; --num_layers 2 (theirs is 5: the project's GCN shape is two layers),
  --eval_frequency 1, --dropout 0, --runs 1, --seed, --e_cap (a layer's entry capacity; automatic by default).  An epoch is one pass
  over a permutation of the training nodes in batches of --batch_size (their script draws --batch_num batches per epoch instead).
* Not built: LADIES' own SuGCN head (their extra linear classifier), a captured (hipGraph) step, partitioned / multi-GPU forms.
  AS-GCN, the adaptive layer-wise sampler, is grapes_amd.asgcn.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional, Sequence

import torch

from . import ops
from .main import load_data
from .modules.gcn import GCN, _WeightedGCNConvFn
from .modules.ladies import KINDS, LayerWiseSampler
from .saint import _GatherX

MAX_TARGETS = 4096                  # ops.classifier_loss: one workgroup's rows


class _TargetLoss(torch.autograd.Function):
    """ops.classifier_loss over the targets' rows of the logits; d loss / d logits is zero on every other row."""

    @staticmethod
    def forward(ctx, z, local_rows, target_ids, y):
        loss, g = ops.classifier_loss(z.contiguous(), local_rows, target_ids, y)
        ctx.g = g
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        return ctx.g * gl, None, None, None


def weighted_structures(edge_index, n: int):
    """One ops.WeightedStructure per layer's local edge list (int32 [2, e]); None for a layer without an entry."""
    out = []
    for ei in edge_index:
        if ei.shape[1] == 0:
            out.append(None)
            continue
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        out.append(ops.WeightedStructure(ops.PreparedGraph(src, dst, n), src, dst))
    return out


def layerwise_gcn(model: GCN, x, structures, edge_weight, tap=None):
    """GCN.forward's routing (hidden layer i on [-i], the last layer on [0]) with every layer as _WeightedGCNConvFn in
    WGCN_UNNORMALIZED mode; structures / edge_weight hold one entry per layer.  A layer without an entry (FastGCN drew no
    neighbour of its rows) outputs its bias.  tap: a list that receives the input of the last layer (grapes_amd.asgcn's variance
    term transforms it)."""
    n_layers = len(model.gcn_layers)
    if len(structures) != n_layers or len(edge_weight) != n_layers:
        raise ValueError(f"layerwise_gcn: {n_layers} layers take {n_layers} structures and weight vectors")
    for i, layer in enumerate(model.gcn_layers):
        last = i == n_layers - 1
        k = 0 if last else -(i + 1)
        ws, w = structures[k], edge_weight[k]
        if last and tap is not None:
            tap.append(x)
        if ws is None:
            x = layer.bias.unsqueeze(0).expand(x.shape[0], -1).contiguous()
            x = x if last else torch.relu(x)
        else:
            x = _WeightedGCNConvFn.apply(x, layer.lin.weight, layer.bias, w, ws, not last, ops.WGCN_UNNORMALIZED, 1.0)
        x = model._drop(x)
    return x


def full_graph_structure(g):
    """(WeightedStructure, weights) of P = D^-1 (A + I) over the whole graph: the stored entries (source = column, target = row)
    and one appended loop per node, each weighing 1 / D_target — a stored loop and the appended one add up to v_ii / D_i = 2 / D_i.
    Built once per graph with index arithmetic; fewer than 2^31 - N entries."""
    N, dev = g.num_nodes, g.device
    if g.nnz + N >= 2 ** 31:
        raise ValueError("LADIES / FastGCN evaluation over a graph with 2^31 or more entries is not built: the full-graph structure "
                         "has a 32-bit entry count")
    deg = g.rowptr[1:] - g.rowptr[:-1]
    ar = torch.arange(N, dtype=torch.int32, device=dev)
    row = torch.repeat_interleave(ar, deg)
    src, dst = torch.cat([g.col, ar]).contiguous(), torch.cat([row, ar]).contiguous()
    w = (1.0 / (deg + 1).to(torch.float32))[dst.long()].contiguous()
    return ops.WeightedStructure(ops.PreparedGraph(src, dst, N), src, dst), w


def evaluate(model, x, g, y, masks, structure=None):
    """The metric (accuracy, or micro-F1 for 2-D labels) of every mask from ONE full-graph forward with P."""
    from .eval import _metrics
    ws, w = structure if structure is not None else full_graph_structure(g)
    L, was = len(model.gcn_layers), model.training
    model.eval()                                                          # (no dropout at inference)
    try:
        with torch.no_grad():
            logits = layerwise_gcn(model, x, [ws] * L, [w] * L)
            return tuple(_metrics(logits[m], y[m])[0] for m in masks)
    finally:
        model.train(was)


class LadiesTrainer:
    """The eager step.  graph: a DeviceGraph (or what LayerWiseSampler takes); x fp32 [N, F]; y int64 [N] or fp32 [N, C];
    model: GCN with num_layers layers; optimizer: any torch optimiser over its parameters."""

    def __init__(self, graph, x, y, model: GCN, optimizer, samp_num: int = 64, kind: str = "ladies", seed: Optional[int] = None,
                 e_cap: Optional[int] = None):
        self.sampler = LayerWiseSampler(graph, samp_num, len(model.gcn_layers), kind=kind, seed=seed, e_cap=e_cap)
        self.x, self.y, self.model, self.optimizer = x, y, model, optimizer
        self._full = None

    def step(self, targets, uniforms=None):
        """One step on a batch of distinct target nodes (at most 4096); returns (loss tensor, batch)."""
        if targets.numel() > MAX_TARGETS:
            raise ValueError(f"LadiesTrainer.step: at most {MAX_TARGETS} targets per batch")
        b = self.sampler.sample(targets, uniforms)
        self.sampler.check()
        self.optimizer.zero_grad()
        xb = _GatherX.apply(self.x, b.node_idx, None, None, False)
        out = layerwise_gcn(self.model, xb, weighted_structures(b.edge_index, b.num_nodes), b.edge_weight)
        loss = _TargetLoss.apply(out, b.local_targets, b.targets, self.y)
        loss.backward()
        self.optimizer.step()
        return loss.detach(), b

    def epoch(self, train_nodes, batch_size: int):
        """One pass over a permutation of train_nodes in batches of batch_size; the mean of the step losses."""
        perm = train_nodes[torch.randperm(train_nodes.numel(), device=train_nodes.device)]
        tot, k = 0.0, 0
        for i in range(0, perm.numel(), batch_size):
            loss, _ = self.step(perm[i:i + batch_size])
            tot, k = tot + float(loss), k + 1
        return tot / max(k, 1)

    def evaluate(self, masks):
        if self._full is None:
            self._full = full_graph_structure(self.sampler.graph)
        return evaluate(self.model, self.x.detach(), self.sampler.graph, self.y, masks, self._full)

    def check(self):
        self.sampler.check()


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="grapes_amd.ladies", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", type=str)
    ap.add_argument("--sampler", default="ladies", choices=list(KINDS))
    ap.add_argument("--samp_num", default=64, type=int)
    ap.add_argument("--batch_size", default=512, type=int)
    ap.add_argument("--hidden_dim", default=256, type=int)
    ap.add_argument("--num_layers", default=2, type=int)
    ap.add_argument("--lr", default=1e-3, type=float)
    ap.add_argument("--max_epoch", default=100, type=int)
    ap.add_argument("--eval_frequency", default=1, type=int)
    ap.add_argument("--dropout", default=0.0, type=float)
    ap.add_argument("--runs", default=1, type=int)
    ap.add_argument("--seed", default=None, type=int)
    ap.add_argument("--e_cap", default=None, type=int)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    args = _parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    if args.dataset is None:
        raise SystemExit("--dataset is required")
    if args.num_layers < 1 or args.samp_num < 1 or not 1 <= args.batch_size <= MAX_TARGETS or args.eval_frequency < 1:
        raise ValueError(f"--num_layers, --samp_num and --eval_frequency are at least 1, --batch_size is 1 .. {MAX_TARGETS}")
    return args


def build_model(F: int, hidden_dim: int, C: int, num_layers: int, dropout: float, device) -> GCN:
    return GCN(F, hidden_dims=[hidden_dim] * (num_layers - 1) + [C], dropout=dropout).to(device)


def run(args, device=None, log=print) -> float:
    from .graph import DeviceGraph
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    data = load_data(args, device)
    if getattr(data, "rowptr", None) is not None:
        g = DeviceGraph(data.rowptr, data.col, data.num_nodes)
    else:
        g = DeviceGraph.from_edge_index(data.edge_index.to(device), data.num_nodes)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    x, y = data.x.to(device).contiguous(), data.y.to(device)
    train_mask, val_mask, test_mask = (m.to(device) for m in (data.train_mask, data.val_mask, data.test_mask))
    model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, args.dropout, device)
    tr = LadiesTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), samp_num=args.samp_num, kind=args.sampler,
                       seed=args.seed, e_cap=args.e_cap)
    train_nodes = torch.nonzero(train_mask, as_tuple=False).reshape(-1)
    val = 0.0
    for epoch in range(1, args.max_epoch + 1):
        loss = tr.epoch(train_nodes, args.batch_size)
        if epoch % args.eval_frequency == 0 or epoch == args.max_epoch:
            val, test = tr.evaluate((val_mask, test_mask))
            log(f"Epoch: {epoch:02d}, Loss: {loss:.4f}, Val: {val:.4f}, Test: {test:.4f}")
        else:
            log(f"Epoch: {epoch:02d}, Loss: {loss:.4f}")
    return val


def main(argv: Optional[Sequence[str]] = None) -> float:
    args = parse_args(argv)
    results = torch.empty(args.runs)
    for r in range(args.runs):
        results[r] = run(args)
    std = float(results.std()) if args.runs > 1 else 0.0
    print(f"Acc: {100 * float(results.mean()):.2f} ± {100 * std:.2f}")
    return float(results.mean())


if __name__ == "__main__":
    main()
