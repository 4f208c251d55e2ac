"""GraphSAGE baseline driver: node-wise neighbour sampling [Hamilton et al., NeurIPS 2017; PyG-recall: NeighborLoader + SAGEConv]
training the project's SAGE stack — the method every paper the reference cites compares against.

    python -m grapes_amd.graphsage --dataset cora --fanouts 25,10 --aggr mean --max_epoch 50

* Per step (SageTrainer, eager): modules.sage.NeighborSampler keeps at most fanouts[d] neighbours per row of layer d for a batch of
  training nodes (fanouts[0] next to the output, as PyG's num_neighbors); SAGE(F, [hidden_dim, ..., C], aggr) runs over the layers'
  local edge lists with GCN's routing; the loss is ops.classifier_loss over the targets' rows (CrossEntropy, or BCEWithLogits for
  2-D labels); Adam.  The state dict is SAGE's (convs.{i}.lin_l.weight / .bias, convs.{i}.lin_r.weight).
* evaluate(): one full-graph forward with every neighbour, over the DeviceGraph's cached preparation; accuracy for 1-D labels,
  micro-F1 for multi-label, as ladies.evaluate.
* Flags: --dataset, --fanouts 25,10 (one per layer, -1 = every neighbour, else 1 .. 64), --aggr mean|sum, --batch_size 512,
  --hidden_dim 256, --lr 1e-3, --max_epoch 100, --eval_frequency 1, --dropout 0, --runs 1, --seed; --num_layers defaults to the
  number of fanouts and must equal it.  An epoch is one pass over a permutation of the training nodes in batches of --batch_size.
* Not built: a captured (hipGraph) step, partitioned / multi-GPU forms, graphs with 2^31 or more entries, aggr max / lstm,
  sampling with replacement, PyG's bipartite (x_src, x_dst) layers — every layer runs on the batch's node_idx rows.
  `--classifier sage` in grapes_amd.main and `--model_type sage` in grapes_amd.full_batch stay refused.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional, Sequence

import torch

from . import ops
from .ladies import MAX_TARGETS, _TargetLoss
from .main import load_data
from .modules.gcn import SAGE
from .modules.sage import NeighborSampler, check_fanouts
from .saint import _GatherX


def evaluate(model: SAGE, x, g, y, masks):
    """The metric (accuracy, or micro-F1 for 2-D labels) of every mask from ONE full-graph forward with every neighbour."""
    from .eval import _metrics
    was = model.training
    model.eval()                                                          # (no dropout at inference)
    try:
        with torch.no_grad():
            logits = model(x, g)
            return tuple(_metrics(logits[m], y[m])[0] for m in masks)
    finally:
        model.train(was)


class SageTrainer:
    """The eager step.  graph: a DeviceGraph (or what NeighborSampler takes); x fp32 [N, F]; y int64 [N] or fp32 [N, C]; model: SAGE
    with len(fanouts) layers; optimizer: any torch optimiser over its parameters."""

    def __init__(self, graph, x, y, model: SAGE, optimizer, fanouts: Sequence[int] = (25, 10), seed: Optional[int] = None):
        if len(fanouts) != len(model.convs):
            raise ValueError(f"SageTrainer: {len(model.convs)} layers take {len(model.convs)} fanouts, not {len(fanouts)}")
        self.sampler = NeighborSampler(graph, fanouts, seed=seed)
        self.x, self.y, self.model, self.optimizer = x, y, model, optimizer

    def step(self, targets, keys=None):
        """One step on a batch of distinct target nodes (at most 4096); returns (loss tensor, batch)."""
        if targets.numel() > MAX_TARGETS:
            raise ValueError(f"SageTrainer.step: at most {MAX_TARGETS} targets per batch")
        b = self.sampler.sample(targets, keys)
        self.sampler.check()
        self.optimizer.zero_grad()
        xb = _GatherX.apply(self.x, b.node_idx, None, None, False)
        out = self.model(xb, b.edge_index)
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
        return evaluate(self.model, self.x.detach(), self.sampler.graph, self.y, masks)

    def check(self):
        self.sampler.check()


def _fanouts(text: str) -> "list[int]":
    try:
        return [int(t) for t in text.split(",") if t.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--fanouts takes integers separated by commas, not {text!r}")


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="grapes_amd.graphsage", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", type=str)
    ap.add_argument("--fanouts", default=[25, 10], type=_fanouts)
    ap.add_argument("--aggr", default="mean", choices=list(ops.SAGE_AGGRS))
    ap.add_argument("--batch_size", default=512, type=int)
    ap.add_argument("--hidden_dim", default=256, type=int)
    ap.add_argument("--num_layers", default=None, type=int)
    ap.add_argument("--lr", default=1e-3, type=float)
    ap.add_argument("--max_epoch", default=100, type=int)
    ap.add_argument("--eval_frequency", default=1, type=int)
    ap.add_argument("--dropout", default=0.0, type=float)
    ap.add_argument("--runs", default=1, type=int)
    ap.add_argument("--seed", default=None, type=int)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    args = _parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    if args.dataset is None:
        raise SystemExit("--dataset is required")
    args.fanouts = check_fanouts(args.fanouts)
    if args.num_layers is None:
        args.num_layers = len(args.fanouts)
    if args.num_layers != len(args.fanouts):
        raise ValueError(f"--fanouts holds one entry per layer: {len(args.fanouts)} given for --num_layers {args.num_layers}")
    if not 1 <= args.batch_size <= MAX_TARGETS or args.eval_frequency < 1 or args.hidden_dim < 1:
        raise ValueError(f"--eval_frequency and --hidden_dim are at least 1, --batch_size is 1 .. {MAX_TARGETS}")
    return args


def build_model(F: int, hidden_dim: int, C: int, num_layers: int, dropout: float, aggr: str, device) -> SAGE:
    return SAGE(F, hidden_dims=[hidden_dim] * (num_layers - 1) + [C], dropout=dropout, aggr=aggr).to(device)


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
    model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, args.dropout, args.aggr, device)
    tr = SageTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), fanouts=args.fanouts, seed=args.seed)
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
