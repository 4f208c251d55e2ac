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
from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .modules.gcn import SAGE
from .modules.sage import NeighborSampler, check_fanouts
from .target_batch import TargetBatchTrainer, full_graph_metrics


def evaluate(model: SAGE, x, g, y, masks):
    """The metric (accuracy, or micro-F1 for 2-D labels) of every mask from ONE full-graph forward with every neighbour."""
    return full_graph_metrics(model, lambda: model(x, g), y, masks)


class SageTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what NeighborSampler takes); x fp32 [N, F]; y int64 [N] or fp32 [N, C]; model: SAGE
    with len(fanouts) layers; optimizer: any torch optimiser over its parameters."""

    def __init__(self, graph, x, y, model: SAGE, optimizer, fanouts: Sequence[int] = (25, 10), seed: Optional[int] = None):
        if len(fanouts) != len(model.convs):
            raise ValueError(f"SageTrainer: {len(model.convs)} layers take {len(model.convs)} fanouts, not {len(fanouts)}")
        super().__init__(x, y, model, optimizer, NeighborSampler(graph, fanouts, seed=seed))

    def step(self, targets, keys=None):
        """TargetBatchTrainer.step; keys: NeighborSampler.sample's."""
        return super().step(targets, keys)

    def _sample(self, targets, keys):
        return self.sampler.sample(targets, keys)

    def _forward(self, xb, b):
        return self.model(xb, b.edge_index)

    def evaluate(self, masks):
        return evaluate(self.model, self.x.detach(), self.sampler.graph, self.y, masks)


def _fanouts(text: str) -> "list[int]":
    try:
        return [int(t) for t in text.split(",") if t.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--fanouts takes integers separated by commas, not {text!r}")


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.graphsage", __doc__.split("\n\n")[0], num_layers=None)
    ap.add_argument("--fanouts", default=[25, 10], type=_fanouts)
    ap.add_argument("--aggr", default="mean", choices=list(ops.SAGE_AGGRS))
    args = parse_with_dataset(ap, argv)
    args.fanouts = check_fanouts(args.fanouts)
    if args.num_layers is None:
        args.num_layers = len(args.fanouts)
    if args.num_layers != len(args.fanouts):
        raise ValueError(f"--fanouts holds one entry per layer: {len(args.fanouts)} given for --num_layers {args.num_layers}")
    check_ranges(args, "eval_frequency", "hidden_dim")
    return args


def build_model(F: int, hidden_dim: int, C: int, num_layers: int, dropout: float, aggr: str, device) -> SAGE:
    return SAGE(F, hidden_dims=[hidden_dim] * (num_layers - 1) + [C], dropout=dropout, aggr=aggr).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, args.dropout, args.aggr, device)
        return SageTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), fanouts=args.fanouts, seed=args.seed)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
