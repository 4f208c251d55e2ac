"""PinSAGE baseline driver: importance neighbourhoods from short random walks [Ying et al., KDD 2018 — recalled; DGL-recall:
PinSAGESampler], the node-classification form — the one family whose cost per seed is independent of every degree.

    python -m grapes_amd.pinsage --dataset cora --num_neighbors 10 --num_random_walks 10 --walk_length 2 --termination_prob 0.5 --num_layers 2

* Per step (PinSAGETrainer, eager): modules.pinsage.PinSAGESampler builds --num_layers blocks, block 0 on the batch's roots and block
  d + 1 on block d's nodes — per seed --num_random_walks restarting walks of at most --walk_length steps (a walk ends before a step with
  probability --termination_prob), the --num_neighbors most visited nodes and their counts (ops.pinsage_neighbors: one launch), then
  the union and the inverted index (ops.pprgo_batch) — the model is modules.pinsage.PinSAGE: PinSAGEConv layers of --hidden_dim columns
  (visit-weighted pooling of relu(Q h + q) by ops.pprgo_aggregate_fwd, W over [self ; pooled], ops.relu_l2norm_fwd), then a linear
  head; the loss is ops.classifier_loss over the [B, C] logits; Adam.
* evaluate(): the mask's nodes run through the same sampled form in batches of --batch_size, drawn by a second sampler with its own
  fixed seed whose offset returns to 0 at every call — evaluation never moves the training stream and sees the same neighbourhoods
  every time; the model is in eval mode; accuracy for 1-D labels, micro-F1 for multi-label (eval._metrics).
* Flags: --dataset, --num_neighbors 10 (1 .. 1023), --num_random_walks 10, --walk_length 2 (their product at most 1024),
  --termination_prob 0.5 (inside [0, 1)), --num_layers 2, --batch_size 512, --hidden_dim 256, --lr 1e-3, --max_epoch 100,
  --eval_frequency 1, --dropout 0, --runs 1, --seed.
* Not built: a captured (hipGraph) step, multi-GPU forms, more than 4096 seeds in a block (the batch structure's limit: fewer roots,
  neighbours or layers), DGL's counting of returns to the root, edge weights, metapaths, bipartite item - user graphs, the max-margin
  ranking loss and hard negatives (this is the node-classification form, like every other driver here), a disk cache, node features
  with a gradient, graphs with 2^31 or more entries.  `--classifier` / `--model_type` routes in grapes_amd.main and
  grapes_amd.full_batch do not take this model.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .modules.pinsage import PinSAGE, PinSAGESampler
from .modules.sampling import draw_seed
from .target_batch import TargetBatchTrainer

EVAL_SEED = 0x915A6E                # the Philox key of evaluation's walks


class PinSAGETrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what PinSAGESampler takes) below 2^31 entries; x fp32 [N, F] without a gradient; y
    int64 [N] or fp32 [N, C]; model: modules.pinsage.PinSAGE, whose layer count is the sampler's num_layers; optimizer: any torch
    optimiser over its parameters.  num_neighbors, num_random_walks, walk_length, termination_prob: PinSAGESampler's.  seed: the
    Philox key of training's walks (None: from torch's generator).  batch_size: evaluate()'s."""

    def __init__(self, graph, x, y, model: PinSAGE, optimizer, num_neighbors: int = 10, num_random_walks: int = 10, walk_length: int = 2,
                 termination_prob: float = 0.5, batch_size: int = 512, seed: Optional[int] = None):
        if x.requires_grad:
            raise ValueError("PinSAGETrainer: node features with a gradient are not built")
        if not isinstance(model, PinSAGE):
            raise TypeError(f"PinSAGETrainer: the model is a modules.pinsage.PinSAGE, not {type(model).__name__}")
        if not 1 <= int(batch_size) <= ops.PPRGO_MAX_ROOTS:
            raise ValueError(f"PinSAGETrainer: batch_size is 1 .. {ops.PPRGO_MAX_ROOTS}")
        kw = dict(num_layers=len(model.convs), num_neighbors=num_neighbors, num_random_walks=num_random_walks, walk_length=walk_length,
                  termination_prob=termination_prob)
        super().__init__(x, y, model, optimizer, PinSAGESampler(graph, seed=draw_seed(seed), **kw))
        self.eval_sampler = PinSAGESampler(self.sampler.graph, seed=EVAL_SEED, **kw)
        self.batch_size = int(batch_size)

    def _sample(self, targets, inject):
        if inject is not None:
            raise ValueError("PinSAGETrainer.step: the walks' draws are not replaceable: there is nothing to inject")
        return self.sampler.sample(targets)

    def _forward(self, xb, b):
        return self.model(xb, b)

    def logits_of(self, nodes):
        """Logits [len(nodes), C] of the given (distinct) nodes through the evaluation sampler's blocks, in batches of batch_size."""
        s, out = self.eval_sampler, []
        for i in range(0, nodes.numel(), self.batch_size):
            b = s.sample(nodes[i:i + self.batch_size])
            s.check()
            out.append(self.model(ops.gather_rows(self.x, b.node_idx), b))
        return torch.cat(out) if out else torch.zeros((0, self.model.out_channels), device=self.x.device)

    def evaluate(self, masks):
        from .eval import _metrics
        was = self.model.training
        self.model.eval()
        self.eval_sampler.philox_offset.zero_()
        try:
            with torch.no_grad():
                res = []
                for m in masks:
                    nodes = torch.nonzero(m, as_tuple=False).reshape(-1)
                    res.append(_metrics(self.logits_of(nodes), self.y[nodes])[0])
                return tuple(res)
        finally:
            self.model.train(was)


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.pinsage", __doc__.split("\n\n")[0], num_layers=2)
    ap.add_argument("--num_neighbors", default=10, type=int)
    ap.add_argument("--num_random_walks", default=10, type=int)
    ap.add_argument("--walk_length", default=2, type=int)
    ap.add_argument("--termination_prob", default=0.5, type=float)
    args = parse_with_dataset(ap, argv)
    ops.pinsage_args(args.num_random_walks, args.walk_length, args.num_neighbors)
    ops.pinsage_term_q(args.termination_prob)
    check_ranges(args, "eval_frequency", "hidden_dim", "num_layers")
    return args


def build_model(F: int, num_classes: int, args, device) -> PinSAGE:
    return PinSAGE(F, [args.hidden_dim] * args.num_layers, num_classes, dropout=args.dropout).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], data.num_classes, args, device)
        return PinSAGETrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), num_neighbors=args.num_neighbors,
                              num_random_walks=args.num_random_walks, walk_length=args.walk_length,
                              termination_prob=args.termination_prob, batch_size=args.batch_size, seed=args.seed)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
