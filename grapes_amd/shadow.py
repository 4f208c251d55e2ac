"""ShaDow-GNN baseline driver: per-root sampled ego-nets [Zeng et al., NeurIPS 2021; PyG-recall: ShaDowKHopSampler, examples/shadow.py]
training a GNN whose depth is independent of its scope — the family that decouples the two.

    python -m grapes_amd.shadow --dataset cora --depth 2 --num_neighbors 10 --num_layers 3 --conv sage --pool true

* Per step (ShadowTrainer, eager): modules.shadow.ShaDowKHopSampler draws one ego-net per training node of the batch (--depth hops, at
  most --num_neighbors entries per expanded row, then the induced subgraph) and concatenates them; the model is modules.shadow.ShaDow —
  SAGE or GCN with --num_layers layers of --hidden_dim columns over the union, the root's row (with --pool true also the mean over its
  ego-net) as the readout, Linear as the head; the loss is ops.classifier_loss over the [B, C] logits; Adam.
* evaluate(): the mask's nodes run through ego-nets in batches of --batch_size, drawn by a second sampler with its own fixed seed that
  starts from offset 0 at every call — evaluation never moves the training stream and sees the same ego-nets every time; the model is
  in eval mode; accuracy for 1-D labels, micro-F1 for multi-label (eval._metrics).
* Flags: --dataset, --depth 2, --num_neighbors 10 (1 .. 64, one value for every hop), --num_layers 3, --conv sage|gcn, --pool true|false,
  --batch_size 512, --hidden_dim 256, --lr 1e-3, --max_epoch 100, --eval_frequency 1, --dropout 0, --runs 1, --seed.
  1 + k + ... + k^depth, the most nodes of one ego-net, must not exceed 1024: the check runs when the flags are parsed.
* Not built: a captured (hipGraph) step, partitioned / multi-GPU forms, PPR-based scopes (the paper's other sampler), per-hop fanouts,
  sampling with replacement, node features with a gradient (node_idx repeats nodes across ego-nets), graphs with 2^31 or more entries.
  `--classifier` / `--model_type` routes in grapes_amd.main and grapes_amd.full_batch do not take this sampler.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .modules.shadow import ShaDow, ShaDowKHopSampler
from .target_batch import TargetBatchTrainer

EVAL_SEED = 0x5ADE                  # the Philox key of evaluation's ego-nets


class ShadowTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what ShaDowKHopSampler takes); x fp32 [N, F] without a gradient; y int64 [N] or fp32
    [N, C]; model: modules.shadow.ShaDow; optimizer: any torch optimiser over its parameters; batch_size: evaluate()'s."""

    def __init__(self, graph, x, y, model: ShaDow, optimizer, depth: int = 2, num_neighbors: int = 10, batch_size: int = 512,
                 seed: Optional[int] = None):
        if x.requires_grad:
            raise ValueError("ShadowTrainer: node features with a gradient are not built: node_idx repeats nodes across ego-nets")
        if not 1 <= int(batch_size) <= ops.SHADOW_MAX_ROOTS:
            raise ValueError(f"ShadowTrainer: batch_size is 1 .. {ops.SHADOW_MAX_ROOTS}")
        super().__init__(x, y, model, optimizer, ShaDowKHopSampler(graph, depth, num_neighbors, seed=seed))
        self.batch_size = int(batch_size)
        self.eval_sampler = ShaDowKHopSampler(self.sampler.graph, depth, num_neighbors, seed=EVAL_SEED)

    def step(self, targets, words=None):
        """TargetBatchTrainer.step; words: ShaDowKHopSampler.sample's."""
        return super().step(targets, words)

    def _sample(self, targets, words):
        return self.sampler.sample(targets, words)

    def _forward(self, xb, b):
        return self.model(xb, b)

    def logits_of(self, nodes):
        """Logits [len(nodes), C] of the given nodes through the evaluation sampler's ego-nets, in batches of batch_size."""
        s, out = self.eval_sampler, []
        for i in range(0, nodes.numel(), self.batch_size):
            b = s.sample(nodes[i:i + self.batch_size])
            s.check()
            out.append(self.model(ops.gather_rows(self.x, b.node_idx), b))
        return torch.cat(out) if out else torch.zeros((0, self.model.head.out_channels), device=self.x.device)

    def evaluate(self, masks):
        from .eval import _metrics
        was = self.model.training
        self.model.eval()
        self.eval_sampler.philox_offset = 0
        try:
            with torch.no_grad():
                res = []
                for m in masks:
                    nodes = torch.nonzero(m, as_tuple=False).reshape(-1)
                    res.append(_metrics(self.logits_of(nodes), self.y[nodes])[0])
                return tuple(res)
        finally:
            self.model.train(was)


def _bool(text: str) -> bool:
    if text.lower() in ("true", "1", "yes"):
        return True
    if text.lower() in ("false", "0", "no"):
        return False
    raise argparse.ArgumentTypeError(f"--pool takes true or false, not {text!r}")


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.shadow", __doc__.split("\n\n")[0], num_layers=3)
    ap.add_argument("--depth", default=2, type=int)
    ap.add_argument("--num_neighbors", default=10, type=int)
    ap.add_argument("--conv", default="sage", choices=["sage", "gcn"])
    ap.add_argument("--pool", default=True, type=_bool)
    args = parse_with_dataset(ap, argv)
    ops.shadow_cap(args.depth, args.num_neighbors)
    check_ranges(args, "eval_frequency", "hidden_dim", "num_layers")
    return args


def build_model(F: int, num_classes: int, args, device) -> ShaDow:
    return ShaDow(F, args.hidden_dim, num_classes, args.num_layers, conv=args.conv, pool=args.pool, dropout=args.dropout).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], data.num_classes, args, device)
        return ShadowTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), depth=args.depth,
                             num_neighbors=args.num_neighbors, batch_size=args.batch_size, seed=args.seed)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
