"""ShaDow-GNN baseline driver: per-root sampled ego-nets [Zeng et al., NeurIPS 2021; PyG-recall: ShaDowKHopSampler, examples/shadow.py]
training a GNN whose depth is independent of its scope — the family that decouples the two.

    python -m grapes_amd.shadow --dataset cora --depth 2 --num_neighbors 10 --num_layers 3 --conv sage --pool true
    python -m grapes_amd.shadow --dataset cora --scope ppr --ppr_k 200 --ppr_alpha 0.25 --ppr_eps 6.1e-5 --num_layers 3

* Per step (ShadowTrainer, eager): modules.shadow.ShaDowKHopSampler draws one ego-net per training node of the batch (--depth hops, at
  most --num_neighbors entries per expanded row, then the induced subgraph) and concatenates them; the model is modules.shadow.ShaDow —
  SAGE or GCN with --num_layers layers of --hidden_dim columns over the union, the root's row (with --pool true also the mean over its
  ego-net) as the readout, Linear as the head; the loss is ops.classifier_loss over the [B, C] logits; Adam.
* --scope ppr: the ego-nets come from modules.shadow.ShaDowPPRSampler instead — the root and the --ppr_k best nodes of an approximate
  personalised PageRank from it (fixed-point forward push, teleport --ppr_alpha, threshold --ppr_eps per stored entry, at most
  --ppr_rounds rounds), then the induced subgraph.  Nothing is drawn: training and evaluation see the same scope of a node every time.
* evaluate(): the mask's nodes run through ego-nets in batches of --batch_size, drawn by a second sampler with its own fixed seed that
  starts from offset 0 at every call — evaluation never moves the training stream and sees the same ego-nets every time; the model is
  in eval mode; accuracy for 1-D labels, micro-F1 for multi-label (eval._metrics).
* Flags: --dataset, --depth 2, --num_neighbors 10 (1 .. 64, one value for every hop), --num_layers 3, --conv sage|gcn, --pool true|false,
  --batch_size 512, --hidden_dim 256, --lr 1e-3, --max_epoch 100, --eval_frequency 1, --dropout 0, --runs 1, --seed;
  --scope khop|ppr (khop), --ppr_k 200 (1 .. 1023), --ppr_alpha 0.25, --ppr_eps 2^-14, --ppr_rounds 32 (1 .. 1024).
  1 + k + ... + k^depth, the most nodes of one ego-net, must not exceed 1024: the check runs when the flags are parsed.
* Not built: a captured (hipGraph) step, partitioned / multi-GPU forms, per-hop fanouts, float or asynchronous PPR, a PPR-weighted readout,
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
from .modules.shadow import ShaDow, ShaDowKHopSampler, ShaDowPPRSampler
from .target_batch import TargetBatchTrainer

EVAL_SEED = 0x5ADE                  # the Philox key of evaluation's ego-nets


class ShadowTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what ShaDowKHopSampler takes); x fp32 [N, F] without a gradient; y int64 [N] or fp32
    [N, C]; model: modules.shadow.ShaDow; optimizer: any torch optimiser over its parameters; batch_size: evaluate()'s.
    scope="khop": ShaDowKHopSampler(depth, num_neighbors, seed); scope="ppr": ShaDowPPRSampler(ppr_k, ppr_alpha, ppr_eps, ppr_rounds),
    which draws nothing — depth, num_neighbors and seed are not read, and evaluation uses the same scopes as training."""

    def __init__(self, graph, x, y, model: ShaDow, optimizer, depth: int = 2, num_neighbors: int = 10, batch_size: int = 512,
                 seed: Optional[int] = None, scope: str = "khop", ppr_k: int = 200, ppr_alpha: float = 0.25, ppr_eps: float = 2 ** -14,
                 ppr_rounds: int = 32):
        if x.requires_grad:
            raise ValueError("ShadowTrainer: node features with a gradient are not built: node_idx repeats nodes across ego-nets")
        if not 1 <= int(batch_size) <= ops.SHADOW_MAX_ROOTS:
            raise ValueError(f"ShadowTrainer: batch_size is 1 .. {ops.SHADOW_MAX_ROOTS}")
        if scope not in ("khop", "ppr"):
            raise ValueError(f"ShadowTrainer: scope={scope!r} is not built (built: khop, ppr)")
        self.scope = scope
        if scope == "ppr":
            super().__init__(x, y, model, optimizer, ShaDowPPRSampler(graph, ppr_k, alpha=ppr_alpha, eps=ppr_eps, max_rounds=ppr_rounds))
            self.eval_sampler = ShaDowPPRSampler(self.sampler.graph, ppr_k, alpha=ppr_alpha, eps=ppr_eps, max_rounds=ppr_rounds)
        else:
            super().__init__(x, y, model, optimizer, ShaDowKHopSampler(graph, depth, num_neighbors, seed=seed))
            self.eval_sampler = ShaDowKHopSampler(self.sampler.graph, depth, num_neighbors, seed=EVAL_SEED)
        self.batch_size = int(batch_size)

    def step(self, targets, words=None):
        """TargetBatchTrainer.step; words: ShaDowKHopSampler.sample's (refused under scope="ppr": nothing is drawn)."""
        if words is not None and self.scope == "ppr":
            raise ValueError("ShadowTrainer.step: words replace the k-hop sampler's draws; the PPR scope draws nothing")
        return super().step(targets, words)

    def _sample(self, targets, words):
        return self.sampler.sample(targets) if self.scope == "ppr" else self.sampler.sample(targets, words)

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
        if self.scope == "khop":
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
    ap.add_argument("--scope", default="khop", choices=["khop", "ppr"])
    ap.add_argument("--ppr_k", default=200, type=int)
    ap.add_argument("--ppr_alpha", default=0.25, type=float)
    ap.add_argument("--ppr_eps", default=2 ** -14, type=float)
    ap.add_argument("--ppr_rounds", default=32, type=int)
    args = parse_with_dataset(ap, argv)
    if args.scope == "ppr":
        if not (0.0 < args.ppr_alpha < 1.0 and 0.0 < args.ppr_eps <= 1.0):
            raise ValueError("--ppr_alpha lies inside (0, 1) and --ppr_eps inside (0, 1]")
        ops.shadow_ppr_args(args.ppr_k, int(round(args.ppr_alpha * 2 ** 16)), max(1, int(round(args.ppr_eps * 2 ** 30))), args.ppr_rounds)
    else:                                                            # a khop namespace carries no PPR field: nothing reads one
        ops.shadow_cap(args.depth, args.num_neighbors)
        if any(getattr(args, name) != ap.get_default(name) for name in ("ppr_k", "ppr_alpha", "ppr_eps", "ppr_rounds")):
            raise ValueError("--ppr_k, --ppr_alpha, --ppr_eps and --ppr_rounds belong to --scope ppr")
        for name in ("scope", "ppr_k", "ppr_alpha", "ppr_eps", "ppr_rounds"):
            delattr(args, name)
    check_ranges(args, "eval_frequency", "hidden_dim", "num_layers")
    return args


def build_model(F: int, num_classes: int, args, device) -> ShaDow:
    return ShaDow(F, args.hidden_dim, num_classes, args.num_layers, conv=args.conv, pool=args.pool, dropout=args.dropout).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], data.num_classes, args, device)
        ppr = {}
        if getattr(args, "scope", "khop") == "ppr":
            ppr = dict(scope="ppr", ppr_k=args.ppr_k, ppr_alpha=args.ppr_alpha, ppr_eps=args.ppr_eps, ppr_rounds=args.ppr_rounds)
        return ShadowTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), depth=args.depth,
                             num_neighbors=args.num_neighbors, batch_size=args.batch_size, seed=args.seed, **ppr)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
