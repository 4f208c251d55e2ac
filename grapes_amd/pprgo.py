"""PPRGo baseline driver: the decoupled / precomputed-propagation family [Bojchevski et al., KDD 2020 — recalled]: an MLP over node
features, and a root's logits as the sum of its k best personalised-PageRank nodes' rows weighted by their scores.

    python -m grapes_amd.pprgo --dataset cora --ppr_k 32 --ppr_alpha 0.5 --ppr_eps 1e-4 --ppr_rounds 32 --normalization row --inference power --nprop_inference 2 --precompute true

* Per step (PPRGoTrainer, eager): modules.pprgo.PPRGoSampler gives the batch — the slot tables of the roots (ops.pprgo_topk: the
  fixed-point forward push of the ShaDow PPR scope without its ego-net; with --precompute true pushed once for the training nodes and
  looked up afterwards), their union and the inverted index (ops.pprgo_batch) — the model is modules.pprgo.PPRGo: an MLP of
  --num_layers bias-free layers of --hidden_dim columns over the union's gathered rows, then ops.pprgo_aggregate_fwd; the loss is
  ops.classifier_loss over the [B, C] logits; Adam.  Nothing is drawn.
* evaluate(masks, inference): "power" — one MLP pass over all nodes and PPRGo.propagate, --nprop_inference rounds of
  Q <- (1 - alpha) S Q + alpha Z over the full graph; "ppr" — the training form in batches of --batch_size.  The model is in eval mode;
  accuracy for 1-D labels, micro-F1 for multi-label (eval._metrics).
* Flags: --dataset, --ppr_k 32 (1 .. 1023), --ppr_alpha 0.5, --ppr_eps 1e-4, --ppr_rounds 32 (1 .. 1024), --normalization row|sym|col,
  --inference power|ppr, --nprop_inference 2, --precompute true|false, --batch_size 512, --hidden_dim 256, --num_layers 2, --lr 1e-3,
  --max_epoch 100, --eval_frequency 1, --dropout 0, --runs 1, --seed.
* Not built: a captured (hipGraph) step, multi-GPU forms, aggregating before the MLP where the hidden width is below the class count,
  a disk cache of the scores, a float or asynchronous push, edge weights, node features with a gradient, asymmetric graphs (the
  power iteration reads the by-target rows), graphs with 2^31 or more entries.  `--classifier` / `--model_type` routes in
  grapes_amd.main and grapes_amd.full_batch do not take this model.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .modules.pprgo import NORMALIZATIONS, PPRGo, PPRGoSampler
from .target_batch import TargetBatchTrainer, full_graph_metrics

INFERENCES = ("power", "ppr")


class PPRGoTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what PPRGoSampler takes), symmetric, below 2^31 entries; x fp32 [N, F] without a
    gradient; y int64 [N] or fp32 [N, C]; model: modules.pprgo.PPRGo; optimizer: any torch optimiser over its parameters.  k, alpha,
    eps, max_rounds, normalization: PPRGoSampler's.  batch_size: evaluate("ppr")'s.  inference, nprop: evaluate()'s defaults."""

    def __init__(self, graph, x, y, model: PPRGo, optimizer, k: int = 32, alpha: float = 0.5, eps: float = 1e-4, max_rounds: int = 32,
                 normalization: str = "row", batch_size: int = 512, inference: str = "power", nprop: int = 2):
        if x.requires_grad:
            raise ValueError("PPRGoTrainer: node features with a gradient are not built")
        if not isinstance(model, PPRGo):
            raise TypeError(f"PPRGoTrainer: the model is a modules.pprgo.PPRGo, not {type(model).__name__}")
        if inference not in INFERENCES:
            raise ValueError(f"PPRGoTrainer: inference={inference!r} is not built (built: power, ppr)")
        if not 1 <= int(batch_size) <= ops.PPRGO_MAX_ROOTS or int(nprop) < 0:
            raise ValueError(f"PPRGoTrainer: batch_size is 1 .. {ops.PPRGO_MAX_ROOTS} and nprop at least 0")
        sampler = PPRGoSampler(graph, k=k, alpha=alpha, eps=eps, max_rounds=max_rounds, normalization=normalization)
        if sampler.symmetry & 1:
            raise ValueError("PPRGoTrainer: an asymmetric graph is not built (the power iteration reads the by-target rows)")
        super().__init__(x, y, model, optimizer, sampler)
        self.batch_size, self.inference, self.nprop = int(batch_size), inference, int(nprop)

    def precompute(self, nodes):
        """PPRGoSampler.precompute: the push once for `nodes`; later batches of such nodes are row lookups."""
        self.sampler.precompute(nodes)
        return self

    def _sample(self, targets, inject):
        if inject is not None:
            raise ValueError("PPRGoTrainer.step: nothing is drawn, so there is nothing to inject")
        return self.sampler.sample(targets)

    def _forward(self, xb, b):
        return self.model(xb, b)

    def logits_of(self, nodes):
        """Logits [len(nodes), C] of the given nodes in the training form, in batches of batch_size."""
        s, out = self.sampler, []
        for i in range(0, nodes.numel(), self.batch_size):
            b = s.sample(nodes[i:i + self.batch_size])
            s.check()
            out.append(self.model(ops.gather_rows(self.x, b.node_idx), b))
        return torch.cat(out) if out else torch.zeros((0, self.model.out_channels), device=self.x.device)

    def evaluate(self, masks, inference: Optional[str] = None):
        inference = self.inference if inference is None else inference
        if inference not in INFERENCES:
            raise ValueError(f"PPRGoTrainer.evaluate: inference={inference!r} is not built (built: power, ppr)")
        s = self.sampler
        if inference == "power":
            return full_graph_metrics(self.model, lambda: PPRGo.propagate(self.model.mlp(self.x), s.graph, s.alpha, self.nprop,
                                                                          s.normalization), self.y, masks)
        from .eval import _metrics
        was = self.model.training
        self.model.eval()
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
    raise argparse.ArgumentTypeError(f"--precompute takes true or false, not {text!r}")


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.pprgo", __doc__.split("\n\n")[0], num_layers=2)
    ap.add_argument("--ppr_k", default=32, type=int)
    ap.add_argument("--ppr_alpha", default=0.5, type=float)
    ap.add_argument("--ppr_eps", default=1e-4, type=float)
    ap.add_argument("--ppr_rounds", default=32, type=int)
    ap.add_argument("--normalization", default="row", choices=list(NORMALIZATIONS))
    ap.add_argument("--inference", default="power", choices=list(INFERENCES))
    ap.add_argument("--nprop_inference", default=2, type=int)
    ap.add_argument("--precompute", default=True, type=_bool)
    args = parse_with_dataset(ap, argv)
    if not (0.0 < args.ppr_alpha < 1.0 and 0.0 < args.ppr_eps <= 1.0):
        raise ValueError("--ppr_alpha lies inside (0, 1) and --ppr_eps inside (0, 1]")
    ops.shadow_ppr_args(args.ppr_k, int(round(args.ppr_alpha * 2 ** 16)), max(1, int(round(args.ppr_eps * 2 ** 30))), args.ppr_rounds)
    if args.nprop_inference < 0:
        raise ValueError("--nprop_inference is at least 0")
    check_ranges(args, "eval_frequency", "hidden_dim", "num_layers")
    return args


def build_model(F: int, num_classes: int, args, device) -> PPRGo:
    return PPRGo(F, [args.hidden_dim] * (args.num_layers - 1) + [num_classes], dropout=args.dropout).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], data.num_classes, args, device)
        tr = PPRGoTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), k=args.ppr_k, alpha=args.ppr_alpha,
                          eps=args.ppr_eps, max_rounds=args.ppr_rounds, normalization=args.normalization, batch_size=args.batch_size,
                          inference=args.inference, nprop=args.nprop_inference)
        if args.precompute:
            tr.precompute(torch.nonzero(data.train_mask.to(device), as_tuple=False).reshape(-1))
        return tr
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
