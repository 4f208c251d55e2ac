"""LABOR baseline driver: layer-neighbour sampling [Balin and Catalyurek, NeurIPS 2023; LABOR-recall: DGL's LaborSampler] training the
project's SAGE stack — neighbour sampling's estimator on a far smaller batch, the method between the node-wise and layer-wise families.

    python -m grapes_amd.labor --dataset cora --fanouts 10,10 --importance_iters 0 --max_epoch 50

* Per step (LaborTrainer, eager): modules.labor.LaborSampler keeps the entries of every row of layer d by ONE variate per candidate
  vertex, shared by all rows (fanouts[0] next to the output); the model is SAGE(F, [hidden_dim, ..., C], aggr="mean") with GCN's routing;
  the loss is ops.classifier_loss over the targets' rows; Adam.  The state dict is SAGE's.
  - importance_iters = 0: every kept entry of a row weighs 1 / kept_s, so the batch runs model(xb, edge_index): SAGEConv's mean over
    the kept entries is exactly the Hajek estimator.
  - importance_iters >= 1: each layer is lin_l over sum_e w_e x_src plus the root term lin_r(x_dst) and lin_l's bias, with SAGE's
    routing, ReLU and dropout and the same parameters: the weighted sum is _WeightedGCNConvFn in WGCN_UNNORMALIZED mode over
    ladies.weighted_structures (a stored loop is an ordinary weighted entry there), the root term one more GEMM, the sum and the
    ReLU ops.gcn2_mix_fwd — existing kernels only.
* evaluate(): graphsage.evaluate — one full-graph forward with every neighbour.
* Flags: --dataset, --fanouts 10,10 (one per layer, -1 = every neighbour, else 1 .. 64), --importance_iters 0 (0 .. 8),
  --layer_dependency (one set of variates for every layer), --batch_size 512, --hidden_dim 256, --lr 1e-3, --max_epoch 100,
  --eval_frequency 1, --dropout 0, --runs 1, --seed; --num_layers defaults to the number of fanouts and must equal it.  The aggregation
  is the mean: there is no --aggr.
* Not built: a captured (hipGraph) step, partitioned / multi-GPU forms, DGL's batch_dependency, sequential Poisson (exact-k) sampling,
  a per-edge-weight form of grapes_rootsum_aggregate_*, graphs with 2^31 or more entries.  `--classifier` / `--model_type` routes in
  grapes_amd.main and grapes_amd.full_batch do not take this sampler.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .graphsage import _fanouts, build_model, evaluate
from .ladies import weighted_structures
from .modules.gcn import SAGE, _WeightedGCNConvFn
from .modules.labor import LaborSampler
from .modules.sage import check_fanouts
from .target_batch import TargetBatchTrainer


class _RootFn(torch.autograd.Function):
    """x Wᵀ, SAGEConv's root term: one GEMM; the backward is one GEMM per operand."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return ops.linear_fwd(x, weight)

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        dout = dout.contiguous()
        dw = ops.linear_bwd_weight(dout, x) if ctx.needs_input_grad[1] else None
        dx = ops.linear_bwd_input(dout, weight) if ctx.needs_input_grad[0] else None
        return dx, dw


class _AddActFn(torch.autograd.Function):
    """act(a + b) in one launch (ops.gcn2_mix_fwd); the backward gates by the saved output and hands the same rows to both."""

    @staticmethod
    def forward(ctx, a, b, relu):
        out = ops.gcn2_mix_fwd(a.contiguous(), b.contiguous(), 1.0, 1.0, relu=relu)
        ctx.relu = relu
        ctx.save_for_backward(out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        g = ops.gcn2_mix_bwd(dout.contiguous(), out, True, 1.0)[0] if ctx.relu else dout
        return g, g, None


def weighted_sage(model: SAGE, x, structures, edge_weight):
    """SAGE.forward's routing (hidden layer i on [-i], the last layer on [0]) with every layer as
    act(lin_l(sum_e w_e x_src) + lin_l.bias + lin_r(x_dst)); structures / edge_weight hold one entry per layer.  A layer without an
    entry aggregates 0."""
    n_layers = len(model.convs)
    if len(structures) != n_layers or len(edge_weight) != n_layers:
        raise ValueError(f"weighted_sage: {n_layers} layers take {n_layers} structures and weight vectors")
    if not x.is_cuda:
        raise ops._lib.GrapesHipError("weighted_sage input must be a cuda tensor (grapes_amd has no CPU path)")
    x = x.contiguous()
    for i, conv in enumerate(model.convs):
        last = i == n_layers - 1
        k = 0 if last else -(i + 1)
        ws, w = structures[k], edge_weight[k]
        bias = conv.lin_l.bias
        if ws is None:
            a = bias.unsqueeze(0).expand(x.shape[0], -1).contiguous()
        else:
            a = _WeightedGCNConvFn.apply(x, conv.lin_l.weight, bias, w, ws, False, ops.WGCN_UNNORMALIZED, 1.0)
        x = model._drop(_AddActFn.apply(a, _RootFn.apply(x, conv.lin_r.weight), not last))
    return x


class LaborTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what LaborSampler takes); x fp32 [N, F]; y int64 [N] or fp32 [N, C]; model: SAGE with
    aggr="mean", a root weight and len(fanouts) layers; optimizer: any torch optimiser over its parameters."""

    def __init__(self, graph, x, y, model: SAGE, optimizer, fanouts: Sequence[int] = (10, 10), importance_iters: int = 0,
                 layer_dependency: bool = False, seed: Optional[int] = None):
        if len(fanouts) != len(model.convs):
            raise ValueError(f"LaborTrainer: {len(model.convs)} layers take {len(model.convs)} fanouts, not {len(fanouts)}")
        if model.aggr != "mean" or any(conv.lin_r is None or conv.lin_l.bias is None for conv in model.convs):
            raise ValueError("LaborTrainer: the model is SAGE with aggr='mean', root_weight=True and bias=True")
        super().__init__(x, y, model, optimizer, LaborSampler(graph, fanouts, importance_iters=importance_iters,
                                                              layer_dependency=layer_dependency, seed=seed))

    def step(self, targets, keys=None):
        """TargetBatchTrainer.step; keys: LaborSampler.sample's."""
        return super().step(targets, keys)

    def _sample(self, targets, keys):
        return self.sampler.sample(targets, keys)

    def _forward(self, xb, b, weighted: Optional[bool] = None):
        """weighted: None = by the batch (the SAGE route for a uniform batch), True forces the weighted route (tests)."""
        if b.uniform and not weighted:
            return self.model(xb, b.edge_index)
        return weighted_sage(self.model, xb, weighted_structures(b.edge_index, b.num_nodes), b.edge_weight)

    def evaluate(self, masks):
        return evaluate(self.model, self.x.detach(), self.sampler.graph, self.y, masks)


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.labor", __doc__.split("\n\n")[0], num_layers=None)
    ap.add_argument("--fanouts", default=[10, 10], type=_fanouts)
    ap.add_argument("--importance_iters", default=0, type=int)
    ap.add_argument("--layer_dependency", action="store_true")
    args = parse_with_dataset(ap, argv)
    args.fanouts = check_fanouts(args.fanouts)
    if args.num_layers is None:
        args.num_layers = len(args.fanouts)
    if args.num_layers != len(args.fanouts):
        raise ValueError(f"--fanouts holds one entry per layer: {len(args.fanouts)} given for --num_layers {args.num_layers}")
    if not 0 <= args.importance_iters <= ops.LABOR_MAX_ITERS:
        raise ValueError(f"--importance_iters is 0 .. {ops.LABOR_MAX_ITERS}, not {args.importance_iters}")
    check_ranges(args, "eval_frequency", "hidden_dim")
    return args


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, args.dropout, "mean", device)
        return LaborTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), fanouts=args.fanouts,
                            importance_iters=args.importance_iters, layer_dependency=args.layer_dependency, seed=args.seed)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
