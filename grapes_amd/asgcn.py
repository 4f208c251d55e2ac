"""AS-GCN baseline driver: the adaptive layer-wise sampler of modules/asgcn.py [AS-GCN-recall: Huang et al., "Adaptive Sampling
Towards Fast Graph Representation Learning", NeurIPS 2018] training the project's GCN with the variance term in the loss — the
baseline of the reference's analysis/significance.py whose sampler is learned.

    python -m grapes_amd.asgcn --dataset cora --max_epoch 50

* Per step (AsgcnTrainer, eager): AdaptiveSampler draws one weighted structure per layer; GCN runs over them as in
  grapes_amd.ladies (every layer ops.WGCN_UNNORMALIZED, one structure per layer); the loss is L = L_c + var_coef L_var, L_c =
  ops.classifier_loss over the targets' rows and L_var the variance of the estimator on the layer that writes the targets' logits
  (d = 0): with H = X_1 Wᵀ that layer's transformed input (a constant of the term: it trains the sampler only), mu_i = sum_j w_ij H_j
  and s_i the entries of target row i, V_i = (1 / s_i) sum_j |s_i w_ij H_j - mu_i|^2 = s_i sum_j w_ij^2 |H_j|^2 - |mu_i|^2,
  L_var = mean_i V_i (ops.asgcn_variance).  One optimiser holds the classifier's and the sampler's parameters.
* The gradient to the sampler.  With G_ij = d L / d w_ij (every layer: the edge-weight gradient of _WeightedGCNConvFn; layer 0: plus
  var_coef d L_var / d w), Gbar_i = sum_j G_ij w_ij and T_j = sum_i w_ij (G_ij - Gbar_i) (ops.asgcn_logq_bwd): d L / d logq_j = -T_j
  — the row sums and the column mass c_j drop out of the row-normalised weights — and d L / d a_j = -[a_j > 0] / g_j sum_d T_j^(d),
  with the mask from the kernel's own a.  a over the batch rows is the 1-wide ops.linear_fwd of the gathered x, so autograd carries
  the rest to w_g (the 1-wide ops.linear_bwd_weight) and b_g.
* evaluate(): grapes_amd.ladies.evaluate, one full-graph propagation with P = D^-1 (A + I) itself.
* Flags: those of grapes_amd.ladies without --sampler, with its defaults, and --var_coef 0.5 [AS-GCN-recall].
* Not built: a captured (hipGraph) step, partitioned / multi-GPU forms, the paper's skip connections and its node-wise variant.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .ladies import LadiesTrainer, build_model, layerwise_gcn, weighted_structures
from .modules.asgcn import AdaptiveSampler
from .modules.gcn import GCN
from .target_batch import TargetBatchTrainer, _TargetLoss


class _SamplerLogit(torch.autograd.Function):
    """a = x w_g + b_g over the batch's gathered rows: the 1-wide GEMM and its weight gradient; x gets no gradient."""

    @staticmethod
    def forward(ctx, xb, w_g, b_g):
        ctx.save_for_backward(xb)
        return ops.linear_fwd(xb, w_g.detach().reshape(1, -1)).reshape(-1) + b_g.detach()

    @staticmethod
    def backward(ctx, da):
        (xb,) = ctx.saved_tensors
        da = da.contiguous()
        return None, ops.linear_bwd_weight(da.reshape(-1, 1), xb).reshape(-1), ops.reduce_sum(da)


class _SamplerWeights(torch.autograd.Function):
    """One layer's sampled weights as a function of the batch's a.  Forward: the sampler's weights as they are.  Backward:
    T = ops.asgcn_logq_bwd of d L / d w, then d L / d a_j = -[a_j > 0] / g_j T_j with a the KERNEL's (a_saved), not the argument."""

    @staticmethod
    def forward(ctx, a_b, weight, src, dst, rows, a_saved, status):
        ctx.save_for_backward(weight, src, dst, rows, a_saved)
        ctx.status = status
        return weight.detach()

    @staticmethod
    def backward(ctx, G):
        weight, src, dst, rows, a_saved = ctx.saved_tensors
        T = ops.asgcn_logq_bwd(src, dst, weight, G.contiguous(), rows, a_saved.numel(), status=ctx.status)
        g = a_saved.clamp(min=0) + 1
        return -(a_saved > 0).to(T.dtype) / g * T, None, None, None, None, None, None


class _VarianceTerm(torch.autograd.Function):
    """L_var of one layer's weights over the constant H (ops.asgcn_variance); the backward scales the kernel's d L_var / d w.
    The trainer evaluates it on every step, also with var_coef = 0 or a frozen sampler, because the step reports loss_var: four
    launches, and one more GEMM that forms H again (_WeightedGCNConvFn keeps its own H to itself)."""

    @staticmethod
    def forward(ctx, weight, src, dst, rows, H, status):
        _, lvar, dw = ops.asgcn_variance(src, dst, weight.detach().contiguous(), rows, H, status=status)
        ctx.dw = dw
        return lvar.view(())

    @staticmethod
    def backward(ctx, gl):
        return ctx.dw * gl, None, None, None, None, None


class AsgcnTrainer(LadiesTrainer):
    """The eager step; epoch(), evaluate() and check() are LadiesTrainer's.  graph: LadiesTrainer's first argument, accepted so
    that the two are built alike and not read — the sampler holds the DeviceGraph it was made over; x fp32 [N, F]; y int64 [N] or
    fp32 [N, C]; model: GCN with sampler.num_layers layers; optimizer: any torch optimiser over the model's AND the sampler's
    parameters; var_coef: the weight of L_var."""

    def __init__(self, graph, x, y, model: GCN, sampler: AdaptiveSampler, optimizer, var_coef: float = 0.5):
        if len(model.gcn_layers) != sampler.num_layers:
            raise ValueError("AsgcnTrainer: the sampler draws one layer per GCN layer")
        TargetBatchTrainer.__init__(self, x, y, model, optimizer, sampler)
        self.var_coef = float(var_coef)

    def _sample(self, targets, uniforms):
        return self.sampler.sample(targets, self.x, uniforms)

    def step(self, targets, uniforms=None):
        """One step on a batch of distinct target nodes (at most 4096); returns (loss tensor, batch); the batch also carries
        loss_c and loss_var (0-d tensors)."""
        sm = self.sampler
        b, xb = self._batch(targets, uniforms)
        weights = b.edge_weight
        if sm.w_g.requires_grad or sm.b_g.requires_grad:
            a_b = _SamplerLogit.apply(xb, sm.w_g, sm.b_g)
            weights = [_SamplerWeights.apply(a_b, w, ei[0], ei[1], rows, b.a, sm.status)
                       for w, ei, rows in zip(b.edge_weight, b.edge_index, b.local_prev)]
        tap = []
        out = layerwise_gcn(self.model, xb, weighted_structures(b.edge_index, b.num_nodes), weights, tap=tap)
        x1 = tap[0]
        loss_c = _TargetLoss.apply(out, b.local_targets, b.targets, self.y)
        H = ops.linear_fwd(x1.detach().contiguous(), self.model.gcn_layers[-1].lin.weight.detach())
        ei = b.edge_index[0]
        loss_var = _VarianceTerm.apply(weights[0], ei[0], ei[1], b.local_prev[0], H, sm.status)
        loss = loss_c + self.var_coef * loss_var if self.var_coef != 0.0 and weights[0].requires_grad else loss_c
        loss.backward()
        self.optimizer.step()
        b.loss_c, b.loss_var = loss_c.detach(), loss_var.detach()
        return (loss_c + self.var_coef * loss_var).detach(), b


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.asgcn", __doc__.split("\n\n")[0])
    ap.add_argument("--samp_num", default=64, type=int)
    ap.add_argument("--e_cap", default=None, type=int)
    ap.add_argument("--var_coef", default=0.5, type=float)
    args = parse_with_dataset(ap, argv)
    check_ranges(args, "num_layers", "samp_num", "eval_frequency")
    if args.var_coef < 0:
        raise ValueError("--var_coef is not negative")
    return args


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, args.dropout, device)
        sampler = AdaptiveSampler(g, args.samp_num, args.num_layers, x.shape[1], seed=args.seed, e_cap=args.e_cap)
        opt = torch.optim.Adam(list(model.parameters()) + list(sampler.parameters()), lr=args.lr)
        return AsgcnTrainer(g, x, y, model, sampler, opt, var_coef=args.var_coef)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
