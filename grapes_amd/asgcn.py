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

import argparse
import sys
from typing import Optional, Sequence

import torch

from . import ops
from .ladies import MAX_TARGETS, _TargetLoss, build_model, evaluate, full_graph_structure, layerwise_gcn, weighted_structures
from .main import load_data
from .modules.asgcn import AdaptiveSampler
from .modules.gcn import GCN
from .saint import _GatherX


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


class AsgcnTrainer:
    """The eager step.  graph: LadiesTrainer's first argument, accepted so that the two are built alike and not read — the sampler
    holds the DeviceGraph it was made over; x fp32 [N, F]; y int64 [N] or fp32 [N, C]; model: GCN with sampler.num_layers layers;
    optimizer: any torch optimiser over the model's AND the sampler's parameters; var_coef: the weight of L_var."""

    def __init__(self, graph, x, y, model: GCN, sampler: AdaptiveSampler, optimizer, var_coef: float = 0.5):
        if len(model.gcn_layers) != sampler.num_layers:
            raise ValueError("AsgcnTrainer: the sampler draws one layer per GCN layer")
        self.x, self.y, self.model, self.sampler, self.optimizer = x, y, model, sampler, optimizer
        self.var_coef = float(var_coef)
        self._full = None

    def step(self, targets, uniforms=None):
        """One step on a batch of distinct target nodes (at most 4096); returns (loss tensor, batch); the batch also carries
        loss_c and loss_var (0-d tensors)."""
        if targets.numel() > MAX_TARGETS:
            raise ValueError(f"AsgcnTrainer.step: at most {MAX_TARGETS} targets per batch")
        sm = self.sampler
        b = sm.sample(targets, self.x, uniforms)
        sm.check()
        self.optimizer.zero_grad()
        xb = _GatherX.apply(self.x, b.node_idx, None, None, False)
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
    ap = argparse.ArgumentParser(prog="grapes_amd.asgcn", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", type=str)
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
    ap.add_argument("--var_coef", default=0.5, type=float)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    args = _parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    if args.dataset is None:
        raise SystemExit("--dataset is required")
    if args.num_layers < 1 or args.samp_num < 1 or not 1 <= args.batch_size <= MAX_TARGETS or args.eval_frequency < 1:
        raise ValueError(f"--num_layers, --samp_num and --eval_frequency are at least 1, --batch_size is 1 .. {MAX_TARGETS}")
    if args.var_coef < 0:
        raise ValueError("--var_coef is not negative")
    return args


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
    sampler = AdaptiveSampler(g, args.samp_num, args.num_layers, x.shape[1], seed=args.seed, e_cap=args.e_cap)
    opt = torch.optim.Adam(list(model.parameters()) + list(sampler.parameters()), lr=args.lr)
    tr = AsgcnTrainer(g, x, y, model, sampler, opt, var_coef=args.var_coef)
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
