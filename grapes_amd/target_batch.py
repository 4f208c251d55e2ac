"""The eager training step on a batch of target nodes, shared by the baselines whose sampler draws layers for such a batch
(grapes_amd.ladies, grapes_amd.asgcn, grapes_amd.graphsage): gather the batch's feature rows, run the model over the sampled
layers, ops.classifier_loss over the targets' rows, backward, optimiser step.  _GatherX is also the gather of saint.py's steps.
"""
from __future__ import annotations

import torch

from . import ops

MAX_TARGETS = 4096                  # ops.classifier_loss: one workgroup's rows


class _GatherX(torch.autograd.Function):
    """X[node_idx[:count]] (rows past the count are left as they are).  Backward: with into_grad the rows' gradients are added
    into X.grad in place (node_idx is duplicate-free) and nothing is returned; otherwise a dense [N, F] gradient is returned."""

    @staticmethod
    def forward(ctx, X, node_idx, count, out, into_grad):
        ctx.save_for_backward(node_idx)
        ctx.count, ctx.X, ctx.into_grad = count, X, into_grad
        return ops.gather_rows(X.detach(), node_idx, d_n=count, out=out)

    @staticmethod
    def backward(ctx, dx):
        (node_idx,) = ctx.saved_tensors
        X = ctx.X
        dx = dx.contiguous()
        if ctx.into_grad and X.grad is not None:
            ops.scatter_rows(X.grad, node_idx, dx, d_n=ctx.count, accumulate=True)
            return None, None, None, None, None
        g = torch.zeros(X.shape, dtype=torch.float32, device=dx.device)
        ops.scatter_rows(g, node_idx, dx, d_n=ctx.count)
        return g, None, None, None, None


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


def full_graph_metrics(model, forward, y, masks):
    """The metric (eval._metrics: accuracy, or micro-F1 for 2-D labels) of every mask from ONE call of forward() -> logits of
    every node, with the model in eval mode (no dropout at inference) and under no_grad; the mode is restored."""
    from .eval import _metrics
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            logits = forward()
            return tuple(_metrics(logits[m], y[m])[0] for m in masks)
    finally:
        model.train(was)


class TargetBatchTrainer:
    """x fp32 [N, F]; y int64 [N] or fp32 [N, C]; optimizer: any torch optimiser; sampler: sample() draws a batch (node_idx,
    targets, local_targets and what the model reads) and check() raises on its status word.  A subclass gives _sample(targets,
    inject) -> batch, _forward(xb, batch) -> logits over the batch's rows, and evaluate(masks) over the full graph."""

    def __init__(self, x, y, model, optimizer, sampler):
        self.x, self.y, self.model, self.optimizer, self.sampler = x, y, model, optimizer, sampler

    def _batch(self, targets, inject):
        """What opens a step: the limit, the draw and its check, zeroed gradients; returns (batch, its gathered feature rows)."""
        if targets.numel() > MAX_TARGETS:
            raise ValueError(f"{type(self).__name__}.step: at most {MAX_TARGETS} targets per batch")
        b = self._sample(targets, inject)
        self.sampler.check()
        self.optimizer.zero_grad()
        return b, _GatherX.apply(self.x, b.node_idx, None, None, False)

    def step(self, targets, inject=None):
        """One step on a batch of distinct target nodes (at most 4096); returns (loss tensor, batch).  inject: values that
        replace the sampler's Philox draws (tests)."""
        b, xb = self._batch(targets, inject)
        loss = _TargetLoss.apply(self._forward(xb, b), b.local_targets, b.targets, self.y)
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

    def check(self):
        self.sampler.check()
