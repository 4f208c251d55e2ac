"""LINKX baseline driver: the scalable model of the large non-homophilous benchmark [Lim et al., NeurIPS 2021; PyG-recall: LINKX] —
an MLP over a node's features, a learned embedding of its adjacency row, and an MLP over their combination.  Nothing is sampled.

    python -m grapes_amd.linkx --dataset cora --hidden_dim 64 --num_node_layers 1 --num_final_layers 2 --bag_grad fused

* Per step (LinkxTrainer, eager): modules.linkx.BagBatcher gives the batch — the rows' column union and the by-column inverted index
  (ops.bag_batch) — the model is modules.linkx.LINKX; the loss is ops.classifier_loss over the [B, C] logits.  The table
  edge_lin.weight [N, H] has a row-sparse gradient: with --bag_grad fused no gradient is written and modules.linkx.BagAdam applies
  torch.optim.SparseAdam's rule to the touched rows inside the backward's segment-sum pass (ops.bag_bwd_adam); with --bag_grad sparse
  the gradient is a sparse COO tensor (ops.bag_bwd) and torch.optim.SparseAdam steps it.  Every other parameter: torch.optim.Adam.
* evaluate(masks): the forward over all N rows in ranges of eval_batch rows; the model in eval mode; accuracy for 1-D labels,
  micro-F1 for multi-label (eval._metrics).
* Flags: --dataset, --hidden_dim 256, --num_node_layers 1, --num_final_layers 2, --dropout 0, --lr 1e-3, --bag_lr (default --lr),
  --bag_grad fused|sparse, --batch_size 512, --max_epoch 100, --eval_frequency 1, --runs 1, --seed.
* Not built: a captured (hipGraph) step, multi-GPU forms, edge weights, num_edge_layers > 1 and batch norm, dense-Adam semantics or
  weight decay for the table, node features with a gradient, graphs with 2^31 or more entries, the LINKX dataset loaders.
  `--classifier` / `--model_type` routes in grapes_amd.main and grapes_amd.full_batch do not take this model.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .modules.linkx import GRADS, BagAdam, BagBatcher, LINKX
from .target_batch import TargetBatchTrainer, full_graph_metrics


class LinkxTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what BagBatcher takes), directed or not, below 2^31 entries; x fp32 [N, F] without a
    gradient; y int64 [N] or fp32 [N, C]; model: modules.linkx.LINKX; optimizer: a torch optimiser over model.dense_parameters() —
    everything except edge_lin.weight.  The table's optimiser is made here from bag_lr (and betas, eps): BagAdam in fused mode,
    torch.optim.SparseAdam in sparse mode.  eval_batch: the rows per forward of evaluate()."""

    def __init__(self, graph, x, y, model: LINKX, optimizer, bag_lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 eval_batch: int = 4096):
        if x.requires_grad:
            raise ValueError("LinkxTrainer: node features with a gradient are not built")
        if not isinstance(model, LINKX):
            raise TypeError(f"LinkxTrainer: the model is a modules.linkx.LINKX, not {type(model).__name__}")
        if not 1 <= int(eval_batch) <= ops.BAG_MAX_ROWS:
            raise ValueError(f"LinkxTrainer: eval_batch is 1 .. {ops.BAG_MAX_ROWS}")
        table = model.edge_lin.weight
        if any(p is table for grp in optimizer.param_groups for p in grp["params"]):
            raise ValueError("LinkxTrainer: the optimiser holds edge_lin.weight; it covers model.dense_parameters() and the table is "
                             "stepped by its own row-sparse optimiser")
        sampler = BagBatcher(graph)                                  # (refuses 2^31 or more entries)
        if sampler.graph.num_nodes != model.edge_lin.num_nodes:
            raise ValueError("LinkxTrainer: the graph has another number of nodes than the model's table")
        super().__init__(x, y, model, optimizer, sampler)
        self.eval_batch = int(eval_batch)
        if model.edge_lin.grad == "fused":
            self.bag_optimizer = BagAdam(model.edge_lin, lr=bag_lr, betas=betas, eps=eps)
        else:
            self.bag_optimizer = torch.optim.SparseAdam([table], lr=bag_lr, betas=betas, eps=eps)

    def _sample(self, targets, inject):
        if inject is not None:
            raise ValueError("LinkxTrainer.step: nothing is drawn, so there is nothing to inject")
        return self.sampler.batch(targets)

    def _forward(self, xb, b):
        return self.model(xb, b)

    def step(self, targets, inject=None):
        """TargetBatchTrainer.step, then the table's step.  (Targets may repeat: each occurrence is a batch row.)"""
        self.bag_optimizer.zero_grad()
        loss, b = super().step(targets, inject)
        self.bag_optimizer.step()
        return loss, b

    def logits_all(self):
        """Logits [N, C] of every node: the forward in ranges of eval_batch rows (one host read for the ranges' entry counts)."""
        g, bag = self.sampler.graph, self.model.edge_lin
        N, B = g.num_nodes, self.eval_batch
        los = list(range(0, N, B))
        ends = torch.tensor([min(lo + B, N) for lo in los], device=g.device)
        es = (g.rowptr[ends] - g.rowptr[torch.tensor(los, device=g.device)]).tolist()
        out = []
        for lo, e in zip(los, es):
            rows = torch.arange(lo, min(lo + B, N), dtype=torch.int32, device=g.device)
            out.append(self.model.head(bag.embed(g, rows, item_cap=ops.bag_fwd_item_cap(e)), self.x[lo:lo + B]))
        return torch.cat(out)

    def evaluate(self, masks):
        return full_graph_metrics(self.model, self.logits_all, self.y, masks)


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.linkx", __doc__.split("\n\n")[0], num_layers=None)
    ap.add_argument("--num_node_layers", default=1, type=int)
    ap.add_argument("--num_final_layers", default=2, type=int)
    ap.add_argument("--bag_lr", default=None, type=float)
    ap.add_argument("--bag_grad", default="fused", choices=list(GRADS))
    args = parse_with_dataset(ap, argv)
    if args.num_layers is not None:
        raise ValueError("--num_layers is not a LINKX flag: --num_node_layers and --num_final_layers")
    if args.bag_lr is None:
        args.bag_lr = args.lr
    if not (args.lr >= 0.0 and args.bag_lr >= 0.0 and 0.0 <= args.dropout < 1.0):
        raise ValueError("--lr and --bag_lr are not negative and --dropout lies inside [0, 1)")
    check_ranges(args, "eval_frequency", "hidden_dim", "num_node_layers", "num_final_layers")
    if not ops.gather_width_ok(args.hidden_dim):
        raise ValueError(f"--hidden_dim {args.hidden_dim} is not a width the gathers are built for (any up to 256, multiples of 4 up to 1024)")
    return args


def build_model(num_nodes: int, F: int, num_classes: int, args, device) -> LINKX:
    return LINKX(num_nodes, F, args.hidden_dim, num_classes, num_node_layers=args.num_node_layers,
                 num_final_layers=args.num_final_layers, dropout=args.dropout, grad=args.bag_grad).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(g.num_nodes, x.shape[1], data.num_classes, args, device)
        return LinkxTrainer(g, x, y, model, torch.optim.Adam(model.dense_parameters(), lr=args.lr), bag_lr=args.bag_lr,
                            eval_batch=min(max(args.batch_size, 1024), ops.BAG_MAX_ROWS))
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
