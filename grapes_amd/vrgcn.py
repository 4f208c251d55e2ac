"""VR-GCN baseline driver: control-variate training on historical activations [Chen, Zhu and Song, ICML 2018] of the project's GCN.

    python -m grapes_amd.vrgcn --dataset cora --fanouts 2,2 --max_epoch 50

* Per step (VrgcnTrainer, eager): modules.sage.NeighborSampler keeps at most fanouts[d] neighbours per row of layer d over a
  loop-free copy of the graph (fanouts[0] next to the output); modules.vrgcn.vrgcn_forward runs GCN(F, [hidden_dim, ..., C]) with
  the estimator — the first layer exact from P X (computed once), every later layer the sampled difference to its history plus the
  history over the row's WHOLE neighbourhood, one fused gather (ops.vrgcn_aggregate_fwd); ops.classifier_loss over the targets'
  rows; Adam; then the histories take the step's activations (ops.scatter_rows).  The state dict is GCN's.
* evaluate(): one exact full-graph GCN forward on the graph as given, as the paper predicts at test time; accuracy for 1-D labels,
  micro-F1 for multi-label.
* Flags: --dataset, --fanouts 2,2 (one per layer, -1 = every neighbour, else 1 .. 64), --batch_size 512, --hidden_dim 256,
  --lr 1e-3, --max_epoch 100, --eval_frequency 1, --runs 1, --seed; --num_layers defaults to the number of fanouts and must equal
  it; --dropout other than 0 is refused.
* Not built: dropout, a captured (hipGraph) step, partitioned / multi-GPU forms, graphs with 2^31 or more entries, directed graphs.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .graph import DeviceGraph
from .graphsage import _fanouts
from .modules.gcn import GCN
from .modules.sage import NeighborSampler, check_fanouts
from .modules.sampling import _graph_of
from .modules.vrgcn import HistoryStore, VRGraph, vrgcn_forward
from .target_batch import MAX_TARGETS, TargetBatchTrainer, _TargetLoss, full_graph_metrics


def loop_free(graph: DeviceGraph) -> DeviceGraph:
    """The graph itself when it stores no (u, u) entry, else a copy without them (gcn_norm replaces stored loops by one unit loop,
    so P is the same)."""
    N, dev = graph.num_nodes, graph.device
    row = torch.repeat_interleave(torch.arange(N, device=dev, dtype=torch.int32), graph.rowptr[1:] - graph.rowptr[:-1])
    keep = row != graph.col
    if bool(keep.all()):
        return graph
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(row[keep].long(), minlength=N), 0, out=rowptr[1:])
    return DeviceGraph(rowptr, graph.col[keep].contiguous(), N)


def evaluate(model: GCN, x, g, y, masks):
    """The metric (accuracy, or micro-F1 for 2-D labels) of every mask from ONE exact full-graph forward."""
    return full_graph_metrics(model, lambda: model(x, g)[0], y, masks)


class VrgcnTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what NeighborSampler takes), symmetric; x fp32 [N, F]; y int64 [N] or fp32 [N, C];
    model: GCN with len(fanouts) layers and no dropout; optimizer: any torch optimiser over its parameters."""

    def __init__(self, graph, x, y, model: GCN, optimizer, fanouts: Sequence[int] = (2, 2), seed: Optional[int] = None):
        if not x.is_cuda:
            raise ops._lib.GrapesHipError("VrgcnTrainer: x must live in HBM (cuda tensor); grapes_amd has no CPU path")
        if len(fanouts) != len(model.gcn_layers):
            raise ValueError(f"VrgcnTrainer: {len(model.gcn_layers)} layers take {len(model.gcn_layers)} fanouts, not {len(fanouts)}")
        if model.dropout != 0.0:
            raise ValueError("VR-GCN with dropout is not built (the paper's estimator under dropout is another one)")
        self.full_graph, _ = _graph_of(graph)
        if self.full_graph.nnz >= 2 ** 31:
            raise ValueError("VR-GCN over a graph with 2^31 or more entries is not built")
        if ops.csr_symmetric_check(self.full_graph.rowptr, self.full_graph.col, self.full_graph.num_nodes) != 0:
            raise ValueError("VrgcnTrainer: the graph must be symmetric with every column id inside [0, num_nodes)")
        g = loop_free(self.full_graph)
        super().__init__(x, y, model, optimizer, NeighborSampler(g, fanouts, seed=seed))
        self.vgraph = VRGraph(g)
        self.px = self.vgraph.propagate(x.detach())
        self.store = HistoryStore(g.num_nodes, [c.out_channels for c in model.gcn_layers[:-1]], g.device)

    def step(self, targets, keys=None):
        """One step on a batch of distinct target nodes (at most 4096); returns (loss tensor, batch).  keys: NeighborSampler.sample's.
        The histories are written after the forward and backward passes, from the activations the forward computed."""
        if targets.numel() > MAX_TARGETS:
            raise ValueError(f"{type(self).__name__}.step: at most {MAX_TARGETS} targets per batch")
        b = self.sampler.sample(targets, keys)
        self.sampler.check()
        self.optimizer.zero_grad()
        logits, acts = vrgcn_forward(self.model, b, self.px, self.store, self.vgraph, status=self.sampler.status)
        rows = torch.arange(b.targets.numel(), dtype=torch.int32, device=logits.device)
        loss = _TargetLoss.apply(logits, rows, b.targets, self.y)
        loss.backward()
        self.optimizer.step()
        for level, rows_l, h in acts:
            self.store.update(level, b.node_idx, rows_l, h)
        b.activations = acts
        return loss.detach(), b

    def evaluate(self, masks):
        return evaluate(self.model, self.x.detach(), self.full_graph, self.y, masks)


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.vrgcn", __doc__.split("\n\n")[0], num_layers=None)
    ap.add_argument("--fanouts", default=[2, 2], type=_fanouts)
    args = parse_with_dataset(ap, argv)
    args.fanouts = check_fanouts(args.fanouts)
    if args.num_layers is None:
        args.num_layers = len(args.fanouts)
    if args.num_layers != len(args.fanouts):
        raise ValueError(f"--fanouts holds one entry per layer: {len(args.fanouts)} given for --num_layers {args.num_layers}")
    if args.dropout != 0.0:
        raise ValueError("--dropout other than 0 is not built for VR-GCN (the paper's estimator under dropout is another one)")
    check_ranges(args, "eval_frequency", "hidden_dim")
    return args


def build_model(F: int, hidden_dim: int, C: int, num_layers: int, device) -> GCN:
    return GCN(F, [hidden_dim] * (num_layers - 1) + [C], dropout=0.0).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, device)
        return VrgcnTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), fanouts=args.fanouts, seed=args.seed)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
