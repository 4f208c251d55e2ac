"""Cluster-GCN baseline driver: partition-based training [Chiang et al., KDD 2019; PyG-recall: ClusterData, ClusterLoader,
ClusterGCNConv, examples/cluster_gcn_reddit.py] — the graph is cut into clusters once and a step trains on the subgraph induced on
the union of a few of them.

    python -m grapes_amd.clustergcn --dataset cora --num_parts 32 --batch_size 4 --partition random

* Per step (ClusterTrainer, eager): modules.cluster.ClusterLoader builds the subgraph induced on --batch_size clusters
  (ops.cluster_batch: no draw, no N-sized node map); the batch's feature rows are gathered; the model is modules.gcn.ClusterGCN —
  ClusterGCNConv layers with --diag_lambda — over the batch's one edge list; the loss is saint.masked_loss over the batch's training
  rows (mean CE, or BCEWithLogits for multi-label); Adam.  A batch without a training row gives a NaN loss with zero gradients, as
  the GraphSAINT step does.
* epoch(): one pass over a permutation of the clusters.  evaluate(): ONE exact full-graph forward, the model in eval mode; accuracy
  for 1-D labels, micro-F1 for multi-label (eval._metrics).
* Flags: --dataset, --num_parts 32, --batch_size 4 (clusters per step), --partition random|range|file|lp[:ROUNDS[:IMBALANCE]],
  --partition_file x.npy (an integer array [N] of cluster ids in [0, num_parts), e.g. METIS's output computed elsewhere, or what
  `python -m grapes_amd.partition` wrote), --diag_lambda 0, --hidden_dim 256, --num_layers 2, --lr 1e-3, --max_epoch 100,
  --eval_frequency 1, --dropout 0, --runs 1, --seed.  --partition lp (30 rounds, imbalance 0.1), lp:ROUNDS, lp:ROUNDS:IMBALANCE:
  a random start seeded by --seed, refined by size-constrained label propagation (modules.cluster.refine_partition); the run
  prints the starting cut, the final cut and the rounds used.
* Not built: a METIS-class partitioner (multilevel coarsening, a swap or rebalancing phase: label propagation stalls once clusters
  sit at their cap; --partition file is the way in for a better assignment), edge or node weights in the partitioner, a captured (hipGraph)
  step, multi-GPU forms, graphs with 2^31 or more entries, GraphSAINT-style normalisation of cluster batches, the paper's stochastic
  multiple-partition variant with a normalisation rebuilt per batch beyond what ClusterGCNConv computes on the union itself.
  `--classifier` / `--model_type` routes in grapes_amd.main and grapes_amd.full_batch do not take this loader.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
from typing import Optional, Sequence

import torch

from .driver import open_graph, parse_with_dataset, repeat_runs
from .modules.cluster import ClusterData, ClusterLoader
from .modules.gcn import ClusterGCN
from .saint import masked_loss
from .target_batch import _GatherX, full_graph_metrics


class ClusterTrainer:
    """The eager step.  cluster_data: a modules.cluster.ClusterData; x fp32 [N, F]; y int64 [N] or fp32 [N, C]; train_mask bool [N];
    model: ClusterGCN; optimizer: any torch optimiser over its parameters; batch_size: clusters per step."""

    def __init__(self, cluster_data: ClusterData, x, y, train_mask, model: ClusterGCN, optimizer, batch_size: int = 4,
                 seed: Optional[int] = None, n_cap: Optional[int] = None, e_cap: Optional[int] = None):
        self.loader = ClusterLoader(cluster_data, batch_size, seed=seed, n_cap=n_cap, e_cap=e_cap)
        self.x, self.y, self.train_mask, self.model, self.optimizer = x, y, train_mask, model, optimizer

    def _train_on(self, b):
        self.loader.check()
        self.optimizer.zero_grad()
        xb = _GatherX.apply(self.x, b.node_idx, None, None, False)
        out = self.model(xb, b.edge_index)
        loss = masked_loss(out, b.node_idx, None, self.train_mask, self.y)
        loss.backward()
        self.optimizer.step()
        return loss.detach(), b

    def step(self, clusters):
        """One step on the union of the given clusters; returns (loss tensor, batch)."""
        return self._train_on(self.loader.batch(clusters))

    def epoch(self):
        """One pass over a permutation of the clusters; the mean of the step losses."""
        tot, k = 0.0, 0
        for b in self.loader:
            loss, _ = self._train_on(b)
            tot, k = tot + float(loss), k + 1
        return tot / max(k, 1)

    def evaluate(self, masks):
        g = self.loader.cluster_data.graph
        return full_graph_metrics(self.model, lambda: self.model(self.x.detach(), g), self.y, masks)

    def check(self):
        self.loader.check()


LP_ROUNDS, LP_IMBALANCE = 30, 0.1


def parse_partition(value: str):
    """(method, rounds, imbalance) of a --partition value: "random", "range", "file", or "lp", "lp:ROUNDS", "lp:ROUNDS:IMBALANCE"
    (label propagation from a random start: ROUNDS a non-negative integer, IMBALANCE a non-negative number).  ValueError for
    anything else."""
    if value in ("random", "range", "file"):
        return value, None, None
    head, *rest = value.split(":")
    if head != "lp" or len(rest) > 2:
        raise ValueError(f"--partition is random, range, file, lp, lp:ROUNDS or lp:ROUNDS:IMBALANCE, not {value!r}")
    try:
        rounds = int(rest[0]) if rest else LP_ROUNDS
        imbalance = float(rest[1]) if len(rest) > 1 else LP_IMBALANCE
    except ValueError:
        raise ValueError(f"--partition {value!r}: ROUNDS is an integer and IMBALANCE a number") from None
    if rounds < 0 or not 0 <= imbalance < float("inf"):
        raise ValueError(f"--partition {value!r}: ROUNDS and IMBALANCE are at least 0")
    return "lp", rounds, imbalance


def _partition_arg(value: str) -> str:
    """argparse's check of --partition: the value itself, kept as given (it is parsed after parse_args)."""
    try:
        parse_partition(value)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return value


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="grapes_amd.clustergcn", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", type=str)
    ap.add_argument("--num_parts", default=32, type=int)
    ap.add_argument("--batch_size", default=4, type=int)
    ap.add_argument("--partition", default="random", type=_partition_arg, metavar="random|range|file|lp[:ROUNDS[:IMBALANCE]]")
    ap.add_argument("--partition_file", default=None, type=str)
    ap.add_argument("--diag_lambda", default=0.0, type=float)
    ap.add_argument("--hidden_dim", default=256, type=int)
    ap.add_argument("--num_layers", default=2, type=int)
    ap.add_argument("--lr", default=1e-3, type=float)
    ap.add_argument("--max_epoch", default=100, type=int)
    ap.add_argument("--eval_frequency", default=1, type=int)
    ap.add_argument("--dropout", default=0.0, type=float)
    ap.add_argument("--runs", default=1, type=int)
    ap.add_argument("--seed", default=None, type=int)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    args = parse_with_dataset(_parser(), argv)
    if min(args.num_parts, args.batch_size, args.hidden_dim, args.num_layers, args.eval_frequency) < 1:
        raise ValueError("--num_parts, --batch_size, --hidden_dim, --num_layers and --eval_frequency are at least 1")
    if args.batch_size > args.num_parts:
        raise ValueError(f"--batch_size counts clusters: at most --num_parts ({args.num_parts})")
    if (args.partition == "file") != (args.partition_file is not None):
        raise ValueError("--partition file goes with --partition_file x.npy, and --partition_file with --partition file")
    return args


def load_partition(path: str) -> torch.Tensor:
    """The cluster of every node from a .npy file: an integer array [N]."""
    import numpy as np
    part = np.load(path)
    if part.ndim != 1 or not np.issubdtype(part.dtype, np.integer):
        raise ValueError(f"--partition_file {path}: an integer array [N] of cluster ids")
    return torch.from_numpy(part.astype(np.int64))


def partition_report(info) -> str:
    """One line on a refinement (modules.cluster.refine_partition's info): the starting cut, the final cut, the rounds used."""
    return (f"Partition: label propagation, cut {info['cuts'][0]} -> {info['cuts'][info['round']]} "
            f"(round {info['round']} of {len(info['moved'])} run; largest cluster {info['max_size']}, cap {info['cap']})")


def build_model(F: int, hidden_dim: int, C: int, num_layers: int, dropout: float, diag_lambda: float, device) -> ClusterGCN:
    return ClusterGCN(F, hidden_dims=[hidden_dim] * (num_layers - 1) + [C], dropout=dropout, diag_lambda=diag_lambda).to(device)


def run(args, device=None, log=print) -> float:
    from .main import load_data
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    data = load_data(args, device)
    g = open_graph(data, device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    x, y = data.x.to(device).contiguous(), data.y.to(device)
    train_mask, val_mask, test_mask = (m.to(device) for m in (data.train_mask, data.val_mask, data.test_mask))
    model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, args.dropout, args.diag_lambda, device)
    method, lp_rounds, lp_imbalance = parse_partition(args.partition)
    part = load_partition(args.partition_file) if method == "file" else None
    if method == "lp":
        cd = ClusterData(g, args.num_parts, method="lp", seed=args.seed, lp_start="random", lp_rounds=lp_rounds, lp_imbalance=lp_imbalance)
        log(partition_report(cd.lp_info))
    else:
        cd = ClusterData(g, args.num_parts, part=part, method=method if part is None else "random", seed=args.seed)
    tr = ClusterTrainer(cd, x, y, train_mask, model, torch.optim.Adam(model.parameters(), lr=args.lr), batch_size=args.batch_size,
                        seed=args.seed)
    val = 0.0
    for epoch in range(1, args.max_epoch + 1):
        loss = tr.epoch()
        if epoch % args.eval_frequency == 0 or epoch == args.max_epoch:
            val, test = tr.evaluate((val_mask, test_mask))
            log(f"Epoch: {epoch:02d}, Loss: {loss:.4f}, Val: {val:.4f}, Test: {test:.4f}")
        else:
            log(f"Epoch: {epoch:02d}, Loss: {loss:.4f}")
    return val


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
