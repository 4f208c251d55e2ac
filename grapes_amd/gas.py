"""GNNAutoScale ("GAS") baseline driver: cluster batches that pull their out-of-batch neighbours from histories [Fey, Lenssen,
Weichert and Leskovec, ICML 2021; pyg_autoscale-recall: ScalableGNN, History, SubgraphLoader] of the project's GCN.

    python -m grapes_amd.gas --dataset cora --num_parts 32 --batch_size 4 --partition lp:30:0.1 --max_epoch 50

* Per step (GasTrainer, eager): modules.gas.GasLoader builds the union of --batch_size clusters over a loop-free copy of the graph
  (ops.cluster_batch) and resolves every entry of every batch row to the local row of an in-batch neighbour or the history row of
  an out-of-batch one (ops.gas_resolve); modules.gas.gas_forward runs GCN(F, [hidden_dim, ..., C]) — the first layer exact from P X
  (computed once), every later layer one fused gather over the row's WHOLE neighbourhood that reads the batch's activations and the
  history table in place (ops.gas_aggregate_fwd); saint.masked_loss over the batch's training rows; Adam; then the histories take
  the step's activations of all the batch's rows (ops.scatter_rows).  The state dict is GCN's.
* train_epoch(): one pass over a permutation of the clusters.  evaluate(): ONE exact full-graph GCN forward on the graph as given
  (vrgcn.evaluate); accuracy for 1-D labels, micro-F1 for multi-label.  reset_histories() zeroes the tables.
* Flags: --dataset, --num_parts 32, --batch_size 4 (clusters per step), --partition random|range|file|lp[:ROUNDS[:IMBALANCE]] and
  --partition_file x.npy as grapes_amd.clustergcn takes them, --hidden_dim 256, --num_layers 2, --lr 1e-3, --max_epoch 100,
  --eval_frequency 1, --runs 1, --seed; --dropout other than 0 is refused.
* Not built: dropout, GAS's weight-decay and gradient-clipping regularisers, history-based inference (evaluation is exact), layers
  other than GCN, a captured (hipGraph) step, multi-GPU forms, histories in pinned host memory (GAS's CPU offload), directed graphs,
  graphs with 2^31 or more entries.  `--classifier` / `--model_type` routes in grapes_amd.main and grapes_amd.full_batch do not
  take this loader.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
from typing import Optional, Sequence

import torch

from . import ops
from .clustergcn import _partition_arg, load_partition, parse_partition, partition_report
from .driver import open_graph, parse_with_dataset, repeat_runs
from .modules.cluster import ClusterData
from .modules.gas import GasLoader, gas_forward, push
from .modules.gcn import GCN
from .modules.sampling import _graph_of
from .modules.vrgcn import HistoryStore, VRGraph
from .saint import masked_loss
from .vrgcn import evaluate, loop_free


def make_cluster_data(graph, num_parts: int, partition="random", seed: Optional[int] = None, log=None) -> ClusterData:
    """The ClusterData of a partition given as GasTrainer takes it: "random", "range", "lp[:ROUNDS[:IMBALANCE]]" (clustergcn's
    parse_partition), the path of a .npy file of cluster ids, or an integer tensor [N] of them."""
    if torch.is_tensor(partition):
        return ClusterData(graph, num_parts, part=partition)
    if partition in ("random", "range"):
        return ClusterData(graph, num_parts, method=partition, seed=seed)
    if partition.split(":")[0] == "lp":
        _, rounds, imbalance = parse_partition(partition)
        cd = ClusterData(graph, num_parts, method="lp", seed=seed, lp_start="random", lp_rounds=rounds, lp_imbalance=imbalance)
        if log is not None:
            log(partition_report(cd.lp_info))
        return cd
    return ClusterData(graph, num_parts, part=load_partition(partition))


class GasTrainer:
    """The eager step.  graph: a DeviceGraph (or what ClusterData takes), symmetric; x fp32 [N, F]; y int64 [N] or fp32 [N, C];
    model: GCN without dropout; optimizer: any torch optimiser over its parameters; num_parts clusters, batch_size of them per step;
    partition: "random" | "range" | "lp[:R[:I]]" | a .npy file | an integer tensor [N]; train_mask bool [N] (None: every node)."""

    def __init__(self, graph, x, y, model: GCN, optimizer, num_parts: int = 32, batch_size: int = 4, partition="random",
                 seed: Optional[int] = None, train_mask=None, log=None):
        if not isinstance(model, GCN):
            raise TypeError("GasTrainer trains the project's GCN (layers other than GCN are not built)")
        if model.dropout != 0.0:
            raise ValueError("GAS with dropout is not built")
        if not x.is_cuda:
            raise ops._lib.GrapesHipError("GasTrainer: x must live in HBM (cuda tensor); grapes_amd has no CPU path")
        self.full_graph, _ = _graph_of(graph)
        if self.full_graph.nnz >= 2 ** 31:
            raise ValueError("GAS over a graph with 2^31 or more entries is not built")
        if ops.csr_symmetric_check(self.full_graph.rowptr, self.full_graph.col, self.full_graph.num_nodes) != 0:
            raise ValueError("GasTrainer: the graph must be symmetric with every column id inside [0, num_nodes)")
        g = loop_free(self.full_graph)
        self.x, self.y, self.model, self.optimizer = x, y, model, optimizer
        self.train_mask = torch.ones(g.num_nodes, dtype=torch.bool, device=x.device) if train_mask is None else train_mask
        self.cluster_data = make_cluster_data(g, num_parts, partition, seed, log)
        self.loader = GasLoader(self.cluster_data, batch_size, seed=seed)
        self.vgraph = VRGraph(g)
        self.px = self.vgraph.propagate(x.detach())
        self.store = HistoryStore(g.num_nodes, [c.out_channels for c in model.gcn_layers[:-1]], g.device)

    def _train_on(self, b):
        self.loader.check()
        self.optimizer.zero_grad()
        logits, acts = gas_forward(self.model, b, self.px, self.store, self.vgraph, status=self.loader.status)
        loss = masked_loss(logits, b.node_idx, None, self.train_mask, self.y)
        loss.backward()
        self.optimizer.step()
        push(self.store, b, acts)
        b.activations = acts
        return loss.detach(), b

    def step(self, clusters):
        """One step on the union of the given clusters; returns (loss tensor, batch).  The histories are written after the forward
        and backward passes, from the activations the forward computed.  A batch without a training row gives a NaN loss with
        zero gradients, as the Cluster-GCN step does."""
        return self._train_on(self.loader.batch(clusters))

    def train_epoch(self) -> float:
        """One pass over a permutation of the clusters; the mean of the step losses."""
        tot, k = 0.0, 0
        for b in self.loader:
            loss, _ = self._train_on(b)
            tot, k = tot + float(loss), k + 1
        return tot / max(k, 1)

    def evaluate(self, masks):
        return evaluate(self.model, self.x.detach(), self.full_graph, self.y, masks)

    def reset_histories(self):
        self.store.reset()

    def check(self):
        self.loader.check()


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(prog="grapes_amd.gas", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", type=str)
    ap.add_argument("--num_parts", default=32, type=int)
    ap.add_argument("--batch_size", default=4, type=int)
    ap.add_argument("--partition", default="random", type=_partition_arg, metavar="random|range|file|lp[:ROUNDS[:IMBALANCE]]")
    ap.add_argument("--partition_file", default=None, type=str)
    ap.add_argument("--hidden_dim", default=256, type=int)
    ap.add_argument("--num_layers", default=2, type=int)
    ap.add_argument("--lr", default=1e-3, type=float)
    ap.add_argument("--max_epoch", default=100, type=int)
    ap.add_argument("--eval_frequency", default=1, type=int)
    ap.add_argument("--dropout", default=0.0, type=float)
    ap.add_argument("--runs", default=1, type=int)
    ap.add_argument("--seed", default=None, type=int)
    args = parse_with_dataset(ap, argv)
    if min(args.num_parts, args.batch_size, args.hidden_dim, args.num_layers, args.eval_frequency) < 1:
        raise ValueError("--num_parts, --batch_size, --hidden_dim, --num_layers and --eval_frequency are at least 1")
    if args.batch_size > args.num_parts:
        raise ValueError(f"--batch_size counts clusters: at most --num_parts ({args.num_parts})")
    if (args.partition == "file") != (args.partition_file is not None):
        raise ValueError("--partition file goes with --partition_file x.npy, and --partition_file with --partition file")
    if args.dropout != 0.0:
        raise ValueError("--dropout other than 0 is not built for GAS")
    return args


def build_model(F: int, hidden_dim: int, C: int, num_layers: int, device) -> GCN:
    return GCN(F, [hidden_dim] * (num_layers - 1) + [C], dropout=0.0).to(device)


def run(args, device=None, log=print) -> float:
    from .main import load_data
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    data = load_data(args, device)
    g = open_graph(data, device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    x, y = data.x.to(device).contiguous(), data.y.to(device)
    train_mask, val_mask, test_mask = (m.to(device) for m in (data.train_mask, data.val_mask, data.test_mask))
    model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, device)
    partition = args.partition_file if args.partition == "file" else args.partition
    tr = GasTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), num_parts=args.num_parts,
                    batch_size=args.batch_size, partition=partition, seed=args.seed, train_mask=train_mask, log=log)
    val = 0.0
    for epoch in range(1, args.max_epoch + 1):
        loss = tr.train_epoch()
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
