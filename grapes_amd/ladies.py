"""LADIES / FastGCN baseline driver: layer-wise importance sampling [LADIES-recall: acbull/LADIES pytorch_ladies.py] training
the project's GCN, the two baselines of the reference's analysis/significance.py beside GraphSAINT that one GCN stack expresses.

    python -m grapes_amd.ladies --dataset cora --sampler ladies --max_epoch 50

* Per step (LadiesTrainer, eager): modules.ladies.LayerWiseSampler draws one weighted structure per layer for a batch of training
  nodes; GCN(F, [hidden_dim, ..., C]) runs over them with every layer in ops.WGCN_UNNORMALIZED mode — out[c] = sum_e w_e H[r] + b, the
  diagonal entries as ordinary entries (the pattern of saint._weighted_gcn, with one structure per layer); the loss is
  ops.classifier_loss over the targets' rows (CrossEntropy, or BCEWithLogits for 2-D labels); Adam.  The state dict is GCN's.
* evaluate(): one full-graph propagation with P = D^-1 (A + I) itself — the graph's entries plus one appended loop per node, weights
  v_ij / D_i, the same WGCN_UNNORMALIZED layers — so inference computes what training estimates; accuracy for 1-D labels, micro-F1
  for multi-label, as graphsaint.evaluate.
* Flags: --dataset, --sampler ladies|fastgcn, --samp_num 64, --batch_size 512, --hidden_dim 256, --lr 1e-3 and --max_epoch 100
  follow the LADIES script's defaults [LADIES-recall]; --num_layers 2 (theirs is 5: the project's GCN shape is two layers),
  --eval_frequency 1, --dropout 0, --runs 1, --seed, --e_cap (a layer's entry capacity; automatic by default).  An epoch is one pass
  over a permutation of the training nodes in batches of --batch_size (their script draws --batch_num batches per epoch instead).
* Not built: LADIES' own SuGCN head (their extra linear classifier), a captured (hipGraph) step, partitioned / multi-GPU forms.
  AS-GCN, the adaptive layer-wise sampler, is grapes_amd.asgcn.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .driver import check_ranges, parse_with_dataset, repeat_runs, target_batch_parser, train_target_batches
from .modules.gcn import GCN, _WeightedGCNConvFn
from .modules.ladies import KINDS, LayerWiseSampler
from .target_batch import TargetBatchTrainer, full_graph_metrics


def weighted_structures(edge_index, n: int):
    """One ops.WeightedStructure per layer's local edge list (int32 [2, e]); None for a layer without an entry."""
    out = []
    for ei in edge_index:
        if ei.shape[1] == 0:
            out.append(None)
            continue
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        out.append(ops.WeightedStructure(ops.PreparedGraph(src, dst, n), src, dst))
    return out


def layerwise_gcn(model: GCN, x, structures, edge_weight, tap=None):
    """GCN.forward's routing (hidden layer i on [-i], the last layer on [0]) with every layer as _WeightedGCNConvFn in
    WGCN_UNNORMALIZED mode; structures / edge_weight hold one entry per layer.  A layer without an entry (FastGCN drew no
    neighbour of its rows) outputs its bias.  tap: a list that receives the input of the last layer (grapes_amd.asgcn's variance
    term transforms it)."""
    n_layers = len(model.gcn_layers)
    if len(structures) != n_layers or len(edge_weight) != n_layers:
        raise ValueError(f"layerwise_gcn: {n_layers} layers take {n_layers} structures and weight vectors")
    for i, layer in enumerate(model.gcn_layers):
        last = i == n_layers - 1
        k = 0 if last else -(i + 1)
        ws, w = structures[k], edge_weight[k]
        if last and tap is not None:
            tap.append(x)
        if ws is None:
            x = layer.bias.unsqueeze(0).expand(x.shape[0], -1).contiguous()
            x = x if last else torch.relu(x)
        else:
            x = _WeightedGCNConvFn.apply(x, layer.lin.weight, layer.bias, w, ws, not last, ops.WGCN_UNNORMALIZED, 1.0)
        x = model._drop(x)
    return x


def full_graph_structure(g):
    """(WeightedStructure, weights) of P = D^-1 (A + I) over the whole graph: the stored entries (source = column, target = row)
    and one appended loop per node, each weighing 1 / D_target — a stored loop and the appended one add up to v_ii / D_i = 2 / D_i.
    Built once per graph with index arithmetic; fewer than 2^31 - N entries."""
    N, dev = g.num_nodes, g.device
    if g.nnz + N >= 2 ** 31:
        raise ValueError("LADIES / FastGCN evaluation over a graph with 2^31 or more entries is not built: the full-graph structure "
                         "has a 32-bit entry count")
    deg = g.rowptr[1:] - g.rowptr[:-1]
    ar = torch.arange(N, dtype=torch.int32, device=dev)
    row = torch.repeat_interleave(ar, deg)
    src, dst = torch.cat([g.col, ar]).contiguous(), torch.cat([row, ar]).contiguous()
    w = (1.0 / (deg + 1).to(torch.float32))[dst.long()].contiguous()
    return ops.WeightedStructure(ops.PreparedGraph(src, dst, N), src, dst), w


def evaluate(model, x, g, y, masks, structure=None):
    """The metric (accuracy, or micro-F1 for 2-D labels) of every mask from ONE full-graph forward with P."""
    ws, w = structure if structure is not None else full_graph_structure(g)
    L = len(model.gcn_layers)
    return full_graph_metrics(model, lambda: layerwise_gcn(model, x, [ws] * L, [w] * L), y, masks)


class LadiesTrainer(TargetBatchTrainer):
    """The eager step.  graph: a DeviceGraph (or what LayerWiseSampler takes); x fp32 [N, F]; y int64 [N] or fp32 [N, C];
    model: GCN with num_layers layers; optimizer: any torch optimiser over its parameters."""

    _full = None                        # full_graph_structure of the sampler's graph, built by the first evaluate()

    def __init__(self, graph, x, y, model: GCN, optimizer, samp_num: int = 64, kind: str = "ladies", seed: Optional[int] = None,
                 e_cap: Optional[int] = None):
        sampler = LayerWiseSampler(graph, samp_num, len(model.gcn_layers), kind=kind, seed=seed, e_cap=e_cap)
        super().__init__(x, y, model, optimizer, sampler)

    def step(self, targets, uniforms=None):
        """TargetBatchTrainer.step; uniforms: LayerWiseSampler.sample's."""
        return super().step(targets, uniforms)

    def _sample(self, targets, uniforms):
        return self.sampler.sample(targets, uniforms)

    def _forward(self, xb, b):
        return layerwise_gcn(self.model, xb, weighted_structures(b.edge_index, b.num_nodes), b.edge_weight)

    def evaluate(self, masks):
        if self._full is None:
            self._full = full_graph_structure(self.sampler.graph)
        return evaluate(self.model, self.x.detach(), self.sampler.graph, self.y, masks, self._full)


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = target_batch_parser("grapes_amd.ladies", __doc__.split("\n\n")[0])
    ap.add_argument("--sampler", default="ladies", choices=list(KINDS))
    ap.add_argument("--samp_num", default=64, type=int)
    ap.add_argument("--e_cap", default=None, type=int)
    args = parse_with_dataset(ap, argv)
    check_ranges(args, "num_layers", "samp_num", "eval_frequency")
    return args


def build_model(F: int, hidden_dim: int, C: int, num_layers: int, dropout: float, device) -> GCN:
    return GCN(F, hidden_dims=[hidden_dim] * (num_layers - 1) + [C], dropout=dropout).to(device)


def run(args, device=None, log=print) -> float:
    def make(g, x, y, data, device):
        model = build_model(x.shape[1], args.hidden_dim, data.num_classes, args.num_layers, args.dropout, device)
        return LadiesTrainer(g, x, y, model, torch.optim.Adam(model.parameters(), lr=args.lr), samp_num=args.samp_num,
                             kind=args.sampler, seed=args.seed, e_cap=args.e_cap)
    return train_target_batches(args, make, device, log)


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))


if __name__ == "__main__":
    main()
