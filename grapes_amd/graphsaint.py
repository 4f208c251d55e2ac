"""GraphSAINT baseline driver (reference graphsaint.py).

    python -m grapes_amd.graphsaint --dataset cora --max_epoch 50 --runs 1

* Flags and defaults of graphsaint.py:13-20: --use_normalization (alone: accepted, unused as in the reference, which passes
  sample_coverage 0; with --sample_coverage K > 0: GraphSAINT's normalised training — saint.py), --hidden_dim 256,
  --dataset, --runs 1, --lr 0.01, --max_epoch 50, --embed_nodes, --node_emb_dim 64.  Added: --batch_size 256 and --walk_length 2
  (graphsaint.py:104 hard-codes them), --num_steps 1, --seed, --engine graph|eager (saint.GraphedSaintTrainer /
  saint.EagerSaintTrainer), --e_cap (edge capacity of a batch), --large_graph auto|true|false (the row-blocked 64-bit
  evaluation of full_graph.py; automatic from 2^31 CSR entries on) and --sampler rw|node|edge (GraphSAINT's three samplers:
  the reference's random walks, or PyG's GraphSAINTNodeSampler / GraphSAINTEdgeSampler, which ignore --walk_length) and
  --sample_coverage 0 (PyG's sample_coverage: with --use_normalization the coverage estimate runs until N * K nodes were sampled;
  without that flag a value above 0 is a ValueError).
* Per run: GCN(F, [hidden_dim, C]) without dropout, Adam(params + embeddings, lr) (graphsaint.py:115-116); per epoch one step per
  batch, then one full-graph forward that yields val and test: accuracy for 1-D labels, TP / FP / FN micro-F1 for multi-label
  (graphsaint.py:46-88).  It prints `Epoch: .., Loss: .., Val: .., Test: ..`; a run's result is its last epoch's val metric, and
  the driver ends with `Acc: mean ± std` over the runs (graphsaint.py:119-127).
* Reference defects not reproduced: `print(data.x.grad.mean())` (graphsaint.py:38) raises without --embed_nodes — not printed;
  `model.cpu()` in test() (graphsaint.py:47) moves the model off the GPU after epoch 1 — evaluation stays on the device;
  `--embed_nodes` is parsed with type=bool, so "False" is True — parsed with main._bool here; with one run the std is NaN —
  printed as 0.00 (as full_batch.py does).

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
from typing import Optional, Sequence

import torch

from .driver import open_graph, parse_with_dataset, repeat_runs
from .main import _bool, _large_flag, load_data


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="grapes_amd.graphsaint", description=__doc__.split("\n\n")[0])
    ap.add_argument("--use_normalization", action="store_true")                     # graphsaint.py:13 (read with --sample_coverage)
    ap.add_argument("--hidden_dim", default=256, type=int)
    ap.add_argument("--dataset", type=str)
    ap.add_argument("--runs", default=1, type=int)
    ap.add_argument("--lr", default=0.01, type=float)
    ap.add_argument("--max_epoch", default=50, type=int)
    ap.add_argument("--embed_nodes", default=False, type=_bool)
    ap.add_argument("--node_emb_dim", default=64, type=int)
    # additions of this driver
    ap.add_argument("--batch_size", default=256, type=int)
    ap.add_argument("--walk_length", default=2, type=int)
    ap.add_argument("--num_steps", default=1, type=int)
    ap.add_argument("--seed", default=None, type=int)
    ap.add_argument("--engine", default="graph", choices=["graph", "eager"])
    ap.add_argument("--e_cap", default=None, type=int)
    ap.add_argument("--large_graph", default="auto", choices=["auto", "true", "false"])
    ap.add_argument("--sampler", default="rw", choices=["rw", "node", "edge"])
    ap.add_argument("--sample_coverage", default=0, type=int)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    args = parse_with_dataset(_parser(), argv)
    if args.sample_coverage < 0 or (args.sample_coverage and not args.use_normalization):
        raise ValueError("--sample_coverage K (K > 0) goes with --use_normalization: the estimate is read by the normalised step alone")
    return args


def evaluate(model, x, g, y, val_mask, test_mask, large_graph: Optional[bool]):
    """(val, test) of graphsaint.py:46-88 from ONE full-graph forward."""
    from . import full_graph
    from .eval import _metrics
    with torch.no_grad():
        if full_graph.use_large_path(g, large_graph):
            both = val_mask | test_mask
            _, _, pred = full_graph.evaluate_rows(model, x, g, y, both, True)
            rows = torch.nonzero(both, as_tuple=False).reshape(-1)
            out = []
            for m in (val_mask, test_mask):
                sel = m[rows]
                p, t = pred[sel], y[rows[sel]]
                if y.dim() == 1:
                    out.append(float((p == t).float().mean().item()) if t.numel() else 0.0)
                else:
                    out.append(_f1(p, t > 0.5))
            return tuple(out)
        logits, _ = model(x, g, large_graph=False)
        return tuple(_metrics(logits[m], y[m])[0] for m in (val_mask, test_mask))


def _f1(y_pred, y_true) -> float:
    """TP / FP / FN micro-F1 of boolean [n, C] predictions: eval._metrics thresholds them (> 0, > 0.5) to themselves."""
    from .eval import _metrics
    return _metrics(y_pred, y_true)[0]


def run(args, device=None, log=print) -> float:
    from . import saint
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    data = load_data(args, device)
    g = open_graph(data, device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    emb = []
    if args.embed_nodes:                                                                     # graphsaint.py:94-101
        log("Using learned node embeddings for features")
        e = torch.empty(data.num_nodes, args.node_emb_dim)
        torch.nn.init.normal_(e)
        x = torch.nn.Parameter(e.to(device), requires_grad=True)
        emb.append(x)
    else:
        x = data.x.to(device).contiguous()
    y = data.y.to(device)
    train_mask, val_mask, test_mask = (m.to(device) for m in (data.train_mask, data.val_mask, data.test_mask))
    model = saint.build_model(x.shape[1], args.hidden_dim, data.num_classes, device)
    # (--use_normalization alone stays unused: the trainers are called as before)
    cov = getattr(args, "sample_coverage", 0)
    norm = dict(sample_coverage=cov, use_normalization=True) if cov else {}
    tr = saint.make_trainer(args.engine, g, x, y, train_mask, model, args.lr, emb, batch_size=args.batch_size,
                            walk_length=args.walk_length, num_steps=args.num_steps, seed=args.seed, e_cap=args.e_cap,
                            sampler=args.sampler, **norm)
    large = _large_flag(args.large_graph)
    val = 0.0
    for epoch in range(1, args.max_epoch + 1):                                               # graphsaint.py:118-121
        loss = tr.epoch()
        val, test = evaluate(model, x.detach(), g, y, val_mask, test_mask, large)
        log(f"Epoch: {epoch:02d}, Loss: {loss:.4f}, Val: {val:.4f}, Test: {test:.4f}")
    return val                                                                               # graphsaint.py:123


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(run, parse_args(argv))                                                # graphsaint.py:119-127


if __name__ == "__main__":
    main()
