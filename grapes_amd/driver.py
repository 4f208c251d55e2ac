"""What every command-line driver does: open the loaded data as a DeviceGraph, repeat a run `--runs` times and print the
reference's `Acc: mean ± std` line; and, for the three drivers that train on batches of target nodes (grapes_amd.ladies,
grapes_amd.asgcn, grapes_amd.graphsage), the flags they share and the run itself.  grapes_amd.main, grapes_amd.full_batch and
grapes_amd.graphsaint keep their own loops (their docstrings say how they differ) and use open_graph and repeat_runs alone.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional, Sequence

import torch

from .target_batch import MAX_TARGETS


def open_graph(data, device):
    """The DeviceGraph of loaded data: its CSR (rowptr / col, on the device already) or its edge_index (reference main.py:134-136)."""
    from .graph import DeviceGraph
    if getattr(data, "rowptr", None) is not None:
        return DeviceGraph(data.rowptr, data.col, data.num_nodes)
    return DeviceGraph.from_edge_index(data.edge_index.to(device), int(data.num_nodes), device=device)


def repeat_runs(run_fn, args) -> float:
    """args.runs calls of run_fn(args), then `Acc: mean ± std` of their results (reference main.py:376-390); the std of one run,
    NaN in the reference, is printed as 0.00.  Returns the mean."""
    results = torch.empty(args.runs)
    for r in range(args.runs):
        results[r] = run_fn(args)
    std = float(results.std()) if args.runs > 1 else 0.0
    print(f"Acc: {100 * float(results.mean()):.2f} ± {100 * std:.2f}")
    return float(results.mean())


def target_batch_parser(prog: str, description: str, num_layers: Optional[int] = 2) -> argparse.ArgumentParser:
    """The flags the target-batch drivers share, with the LADIES script's defaults (grapes_amd.ladies has the sources)."""
    ap = argparse.ArgumentParser(prog=prog, description=description)
    ap.add_argument("--dataset", type=str)
    ap.add_argument("--batch_size", default=512, type=int)
    ap.add_argument("--hidden_dim", default=256, type=int)
    ap.add_argument("--num_layers", default=num_layers, type=int)
    ap.add_argument("--lr", default=1e-3, type=float)
    ap.add_argument("--max_epoch", default=100, type=int)
    ap.add_argument("--eval_frequency", default=1, type=int)
    ap.add_argument("--dropout", default=0.0, type=float)
    ap.add_argument("--runs", default=1, type=int)
    ap.add_argument("--seed", default=None, type=int)
    return ap


def parse_with_dataset(ap: argparse.ArgumentParser, argv: Optional[Sequence[str]]) -> argparse.Namespace:
    args = ap.parse_args(list(sys.argv[1:] if argv is None else argv))
    if args.dataset is None:
        raise SystemExit("--dataset is required")
    return args


def check_ranges(args, *at_least_1: str) -> None:
    """ValueError unless the named flags are at least 1 and --batch_size is 1 .. MAX_TARGETS (one batch is one loss launch)."""
    if any(getattr(args, n) < 1 for n in at_least_1) or not 1 <= args.batch_size <= MAX_TARGETS:
        names = [f"--{n}" for n in at_least_1]
        raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} are at least 1, --batch_size is 1 .. {MAX_TARGETS}")


def train_target_batches(args, make, device=None, log=print) -> float:
    """One run of a target-batch driver.  make(g, x, y, data, device) -> trainer (a target_batch.TargetBatchTrainer) is called
    after torch.manual_seed(args.seed), so the model's initialisation is the first thing drawn.  Per epoch one pass over a
    permutation of the training nodes in batches of --batch_size; val and test every --eval_frequency epochs and after the last
    one.  Returns the last val metric."""
    from .main import load_data
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    data = load_data(args, device)
    g = open_graph(data, device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    x, y = data.x.to(device).contiguous(), data.y.to(device)
    train_mask, val_mask, test_mask = (m.to(device) for m in (data.train_mask, data.val_mask, data.test_mask))
    tr = make(g, x, y, data, device)
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
