"""Full-batch GCN training driver: the baseline every GRAPES result is compared against (reference full-batch.py).

    python -m grapes_amd.full_batch --dataset cora --max_epochs 30 --runs 10

* Flags and defaults of the reference's `Arguments` (full-batch.py:26-50) — they differ from main.py's (`eval_on_cpu`,
  `eval_full_batch` false, `log_wandb` true).  `--config_file` is read first and the command line wins (full-batch.py:146-150).
  Flags that change nothing here are accepted and ignored: `log_wandb`, `notes`, `eval_on_cpu`, `eval_full_batch` and the
  sampler's (`sampling_hops`, `num_samples`, `use_indicators`, `lr_gf`, `loss_coef`, `log_z_init`, `reg_param`, `batch_size`).
  Added: `--classifier gcn|gat|gcn2|pna|gatv2` (gat: the reference's GAT, modules/gcn.py:45-72, trained by autograd over the whole graph;
  below 2^31 entries, no dropout; gcn2: modules/gcn.py:76-117's GCN2 with `--gcn2_alpha`, `--gcn2_theta`, `--gcn2_shared_weights` and
  `--dropout`, trained the same way; pna: modules/gcn.py:120-149's PNA with `--pna_aggregators`, `--pna_scalers`, `--dropout` and the
  graph's in-degree histogram, trained the same way; gatv2: GATv2 with `--gat_heads` heads, trained the same way, no dropout), `--seed` (the synthetic data and the weights) and `--large_graph auto|true|false` (the row-blocked 64-bit path of
  full_graph.train_step: automatic from 2^31 CSR entries on).
* Model `GCN(F, [hidden_dim, C], dropout)` and `Adam(lr=lr_gc)` (full-batch.py:72-76).  Each epoch is one full_graph.train_step
  over the whole graph — mean CrossEntropy, or mean BCEWithLogits for 2-D labels, on the train rows — then `step()`
  (full-batch.py:100-107).
* Validation when (epoch + 1) % eval_frequency == 0, on THIS epoch's training logits of the validation rows, taken before the
  optimiser step (full-batch.py:116-120).  Test: one more forward pass over the whole graph (full-batch.py:130-134).  Then
  `Acc: mean ± std` of 100 * test_f1 over the runs (full-batch.py:152-157).
* Kept from the reference: the module is never put in .eval(), so dropout is active in the validation logits and in the test
  pass.  Changed: the reference logs `loss_c=0.000000` (acc_loss_c is never updated); the real loss is printed.  For
  multi-label targets the reference's accuracy_score raises; the TP / FP / FN micro-F1 of eval.py:57-70 is reported instead.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
import sys
import time
from typing import Optional, Sequence

import torch

from .driver import open_graph, repeat_runs
from .main import _EAGER_CLASSIFIERS, _bool, _large_flag, build_classifier, check_classifier, load_data, read_config_file

# (name, type, default) — full-batch.py:26-50
_FLAGS = [
    ("dataset", str, "cora"), ("sampling_hops", int, 2), ("num_samples", int, 16), ("lr_gc", float, 1e-3),
    ("use_indicators", bool, True), ("lr_gf", float, 1e-4), ("loss_coef", float, 1e4), ("log_z_init", float, 0.0),
    ("reg_param", float, 0.0), ("dropout", float, 0.0), ("model_type", str, "gcn"), ("hidden_dim", int, 256),
    ("max_epochs", int, 30), ("batch_size", int, 512), ("eval_frequency", int, 5), ("eval_on_cpu", bool, False),
    ("eval_full_batch", bool, False), ("runs", int, 10), ("notes", str, None), ("log_wandb", bool, True),
    ("config_file", str, None),
]
# additions of this driver (not in the reference)
_EXTRA = [("seed", int, None), ("large_graph", str, "auto"), ("classifier", str, "gcn"),
          ("gcn2_alpha", float, 0.1), ("gcn2_theta", float, 0.5), ("gcn2_shared_weights", bool, True),
          ("pna_aggregators", str, "mean,min,max,std"), ("pna_scalers", str, "identity,amplification,attenuation"),
          ("gat_heads", int, 1)]


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="grapes_amd.full_batch", description=__doc__.split("\n\n")[0])
    for name, typ, default in _FLAGS + _EXTRA:
        if name == "large_graph":
            ap.add_argument("--large_graph", choices=["auto", "true", "false"], default=default)
        elif name == "classifier":
            # (absent from the namespace unless given: a plain run's arguments stay the reference's + seed, large_graph)
            ap.add_argument("--classifier", choices=["gcn", "gat", "gcn2", "pna", "gatv2"], default=argparse.SUPPRESS)
        elif name.startswith("gcn2_") or name.startswith("pna_") or name == "gat_heads":
            # (--classifier gcn2's / pna's / gatv2's hyper-parameters: absent unless given, defaults in main.build_gcn2 / build_pna /
            # build_gatv2)
            ap.add_argument(f"--{name}", type=_bool if typ is bool else typ, default=argparse.SUPPRESS)
        else:
            ap.add_argument(f"--{name}", type=_bool if typ is bool else typ, default=default)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    """full-batch.py:143-150: with --config_file the file's flags are read first and the command line is parsed on top."""
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = _parser()
    args = ap.parse_args(argv)
    if args.config_file is not None:
        args = ap.parse_args(read_config_file(args.config_file) + argv)
    if args.model_type != "gcn":
        raise NotImplementedError("only model_type=gcn is built (full-batch.py:72-73 builds no other model)")
    if getattr(args, "classifier", "gcn") in _EAGER_CLASSIFIERS:
        check_classifier(args)
    return args


def train(args, device=None, log=print) -> float:
    from . import full_graph
    from .eval import _metrics
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    data = load_data(args, device)
    g = open_graph(data, device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    x = data.x.to(device).contiguous()
    y = data.y.to(device)
    large = _large_flag(args.large_graph)
    kind = getattr(args, "classifier", "gcn")
    gat = kind in _EAGER_CLASSIFIERS                   # (all train by autograd over the whole graph and return the logits alone)
    if gat and full_graph.use_large_path(g, large):
        raise ValueError(f"--classifier {kind}: graphs with 2^31 or more entries (the row-blocked path) take a GCN classifier")
    gcn_c = build_classifier(args, x.shape[1], data.num_classes, g).to(device)                               # full-batch.py:73
    optimizer_c = torch.optim.Adam(gcn_c.parameters(), lr=args.lr_gc)                                        # full-batch.py:76
    train_mask, val_mask, test_mask = (m.to(device) for m in (data.train_mask, data.val_mask, data.test_mask))
    val_idx = val_mask.nonzero().squeeze(1)
    for epoch in range(1, args.max_epochs + 1):
        t0 = time.time()
        evaluating = (epoch + 1) % args.eval_frequency == 0
        optimizer_c.zero_grad()                                                                               # full-batch.py:103
        if gat:                                                                                               # (autograd over the whole graph)
            logits = gcn_c(x, g)
            loss_c = full_graph._autograd_loss(logits[train_mask], y[train_mask])
            loss_c.backward()
            loss_c, val_logits = loss_c.detach(), (logits.detach()[val_idx] if evaluating else None)
            del logits
        else:
            loss_c, val_logits = full_graph.train_step(gcn_c, x, g, y, train_mask, eval_rows=val_idx if evaluating else None,
                                                       large_graph=large)                                     # full-batch.py:100-104
        optimizer_c.step()                                                                                    # full-batch.py:105
        log(f"epoch {epoch}: loss_c={float(loss_c):.6f}, {time.time() - t0:.2f}s")
        if evaluating:                                                                                        # full-batch.py:116-126
            _, f1 = _metrics(val_logits, y[val_idx])
            log(f"loss_c={float(loss_c):.6f}, valid_f1={f1:.3f}")
    test_idx = test_mask.nonzero().squeeze(1)                                                                 # full-batch.py:130-134
    if full_graph.use_large_path(g, large):
        with torch.no_grad():
            test_acc, test_f1 = full_graph.evaluate_rows(gcn_c, x, g, y, test_mask, False)
    else:
        with torch.no_grad():
            logits = gcn_c(x, g) if gat else gcn_c(x, g, large_graph=False)[0]
            test_acc, test_f1 = _metrics(logits[test_idx], y[test_idx])
            del logits
    log(f"test_accuracy={test_acc:.3f}, test_f1={test_f1:.3f}")
    return test_f1


def main(argv: Optional[Sequence[str]] = None) -> float:
    return repeat_runs(train, parse_args(argv))                                                               # full-batch.py:152-157


if __name__ == "__main__":
    main()
