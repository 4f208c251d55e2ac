"""A graph partition for Cluster-GCN, written to a file: a balanced start refined by size-constrained synchronous label
propagation (modules.cluster.refine_partition; the rule is in include/grapes_hip.h, the kernels in csrc/partition_kernels.hip).

    python -m grapes_amd.partition --dataset cora --num_parts 32 --out part.npy
    python -m grapes_amd.clustergcn --dataset cora --num_parts 32 --partition file --partition_file part.npy

* Flags: --dataset, --num_parts, --rounds 30, --imbalance 0.1 (a cluster may reach ceil(N / P) + floor(imbalance N / P) nodes),
  --start random|range, --seed (the random start's), --out x.npy.
* Writes an int32 array [N] of cluster ids in [0, num_parts) and prints the starting cut, the final cut and the rounds used.
* Not built: METIS-class quality — once clusters sit at their cap the rule stalls.

Datasets as in grapes_amd.main: a synthetic stand-in by name, or `module:function`.
"""
from __future__ import annotations

import argparse
from typing import Optional, Sequence

import torch

from .driver import open_graph, parse_with_dataset


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="grapes_amd.partition", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", type=str)
    ap.add_argument("--num_parts", type=int, required=True)
    ap.add_argument("--rounds", default=30, type=int)
    ap.add_argument("--imbalance", default=0.1, type=float)
    ap.add_argument("--start", default="random", choices=["random", "range"])
    ap.add_argument("--seed", default=None, type=int)
    ap.add_argument("--out", type=str, required=True)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    args = parse_with_dataset(_parser(), argv)
    if args.num_parts < 1 or args.rounds < 0 or not args.imbalance >= 0:
        raise ValueError("--num_parts is at least 1, --rounds and --imbalance at least 0")
    return args


def run(args, device=None, log=print):
    """Refines and writes the partition; returns (part int32 [N] on the device, info)."""
    import numpy as np
    from .clustergcn import partition_report
    from .main import load_data
    from .modules.cluster import make_partition, refine_partition
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    g = open_graph(load_data(args, device), device)
    start = make_partition(g.num_nodes, args.num_parts, args.start, args.seed)
    part, info = refine_partition(g, start, args.num_parts, rounds=args.rounds, imbalance=args.imbalance)
    np.save(args.out, part.cpu().numpy().astype(np.int32))
    log(partition_report(info))
    return part, info


def main(argv: Optional[Sequence[str]] = None):
    return run(parse_args(argv))


if __name__ == "__main__":
    main()
