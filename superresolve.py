#!/usr/bin/env python3
"""Offline super-resolution entry point: an LR event store in, the HR event
stream out as a new EVS store (engine/superresolve.py)."""

import argparse
import logging
import sys
from pathlib import Path

import torch
import yaml

from esr_amd.data import read_datalist
from esr_amd.data.store import GROUP_LEVELS, EventStore
from esr_amd.engine import load_model_from_checkpoint
from esr_amd.engine.superresolve import (super_resolve_store,
                                         super_resolve_stores)


def partition_by_resolution(pairs, group):
    """Split (src, dst) pairs into lists of one LR resolution each, keeping
    the list's order inside every part; `super_resolve_stores` runs one
    resolution at a time."""
    parts = {}
    level = GROUP_LEVELS.get(group, 1)
    for src, dst in pairs:
        H, W = EventStore(src).sensor_resolution
        parts.setdefault((round(H / level), round(W / level)),
                         []).append((src, dst))
    return list(parts.values())


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--input", type=str, default=None,
                   help="one EVS store; --output is then the store to write")
    p.add_argument("--data_list", type=str, default=None,
                   help="txt of EVS stores, processed one after the other; "
                        "--output is then a directory of <name>.evs stores")
    p.add_argument("--group", type=str, required=True,
                   help="event group of the input to super-resolve")
    p.add_argument("--output", type=str, required=True)
    p.add_argument("--scale", type=int, default=2)
    p.add_argument("--seqn", type=int, default=3)
    p.add_argument("--window", type=float, default=2048,
                   help="events per window, or seconds with --mode time")
    p.add_argument("--mode", choices=["events", "time"], default="events")
    p.add_argument("--redistribute", choices=["linear", "random"],
                   default="linear")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--capacity", type=int, default=None,
                   help="most events one window may emit (default "
                        "max(1024, 4 * scale^2 * longest window))")
    p.add_argument("--cell_cap", type=int, default=1023)
    p.add_argument("--amp", choices=["none", "bf16", "fp16"], default="none")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--no_graphs", action="store_true")
    p.add_argument("--max_windows", type=int, default=None)
    p.add_argument("--lanes", type=int, default=1,
                   help="with --data_list: recordings in flight at once, as "
                        "rows of one batched graph replay (default 1: one "
                        "recording after the other)")
    args = p.parse_args()

    logging.basicConfig(level=logging.WARNING, stream=sys.stderr)
    if (args.input is None) == (args.data_list is None):
        raise SystemExit("provide exactly one of --input and --data_list")
    amp_dtype = {"none": None, "bf16": torch.bfloat16,
                 "fp16": torch.float16}[args.amp]
    device = torch.device(args.device if torch.cuda.is_available() else "cpu")
    window = int(args.window) if args.mode == "events" else args.window
    model, _ = load_model_from_checkpoint(args.model_path, device=device,
                                          seqn=args.seqn)

    if args.input is not None:
        pairs = [(args.input, Path(args.output))]
    else:
        out_root = Path(args.output)
        out_root.mkdir(parents=True, exist_ok=True)
        pairs = [(src, out_root / f"{Path(src).stem}.evs")
                 for src in read_datalist(args.data_list)]

    if args.lanes < 1:
        raise SystemExit("--lanes must be positive")
    kw = dict(group=args.group, scale=args.scale, seqn=args.seqn,
              window=window, mode=args.mode, redistribute=args.redistribute,
              seed=args.seed, capacity=args.capacity, cell_cap=args.cell_cap,
              device=device, use_graphs=not args.no_graphs,
              amp_dtype=amp_dtype, max_windows=args.max_windows,
              checkpoint=args.model_path)
    summaries = {}
    if args.lanes > 1 and args.data_list is not None:
        done = {}
        for part in partition_by_resolution(pairs, args.group):
            done.update(super_resolve_stores(
                model, [(src, str(dst)) for src, dst in part],
                lanes=args.lanes, **kw))
        summaries = {str(dst): done[str(dst)] for _, dst in pairs}
    else:
        for src, dst in pairs:
            summaries[str(dst)] = super_resolve_store(model, src, str(dst),
                                                      **kw)
    out = next(iter(summaries.values())) if args.input is not None \
        else summaries
    print(yaml.safe_dump(out, sort_keys=False), end="")


if __name__ == "__main__":
    main()
