#!/usr/bin/env python3
"""Measure the CPU dataloader feed rate vs worker count.

8-GPU readiness: a node feeding 8 ranks at the flagship step rate needs
~23k items/s aggregate (batch 64 x 8 ranks x ~7.5 steps/s x 6 windows
-> items = sequence elements; see profiles/README.md).  This measures
items/s of SequenceDataLoader at several num_workers on the actual host
and reports the worker count needed per rank.

Usage: python tools/bench_dataloader.py [--seconds 12] [--workers 0 2 4 8]
       python tools/bench_dataloader.py --device [cuda:0] [--reps 7]

--device measures DeviceSequenceLoader (events resident on the device, one
splat kernel per batch) on the same synthetic data set instead: items/s as
the median of --reps timed repetitions after a warm-up, the device
synchronised before every clock read, and the per-batch split into job-table
build (host), H2D copy, zero and kernel.
"""

import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _dl_config(datalist, workers, batch):
    ds = {
        "scale": 2, "ori_scale": "down2", "time_bins": 1,
        "need_gt_frame": False, "need_gt_events": True,
        "mode": "events", "window": 2048, "sliding_window": 1024,
        "data_augment": {"enabled": True,
                         "augment": ["Horizontal", "Vertical", "Polarity"],
                         "augment_prob": [0.5, 0.5, 0.5]},
        "hot_filter": {"enabled": False},
        "sequence": {"sequence_length": 8, "seqn": 3, "step_size": None,
                     "pause": {"enabled": False,
                               "proba_pause_when_running": 0.05,
                               "proba_pause_when_paused": 0.9}},
    }
    return {"use_ddp": False, "path_to_datalist_txt": str(datalist),
            "batch_size": batch, "shuffle": True, "num_workers": workers,
            "pin_memory": False, "drop_last": True, "dataset": ds,
            "persistent_workers": workers > 0}


def _device_arm(args, datalist):
    import torch
    from esr_amd.data import DeviceSequenceLoader

    cfg = _dl_config(datalist, 0, args.batch)
    cfg["dataset"]["fields"] = ["inp_scaled_cnt", "gt_cnt"]
    cfg["device_resident"] = True
    device = torch.device(args.device)
    on_gpu = device.type == "cuda"
    loader = DeviceSequenceLoader(cfg, device)
    if len(loader) == 0:
        raise SystemExit(f"--batch {args.batch} exceeds the "
                         f"{len(loader.dataset)} items of the data set")

    def sync():
        if on_gpu:
            torch.cuda.synchronize(device)

    def batches(n):
        done = 0
        while done < n:
            for _ in loader:
                done += 1
                if done == n:
                    break

    batches(args.warmup)
    sync()
    rates = []
    for _ in range(max(args.reps, 5)):
        sync()
        t0 = time.perf_counter()
        batches(args.batches)
        sync()
        dt = time.perf_counter() - t0
        # one loader batch = batch sequences x 8 windows = items
        rates.append(args.batches * args.batch * 8 / dt)
    med = statistics.median(rates)
    print(f"device loader on {device} "
          f"({'HIP kernel' if loader._ext is not None else 'torch splat'}), "
          f"{loader.resident_bytes / 2**20:.1f} MiB resident, batch "
          f"{args.batch} x 8 windows")
    print(f"items/s  median {med:.0f}  min {min(rates):.0f}  "
          f"max {max(rates):.0f}  over {len(rates)} reps of {args.batches} "
          f"batches  ({1e6 * args.batch * 8 / med:.0f} us per batch)")

    # per-batch split; the device stages are timed back to back with events
    n = args.batches
    indices = loader.last_indices
    t0 = time.perf_counter()
    for _ in range(n):
        loader.job_table(indices)
    host_us = 1e6 * (time.perf_counter() - t0) / n
    print(f"split per batch: job table (host) {host_us:.1f} us", end="")
    if on_gpu:
        stage = loader._stage[0]["jobs"]
        stages = {
            "H2D": lambda: loader._jobs.copy_(stage, non_blocking=True),
            "zero": lambda: loader._out.zero_(),
            "kernel": lambda: loader._splat(zero=False),
        }
        for name, fn in stages.items():
            for _ in range(10):
                fn()
            sync()
            beg = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            beg.record()
            for _ in range(n):
                fn()
            end.record()
            sync()
            print(f", {name} {1e3 * beg.elapsed_time(end) / n:.1f} us",
                  end="")
    print()
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--workers", type=int, nargs="*", default=[0, 2, 4, 8])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--fields", action="store_true",
                    help="restrict items to the trainer's 3 fields")
    ap.add_argument("--device", nargs="?", const="cuda:0", default=None,
                    help="measure DeviceSequenceLoader on this device "
                         "instead of the CPU workers")
    ap.add_argument("--reps", type=int, default=7,
                    help="--device: timed repetitions (at least 5)")
    ap.add_argument("--batches", type=int, default=200,
                    help="--device: batches per repetition")
    ap.add_argument("--warmup", type=int, default=50,
                    help="--device: untimed batches first")
    args = ap.parse_args()

    from esr_amd.data import SequenceDataLoader, make_synthetic_dataset

    tmp = tempfile.mkdtemp(prefix="dlbench")
    datalist = make_synthetic_dataset(Path(tmp), num_sequences=4,
                                      resolution=(128, 128),
                                      num_events=400_000, seed=3)
    if args.device is not None:
        _device_arm(args, datalist)
        return
    print(f"{'workers':>8s} {'items/s':>10s} {'seq items/s':>12s}")
    results = {}
    for w in args.workers:
        cfg = _dl_config(datalist, w, args.batch)
        if args.fields:
            cfg["dataset"]["fields"] = ["inp_scaled_cnt", "gt_cnt", "inp_cnt"]
        dl = SequenceDataLoader(cfg)
        it = iter(dl)
        next(it)  # warm workers
        n = 0
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.seconds:
            try:
                next(it)
            except StopIteration:
                it = iter(dl)
                continue
            n += 1
        dt = time.perf_counter() - t0
        # one loader batch = batch sequences x 8 windows = items
        items = n * args.batch * 8
        results[w] = items / dt
        print(f"{w:8d} {items / dt:10.0f} {n * args.batch / dt:12.1f}")
    best = max(results.values())
    need = 23000
    print(f"\nnode target ~{need} items/s over 8 ranks -> "
          f"{need / 8:.0f}/rank; best measured {best:.0f} items/s "
          f"({'OK with' if best >= need / 8 else 'needs more than'} "
          f"measured workers per rank)")


if __name__ == "__main__":
    main()
