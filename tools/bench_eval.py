#!/usr/bin/env python3
"""Evaluation benchmark: windows/s of `infer_sequence` (the CPU-fed harness)
and of `infer_sequence_device`, on the same seeded checkpoint-less model and
the same synthetic file at 128 -> 256, without images.

Runs alternate (harness, device, harness, device, ...), the clock is read
after a device synchronisation on both sides, and every run is reported; so
is the time of one `restoration_metrics` call on the evaluator's four planes.

  python tools/bench_eval.py [--runs 3] [--events 2000000] [--amp none]
"""

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def dataloader_config(seql: int):
    return {
        "batch_size": 1, "shuffle": False, "num_workers": 0,
        "pin_memory": False, "drop_last": False, "use_ddp": False,
        "dataset": {
            "scale": 2, "ori_scale": "down2", "time_bins": 1,
            "mode": "events", "window": 2048, "sliding_window": 1024,
            "need_gt_frame": False, "need_gt_events": True,
            "real_world_test": False,
            "data_augment": {"enabled": False, "augment": [],
                             "augment_prob": []},
            "hot_filter": {"enabled": False},
            "sequence": {"sequence_length": seql, "seqn": 3,
                         "step_size": None,
                         "pause": {"enabled": False,
                                   "proba_pause_when_running": 0.05,
                                   "proba_pause_when_paused": 0.9}},
        },
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--seql", type=int, default=9)
    ap.add_argument("--basech", type=int, default=8)
    ap.add_argument("--amp", choices=["none", "bf16", "fp16"], default="none")
    ap.add_argument("--kernel-calls", type=int, default=200)
    ap.add_argument("--device", default="cuda:0"
                    if torch.cuda.is_available() else "cpu")
    args = ap.parse_args()

    from esr_amd.data.synthetic import write_synthetic_store
    from esr_amd.engine.device_inference import infer_sequence_device
    from esr_amd.engine.inference import build_metrics, infer_sequence
    from esr_amd.loss.device_metrics import metric_sums
    from esr_amd.models import build_model

    device = torch.device(args.device)
    on_gpu = device.type == "cuda"
    amp = {"none": None, "bf16": torch.bfloat16,
           "fp16": torch.float16}[args.amp]

    def sync():
        if on_gpu:
            torch.cuda.synchronize(device)

    torch.manual_seed(0)
    model = build_model("ESRNet", inch=2, basech=args.basech, num_frame=3,
                        upsampler="pixelshuffle").to(device).eval()
    metrics = build_metrics(device)
    cfg = dataloader_config(args.seql)

    with tempfile.TemporaryDirectory() as tmp:
        path = write_synthetic_store(Path(tmp) / "bench.evs", (256, 256),
                                     args.events, seed=0)

        def harness():
            return infer_sequence(cfg, path, model, device, metrics=metrics,
                                  save_images=False)

        def resident():
            return infer_sequence_device(cfg, path, model, device,
                                         metrics=metrics, save_images=False,
                                         amp_dtype=amp, return_maps=True)

        # one untimed run each: library plans, kernel selection
        harness()
        _, maps = resident()
        windows = int(maps["table"].size(0))

        runs = {"harness": [], "device": []}
        results = {}
        for _ in range(args.runs):
            for name, fn in (("harness", harness), ("device", resident)):
                sync()
                t0 = time.perf_counter()
                out = fn()
                sync()
                runs[name].append(windows / (time.perf_counter() - t0))
                results[name] = out[0] if isinstance(out, tuple) else out

    # the fused kernel alone, on planes shaped like the evaluator's
    esr, gt = maps["esr"][:1], maps["gt"][:1]
    pred = torch.cat([esr, maps["bicubic"][:1]]).contiguous()
    tgt = gt.repeat(2, 1, 1, 1).contiguous()
    kernel_us = None
    if on_gpu:
        for _ in range(10):
            metric_sums(pred, tgt)
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        sync()
        ev0.record()
        for _ in range(args.kernel_calls):
            metric_sums(pred, tgt)
        ev1.record()
        sync()
        kernel_us = ev0.elapsed_time(ev1) * 1e3 / args.kernel_calls

    print(json.dumps({
        "metric": "eval_windows_per_s", "device": str(device),
        "amp": args.amp, "windows": windows,
        "map": list(pred.shape[-2:]),
        "harness_windows_per_s": [round(v, 2) for v in runs["harness"]],
        "device_windows_per_s": [round(v, 2) for v in runs["device"]],
        "device_wins_every_run": all(
            d > h for d, h in zip(runs["device"], runs["harness"])),
        "restoration_metrics_us_per_call": None if kernel_us is None
        else round(kernel_us, 2),
        "device_time_per_window_ms": round(results["device"]["time"] * 1e3, 3),
        "harness_forward_per_window_ms":
            round(results["harness"]["time"] * 1e3, 3),
        "esr_ssim": {k: results[k]["esr_ssim"] for k in results},
    }))


if __name__ == "__main__":
    main()
