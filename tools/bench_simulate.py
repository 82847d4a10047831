#!/usr/bin/env python3
"""Event-simulator benchmark: the numpy oracle (`simulate_events_log`) and
the device simulator (`DeviceEventSimulator`) on the same log frames, in the
same process: frame pairs/s and events/s, and the device's stages (count,
scan, emit, the two sorts, unpack, download) timed with device events.

Two sizes: 64 frames at 256x256, and 16 frames at 720x1280, each at five
levels (1, 2, 4, 8, 16), as the dataset generation runs them.  The frames are
a smooth random texture panned at 240 fps; the log frames of every level are
made once on the device and handed to both sides.  The device is checked
against the oracle (every row equal) before it is timed.

  python tools/bench_simulate.py [--runs 3] [--sizes small large]
"""

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SIZES = {"small": (64, 256, 256), "large": (16, 720, 1280)}
LEVELS = (1, 2, 4, 8, 16)


def panned_texture(T, H, W, seed=0):
    """A low-pass random texture in [0, 1], panned by (1, 2) pixels a frame."""
    rng = np.random.default_rng(seed)
    h, w = H + T, W + 2 * T
    spec = np.fft.rfft2(rng.random((h, w)))
    fy = np.fft.fftfreq(h)[:, None]
    fx = np.fft.rfftfreq(w)[None, :]
    tex = np.fft.irfft2(spec * np.exp(-(fy ** 2 + fx ** 2) * (2 * np.pi * 4) ** 2
                                      / 2), s=(h, w))
    tex = (tex - tex.min()) / np.ptp(tex)
    return np.stack([tex[t:t + H, 2 * t:2 * t + W] for t in range(T)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", choices=list(SIZES),
                    default=list(SIZES))
    ap.add_argument("--cp", type=float, default=0.2)
    ap.add_argument("--cn", type=float, default=0.2)
    ap.add_argument("--refractory", type=float, default=1e-4)
    ap.add_argument("--max_chunk_events", type=int, default=1 << 22)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()

    from esr_amd.data.simulate import simulate_events_log
    from esr_amd.data.simulate_device import (STAGES, DeviceEventSimulator,
                                              _log_frames, _stack_chunks)
    from esr_amd.ops.native import require_ext

    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("bench_simulate.py measures the device: a GPU is "
                         "required")
    require_ext()
    walk = (args.cp, args.cn, args.refractory)

    def sim_for(logf, profile=False):
        return DeviceEventSimulator(logf.shape[1], logf.shape[2], *walk,
                                    device, args.max_chunk_events,
                                    profile=profile)

    for size in args.sizes:
        T, H, W = SIZES[size]
        frames = torch.from_numpy(panned_texture(T, H, W)).to(device)
        ts = np.arange(T) / 240.0
        logs = {lvl: _log_frames(frames, lvl) for lvl in LEVELS}
        logs_np = {lvl: v.cpu().numpy() for lvl, v in logs.items()}

        # untimed: the check, and the first launches of every kernel
        events = {}
        for lvl in LEVELS:
            want = simulate_events_log(logs_np[lvl], ts, *walk)
            got = _stack_chunks(sim_for(logs[lvl]).feed(logs[lvl], ts))
            if not np.array_equal(got, want):
                raise SystemExit(f"{size} level {lvl}: the device simulator "
                                 "differs from the oracle")
            events[lvl] = int(want.shape[1])
        total = sum(events.values())
        pairs = (T - 1) * len(LEVELS)

        oracle_s, device_s, stages = [], [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            for lvl in LEVELS:
                simulate_events_log(logs_np[lvl], ts, *walk)
            oracle_s.append(time.perf_counter() - t0)

            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for lvl in LEVELS:       # set-up, upload-free feed, download
                for _chunk in sim_for(logs[lvl]).feed(logs[lvl], ts):
                    pass
            torch.cuda.synchronize(device)
            device_s.append(time.perf_counter() - t0)

            # the stages in a run of their own: the events serialise them
            ms = {s: 0.0 for s in STAGES}
            for lvl in LEVELS:
                sim = sim_for(logs[lvl], profile=True)
                for _chunk in sim.feed(logs[lvl], ts):
                    pass
                for s, v in sim.timer.totals_ms().items():
                    ms[s] += v
            stages.append({s: round(v, 3) for s, v in ms.items()})

        print(json.dumps({
            "metric": "simulate_frame_pairs_per_s", "size": size,
            "frames": T, "resolution": [H, W], "levels": list(LEVELS),
            "cp": args.cp, "cn": args.cn, "refractory": args.refractory,
            "events": events, "events_total": total, "frame_pairs": pairs,
            "oracle_seconds": [round(t, 4) for t in oracle_s],
            "device_seconds": [round(t, 4) for t in device_s],
            "oracle_frame_pairs_per_s": [round(pairs / t, 1)
                                         for t in oracle_s],
            "device_frame_pairs_per_s": [round(pairs / t, 1)
                                         for t in device_s],
            "oracle_events_per_s": [round(total / t) for t in oracle_s],
            "device_events_per_s": [round(total / t) for t in device_s],
            "device_beats_oracle_every_run": all(
                d < o for d, o in zip(device_s, oracle_s)),
            "device_stage_ms": stages,
        }))


if __name__ == "__main__":
    main()
