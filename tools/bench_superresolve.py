#!/usr/bin/env python3
"""Offline super-resolution benchmark: windows/s and output events/s of
`super_resolve_store` on the device, against what was possible before it: a
`StreamingESR.push_events` loop that downloads each window's events.  Same
seeded checkpoint-less model, same synthetic recording at 128 -> 256 with
windows of 2048 events.

An untrained net predicts next to no events, so both sides run the net plus
`--lift` x its mid input frame (default scale^2 = 4: about four HR events per
LR event, what a trained 2x model emits).

Runs alternate (loop, device, loop, device, ...), the clock is read after a
device synchronisation on both sides and every run is reported; so are the
time of one `sr_emit_window` call on a predicted window and its share of a
step.

  python tools/bench_superresolve.py [--runs 3] [--events 2000000]

With `--recordings R --lanes N [N ...]` the benchmark is another one: R
synthetic recordings of unequal length (0.4 x to 1.6 x `--events`, shuffled)
converted by today's loop around `super_resolve_store` and by
`super_resolve_stores` with N lanes, the arms alternating in one process.  A
run includes set-up, capture and writing the stores.  It also times
`sr_emit_lanes` alone at S = 8 next to 8 calls of `sr_emit_window`.

  python tools/bench_superresolve.py --recordings 16 --lanes 4 8 16
"""

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


class Lifted(torch.nn.Module):
    def __init__(self, net, lift):
        super().__init__()
        self.net = net
        self.lift = float(lift)
        self.time_propagate = net.time_propagate

    def reset_states(self):
        self.net.reset_states()

    def forward(self, x):
        return self.net(x) + self.lift * x[:, (x.size(1) - 1) // 2]


def recordings_arm(args, model, device, amp, sync):
    """Loop of `super_resolve_store` against `super_resolve_stores`."""
    from esr_amd.data.synthetic import write_synthetic_store
    from esr_amd.engine.superresolve import (super_resolve_store,
                                             super_resolve_stores)
    from esr_amd.ops.native import get_ext

    R = args.recordings
    rng = np.random.default_rng(0)
    factors = rng.permutation(np.linspace(0.4, 1.6, R))
    kw = dict(group="down2", scale=2, seqn=3, window=args.window,
              device=device, amp_dtype=amp, chunk_windows=args.chunk_windows)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        srcs = [write_synthetic_store(tmp / f"rec{i}.evs", (256, 256),
                                      int(args.events * f), levels=(1, 2),
                                      num_images=0, seed=i)
                for i, f in enumerate(factors)]

        def loop(tag):
            return [super_resolve_store(model, src,
                                        str(tmp / f"{tag}_{i}.evs"), **kw)
                    for i, src in enumerate(srcs)]

        def lanes(n, tag):
            pairs = [(src, str(tmp / f"{tag}_{i}.evs"))
                     for i, src in enumerate(srcs)]
            return list(super_resolve_stores(model, pairs, lanes=n,
                                             **kw).values())

        arms = {"loop": lambda: loop("loop")}
        for n in args.lanes:
            arms[f"lanes{n}"] = (lambda n=n: lanes(n, f"lanes{n}"))
        # one untimed run each: library plans, kernel selection
        summaries = {name: run() for name, run in arms.items()}
        windows = sum(s["windows_emitted"] for s in summaries["loop"])
        events_out = sum(s["events_out"] for s in summaries["loop"])
        same = {name: [s["events_out"] for s in ss]
                == [s["events_out"] for s in summaries["loop"]]
                for name, ss in summaries.items()}
        times = {name: [] for name in arms}
        for _ in range(args.runs):
            for name, run in arms.items():
                sync()
                t0 = time.perf_counter()
                run()
                sync()
                times[name].append(time.perf_counter() - t0)

        # the emission alone at S = 8: one sr_emit_lanes call next to 8
        # sr_emit_window calls on the same predicted windows
        emit_us = {}
        ext = get_ext() if device.type == "cuda" else None
        if ext is not None and hasattr(ext, "sr_emit_lanes"):
            S = 8
            _, kept = super_resolve_store(model, srcs[0], str(tmp / "k.evs"),
                                          max_windows=S + 2, keep=True, **kw)
            pred = kept["pred"][-S:].contiguous()
            cap = summaries["loop"][0]["capacity"]
            dts = (torch.uint16, torch.uint16, torch.float64, torch.int8)
            cols = [torch.zeros(S, cap, dtype=dt, device=device)
                    for dt in dts]
            cs = torch.zeros(S, 5, dtype=torch.int64, device=device)
            win = torch.tensor([[0.0, 1.0]] * S, dtype=torch.float64,
                               device=device)
            ctl = torch.tensor([[1, cap]] * S, dtype=torch.int64,
                               device=device)
            ncells = pred[0].numel()
            scratch = ext.sr_emit_lanes_scratch(pred, S, ncells, cap)
            one = ext.sr_emit_scratch(pred, ncells, cap)

            def emit_lanes():
                cs.zero_()
                ext.sr_emit_lanes(pred, win, cols, cs, ctl, cap, 1023, 0, 0,
                                  scratch)

            def emit_windows():
                cs.zero_()
                for s in range(S):
                    ext.sr_emit_window(pred[s], win[s],
                                       [c[s] for c in cols], cs[s], cap,
                                       1023, 0, 0, one)
            for name, fn in (("sr_emit_lanes_s8", emit_lanes),
                             ("sr_emit_window_x8", emit_windows)):
                for _ in range(10):
                    fn()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                sync()
                e0.record()
                for _ in range(args.kernel_calls):
                    fn()
                e1.record()
                sync()
                emit_us[name] = round(
                    e0.elapsed_time(e1) * 1e3 / args.kernel_calls, 1)

    print(json.dumps({
        "metric": "superresolve_lanes_windows_per_s", "device": str(device),
        "amp": args.amp, "lift": args.lift, "window": args.window,
        "recordings": R, "windows": windows, "events_out": events_out,
        "windows_per_recording": [s["windows_emitted"]
                                  for s in summaries["loop"]],
        "same_events_out_as_loop": same,
        "seconds": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "windows_per_s": {k: [round(windows / t, 1) for t in v]
                          for k, v in times.items()},
        "events_out_per_s": {k: [round(events_out / t) for t in v]
                             for k, v in times.items()},
        "beats_loop_every_run": {
            k: all(a < b for a, b in zip(v, times["loop"]))
            for k, v in times.items() if k != "loop"},
        "emit_us_per_call": emit_us,
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--events", type=int, default=2_000_000,
                    help="events of the 256x256 recording; its down2 group "
                         "(the input) holds a quarter of them")
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--basech", type=int, default=8)
    ap.add_argument("--lift", type=float, default=4.0)
    ap.add_argument("--amp", choices=["none", "bf16", "fp16"], default="none")
    ap.add_argument("--chunk_windows", type=int, default=256)
    ap.add_argument("--kernel-calls", type=int, default=200)
    ap.add_argument("--device", default="cuda:0"
                    if torch.cuda.is_available() else "cpu")
    ap.add_argument("--recordings", type=int, default=0,
                    help="run the lanes arm instead: this many recordings of "
                         "unequal length around --events")
    ap.add_argument("--lanes", type=int, nargs="+", default=[8],
                    help="lane counts of the lanes arm")
    args = ap.parse_args()

    from esr_amd.data.store import EventStore
    from esr_amd.data.synthetic import write_synthetic_store
    from esr_amd.engine.streaming import StreamingESR
    from esr_amd.engine.superresolve import super_resolve_store, tile_windows
    from esr_amd.models import build_model
    from esr_amd.ops.native import get_ext

    device = torch.device(args.device)
    on_gpu = device.type == "cuda"
    amp = {"none": None, "bf16": torch.bfloat16,
           "fp16": torch.float16}[args.amp]

    def sync():
        if on_gpu:
            torch.cuda.synchronize(device)

    torch.manual_seed(0)
    net = build_model("ESRNet", inch=2, basech=args.basech, num_frame=3,
                      upsampler="pixelshuffle")
    model = Lifted(net, args.lift).to(device).eval()
    if args.recordings:
        return recordings_arm(args, model, device, amp, sync)

    with tempfile.TemporaryDirectory() as tmp:
        src = write_synthetic_store(Path(tmp) / "bench.evs", (256, 256),
                                    args.events, levels=(1, 2), num_images=0,
                                    seed=0)
        st = EventStore(src)
        n = st.num_events("down2")
        ev = torch.from_numpy(st.events("down2", 0, n)).float()
        tiles = tile_windows(np.asarray(st.ts("down2")[:n]), "events",
                             args.window)
        spans = list(zip(tiles["begin"].tolist(), tiles["end"].tolist()))

        def device_path():
            return super_resolve_store(
                model, src, str(Path(tmp) / "hr.evs"), group="down2", scale=2,
                seqn=3, window=args.window, device=device, amp_dtype=amp,
                chunk_windows=args.chunk_windows, keep=False)

        def push_loop():
            """The route that existed before: one push_events per window,
            each window's events downloaded, rows stacked on the host."""
            srv = StreamingESR(model, (128, 128), scale=2, seqn=3,
                               device=device, use_graphs=True, amp_dtype=amp)
            srv.reset()
            rows = 0
            for a, b in spans:
                out = srv.push_events(ev[:, a:b])
                if out is not None:
                    rows += int(out.cpu().shape[0])
            return rows

        # one untimed run each: library plans, kernel selection, capture
        push_loop()
        summary = device_path()
        windows = summary["windows_emitted"]

        runs = {"push_loop": [], "device": []}
        loop_rows = 0
        for _ in range(args.runs):
            sync()
            t0 = time.perf_counter()
            loop_rows = push_loop()
            sync()
            runs["push_loop"].append(time.perf_counter() - t0)
            sync()
            t0 = time.perf_counter()
            summary = device_path()
            sync()
            runs["device"].append(time.perf_counter() - t0)

        # the emission alone, on one predicted window
        emit_us = None
        ext = get_ext() if on_gpu else None
        if ext is not None and hasattr(ext, "sr_emit_window"):
            _, kept = super_resolve_store(
                model, src, str(Path(tmp) / "k.evs"), group="down2", scale=2,
                seqn=3, window=args.window, device=device, amp_dtype=amp,
                max_windows=8, keep=True)
            pred = kept["pred"][-1].contiguous()
            cap = summary["capacity"]
            cols = [torch.zeros(cap, dtype=torch.uint16, device=device),
                    torch.zeros(cap, dtype=torch.uint16, device=device),
                    torch.zeros(cap, dtype=torch.float64, device=device),
                    torch.zeros(cap, dtype=torch.int8, device=device)]
            cs = torch.zeros(5, dtype=torch.int64, device=device)
            win = torch.tensor([0.0, 1.0], dtype=torch.float64, device=device)
            scratch = ext.sr_emit_scratch(pred, pred.numel(), cap)

            def emit():
                cs.zero_()
                ext.sr_emit_window(pred, win, cols, cs, cap, 1023, 0, 0,
                                   scratch)
            for _ in range(10):
                emit()
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            sync()
            e0.record()
            for _ in range(args.kernel_calls):
                emit()
            e1.record()
            sync()
            emit_us = e0.elapsed_time(e1) * 1e3 / args.kernel_calls

    dev_wps = [windows / t for t in runs["device"]]
    loop_wps = [windows / t for t in runs["push_loop"]]
    step_us = 1e6 * min(runs["device"]) / windows
    print(json.dumps({
        "metric": "superresolve_windows_per_s", "device": str(device),
        "amp": args.amp, "lift": args.lift, "window": args.window,
        "windows": windows, "events_in": summary["events_in"],
        "events_out": summary["events_out"],
        "events_dropped": summary["events_dropped"],
        "push_loop_events_out": loop_rows,
        "device_windows_per_s": [round(v, 1) for v in dev_wps],
        "push_loop_windows_per_s": [round(v, 1) for v in loop_wps],
        "device_events_out_per_s": [round(summary["events_out"] / t)
                                    for t in runs["device"]],
        "push_loop_events_out_per_s": [round(loop_rows / t)
                                       for t in runs["push_loop"]],
        "device_wins_every_run": all(d > p for d, p in zip(dev_wps,
                                                           loop_wps)),
        "device_step_us": round(step_us, 1),
        "sr_emit_window_us_per_call": None if emit_us is None
        else round(emit_us, 1),
        "emit_share_of_step": None if emit_us is None
        else round(emit_us / step_us, 3),
    }))


if __name__ == "__main__":
    main()
