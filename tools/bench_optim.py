#!/usr/bin/env python3
"""Optimizer-phase microbenchmark: capturable foreach Adam vs FlatAdam.

The flagship parameter set (ESRNet basech 8, ~1.8 M fp32 params) with
seeded gradients; ONLY ``optimizer.step()`` is captured in a hipGraph and
replayed.  Arms, alternated ``--repeats`` times so the run-to-run spread is
visible:

    adam         torch.optim.Adam(capturable=True)   (the graphed trainer's
                                                       optimizer before
                                                       FlatAdam: the baseline)
    flat         FlatAdam, loss scaling off           (2 launches)
    flat_scaled  FlatAdam, loss scaling on            (3 launches)
    flat_clip         FlatAdam, gradient-norm clipping     (4 launches)
    flat_scaled_clip  FlatAdam, loss scaling and clipping  (4 launches)

The clipping arms clip on every replay (max_grad_norm 1.0 against a seeded
gradient of norm 1.3).

Reports microseconds per step per arm and repeat, the bytes the algorithm
has to move (fp32 streams x 4n, computed from the shapes) over that time
against the 6.29 TB/s measured copy rate, and - with ``--launch-counts`` -
the kernel launches per replay and each kernel's mean time, taken from one
``rocprofv3 --kernel-trace --stats`` run per arm of this script itself
(``--profile-arm``, a fresh child process each; timing is done with the
profiler off).

Usage (GPU box):
    python tools/bench_optim.py --replays 200 --repeats 3 --launch-counts
"""

import argparse
import csv
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

ARMS = ("adam", "flat", "flat_scaled", "flat_clip", "flat_scaled_clip")
CLIP_MAX_NORM = 1.0
COPY_RATE_TBS = 6.29  # measured device copy rate, MI355X
# fp32 streams of length n one step has to move: read p, g, m, v and write
# p, m, v; the finite check, or the stats pass that replaces it with
# clipping on, reads g once more
STREAMS = {"adam": 7, "flat": 7, "flat_scaled": 8, "flat_clip": 8,
           "flat_scaled_clip": 8}


def build_arm(name, device):
    """Model params + seeded grads + optimizer for one arm; returns
    (optimizer, numel, captured graph)."""
    import torch
    from esr_amd.engine.capture import capture_graph
    from esr_amd.models import build_model
    from esr_amd.optim import FlatAdam

    torch.manual_seed(0)
    model = build_model("ESRNet", inch=2, basech=8, num_frame=3,
                        upsampler="pixelshuffle").to(device)
    params = [p for p in model.parameters() if p.requires_grad]
    numel = sum(p.numel() for p in params)
    gen = torch.Generator(device=device).manual_seed(1)
    grads = [torch.randn(p.shape, device=device, generator=gen) * 1e-3
             for p in params]
    if name == "adam":
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        for p, g in zip(params, grads):
            p.grad = g
    else:
        ls = {} if "scaled" in name else None
        clip = CLIP_MAX_NORM if name.endswith("clip") else None
        opt = FlatAdam(params, lr=1e-3, loss_scale=ls, max_grad_norm=clip)
        scale = opt.loss_scale_value
        with torch.no_grad():
            for p, g in zip(params, grads):
                p.grad.copy_(g * scale)
    graph, _ = capture_graph(opt.step, warmup=3)
    return opt, numel, graph


def time_replays(graph, replays):
    import torch
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / replays  # us per step


def profile_arm(name, replays):
    """Child mode for rocprofv3: capture one arm and replay it."""
    import torch
    _, _, graph = build_arm(name, torch.device("cuda:0"))
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()


def launch_counts(replays, out_dir, timeout):
    """Kernel launches per replay and arm from rocprofv3's kernel stats: a
    kernel launched k times per replay shows calls = k * replays + a few
    set-up calls (< replays), so floor(calls / replays) = k."""
    prof = out_dir / "prof"
    prof.mkdir(parents=True, exist_ok=True)
    counts = {}
    for arm in ARMS:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format",
               "csv", "-d", str(prof), "-o", arm, "--", sys.executable,
               str(Path(__file__).resolve()), "--profile-arm", arm,
               "--replays", str(replays)]
        proc = subprocess.run(cmd, capture_output=True, text=True,
                              timeout=timeout, cwd=str(REPO))
        if proc.returncode != 0:
            raise RuntimeError(f"rocprofv3 run of arm {arm} failed "
                               f"({proc.returncode}): {proc.stderr[-1500:]}")
        stats = sorted(prof.rglob(f"{arm}_kernel_stats.csv"))
        if not stats:
            raise RuntimeError(f"no {arm}_kernel_stats.csv under {prof}")
        per_kernel, mean_us = {}, {}
        with open(stats[-1], newline="") as f:
            for row in csv.DictReader(f):
                k = int(row["Calls"]) // replays
                if k:  # instantiations sharing the 80-char prefix add up
                    key = row["Name"][:80]
                    per_kernel[key] = per_kernel.get(key, 0) + k
                    if row.get("AverageNs"):
                        mean_us[key] = round(float(row["AverageNs"]) / 1e3, 2)
        counts[arm] = {"launches_per_step": sum(per_kernel.values()),
                       "kernels": per_kernel, "kernel_mean_us": mean_us}
        # the raw trace is large; the aggregated stats are the evidence
        for fn in prof.rglob(f"{arm}_*"):
            if fn.is_file() and not fn.name.endswith("_stats.csv"):
                fn.unlink()
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launch-counts", action="store_true",
                    help="count launches per replay with one rocprofv3 run "
                         "per arm (child processes)")
    ap.add_argument("--profile-timeout", type=int, default=240)
    ap.add_argument("--out", default="runs/bench_optim")
    ap.add_argument("--profile-arm", choices=ARMS, default=None,
                    help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.replays < 1 or args.repeats < 1:
        ap.error("--replays and --repeats must be >= 1")

    if args.profile_arm:
        profile_arm(args.profile_arm, args.replays)
        return

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_optim.py measures on the GPU; no GPU found")
    out_dir = REPO / args.out
    out_dir.mkdir(parents=True, exist_ok=True)

    counts = None
    if args.launch_counts:  # before this process opens the GPU
        counts = launch_counts(args.replays, out_dir, args.profile_timeout)

    device = torch.device("cuda:0")
    arms = {name: build_arm(name, device) for name in ARMS}
    numel = arms["adam"][1]
    for _, _, graph in arms.values():
        for _ in range(args.warmup):
            graph.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in ARMS}
    for _ in range(args.repeats):
        for name in ARMS:  # alternate the arms inside every repeat
            times[name].append(time_replays(arms[name][2], args.replays))

    result = {"numel": numel, "replays": args.replays, "arms": {}}
    for name in ARMS:
        us = times[name]
        best = min(us)
        nbytes = STREAMS[name] * 4 * numel
        rate = nbytes / (best * 1e-6) / 1e12
        result["arms"][name] = {
            "us_per_step": [round(t, 2) for t in us],
            "min_us": round(best, 2), "max_us": round(max(us), 2),
            "bytes_per_step": nbytes,
            "tb_per_s_at_min": round(rate, 3),
            "share_of_copy_rate": round(rate / COPY_RATE_TBS, 3),
            "launches_per_step": counts[name]["launches_per_step"]
            if counts else None,
        }
        if counts:
            result["arms"][name]["kernels"] = counts[name]["kernels"]
            result["arms"][name]["kernel_mean_us"] = \
                counts[name]["kernel_mean_us"]
    opt = arms["flat_scaled"][0]
    result["flat_scaled_skipped_steps"] = opt.skipped_steps
    for name in ("flat_clip", "flat_scaled_clip"):
        opt = arms[name][0]
        result[f"{name}_grad_norm"] = round(opt.grad_norm_value, 6)
        result[f"{name}_clipped_steps"] = opt.clipped_steps
        result[f"{name}_skipped_steps"] = opt.skipped_steps
    with open(out_dir / "bench_optim.json", "w") as f:
        json.dump(result, f, indent=2)

    print(f"optimizer phase, {numel} fp32 params, {args.replays} graph "
          f"replays per timing, {args.repeats} alternated repeats")
    print("| arm | us/step per repeat | launches/step | MB/step | "
          "TB/s at min | share of 6.29 TB/s |")
    print("|---|---|---|---|---|---|")
    for name, r in result["arms"].items():
        print(f"| {name} | {' / '.join(f'{t:.1f}' for t in r['us_per_step'])}"
              f" | {r['launches_per_step'] if counts else 'not counted'} | "
              f"{r['bytes_per_step'] / 1e6:.1f} | {r['tb_per_s_at_min']:.2f}"
              f" | {100 * r['share_of_copy_rate']:.0f}% |")
    if counts:
        for name in ARMS:
            print(f"kernel mean us, {name}: "
                  f"{json.dumps(counts[name]['kernel_mean_us'])}")
    print(json.dumps({k: v for k, v in result.items() if k != "arms"}
                     | {"min_us": {n: r["min_us"]
                                   for n, r in result["arms"].items()}}))


if __name__ == "__main__":
    main()
