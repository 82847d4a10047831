"""Evaluation on the device: `infer_sequence` without a host round trip per
window.

`infer_sequence` (engine/inference.py) builds every window on the CPU, runs
one eager forward, copies the prediction to the host and computes twelve
metrics there, each ending in `.item()`.  `infer_sequence_device` evaluates
the same windows from pieces that already live on the device:

  * the file's events, packed one word each, and the whole job table are
    uploaded once (`pack_events`, `evs_batch_splat` of data/device_loader.py);
  * per window: a device-to-device copy of the window's job rows, two splat
    launches (HR input frames + HR GT, and the LR count map as a GT-style job
    on the LR grid), the forward with the recurrence in one static state
    buffer, the bicubic baseline, ONE fused metrics call
    (loss/device_metrics.py) over [esr, bicubic] x 2 channels, LPIPS, and the
    row written into a device table;
  * on CUDA all of that is one captured graph replayed per window; nothing
    synchronises until the single table download at the end.

The CPU harness stays and is the oracle (tests/test_device_eval.py): same
windows, same result keys, same results.yml.  Rendered PNGs, augmentation,
noise, hot-pixel filtering, custom resolutions and pauses are the harness's;
asking for them here is a ValueError.
"""

from __future__ import annotations

import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
import yaml

from ..data.device_loader import FLAG_GT, batch_splat_torch, pack_events
from ..data.sequence import SequenceDataset
from ..loss.device_metrics import finalize, metric_sums
from ..ops.native import require_ext
from .capture import amp_autocast, capture_graph, state_holder
from .inference import build_metrics

__all__ = ["infer_sequence_device", "TIME_NOTE"]

_DEFAULT_MAX_BYTES = 8 << 30
_NAMES = ("esr", "bicubic")
_ROW = 4 * 5 + 2          # [esr, bicubic] x 2 channels x 5 sums, 2 lpips
TIME_NOTE = ("per window: splat + forward + metrics on the device "
             "(infer_sequence times the forward alone)")


def _refuse(cfg: dict, save_images: bool) -> None:
    ds = cfg["dataset"]

    def no(key, why=""):
        raise ValueError(f"infer_sequence_device does not support {key}"
                         f"{why}; use infer_sequence")

    for key in ("data_augment", "hot_filter", "add_noise"):
        if (ds.get(key) or {}).get("enabled", False):
            no(f"dataset.{key}.enabled")
    if ds.get("custom_resolution") is not None:
        no("dataset.custom_resolution")
    if ds.get("real_world_test", False):
        no("dataset.real_world_test")
    if ((ds.get("sequence") or {}).get("pause") or {}).get("enabled", False):
        no("dataset.sequence.pause.enabled")
    if not ds.get("need_gt_events", False):
        no("dataset.need_gt_events: false", " (the metrics need a GT)")
    if int(cfg.get("batch_size", 1)) != 1:
        no(f"batch_size = {cfg.get('batch_size')}", " (windows are "
           "evaluated one at a time)")
    if save_images:
        no("save_images=True", " (rendered PNGs stay with the CPU harness)")


def _upload(ds: SequenceDataset, n_items: int, seqn: int, mid_idx: int,
            resident_cfg, device):
    """Pack the file's events and build the job table of every item; one
    upload each.  Returns (packed, hr_jobs [n, seqn+1, 4], lr_jobs [n, 1, 4],
    max_job_len)."""
    d = ds.dataset
    max_bytes = _DEFAULT_MAX_BYTES
    if isinstance(resident_cfg, dict):
        max_bytes = int(resident_cfg.get("max_bytes", _DEFAULT_MAX_BYTES))
    prefixes = [d.inp_prefix]
    if d.gt_prefix != d.inp_prefix:
        prefixes.append(d.gt_prefix)
    counts = [d.store.num_events(p) for p in prefixes]
    total = sum(counts)
    need = 4 * total + 16 * n_items * (seqn + 2)
    if need > max_bytes:
        raise ValueError(
            f"device_resident: the packed events and job table need {need} "
            f"bytes, more than device_resident.max_bytes = {max_bytes}")
    if total > 2 ** 31 - 1:
        raise ValueError(f"device_resident: {total} events exceed the int32 "
                         f"row index of the job table")
    packed = np.empty(total, dtype=np.int32)
    base, off = {}, 0
    st = d.store
    for p, n in zip(prefixes, counts):
        packed[off:off + n] = pack_events(
            st._arr(f"{p}_xs")[:n], st._arr(f"{p}_ys")[:n],
            st._arr(f"{p}_ps")[:n], name=f"{st.path} [{p}]")
        base[p] = off
        off += n

    hr = np.zeros((n_items, seqn + 1, 4), dtype=np.int32)
    lr = np.zeros((n_items, 1, 4), dtype=np.int32)
    ib, gb = base[d.inp_prefix], base[d.gt_prefix]
    longest = 0
    for i in range(n_items):
        _, steps = ds.window_plan(i)
        for l in range(seqn):
            w, _ = steps[l]
            i0, i1 = d.event_indices[w]
            hr[i, l] = (ib + i0, ib + max(i1, i0), 0, 0)
            longest = max(longest, i1 - i0)
        w, _ = steps[mid_idx]
        i0, i1 = d.event_indices[w]
        g0, g1 = d.gt_event_indices[w]
        hr[i, seqn] = (gb + g0, gb + max(g1, g0), FLAG_GT, 0)
        # the LR count map: the mid step's input events on their own grid
        lr[i, 0] = (ib + i0, ib + max(i1, i0), FLAG_GT, 0)
        longest = max(longest, g1 - g0)
    return (torch.from_numpy(packed).to(device),
            torch.from_numpy(hr).to(device), torch.from_numpy(lr).to(device),
            int(longest))


@torch.no_grad()
def infer_sequence_device(dataloader_config, data_path, model, device,
                          output_path=None, metrics=None, save_images=True,
                          max_batches=None, use_graphs=True, amp_dtype=None,
                          return_maps=False):
    """`infer_sequence` on the device.  Returns the same result dict (plus
    `time_note`) and writes the same results.yml; with `return_maps` returns
    `(result, maps)`, maps holding the stacked per-window `inp`, `gt`, `lr`,
    `esr`, `bicubic` tensors and the raw float64 `table` of sums."""
    cfg = dataloader_config
    _refuse(cfg, save_images)
    device = torch.device(device)
    on_gpu = device.type == "cuda"
    metrics = metrics or build_metrics(device)

    ds = SequenceDataset(data_path, cfg["dataset"])    # never indexed
    seqn = int(cfg["dataset"]["sequence"]["seqn"])
    mid_idx = (seqn - 1) // 2
    lrH, lrW = ds.inp_sensor_resolution
    kH, kW = ds.gt_sensor_resolution
    if kH % lrH or kW % lrW or kH // lrH != kW // lrW:
        raise ValueError(
            f"infer_sequence_device needs the GT resolution "
            f"(gt_sensor_resolution {kH}x{kW}) to be a whole multiple of the "
            f"input resolution {lrH}x{lrW}; use infer_sequence")
    if ds.L < seqn:
        raise ValueError(f"sequence_length {ds.L} is shorter than seqn "
                         f"{seqn}")
    n_items = len(ds) if max_batches is None else min(len(ds), max_batches)

    ext = None
    if on_gpu:
        ext = require_ext()
        if not hasattr(ext, "evs_batch_splat"):
            raise RuntimeError("the native extension lacks evs_batch_splat; "
                               "rebuild it (python -m esr_amd.ops.native."
                               "build)")
    packed, hr_jobs, lr_jobs, max_job_len = _upload(
        ds, n_items, seqn, mid_idx, cfg.get("device_resident"), device)

    # static buffers
    hr_out = torch.zeros(seqn + 1, 2, kH, kW, device=device)
    lr_out = torch.zeros(1, 2, lrH, lrW, device=device)
    hr_job = torch.zeros(seqn + 1, 4, dtype=torch.int32, device=device)
    lr_job = torch.zeros(1, 4, dtype=torch.int32, device=device)
    row = torch.zeros(_ROW, dtype=torch.float64, device=device)
    table = torch.zeros(n_items, _ROW, dtype=torch.float64, device=device)
    inp = hr_out[:seqn][None]                # [1, seqn, 2, kH, kW]
    gt = hr_out[seqn:]                       # [1, 2, kH, kW]

    model.eval()
    if hasattr(model, "reset_states"):
        model.reset_states()

    def forward():
        with amp_autocast(amp_dtype, device, cache_enabled=False):
            return model(inp).float()

    # the recurrence lives in one static buffer, read and written in place;
    # one dry forward on empty frames gives its shape (None and zeros are the
    # same to ConvGRUCell).  A tuple state (ConvLSTM) stays with the model.
    holder = state_holder(model)
    state = None
    if holder is not None:
        forward()
        if isinstance(holder.state, torch.Tensor):
            state = torch.zeros_like(holder.state)
        model.reset_states()
    graphed = bool(use_graphs) and on_gpu and \
        (holder is None or state is not None)

    def splat(jobs, out):
        if ext is not None:
            ext.evs_batch_splat(packed, jobs, out, lrH, lrW, max_job_len)
        else:
            batch_splat_torch(packed, jobs, out, lrH, lrW)

    def body():
        hr_out.zero_()
        lr_out.zero_()
        splat(hr_job, hr_out)
        splat(lr_job, lr_out)
        if state is not None:
            holder.state = state
        esr = forward()
        if state is not None:
            state.copy_(holder.state)
            holder.state = state
        if esr.shape[-2:] != gt.shape[-2:]:
            esr = F.interpolate(esr, size=gt.shape[-2:], mode="bicubic",
                                align_corners=False)
        bic = F.interpolate(lr_out, size=(kH, kW), mode="bicubic",
                            align_corners=False)
        sums = metric_sums(torch.cat([esr, bic]), gt.repeat(2, 1, 1, 1))
        lp = torch.stack([metrics["lpips"](esr, gt).reshape(()),
                          metrics["lpips"](bic, gt).reshape(())])
        row.copy_(torch.cat([sums.reshape(-1), lp.double()]))
        return esr, bic

    graph = None
    if graphed:
        # warm-up runs execute the body on empty jobs and advance the state
        graph, (esr, bic) = capture_graph(
            body, warmup=2, device=device,
            after_warmup=(state.zero_ if state is not None else None))

    maps = {k: [] for k in ("inp", "gt", "lr", "esr", "bicubic")}
    events, host_times = [], []
    for i in range(n_items):
        hr_job.copy_(hr_jobs[i])             # device to device
        lr_job.copy_(lr_jobs[i])
        if on_gpu:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev1 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        else:
            t0 = time.time()
        if graph is not None:
            graph.replay()
        else:
            esr, bic = body()
        if on_gpu:
            ev1.record()
            events.append((ev0, ev1))
        else:
            host_times.append(time.time() - t0)
        table[i].copy_(row)
        if return_maps:
            for k, v in (("inp", inp[0]), ("gt", gt[0]), ("lr", lr_out[0]),
                         ("esr", esr[0]), ("bicubic", bic[0])):
                maps[k].append(v.clone())

    # the one synchronisation: download the table, read the timers
    sums = table.cpu()
    if on_gpu:
        host_times = [a.elapsed_time(b) / 1e3 for a, b in events]
    fin = finalize(sums[:, :20].reshape(n_items * 4, 5), 2, kH, kW)

    result = {}
    n = max(n_items, 1)
    for j, name in enumerate(_NAMES):
        for key in ("l1", "mse", "rmse", "ssim", "psnr"):
            # finalize's images alternate esr, bicubic per window
            result[f"{name}_{key}"] = sum(fin[key][j::2]) / n
        result[f"{name}_lpips"] = sum(sums[:, 20 + j].tolist()) / n
    result["time"] = sum(host_times) / n
    result["params"] = sum(p.numel() for p in model.parameters()) / 1e6
    keys = [f"{name}_{k}" for name in _NAMES
            for k in ("l1", "mse", "rmse", "lpips", "ssim", "psnr")]
    result = {k: result[k] for k in keys + ["time", "params"]}
    result["time_note"] = TIME_NOTE
    lp = metrics.get("lpips")
    if lp is not None and hasattr(lp, "paper_comparable") \
            and not lp.paper_comparable:
        result["lpips_note"] = ("random-init backbone (no ImageNet checkpoint"
                                " in env): lpips values are relative-only")
    if output_path is not None:
        Path(output_path).mkdir(parents=True, exist_ok=True)
        with open(Path(output_path) / "results.yml", "w") as f:
            yaml.safe_dump({"evaluation results": result}, f)
    if return_maps:
        out = {k: torch.stack(v) if v else torch.empty(0, device=device)
               for k, v in maps.items()}
        out["table"] = sums
        return result, out
    return result
