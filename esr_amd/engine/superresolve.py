"""Offline super-resolution of a recording: LR event store in, HR event
store out.

`infer_sequence_device` evaluates windows and `StreamingESR.push_events`
hands back one window's events on a [0, 1] clock; `super_resolve_store`
strings the windows of a whole recording together, puts the predicted events
back on the recording's own float64 clock and writes them as an EVS store.

  * `tile_windows` cuts the recording into non-overlapping windows (by event
    count or by duration);
  * step k splats windows k-seqn+1 .. k as input jobs (`evs_batch_splat`, the
    training loader's LR -> HR mapping), runs the recurrent forward with the
    state in one static buffer, and emits the prediction as the events of
    window k-seqn+1+mid (`sr_emit_window`, ops/native/src/sr_emit.hip);
  * on CUDA the packed events and the job / (t0, t1) tables are uploaded
    once, each step is device-to-device row copies, ONE graph replay and a
    device-to-device copy of the window's counts into a table; the emitted
    rows gather in chunk buffers of `chunk_windows * capacity` rows that are
    drained with one synchronisation per `chunk_windows` steps.  The drain
    is single-buffered: the device idles while a chunk is downloaded and
    written;
  * on the CPU the same function runs the torch forms (`batch_splat_torch`,
    `emit_window_torch`) uncaptured; that is the kernels' oracle.

The first `mid` and last `seqn-1-mid` windows get no prediction and are not
emitted (no edge padding); the summary reports the covered time span.

`super_resolve_stores` converts a list of recordings with several of them in
flight: each occupies a lane (a batch row) of one tick, and `sr_emit_lanes`
appends every lane's rows to that lane's own chunk.  Its output per recording
is `super_resolve_store`'s, byte for byte.
"""

from __future__ import annotations

import logging
import time
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from ..data.device_loader import batch_splat_torch, pack_events
from ..data.store import GROUP_LEVELS, EventStore, EventStoreWriter
from ..ops.native import get_ext
from .capture import amp_autocast, capture_graph, state_holder

__all__ = ["super_resolve_store", "super_resolve_stores", "tile_windows", "emit_window_torch",
           "hash_phase_torch", "cell_counts_torch", "PHASE_Q"]

log = logging.getLogger(__name__)

PHASE_Q = 1 << 20
_MAX_DIM = 32767
_MODES = {"linear": 0, "random": 1}
_LEVEL_NAMES = {1: "ori", 2: "down2", 4: "down4", 8: "down8", 16: "down16"}
_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# window tiling

def tile_windows(ts, mode: str, window) -> dict:
    """Cut sorted timestamps `ts` into non-overlapping windows.

    events: window w is rows [w*W, (w+1)*W); t0 = ts[w*W], t1 = ts[(w+1)*W]
    (the last timestamp for the final window).  time: `window` is a duration
    T in seconds, boundaries ts[0] + w*T, rows by np.searchsorted (left).
    A trailing partial window is dropped.  Returns begin / end (int64 rows),
    t0 / t1 (float64), and tail_events, the rows past the last window."""
    ts = np.asarray(ts, dtype=np.float64)
    N = int(ts.shape[0])
    if mode == "events":
        W = int(window)
        if W < 1 or W != window:
            raise ValueError(f"window must be a positive event count, got "
                             f"{window}")
        n = N // W
        begin = np.arange(n, dtype=np.int64) * W
        end = begin + W
        t0 = ts[begin] if n else np.zeros(0)
        t1 = ts[np.minimum(end, N - 1)] if n else np.zeros(0)
    elif mode == "time":
        T = float(window)
        if not T > 0:
            raise ValueError(f"window must be a positive duration, got "
                             f"{window}")
        n = int(np.floor((ts[-1] - ts[0]) / T)) if N else 0
        edges = ts[0] + np.arange(n + 1, dtype=np.float64) * T if N \
            else np.zeros(1)
        # the last edge may round past the last timestamp
        while n and edges[n] > ts[-1]:
            n -= 1
        edges = edges[:n + 1]
        rows = np.searchsorted(ts, edges, side="left").astype(np.int64)
        begin, end = rows[:-1], rows[1:]
        t0, t1 = edges[:-1], edges[1:]
    else:
        raise ValueError(f"mode must be 'events' or 'time', got {mode!r}")
    last = int(end[-1]) if n else 0
    return {"begin": np.asarray(begin, dtype=np.int64),
            "end": np.asarray(end, dtype=np.int64),
            "t0": np.asarray(t0, dtype=np.float64),
            "t1": np.asarray(t1, dtype=np.float64),
            "tail_events": N - last}


# ---------------------------------------------------------------------------
# torch form of sr_emit_window

def cell_counts_torch(pred: torch.Tensor, cell_cap: int = 1023) -> torch.Tensor:
    """Events per cell: 0 for NaN, else clamp(round-half-even(v), 0,
    cell_cap); int64, same shape."""
    v = pred.float()
    n = torch.round(v).clamp(0, float(cell_cap))
    return torch.where(torch.isnan(v), torch.zeros_like(n), n).long()


def _mul32(a: torch.Tensor, k: int) -> torch.Tensor:
    """a * k modulo 2^32 on int64 tensors holding uint32 values."""
    lo = a * (k & 0xFFFF)
    hi = ((a * (k >> 16)) & 0xFFFF) << 16
    return (lo + hi) & _M32


def _fmix32(h: torch.Tensor) -> torch.Tensor:
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def hash_phase_torch(seed: int, window_index: int, c: torch.Tensor,
                     j: torch.Tensor) -> torch.Tensor:
    """The random phase in [0, Q] of event j of cell c: sr_emit.hip's hash,
    uint32 arithmetic carried in int64."""
    h0 = ((seed & _M32) + (window_index & _M32) * 0x9E3779B9) & _M32
    h = _fmix32(torch.full_like(c, h0))
    h = _fmix32(h ^ (c & _M32))
    h = _fmix32((h + _mul32(j & _M32, 0x9E3779B9)) & _M32)
    return h % (PHASE_Q + 1)


def emit_window_torch(pred: torch.Tensor, t0: float, t1: float, *,
                      capacity: int, cell_cap: int = 1023,
                      mode: str = "linear", seed: int = 0,
                      window_index: int = 0) -> dict:
    """One predicted window [2, kH, kW] -> event rows; the semantics of
    `sr_emit_window`, bit for bit.  Returns xs / ys (uint16), ts (float64),
    ps (int8) numpy columns of the kept events in file order, the int64
    `counts` map, `q` (the kept events' phases) and total / emitted /
    dropped."""
    if mode not in _MODES:
        raise ValueError(f"redistribute mode must be one of {list(_MODES)}")
    _, kH, kW = pred.shape
    counts = cell_counts_torch(pred, cell_cap)
    n = counts.reshape(-1)
    offs = torch.cumsum(n, 0) - n
    total = int(n.sum().item())
    emitted = min(total, int(capacity))
    keep = torch.minimum(n, (capacity - offs).clamp(min=0))
    c = torch.repeat_interleave(torch.arange(n.numel(), device=n.device), keep)
    j = torch.arange(emitted, device=n.device) - offs[c]
    nc = n[c]
    if mode == "linear":
        q = torch.where(nc == 1, torch.zeros_like(j),
                        (j * PHASE_Q) // (nc - 1).clamp(min=1))
    else:
        q = hash_phase_torch(int(seed), int(window_index), c, j)
    q, order = torch.sort(q, stable=True)
    c = c[order]
    plane = kH * kW
    r = c % plane
    frac = (PHASE_Q + 99 * q).double() / float(100 * PHASE_Q)
    lo = torch.tensor(float(t0), dtype=torch.float64, device=n.device)
    hi = torch.tensor(float(t1), dtype=torch.float64, device=n.device)
    ts = lo + (hi - lo) * frac              # three ops, each rounded once
    ts = torch.minimum(torch.maximum(ts, lo), hi)
    neg = c >= plane
    return {"xs": (r % kW).cpu().numpy().astype(np.uint16),
            "ys": (r // kW).cpu().numpy().astype(np.uint16),
            "ts": ts.cpu().numpy(),
            "ps": torch.where(neg, -1, 1).cpu().numpy().astype(np.int8),
            "q": q.cpu().numpy(), "counts": counts,
            "total": total, "emitted": emitted, "dropped": total - emitted}


# ---------------------------------------------------------------------------

def _output_group(group: str, scale: int) -> str:
    level = GROUP_LEVELS.get(group)
    if level is not None and level % scale == 0 \
            and level // scale in _LEVEL_NAMES:
        return _LEVEL_NAMES[level // scale]
    return "sr"


@torch.no_grad()
def super_resolve_store(model, src, dst, *, group, scale, seqn=3, window=2048,
                        mode="events", redistribute="linear", seed=0,
                        capacity=None, cell_cap=1023, chunk_windows=256,
                        device="cuda:0", use_graphs=True, amp_dtype=None,
                        max_windows=None, keep=False, checkpoint=None):
    """Super-resolve group `group` of the EVS store `src` by `scale` and
    write the HR events as a new store `dst`.  Returns the summary dict that
    also goes into dst's meta.json under "sr" (plus `seconds`); with `keep`
    returns `(summary, kept)`, kept holding per emitted window the fp32
    predictions `pred` [n, 2, kH, kW], the clamped `counts` (int64), the
    window indices `windows` and the int64 `stats` table [n, 3] of
    total / emitted / dropped."""
    t_start = time.perf_counter()
    if redistribute not in _MODES:
        raise ValueError(f"redistribute must be one of {list(_MODES)}, got "
                         f"{redistribute!r}")
    if int(scale) != scale or int(scale) < 1:
        raise ValueError(f"scale must be a positive integer, got {scale!r}")
    scale, seqn = int(scale), int(seqn)
    chunk_windows = int(chunk_windows)
    if seqn < 1 or chunk_windows < 1 or int(cell_cap) < 1 \
            or int(cell_cap) > 65535:
        raise ValueError("seqn and chunk_windows must be positive and "
                         "cell_cap must lie in [1, 65535]")
    cell_cap = int(cell_cap)
    device = torch.device(device)
    on_gpu = device.type == "cuda"

    store = EventStore(src)
    if group not in store.groups:
        raise ValueError(f"{src}: no group {group!r} (has "
                         f"{sorted(store.groups)})")
    level = GROUP_LEVELS.get(group, 1)
    H, W = store.sensor_resolution
    lrH, lrW = round(H / level), round(W / level)
    kH, kW = lrH * scale, lrW * scale
    if kH > _MAX_DIM or kW > _MAX_DIM:
        raise ValueError(f"HR grid {kH}x{kW} exceeds {_MAX_DIM} pixels, the "
                         f"15-bit coordinate of a packed event")

    n_src = store.num_events(group)
    src_ts = np.asarray(store.ts(group)[:n_src], dtype=np.float64) if n_src \
        else np.zeros(0)
    tiles = tile_windows(src_ts, mode, window)
    n_tiled = int(tiles["begin"].shape[0])
    n_win = n_tiled if max_windows is None else min(n_tiled, int(max_windows))
    if n_win < seqn:
        raise ValueError(f"{src} [{group}]: {n_win} windows, fewer than "
                         f"seqn = {seqn}")
    mid = (seqn - 1) // 2
    n_steps = n_win - seqn + 1
    begin, end = tiles["begin"][:n_win], tiles["end"][:n_win]
    longest = int((end - begin).max())
    if capacity is None:
        capacity = max(1024, 4 * scale * scale * longest)
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError(f"capacity must be positive, got {capacity}")
    if n_src > 2 ** 31 - 1:
        raise ValueError(f"{n_src} events exceed the int32 row index of the "
                         f"job table")

    ext = None
    if on_gpu:
        ext = get_ext()
        if ext is None or not hasattr(ext, "sr_emit_window"):
            ext = None
            warnings.warn(
                "super_resolve_store: the native sr_emit_window kernel is not "
                "built (run `python -m esr_amd.ops.native.build`); using the "
                "torch forms", RuntimeWarning, stacklevel=2)

    # one upload each: packed events, job table, (t0, t1) table
    packed = torch.from_numpy(pack_events(
        store._arr(f"{group}_xs")[:n_src], store._arr(f"{group}_ys")[:n_src],
        store._arr(f"{group}_ps")[:n_src], name=f"{src} [{group}]").copy()
    ).to(device)
    jobs_np = np.zeros((n_steps, seqn, 4), dtype=np.int32)
    for l in range(seqn):
        jobs_np[:, l, 0] = begin[l:l + n_steps]
        jobs_np[:, l, 1] = end[l:l + n_steps]
    win_np = np.stack([tiles["t0"][mid:mid + n_steps],
                       tiles["t1"][mid:mid + n_steps]], axis=1)
    jobs = torch.from_numpy(jobs_np).to(device)
    wins = torch.from_numpy(np.ascontiguousarray(win_np)).to(device)

    # static buffers
    hr_out = torch.zeros(seqn, 2, kH, kW, device=device)
    inp = hr_out[None]                                  # [1, seqn, 2, kH, kW]
    job = torch.zeros(seqn, 4, dtype=torch.int32, device=device)
    win = torch.zeros(2, dtype=torch.float64, device=device)

    model = model.to(device).eval()
    if hasattr(model, "reset_states"):
        model.reset_states()

    def forward():
        with amp_autocast(amp_dtype, device, cache_enabled=False):
            return model(inp).float()

    holder = state_holder(model)
    state = None
    if holder is not None:
        probe = forward()
        if isinstance(holder.state, (tuple, list)):
            model.reset_states()
            raise NotImplementedError(
                "super_resolve_store keeps the recurrence in one static "
                "tensor; a tuple state (ConvLSTM) is not supported")
        if isinstance(holder.state, torch.Tensor):
            state = torch.zeros_like(holder.state)
        model.reset_states()
    else:
        probe = forward()
    if tuple(probe.shape) != (1, 2, kH, kW):
        raise ValueError(f"the model maps [1, {seqn}, 2, {kH}, {kW}] to "
                         f"{tuple(probe.shape)}, not to [1, 2, {kH}, {kW}]")
    del probe

    def splat():
        if ext is not None:
            ext.evs_batch_splat(packed, job, hr_out, lrH, lrW, longest)
        else:
            batch_splat_torch(packed, job, hr_out, lrH, lrW)

    def predict():
        hr_out.zero_()
        splat()
        if state is not None:
            holder.state = state
        pred = forward()
        if state is not None:
            state.copy_(holder.state)
            holder.state = state
        return pred[0].contiguous()

    out_group = _output_group(group, scale)
    writer = EventStoreWriter(dst, (kH, kW))
    appender = writer.open_group(out_group)
    first_window = mid                       # window index of step 0
    kept = {"pred": [], "counts": []}
    rmode = _MODES[redistribute]

    if ext is not None:
        # ---- device path -------------------------------------------------
        rows = chunk_windows * capacity
        cols = [torch.zeros(rows, dtype=torch.uint16, device=device),
                torch.zeros(rows, dtype=torch.uint16, device=device),
                torch.zeros(rows, dtype=torch.float64, device=device),
                torch.zeros(rows, dtype=torch.int8, device=device)]
        cs = torch.zeros(5, dtype=torch.int64, device=device)
        cs0 = torch.tensor([0, 0, 0, 0, first_window], dtype=torch.int64,
                           device=device)
        zero_cursor = torch.zeros(1, dtype=torch.int64, device=device)
        stats = torch.zeros(n_steps, 3, dtype=torch.int64, device=device)
        scratch = ext.sr_emit_scratch(hr_out, 2 * kH * kW, capacity)

        def body():
            pred = predict()
            ext.sr_emit_window(pred, win, cols, cs, capacity, cell_cap,
                               rmode, int(seed), scratch)
            return pred

        graph = None
        if use_graphs:
            # warm-up runs execute the body on empty jobs: they advance the
            # state, the cursor and the window index, all put back here
            def rewind():
                if state is not None:
                    state.zero_()
                cs.copy_(cs0)
            graph, pred = capture_graph(body, warmup=2, device=device,
                                        after_warmup=rewind)
        cs.copy_(cs0)

        def drain():
            n = int(cs[0].item())            # the chunk's one synchronisation
            if not 0 <= n <= rows:
                raise RuntimeError(f"append cursor {n} outside the chunk of "
                                   f"{rows} rows")
            appender.append(*(c[:n].cpu().numpy() for c in cols))
            cs[:1].copy_(zero_cursor)

        for k in range(n_steps):
            job.copy_(jobs[k])               # device to device
            win.copy_(wins[k])
            if graph is not None:
                graph.replay()
            else:
                pred = body()
            stats[k].copy_(cs[1:4])
            if keep:
                kept["pred"].append(pred.clone())
                kept["counts"].append(
                    scratch[0].view(2, kH, kW).long().clone())
            if (k + 1) % chunk_windows == 0 or k + 1 == n_steps:
                drain()
        stats_np = stats.cpu().numpy()
    else:
        # ---- torch forms, uncaptured: the oracle --------------------------
        stats_np = np.zeros((n_steps, 3), dtype=np.int64)
        pending = []
        for k in range(n_steps):
            job.copy_(jobs[k])
            win.copy_(wins[k])
            pred = predict()
            ev = emit_window_torch(
                pred, float(win_np[k, 0]), float(win_np[k, 1]),
                capacity=capacity, cell_cap=cell_cap, mode=redistribute,
                seed=seed, window_index=first_window + k)
            stats_np[k] = (ev["total"], ev["emitted"], ev["dropped"])
            pending.append(ev)
            if keep:
                kept["pred"].append(pred.clone())
                kept["counts"].append(ev["counts"].clone())
            if (k + 1) % chunk_windows == 0 or k + 1 == n_steps:
                appender.append(*(np.concatenate([e[f] for e in pending])
                                  for f in ("xs", "ys", "ts", "ps")))
                pending = []
    if hasattr(model, "reset_states"):
        model.reset_states()
    appender.close()

    overflowed = np.nonzero(stats_np[:, 2] > 0)[0] + first_window
    events_out = int(stats_np[:, 1].sum())
    dropped = int(stats_np[:, 2].sum())
    if overflowed.size:
        log.warning(
            "super_resolve_store: %d of %d windows overflowed capacity %d; "
            "%d events dropped (%s)", overflowed.size, n_steps, capacity,
            dropped, dst)
    summary = {
        "source": str(src), "group": group, "output_group": out_group,
        "checkpoint": None if checkpoint is None else str(checkpoint),
        "scale": scale, "seqn": seqn,
        "window": int(window) if mode == "events" else float(window),
        "mode": mode, "redistribute": redistribute, "seed": int(seed),
        "capacity": capacity, "cell_cap": cell_cap,
        "windows_tiled": n_tiled, "windows_emitted": n_steps,
        "windows_skipped_edges": n_win - n_steps,
        "tail_events_dropped": int(tiles["tail_events"]),
        "events_in": int(end[n_win - 1] - begin[0]),
        "events_out": events_out, "events_dropped": dropped,
        "windows_overflowed": int(overflowed.size),
        "overflowed_windows": [int(w) for w in overflowed[:100]],
        "covered": [float(win_np[0, 0]), float(win_np[-1, 1])],
    }
    writer.meta["sr"] = dict(summary)
    writer.close()
    summary["seconds"] = time.perf_counter() - t_start
    if keep:
        dev_stats = torch.from_numpy(stats_np)
        return summary, {
            "pred": torch.stack(kept["pred"]),
            "counts": torch.stack(kept["counts"]),
            "windows": list(range(first_window, first_window + n_steps)),
            "stats": dev_stats}
    return summary


# ---------------------------------------------------------------------------
# several recordings at once: lanes of one batched tick

def _open_recording(src, dst, *, group, scale, seqn, window, mode, capacity,
                    max_windows):
    """Open and tile one source the way `super_resolve_store` does, without
    writing anything; raises ValueError naming the file."""
    store = EventStore(src)
    if group not in store.groups:
        raise ValueError(f"{src}: no group {group!r} (has "
                         f"{sorted(store.groups)})")
    level = GROUP_LEVELS.get(group, 1)
    H, W = store.sensor_resolution
    lrH, lrW = round(H / level), round(W / level)
    if lrH * scale > _MAX_DIM or lrW * scale > _MAX_DIM:
        raise ValueError(f"{src}: HR grid {lrH * scale}x{lrW * scale} exceeds "
                         f"{_MAX_DIM} pixels, the 15-bit coordinate of a "
                         f"packed event")
    n_src = store.num_events(group)
    src_ts = np.asarray(store.ts(group)[:n_src], dtype=np.float64) if n_src \
        else np.zeros(0)
    tiles = tile_windows(src_ts, mode, window)
    n_tiled = int(tiles["begin"].shape[0])
    n_win = n_tiled if max_windows is None else min(n_tiled, int(max_windows))
    if n_win < seqn:
        raise ValueError(f"{src} [{group}]: {n_win} windows, fewer than "
                         f"seqn = {seqn}")
    if n_src > 2 ** 31 - 1:
        raise ValueError(f"{src}: {n_src} events exceed the int32 row index "
                         f"of the job table")
    mid = (seqn - 1) // 2
    n_steps = n_win - seqn + 1
    begin, end = tiles["begin"][:n_win], tiles["end"][:n_win]
    longest = int((end - begin).max())
    if capacity is None:
        capacity = max(1024, 4 * scale * scale * longest)
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError(f"capacity must be positive, got {capacity}")
    jobs_np = np.zeros((n_steps, seqn, 4), dtype=np.int64)
    for l in range(seqn):
        jobs_np[:, l, 0] = begin[l:l + n_steps]
        jobs_np[:, l, 1] = end[l:l + n_steps]
    win_np = np.ascontiguousarray(np.stack(
        [tiles["t0"][mid:mid + n_steps], tiles["t1"][mid:mid + n_steps]],
        axis=1))
    return SimpleNamespace(
        src=src, dst=dst, store=store, lr=(lrH, lrW), n_src=n_src,
        n_tiled=n_tiled, n_win=n_win, n_steps=n_steps, longest=longest,
        capacity=capacity, jobs_np=jobs_np, win_np=win_np,
        tail_events=int(tiles["tail_events"]),
        events_in=int(end[n_win - 1] - begin[0]))


@torch.no_grad()
def super_resolve_stores(model, pairs, *, lanes, group, scale, seqn=3,
                         window=2048, mode="events", redistribute="linear",
                         seed=0, capacity=None, cell_cap=1023,
                         chunk_windows=256, device="cuda:0", use_graphs=True,
                         amp_dtype=None, max_windows=None, keep=False,
                         checkpoint=None, max_bytes=8 << 30):
    """`super_resolve_store` for a list of `(src, dst)` pairs with up to
    `lanes` recordings in flight: lane s is row s of a batch-`lanes` tick
    (fetch, splat, forward, `sr_emit_lanes`), on CUDA one control-block
    upload and one graph replay.  A lane whose recording ends is handed to
    the next recording of the list; recordings start in list order.  Every
    `dst` and its summary (minus `seconds`) are what `super_resolve_store`
    with the same arguments writes for that pair alone, given a model whose
    result for one sample does not depend on the rest of the batch.

    All sources must share one LR resolution; the recurrent state's dim 0
    must be a multiple m of the lane count, lane s owning rows s, lanes + s,
    ..., (m-1)*lanes + s.  The packed events of `lanes` recordings stay on
    the device, at most `max_bytes`.  Returns `{dst: summary}`, with `keep`
    `{dst: (summary, kept)}` as `super_resolve_store` returns them."""
    if redistribute not in _MODES:
        raise ValueError(f"redistribute must be one of {list(_MODES)}, got "
                         f"{redistribute!r}")
    if int(scale) != scale or int(scale) < 1:
        raise ValueError(f"scale must be a positive integer, got {scale!r}")
    scale, seqn = int(scale), int(seqn)
    chunk_windows, lanes = int(chunk_windows), int(lanes)
    if seqn < 1 or chunk_windows < 1 or int(cell_cap) < 1 \
            or int(cell_cap) > 65535:
        raise ValueError("seqn and chunk_windows must be positive and "
                         "cell_cap must lie in [1, 65535]")
    if lanes < 1:
        raise ValueError(f"lanes must be positive, got {lanes}")
    cell_cap = int(cell_cap)
    device = torch.device(device)
    on_gpu = device.type == "cuda"
    pairs = [(str(src), str(dst)) for src, dst in pairs]
    if not pairs:
        return {}

    # every source is opened and tiled before anything is written
    recs = [_open_recording(src, dst, group=group, scale=scale, seqn=seqn,
                            window=window, mode=mode, capacity=capacity,
                            max_windows=max_windows) for src, dst in pairs]
    lrH, lrW = recs[0].lr
    for r in recs[1:]:
        if r.lr != (lrH, lrW):
            raise ValueError(
                f"{r.src} [{group}]: LR resolution {r.lr[0]}x{r.lr[1]} "
                f"differs from {lrH}x{lrW} of {recs[0].src}")
    kH, kW = lrH * scale, lrW * scale
    L = min(lanes, len(recs))
    slot = max(max(r.n_src for r in recs), 1)
    if L * slot * 4 > max_bytes or L * slot > 2 ** 31 - 1:
        raise ValueError(
            f"the event arena of {L} lanes x {slot} events takes "
            f"{L * slot * 4} bytes; at most max_bytes = {max_bytes} bytes "
            f"and {2 ** 31 - 1} events fit")
    max_steps = max(r.n_steps for r in recs)
    capacity_max = max(r.capacity for r in recs)
    longest_max = max(r.longest for r in recs)
    mid = (seqn - 1) // 2
    rmode = _MODES[redistribute]
    out_group = _output_group(group, scale)

    ext = None
    if on_gpu:
        ext = get_ext()
        if ext is None or not hasattr(ext, "sr_emit_lanes"):
            ext = None
            warnings.warn(
                "super_resolve_stores: the native sr_emit_lanes kernel is not "
                "built (run `python -m esr_amd.ops.native.build`); using the "
                "torch forms", RuntimeWarning, stacklevel=2)

    # static buffers: the graph's addresses never change
    arena = torch.zeros(L * slot, dtype=torch.int32, device=device)
    jobs_tab = torch.zeros(L * max_steps, seqn * 4, dtype=torch.int32,
                           device=device)
    wins_tab = torch.zeros(L * max_steps, 2, dtype=torch.float64,
                           device=device)
    lane_base = torch.arange(L, device=device) * max_steps
    hr_out = torch.zeros(L * seqn, 2, kH, kW, device=device)
    inp = hr_out.view(L, seqn, 2, kH, kW)
    job = torch.zeros(L, seqn * 4, dtype=torch.int32, device=device)
    win = torch.zeros(L, 2, dtype=torch.float64, device=device)
    # control block, one upload per tick: lane_ctl [L, 2] = {active,
    # capacity_s} as sr_emit_lanes reads it, then reset [L] and step [L]
    ctl = torch.zeros(4 * L, dtype=torch.int64, device=device)
    lane_ctl = ctl[:2 * L].view(L, 2)
    reset_c, step_c = ctl[2 * L:3 * L], ctl[3 * L:]

    model = model.to(device).eval()
    if hasattr(model, "reset_states"):
        model.reset_states()

    def forward():
        with amp_autocast(amp_dtype, device, cache_enabled=False):
            return model(inp).float()

    holder = state_holder(model)
    state = None
    probe = forward()
    if holder is not None:
        st = holder.state
        model.reset_states()
        if isinstance(st, (tuple, list)):
            raise NotImplementedError(
                "super_resolve_stores keeps the recurrence in one static "
                "tensor; a tuple state (ConvLSTM) is not supported")
        if isinstance(st, torch.Tensor):
            if st.dim() < 1 or st.size(0) % L:
                raise ValueError(
                    f"the recurrent state {tuple(st.shape)} has no whole "
                    f"number of rows per lane ({L} lanes)")
            state = torch.zeros_like(st)
    if tuple(probe.shape) != (L, 2, kH, kW):
        raise ValueError(f"the model maps [{L}, {seqn}, 2, {kH}, {kW}] to "
                         f"{tuple(probe.shape)}, not to [{L}, 2, {kH}, {kW}]")
    del probe
    rows_per_lane = state.size(0) // L if state is not None else 0

    def lane_rows(flags):
        """[L] lane flags -> a mask over the state's rows s, L+s, ..."""
        return (flags != 0).repeat(rows_per_lane).view(
            -1, *([1] * (state.dim() - 1)))

    def predict():
        # this tick's job rows and (t0, t1) of every lane, by step index
        idx = lane_base + step_c.clamp(0, max_steps - 1)
        torch.index_select(jobs_tab, 0, idx, out=job)
        torch.index_select(wins_tab, 0, idx, out=win)
        job.mul_(lane_ctl[:, :1] != 0)        # an idle lane's jobs are empty
        hr_out.zero_()
        if ext is not None:
            ext.evs_batch_splat(arena, job.view(L * seqn, 4), hr_out, lrH,
                                lrW, longest_max)
        else:
            batch_splat_torch(arena, job.view(L * seqn, 4), hr_out, lrH, lrW)
        if state is not None:
            state.masked_fill_(lane_rows(reset_c), 0)
            holder.state = state
        pred = forward()
        if state is not None:
            new = holder.state.to(state.dtype)
            state.copy_(torch.where(lane_rows(lane_ctl[:, 0]), new, state))
            holder.state = state
        return pred.contiguous()

    # per-lane emission state
    if ext is not None:
        rows = chunk_windows * capacity_max
        cols = [torch.zeros(L, rows, dtype=dt, device=device)
                for dt in (torch.uint16, torch.uint16, torch.float64,
                           torch.int8)]
        cs = torch.zeros(L, 5, dtype=torch.int64, device=device)
        cs0 = torch.tensor([0, 0, 0, 0, mid], dtype=torch.int64,
                           device=device)
        zero_cursor = torch.zeros(1, dtype=torch.int64, device=device)
        # row max_steps of every lane takes the writes of idle lanes
        stats = torch.zeros(L * (max_steps + 1), 3, dtype=torch.int64,
                            device=device)
        stats_base = torch.arange(L, device=device) * (max_steps + 1)
        scratch = ext.sr_emit_lanes_scratch(hr_out, L, 2 * kH * kW,
                                            capacity_max)
        stage = [{"block": torch.zeros(4 * L, dtype=torch.int64,
                                       pin_memory=True), "done": None}
                 for _ in range(2)]

        def body():
            pred = predict()
            ext.sr_emit_lanes(pred, win, cols, cs, lane_ctl, capacity_max,
                              cell_cap, rmode, int(seed), scratch)
            row = torch.where(lane_ctl[:, 0] != 0,
                              step_c.clamp(0, max_steps - 1),
                              torch.full_like(step_c, max_steps))
            stats.index_copy_(0, stats_base + row, cs[:, 1:4])
            return pred

        graph = None
        if use_graphs:
            # with an all-zero control block every lane is idle: the warm-up
            # runs splat, commit and emit nothing
            ctl.zero_()
            graph, pred_out = capture_graph(body, warmup=2, device=device)

    lane = [None] * L
    queue = iter(recs)
    results = {}
    ticks = 0

    def start(s):
        """Hand lane s to the next recording of the list, if any."""
        rec = next(queue, None)
        if rec is None:
            lane[s] = None
            return
        st = rec.store
        packed = pack_events(
            st._arr(f"{group}_xs")[:rec.n_src],
            st._arr(f"{group}_ys")[:rec.n_src],
            st._arr(f"{group}_ps")[:rec.n_src], name=f"{rec.src} [{group}]")
        arena[s * slot:s * slot + rec.n_src].copy_(
            torch.from_numpy(packed.copy()))
        jobs_np = rec.jobs_np.copy()
        jobs_np[:, :, :2] += s * slot         # row indices into the arena
        lo = s * max_steps
        jobs_tab[lo:lo + rec.n_steps].copy_(torch.from_numpy(
            jobs_np.astype(np.int32).reshape(rec.n_steps, seqn * 4)))
        wins_tab[lo:lo + rec.n_steps].copy_(torch.from_numpy(rec.win_np))
        if ext is not None:
            cs[s].copy_(cs0)                  # cursor 0, window index mid
        writer = EventStoreWriter(rec.dst, (kH, kW))
        lane[s] = SimpleNamespace(
            rec=rec, step=0, gathered=0, reset=True, writer=writer,
            appender=writer.open_group(out_group), pending=[],
            stats_np=np.zeros((rec.n_steps, 3), dtype=np.int64),
            kept={"pred": [], "counts": []}, t_start=time.perf_counter())

    def drain(s):
        ln = lane[s]
        if ext is not None:
            n = int(cs[s, 0].item())          # the drain's one synchronisation
            if not 0 <= n <= rows:
                raise RuntimeError(f"append cursor {n} of lane {s} outside "
                                   f"the chunk of {rows} rows")
            ln.appender.append(*(c[s, :n].cpu().numpy() for c in cols))
            cs[s, :1].copy_(zero_cursor)
        else:
            ln.appender.append(*(np.concatenate([e[f] for e in ln.pending])
                                 for f in ("xs", "ys", "ts", "ps")))
            ln.pending = []
        ln.gathered = 0

    def finish(s):
        ln, rec = lane[s], lane[s].rec
        ln.appender.close()
        if ext is not None:
            lo = s * (max_steps + 1)
            ln.stats_np = stats[lo:lo + rec.n_steps].cpu().numpy()
        stats_np = ln.stats_np
        overflowed = np.nonzero(stats_np[:, 2] > 0)[0] + mid
        dropped = int(stats_np[:, 2].sum())
        if overflowed.size:
            log.warning(
                "super_resolve_stores: %d of %d windows overflowed capacity "
                "%d; %d events dropped (%s)", overflowed.size, rec.n_steps,
                rec.capacity, dropped, rec.dst)
        summary = {
            "source": rec.src, "group": group, "output_group": out_group,
            "checkpoint": None if checkpoint is None else str(checkpoint),
            "scale": scale, "seqn": seqn,
            "window": int(window) if mode == "events" else float(window),
            "mode": mode, "redistribute": redistribute, "seed": int(seed),
            "capacity": rec.capacity, "cell_cap": cell_cap,
            "windows_tiled": rec.n_tiled, "windows_emitted": rec.n_steps,
            "windows_skipped_edges": rec.n_win - rec.n_steps,
            "tail_events_dropped": rec.tail_events,
            "events_in": rec.events_in,
            "events_out": int(stats_np[:, 1].sum()),
            "events_dropped": dropped,
            "windows_overflowed": int(overflowed.size),
            "overflowed_windows": [int(w) for w in overflowed[:100]],
            "covered": [float(rec.win_np[0, 0]), float(rec.win_np[-1, 1])],
        }
        ln.writer.meta["sr"] = dict(summary)
        ln.writer.close()
        summary["seconds"] = time.perf_counter() - ln.t_start
        if keep:
            results[rec.dst] = (summary, {
                "pred": torch.stack(ln.kept["pred"]),
                "counts": torch.stack(ln.kept["counts"]),
                "windows": list(range(mid, mid + rec.n_steps)),
                "stats": torch.from_numpy(stats_np)})
        else:
            results[rec.dst] = summary

    try:
        for s in range(L):
            start(s)
        while any(ln is not None for ln in lane):
            block = [0] * (4 * L)
            for s, ln in enumerate(lane):
                if ln is not None:
                    block[2 * s], block[2 * s + 1] = 1, ln.rec.capacity
                    block[2 * L + s] = int(ln.reset)
                    block[3 * L + s] = ln.step
                    ln.reset = False
            if ext is not None:
                # double-buffered pinned staging: a block is rewritten only
                # after the copy that read it two ticks ago has finished
                stg = stage[ticks % 2]
                if stg["done"] is not None:
                    stg["done"].synchronize()
                stg["block"].copy_(torch.tensor(block, dtype=torch.int64))
                ctl.copy_(stg["block"], non_blocking=True)
                stg["done"] = torch.cuda.Event()
                stg["done"].record(torch.cuda.current_stream(device))
                if graph is not None:
                    graph.replay()
                    pred = pred_out
                else:
                    pred = body()
            else:
                ctl.copy_(torch.tensor(block, dtype=torch.int64))
                pred = predict()
            ticks += 1
            for s, ln in enumerate(lane):
                if ln is None:
                    continue
                rec = ln.rec
                if ext is None:
                    ev = emit_window_torch(
                        pred[s], float(rec.win_np[ln.step, 0]),
                        float(rec.win_np[ln.step, 1]), capacity=rec.capacity,
                        cell_cap=cell_cap, mode=redistribute, seed=seed,
                        window_index=mid + ln.step)
                    ln.stats_np[ln.step] = (ev["total"], ev["emitted"],
                                            ev["dropped"])
                    ln.pending.append(ev)
                if keep:
                    ln.kept["pred"].append(pred[s].clone())
                    ln.kept["counts"].append(
                        ev["counts"].clone() if ext is None else
                        scratch[0].view(L, 2, kH, kW)[s].long().clone())
                ln.step += 1
                ln.gathered += 1
                ended = ln.step == rec.n_steps
                if ln.gathered == chunk_windows or ended:
                    drain(s)
                if ended:
                    finish(s)
                    start(s)
    finally:
        for ln in lane:
            if ln is not None:                # an error mid-run: close files
                ln.appender.close()
        if hasattr(model, "reset_states"):
            model.reset_states()
    return {rec.dst: results[rec.dst] for rec in recs}      # list order
