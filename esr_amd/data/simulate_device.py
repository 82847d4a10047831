"""Event simulation on the device: frames -> multi-scale EVS stores.

`data/simulate.py` holds the model and its numpy oracle
(`simulate_events_log`).  This module runs the same model through the
kernels of `ops/native/src/esim.hip`: one thread per pixel walks the
intervals of a slab of float64 log frames; a scan gives each pixel its
offset; two radix sorts give the oracle's order; the typed columns come
back in chunks of at most `max_chunk_events` rows.  Results equal the
oracle's bit for bit, order included.

  DeviceEventSimulator           per-pixel state on the device, fed slab by
                                 slab (the last frame of one slab is the
                                 first of the next)
  simulate_events_device         one call, [4, N] float64 as the oracle
  frames_to_event_store_device   frames (array, memmap or lazy sequence) ->
                                 bicubic scales -> log -> simulator -> store,
                                 nothing held for longer than a slab

With device="cpu", or on a GPU without the built extension (a RuntimeWarning
says so), the same functions run the oracle slab by slab.
"""

from __future__ import annotations

import warnings

import numpy as np
import torch
import torch.nn.functional as F

from ..ops.native import get_ext
from .simulate import (_LOG_EPS, check_timestamps, sample_contrast_thresholds,
                       simulate_log_slab)
from .store import EventStoreWriter

__all__ = ["DeviceEventSimulator", "simulate_events_device",
           "frames_to_event_store_device", "LEVEL_NAMES"]

LEVEL_NAMES = {1: "ori", 2: "down2", 4: "down4", 8: "down8", 16: "down16"}

MAX_DIM = 32767                 # the pack_events word holds 15-bit x and y
MAX_CROSSINGS = 65535           # per pixel and interval
MAX_INTERVALS = 4096            # per chunk (esim.hip: ES_MAX_INTERVALS)
STAGES = ("count", "scan", "emit", "sort_key", "sort_t", "unpack",
          "download")


class _StageTimer:
    """Device-event timing of the simulator's stages (tools/bench_simulate)."""

    def __init__(self):
        self.pairs = []

    def __call__(self, name, fn):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.pairs.append((name, a, b))
        return out

    def totals_ms(self) -> dict:
        torch.cuda.synchronize()
        out = {s: 0.0 for s in STAGES}
        for name, a, b in self.pairs:
            out[name] += a.elapsed_time(b)
        return out


class DeviceEventSimulator:
    """The simulator of `simulate_events_log`, with the per-pixel state
    (`ref`, `t_last`) kept between calls of `feed`.

    max_chunk_events sizes the chunk buffers once and bounds the memory; a
    chunk covers as many intervals of the slab as fit (the count pass is
    repeated over half as many when they do not).  intervals_per_chunk caps
    that number from the start.  `halvings` counts the repeats.
    """

    def __init__(self, H, W, cp, cn, refractory=0.0, device="cuda:0",
                 max_chunk_events=1 << 22, intervals_per_chunk=None,
                 profile=False):
        H, W = int(H), int(W)
        if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
            raise ValueError(f"H and W must lie in [1, {MAX_DIM}]")
        if not (cp > 0 and cn > 0):
            raise ValueError("contrast thresholds must be positive")
        if not refractory >= 0:
            raise ValueError("the refractory period must be >= 0")
        max_chunk_events = int(max_chunk_events)
        if not 1 <= max_chunk_events <= 1 << 30:
            raise ValueError("max_chunk_events must lie in [1, 2^30]")
        if intervals_per_chunk is not None and intervals_per_chunk < 1:
            raise ValueError("intervals_per_chunk must be positive")
        self.H, self.W = H, W
        self.cp, self.cn = float(cp), float(cn)
        self.refractory = float(refractory)
        self.device = torch.device(device)
        self.max_chunk_events = max_chunk_events
        self.intervals_per_chunk = intervals_per_chunk
        self.ext = None
        if self.device.type == "cuda":
            self.ext = get_ext()
            if self.ext is None or not hasattr(self.ext, "esim_emit"):
                self.ext = None
                warnings.warn(
                    "DeviceEventSimulator: the native esim kernels are not "
                    "built (run `python -m esr_amd.ops.native.build`); using "
                    "the numpy simulator", RuntimeWarning, stacklevel=2)
        self.timer = _StageTimer() if profile and self.ext is not None else None
        self._scratch = self._cols = self._stats = None
        self.reset()

    @property
    def native(self) -> bool:
        return self.ext is not None

    def reset(self) -> None:
        """Forget the state: the next slab starts a recording."""
        self._ref = self._t_last = None
        self._last_t = None
        self.halvings = 0
        self.chunks = 0

    # -- feeding ----------------------------------------------------------
    def feed(self, logf_slab, ts_slab):
        """Simulate the intervals of a slab: log frames float64 [S, H, W] (a
        tensor on the device or an array) and their S timestamps.  Returns an
        iterator of (xs uint16, ys uint16, ts float64, ps int8) numpy chunks
        in the oracle's order; it must be run to its end before the next
        slab.  ValueError: bad timestamps, a slab that does not continue the
        last one, non-finite log frames, more than 65535 crossings of a pixel
        in one interval, or one interval with more than max_chunk_events
        events.  The state is then that before the failing chunk."""
        ts = check_timestamps(ts_slab)
        if tuple(logf_slab.shape) != (ts.shape[0], self.H, self.W):
            raise ValueError(
                f"expected log frames [{ts.shape[0]}, {self.H}, {self.W}], "
                f"got {tuple(logf_slab.shape)}")
        if ts.shape[0] == 0:
            return iter(())
        if self._last_t is not None and ts[0] != self._last_t:
            raise ValueError(
                "the first frame of a slab must be the last of the slab "
                f"before it (t = {self._last_t!r}, got {ts[0]!r})")
        if self.native:
            return self._feed_native(logf_slab, ts)
        return self._feed_oracle(logf_slab, ts)

    def _feed_oracle(self, logf_slab, ts):
        if isinstance(logf_slab, torch.Tensor):
            logf_slab = logf_slab.detach().cpu().numpy()
        logf = np.asarray(logf_slab, dtype=np.float64)
        if not np.isfinite(logf).all():
            raise ValueError("non-finite log frames")
        if self._ref is None:
            self._ref = logf[0].copy()
            self._t_last = np.full((self.H, self.W), -np.inf)
        ev, ref, t_last = simulate_log_slab(
            logf, ts, self.cp, self.cn, self.refractory, self._ref,
            self._t_last)
        self._ref, self._t_last, self._last_t = ref, t_last, ts[-1]
        if ev.shape[1]:
            self.chunks += 1
            yield (ev[0].astype(np.uint16), ev[1].astype(np.uint16), ev[2],
                   ev[3].astype(np.int8))

    def _timed(self, name, fn):
        return self.timer(name, fn) if self.timer is not None else fn()

    def _feed_native(self, logf_slab, ts):
        ext, dev = self.ext, self.device
        logf = torch.as_tensor(logf_slab).to(
            device=dev, dtype=torch.float64).contiguous()
        S = logf.shape[0]
        npix = self.H * self.W
        cap = self.max_chunk_events
        if self._scratch is None:
            self._scratch = ext.esim_scratch(logf, npix, cap)
            self._stats = torch.zeros(3, dtype=torch.int64, device=dev)
            self._cols = [torch.zeros(cap, dtype=dt, device=dev)
                          for dt in (torch.uint16, torch.uint16,
                                     torch.float64, torch.int8)]
        if self._ref is None:
            self._ref = logf[0].clone()
            self._t_last = torch.full((self.H, self.W), float("-inf"),
                                      dtype=torch.float64, device=dev)
        ts_dev = torch.from_numpy(ts).to(dev)
        walk = (self.cp, self.cn, self.refractory)
        scratch, stats, cols = self._scratch, self._stats, self._cols

        k = 0
        n_max = min(self.intervals_per_chunk or MAX_INTERVALS, MAX_INTERVALS)
        while k < S - 1:
            n = min(n_max, S - 1 - k)
            while True:
                self._timed("count", lambda: ext.esim_count(
                    logf, ts_dev, self._ref, self._t_last, k, n, *walk,
                    scratch, stats))
                self._timed("scan", lambda: ext.esim_scan(npix, scratch,
                                                          stats))
                total, max_cross, bad = (int(v) for v in stats.tolist())
                if bad:
                    raise ValueError(
                        "non-finite log frames, or more than "
                        f"{MAX_CROSSINGS} crossings of one pixel in one "
                        f"interval (frames {k}..{k + n} of the slab)")
                if total <= cap:
                    break
                if n == 1:
                    raise ValueError(
                        f"interval {k + 1} of the slab alone has {total} "
                        f"events, more than max_chunk_events = {cap}")
                n = n_max = n // 2
                self.halvings += 1
            layout = self._timed("emit", lambda: ext.esim_emit(
                logf, ts_dev, self._ref, self._t_last, k, n, *walk, max_cross,
                scratch))
            k += n
            if total == 0:
                continue
            self._timed("sort_key", lambda: ext.esim_sort(
                0, total, self.W, *layout, scratch))
            self._timed("sort_t", lambda: ext.esim_sort(
                1, total, self.W, *layout, scratch))
            self._timed("unpack", lambda: ext.esim_unpack(total, scratch,
                                                          cols))
            out = self._timed("download", lambda: tuple(
                c[:total].cpu().numpy() for c in cols))
            self.chunks += 1
            yield out
        self._last_t = ts[-1]


def _stack_chunks(chunks) -> np.ndarray:
    chunks = list(chunks)
    if not chunks:
        return np.zeros((4, 0))
    return np.stack([np.concatenate([c[i] for c in chunks]).astype(np.float64)
                     for i in range(4)])


def simulate_events_device(logf, timestamps, cp, cn, refractory=0.0,
                           device="cuda:0", max_chunk_events=1 << 22,
                           intervals_per_chunk=None) -> np.ndarray:
    """`simulate_events_log` on the device: [4, N] float64 (x, y, t, p),
    equal to the oracle's."""
    T, H, W = logf.shape
    sim = DeviceEventSimulator(H, W, cp, cn, refractory, device,
                               max_chunk_events, intervals_per_chunk)
    return _stack_chunks(sim.feed(logf, timestamps))


def _frame_block(frames, a: int, b: int) -> np.ndarray:
    """Frames a..b-1 of anything indexable by frame, float64 [b-a, H, W]."""
    return np.stack([np.asarray(frames[i], dtype=np.float64)
                     for i in range(a, b)])


def _log_frames(block: torch.Tensor, level: int) -> torch.Tensor:
    """float64 [n, H, W] frames in [0, 1] -> float64 log frames at `level`:
    fp32 bicubic and clamp as simulate._scale_frames, then log(x + 1e-3)."""
    if level != 1:
        H, W = block.shape[1:]
        block = F.interpolate(block.float().unsqueeze(1),
                              size=(H // level, W // level), mode="bicubic",
                              align_corners=False).clamp(0, 1).squeeze(1)
    return torch.log(block.double() + _LOG_EPS)


def frames_to_event_store_device(path, frames, timestamps,
                                 levels=(1, 2, 4, 8, 16), cp=None, cn=None,
                                 seed: int = 0, refractory: float = 0.0,
                                 store_images: bool = True,
                                 device="cuda:0", frame_chunk: int = 64,
                                 log_sink=None,
                                 max_chunk_events: int = 1 << 22) -> str:
    """Simulate per-scale event streams from frames and write an EVS store,
    slab by slab (`frames_to_event_store` for videos that do not fit in
    memory, on the device).

    frames: anything indexable by frame (array, memmap, lazy image
    sequence), each [H, W] in [0, 1]; frame_chunk: frames per slab, the
    shared one included.  Thresholds are sampled as `frames_to_event_store`
    does.  log_sink(level, k0, logf_slab) receives every slab of log frames
    that is simulated (k0 = index of its first frame): the scaling runs in
    fp32 on the device, so the oracle of this pipeline is
    `simulate_events_log` on those frames.
    """
    rng = np.random.default_rng(seed)
    if cp is None or cn is None:
        cp, cn = sample_contrast_thresholds(rng)
    ts = check_timestamps(timestamps)
    T = len(frames)
    if ts.shape[0] != T:
        raise ValueError("one timestamp per frame is required")
    if T < 1:
        raise ValueError("at least one frame is required")
    frame_chunk = int(frame_chunk)
    if frame_chunk < 2:
        raise ValueError("frame_chunk must be at least 2")
    dev = torch.device(device)
    H, W = np.asarray(frames[0]).shape
    for lvl in levels:
        if lvl not in LEVEL_NAMES or H // lvl < 1 or W // lvl < 1:
            raise ValueError(f"level {lvl} does not fit frames {H}x{W}")

    with EventStoreWriter(path, (H, W)) as w:
        w.meta["contrast_thresholds"] = [float(cp), float(cn)]
        w.meta["refractory"] = float(refractory)
        sims = {lvl: DeviceEventSimulator(
            H // lvl, W // lvl, cp, cn, refractory, dev, max_chunk_events)
            for lvl in levels}
        groups = {lvl: w.open_group(LEVEL_NAMES[lvl]) for lvl in levels}
        images = w.open_images((H, W)) if store_images else None
        last = {}                    # level -> the last log frame, [1, h, w]
        try:
            a = 0
            while a < T:
                # the first slab brings frame_chunk frames, later ones the
                # frame they share with their predecessor plus the rest
                b = min(a + frame_chunk - (1 if a else 0), T)
                block_np = _frame_block(frames, a, b)
                if images is not None:
                    # rounded, so that 8-bit sources are stored as they were
                    images.append(np.rint(block_np * 255).clip(0, 255)
                                  .astype(np.uint8), ts[a:b])
                block = torch.from_numpy(block_np).to(dev)
                k0 = a - 1 if a else 0
                for lvl in levels:
                    logf = _log_frames(block, lvl)
                    if a:
                        logf = torch.cat([last[lvl], logf])
                    last[lvl] = logf[-1:].clone()
                    if log_sink is not None:
                        log_sink(lvl, k0, logf)
                    for chunk in sims[lvl].feed(logf, ts[k0:b]):
                        groups[lvl].append(*chunk)
                a = b
        finally:
            for g in groups.values():
                g.close()
            if images is not None:
                images.close()
    return str(path)
