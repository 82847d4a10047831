"""Multi-stream serving: many event streams in one graph replay.

`StreamingESR` serves one stream; S cameras mean S servers, S weight copies
and S captured graphs replayed one after the other.  The model is
launch-latency-bound (docs/ARCHITECTURE.md, section 1), so a batch-1 replay
leaves the GPU mostly idle.  `MultiStreamESR` serves up to `max_streams`
independent streams from ONE model and ONE captured graph:

  * the sliding windows of all streams live in one static buffer
    [seqn, S, 2, kH, kW], which transposed to [S, seqn, ...] is the model's
    frame-major input without a copy;
  * the recurrent state is one tensor [2S, C, h, w]; stream s owns rows s
    (forward scan) and S+s (backward scan);
  * per tick the host writes the concatenated events and one small control
    block (segment offsets, has_window / ready / reset flags per stream);
    everything that depends on them (window shift, splat, state masking,
    forward, state commit) runs on the device inside the graph
    (ops/native/src/stream_ingest.hip).

Every stream behaves exactly as if it had a `StreamingESR` of its own: no
output and no state advance before `seqn` windows, and a stream absent from
a tick keeps its window and state untouched.

On CPU, or without the native extension, ingest is plain torch and nothing
is captured; that path is also the oracle the HIP kernels are tested against.
"""

from __future__ import annotations

import warnings

import torch

from ..ops.native import get_ext
from .capture import amp_autocast, capture_graph, state_holder
from .streaming import counts_to_events

__all__ = ["MultiStreamESR", "window_advance_torch", "splat_ragged_torch"]

HAS_WINDOW, READY, RESET = 0, 1, 2      # rows of the control tensor


def window_advance_torch(buf: torch.Tensor, ctrl: torch.Tensor) -> None:
    """Torch form of `stream_window_advance`: in place on
    buf [seqn, S, 2, kH, kW] with ctrl int32 [3, S]."""
    reset = ctrl[RESET] != 0
    shift = (ctrl[HAS_WINDOW] != 0) & ~reset
    buf[:, reset] = 0
    if bool(shift.any()):
        moved = buf[1:, shift].clone()
        buf[:-1, shift] = moved
        buf[-1, shift] = 0


def splat_ragged_torch(events: torch.Tensor, offsets: torch.Tensor,
                       ctrl: torch.Tensor, buf: torch.Tensor,
                       scale: int) -> None:
    """Torch form of `stream_splat_ragged`: adds the tick's events
    ([cap, 4] LR rows, stream s owning rows offsets[s]..offsets[s+1]) into
    buf[seqn-1] in place."""
    S, kH, kW = buf.size(1), buf.size(3), buf.size(4)
    total = min(int(offsets[S]), events.size(0))
    if total <= 0:
        return
    ev = events[:total]
    row = torch.arange(total, device=ev.device)
    s = (row[:, None] >= offsets[1:S].long()[None, :]).sum(1)
    fx, fy, p = ev[:, 0].floor(), ev[:, 1].floor(), ev[:, 3]
    valid = (p != 0) & (fx >= 0) & (fx < kW // scale) & (fy >= 0) \
        & (fy < kH // scale) & (ctrl[HAS_WINDOW].long()[s] != 0)
    s, fx, fy, p = s[valid], fx[valid], fy[valid], p[valid]
    ch = (~(p > 0)).long()
    lin = ((s * 2 + ch) * kH + fy.long() * scale) * kW + fx.long() * scale
    buf[-1].view(-1).index_add_(0, lin, p.abs())


class MultiStreamESR:
    """Stateful sliding-window SR server for up to `max_streams` streams.

    `open()` hands out a slot id; `step({sid: events})` pushes one LR event
    window ([4, n]: x, y, t, p in LR pixel coordinates) for each listed
    stream and returns `{sid: [2, kH, kW]}` for the listed streams that have
    pushed at least `seqn` windows.
    """

    def __init__(self, model, lr_resolution, scale: int = 2, seqn: int = 3,
                 max_streams: int = 8, max_events: int = 1 << 16,
                 device="cuda:0", use_graphs: bool = True,
                 amp_dtype=torch.bfloat16):
        self.model = model.to(device).eval()
        self.device = torch.device(device)
        self.lr_res = tuple(lr_resolution)
        self.hr_res = (self.lr_res[0] * scale, self.lr_res[1] * scale)
        self.scale = int(scale)
        self.seqn = int(seqn)
        self.max_streams = S = int(max_streams)
        self.max_events = int(max_events)
        self.amp_dtype = amp_dtype
        on_gpu = self.device.type == "cuda"
        ext = get_ext() if on_gpu else None
        self._ext = ext if ext is not None \
            and hasattr(ext, "stream_splat_ragged") else None
        self.use_graphs = bool(use_graphs) and self._ext is not None
        if on_gpu and self._ext is None:
            # the issue's documented fallback, but never a silent one: the
            # torch ingest is off the HIP path and cannot be captured
            warnings.warn(
                "MultiStreamESR: the native stream_ingest kernels are not "
                "built (run `python -m esr_amd.ops.native.build`); using "
                "the torch ingest without graph capture", RuntimeWarning,
                stacklevel=2)

        holder = state_holder(self.model)
        lstm = getattr(holder, "lstm", None)
        if getattr(lstm, "recurrent_block_type", None) == "convlstm":
            raise NotImplementedError(
                "MultiStreamESR needs a single-tensor recurrent state; "
                "recurrent_block_type='convlstm' carries a tuple")

        # static device buffers
        self._buf = torch.zeros(self.seqn, S, 2, *self.hr_res,
                                device=self.device)
        self._events = torch.zeros(self.max_events, 4, device=self.device)
        self._control = torch.zeros(4 * S + 1, dtype=torch.int32,
                                    device=self.device)
        self._offsets = self._control[:S + 1]
        self._ctrl = self._control[S + 1:].view(3, S)
        # host staging, double-buffered: a block is rewritten only after
        # the copies that read it two ticks ago have finished
        self._stage = [self._make_stage(on_gpu) for _ in range(2)]
        self._tick = 0

        # one dry forward on empty windows fixes the state's shape and dtype
        self._state = None
        if holder is not None:
            holder.state = None
            self._forward(self._buf.transpose(0, 1))
            st = holder.state
            if isinstance(st, tuple):
                raise NotImplementedError(
                    "MultiStreamESR needs a single-tensor recurrent state")
            if st is not None:
                self._state = torch.zeros_like(st)
            holder.state = self._state

        # slot bookkeeping (host)
        self._open = [False] * S
        self._count = [0] * S           # windows pushed since open/reset
        self._pending_reset = [False] * S
        self._graph = None
        self._out = None

    # ------------------------------------------------------------------
    def _make_stage(self, pinned: bool):
        S = self.max_streams
        return {"events": torch.zeros(self.max_events, 4, pin_memory=pinned),
                "control": torch.zeros(4 * S + 1, dtype=torch.int32,
                                       pin_memory=pinned),
                "done": None}

    # -- slots ---------------------------------------------------------
    def open(self) -> int:
        """Claim a free slot; the stream starts with an empty window and a
        zero recurrent state."""
        for sid, taken in enumerate(self._open):
            if not taken:
                self._open[sid] = True
                self._count[sid] = 0
                self._pending_reset[sid] = True
                return sid
        raise RuntimeError(
            f"all {self.max_streams} stream slots are taken")

    def close(self, sid: int) -> None:
        self._check(sid)
        self._open[sid] = False
        self._count[sid] = 0
        self._pending_reset[sid] = True

    def reset(self, sid: int) -> None:
        """Forget the window and the recurrence of one stream."""
        self._check(sid)
        self._count[sid] = 0
        self._pending_reset[sid] = True

    def _check(self, sid):
        if not (isinstance(sid, int) and 0 <= sid < self.max_streams
                and self._open[sid]):
            raise KeyError(f"stream {sid!r} is not open")

    # -- the per-tick device work (captured as one graph) --------------
    @torch.no_grad()
    def _forward(self, inp: torch.Tensor) -> torch.Tensor:
        with amp_autocast(self.amp_dtype, self.device, cache_enabled=False):
            return self.model(inp).float()      # no-op on an fp32 output

    @torch.no_grad()
    def _tick_body(self) -> torch.Tensor:
        if self._ext is not None:
            self._ext.stream_window_advance(self._buf, self._ctrl)
            self._ext.stream_splat_ragged(self._events, self._offsets,
                                          self._ctrl, self._buf, self.scale)
        else:
            window_advance_torch(self._buf, self._ctrl)
            splat_ragged_torch(self._events, self._offsets, self._ctrl,
                               self._buf, self.scale)
        holder = state_holder(self.model)
        if self._state is not None:
            # rows s and S+s belong to stream s
            reset = (self._ctrl[RESET] != 0).repeat(2).view(-1, 1, 1, 1)
            self._state.masked_fill_(reset, 0)
            holder.state = self._state
        # [S, seqn, 2, kH, kW] view; the model's own transpose + reshape to
        # frame-major lands back on the contiguous buffer
        out = self._forward(self._buf.transpose(0, 1))
        if self._state is not None:
            ready = (self._ctrl[READY] != 0).repeat(2).view(-1, 1, 1, 1)
            new = holder.state.to(self._state.dtype)
            self._state.copy_(torch.where(ready, new, self._state))
            holder.state = self._state
        return out

    def _capture(self) -> None:
        # with an all-zero control block the body shifts, splats, resets
        # and commits nothing, so warm-up runs leave windows and state as
        # they are
        self._control.zero_()
        self._graph, self._out = capture_graph(self._tick_body, warmup=2,
                                               device=self.device)

    # -- serving -------------------------------------------------------
    @torch.no_grad()
    def _run(self, windows: dict) -> list[int]:
        """One tick; returns the ready slot ids (output in self._out)."""
        S = self.max_streams
        for sid in windows:
            self._check(sid)
        order = sorted(windows)
        sizes = []
        for sid in order:
            ev = windows[sid]
            if ev.dim() != 2 or ev.size(0) != 4:
                raise ValueError("events must be [4, n] (x, y, t, p)")
            sizes.append(ev.size(1))
        total = sum(sizes)
        if total > self.max_events:
            raise ValueError(
                f"{total} events in one tick exceed max_events="
                f"{self.max_events}")
        if not order:
            return []

        if self.use_graphs and self._graph is None:
            self._capture()

        # 1. plan the tick without touching the server's bookkeeping
        control = [0] * (4 * S + 1)     # offsets [S+1] | ctrl [3, S]
        count = list(self._count)
        ready = []
        spans = []
        off = 0
        for sid in range(S):
            control[sid] = off
            if sid in windows:
                n = windows[sid].size(1)
                spans.append((sid, off, n))
                off += n
                control[S + 1 + HAS_WINDOW * S + sid] = 1
                count[sid] = min(count[sid] + 1, self.seqn)
                if count[sid] >= self.seqn:
                    control[S + 1 + READY * S + sid] = 1
                    ready.append(sid)
            if self._pending_reset[sid]:
                control[S + 1 + RESET * S + sid] = 1
        control[S] = off

        # 2. stage the events; a window that cannot be copied (dtype,
        # device) raises here, before anything the kernels read has changed
        # hands: the event rows are dead until the control block names them
        stage = self._stage[self._tick % 2]
        if stage["done"] is not None:
            stage["done"].synchronize()
        on_host = all(not windows[sid].is_cuda for sid in order)
        dst = stage["events"] if on_host else self._events
        for sid, o, n in spans:
            dst[o:o + n].copy_(windows[sid].t(), non_blocking=True)
        stage["control"].copy_(torch.tensor(control, dtype=torch.int32))

        # 3. commit the bookkeeping, then hand the tick to the device
        self._tick += 1
        self._count = count
        self._pending_reset = [False] * S
        if on_host and total:
            self._events[:total].copy_(stage["events"][:total],
                                       non_blocking=True)
        self._control.copy_(stage["control"], non_blocking=True)
        if self.device.type == "cuda":
            stage["done"] = torch.cuda.Event()
            stage["done"].record(torch.cuda.current_stream(self.device))

        if self._graph is not None:
            self._graph.replay()
        else:
            self._out = self._tick_body()
        return ready

    @torch.no_grad()
    def step(self, windows: dict) -> dict:
        """Push one LR event window per listed stream; returns
        `{sid: HR count map [2, kH, kW]}` for the listed streams that are
        warm.  Streams not listed keep their window and state."""
        ready = self._run(windows)
        # clones: the graph writes into one static output buffer
        return {sid: self._out[sid].clone() for sid in ready}

    @torch.no_grad()
    def step_events(self, windows: dict, capacity: int | None = None,
                    mode: str = "linear") -> dict:
        """Like `step`, but each warm stream's prediction comes back as an
        HR event stream [n, 4] (x, y, t, p sorted by t), as in
        `StreamingESR.push_events`."""
        ready = self._run(windows)
        if not ready:
            return {}
        return dict(zip(ready, counts_to_events(self._out[ready], mode,
                                                capacity)))
