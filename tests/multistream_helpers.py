"""Shared schedule and oracles for the MultiStreamESR tests (CPU and GPU)."""

import copy

import torch

from esr_amd.engine.streaming import StreamingESR
from esr_amd.ops.events import events_to_channels

LR = (16, 24)            # H, W: non-square so an H/W swap shows
SCALE = 2
HR = (LR[0] * SCALE, LR[1] * SCALE)
SEQN = 3
MAX_STREAMS = 3
A, C, B = 0, 1, 2        # open() hands out the lowest free slot; B joins last

# Which streams push at which tick.  A pushes every tick; B joins at tick 2
# and skips tick 4; C pushes at 0..3, is reset after tick 3 and pushes again
# at 4..6, then is closed and its slot re-opened (ticks 7..9: the slot's next
# owner, a fresh stream).
PUSHES = [
    {A, C}, {A, C}, {A, B, C}, {A, B, C}, {A, C}, {A, B, C}, {A, B, C},
    {A, C}, {A, B, C}, {A, C},
]
OPEN_BEFORE = {0: [A, C], 2: [B]}
RESET_AFTER = {3: [C]}
REOPEN_AFTER = {6: [C]}
# a stream is warm from its third push since open/reset
WARM = [
    set(), set(), {A, C}, {A, C}, {A}, {A, B}, {A, B, C},
    {A}, {A, B}, {A, C},
]


def window(sid, tick):
    """LR event window [4, n] of stream `sid` at `tick`; n differs per
    stream and tick so the concatenation is ragged."""
    g = torch.Generator().manual_seed(1000 * sid + tick)
    n = 90 + 37 * sid + 11 * tick
    H, W = LR
    return torch.stack([
        (torch.rand(n, generator=g) * W).floor(),
        (torch.rand(n, generator=g) * H).floor(),
        torch.sort(torch.rand(n, generator=g)).values,
        torch.randint(0, 2, (n,), generator=g).float() * 2 - 1])


def run_multistream(srv):
    """Drive `srv` through the schedule; returns one {sid: map} per tick."""
    outs = []
    for tick, pushing in enumerate(PUSHES):
        for sid in OPEN_BEFORE.get(tick, ()):
            assert srv.open() == sid
        outs.append(srv.step({sid: window(sid, tick) for sid in pushing}))
        for sid in RESET_AFTER.get(tick, ()):
            srv.reset(sid)
        for sid in REOPEN_AFTER.get(tick, ()):
            srv.close(sid)
            assert srv.open() == sid
    return outs


def run_single_servers(model, device="cpu"):
    """The same schedule on one StreamingESR per stream, each holding its
    own copy of the model and fed only that stream's windows."""
    def make():
        return StreamingESR(copy.deepcopy(model), LR, scale=SCALE, seqn=SEQN,
                            device=device, use_graphs=False, amp_dtype=None)
    servers = {A: make(), B: make(), C: make()}
    outs = []
    for tick, pushing in enumerate(PUSHES):
        res = {}
        for sid in sorted(pushing):
            out = servers[sid].push(window(sid, tick))
            if out is not None:
                res[sid] = out
        outs.append(res)
        for sid in RESET_AFTER.get(tick, ()):
            servers[sid].reset()
        for sid in REOPEN_AFTER.get(tick, ()):
            servers[sid] = make()
    return outs


@torch.no_grad()
def run_batched_oracle(model):
    """Plain-python form of the batched semantics on CPU: per-stream frame
    lists and state rows, the model called at batch MAX_STREAMS like the
    server does, so the comparison isolates the window / warm-up / state
    bookkeeping from any batch-size effect of the convolutions."""
    model = copy.deepcopy(model).eval()
    S = MAX_STREAMS
    zero = torch.zeros(2, *HR)
    frames = {s: [zero] * SEQN for s in range(S)}
    count = {s: 0 for s in range(S)}
    state = None
    outs = []
    for tick, pushing in enumerate(PUSHES):
        for sid in pushing:
            w = window(sid, tick)
            f = events_to_channels(w[0].floor() * SCALE, w[1].floor() * SCALE,
                                   w[3], HR)
            frames[sid] = frames[sid][1:] + [f]
            count[sid] += 1
        ready = [s for s in sorted(pushing) if count[s] >= SEQN]
        x = torch.stack([torch.stack(frames[s]) for s in range(S)])
        model.time_propagate.state = None if state is None else state.clone()
        out = model(x)
        new = model.time_propagate.state
        if state is None:
            state = torch.zeros_like(new)
        for s in ready:
            state[s] = new[s]
            state[S + s] = new[S + s]
        outs.append({s: out[s].clone() for s in ready})
        for sid in list(RESET_AFTER.get(tick, ())) + \
                list(REOPEN_AFTER.get(tick, ())):
            frames[sid] = [zero] * SEQN
            count[sid] = 0
            state[sid] = 0
            state[S + sid] = 0
    return outs


# ---------------------------------------------------------------------------
# ingest kernels: independent per-element oracle and case builder

def ingest_loop_oracle(buf, events, offsets, ctrl, scale):
    """Per-stream / per-event python loops over the documented rule of
    stream_window_advance + stream_splat_ragged; returns a new buffer."""
    import math
    out = buf.clone()
    seqn, S, _, kH, kW = buf.shape
    off = offsets.tolist()
    has, _, reset = ctrl.tolist()
    for s in range(S):
        if reset[s]:
            out[:, s] = 0
        if has[s]:
            for f in range(seqn - 1):
                out[f, s] = out[f + 1, s]
            out[seqn - 1, s] = 0
    rows = events.tolist()
    for s in range(S):
        if not has[s]:
            continue
        for i in range(off[s], min(off[s + 1], len(rows))):
            x, y, _, p = rows[i]
            if p == 0 or not (math.isfinite(x) and math.isfinite(y)):
                continue
            xi, yi = math.floor(x) * scale, math.floor(y) * scale
            if 0 <= xi < kW and 0 <= yi < kH:
                out[seqn - 1, s, 0 if p > 0 else 1, yi, xi] += abs(p)
    return out


def ingest_events(lr, sizes, cap, seed=0):
    """Ragged event buffer [cap, 4] with segment lengths `sizes` (rows past
    their sum are zero) and int32 offsets.  Coordinates are fractional and
    reach from -1 to W (H) inclusive; p is -1, 0 (padding) or +1; every
    non-empty segment starts with a pile of events on one pixel and with
    the four out-of-range corners."""
    g = torch.Generator().manual_seed(seed)
    lrH, lrW = lr
    total = sum(sizes)
    assert total <= cap
    ev = torch.zeros(cap, 4)
    ev[:total, 0] = torch.rand(total, generator=g) * (lrW + 2) - 1.5
    ev[:total, 1] = torch.rand(total, generator=g) * (lrH + 2) - 1.5
    ev[:total, 2] = torch.rand(total, generator=g)
    ev[:total, 3] = torch.randint(-1, 2, (total,), generator=g).float()
    offsets = [0]
    for n in sizes:
        o = offsets[-1]
        if n >= 12:
            ev[o:o + 6, 0], ev[o:o + 6, 1] = 3.7, 2.2     # one pixel, 6 times
            ev[o:o + 4, 3] = 1.0
            ev[o + 4:o + 6, 3] = -1.0
            edge = torch.tensor([[-1.0, 2.0], [float(lrW), 2.0],
                                 [2.0, -1.0], [2.0, float(lrH)],
                                 [-0.5, 1.0], [lrW - 0.25, lrH - 0.25]])
            ev[o + 6:o + 12, :2] = edge
            ev[o + 6:o + 12, 3] = 1.0
        offsets.append(o + n)
    offsets = torch.tensor(offsets, dtype=torch.int32)
    return ev, offsets


# (has_window, reset) per stream for the main case, whose segments are
# [40 rows, empty, the rest]:
INGEST_CTRL = {
    # stream 1 has a window with no events: it only shifts
    "all_push": ([1, 1, 1], [0, 0, 0]),
    # stream 1 untouched; stream 2 reset, then this tick's splat
    "idle_and_reset_push": ([1, 0, 1], [0, 0, 1]),
    # stream 0 reset without a window: all zero, its 40 rows ignored
    "reset_idle": ([0, 0, 1], [1, 0, 0]),
    # stream 0 idle with rows in its segment: unchanged
    "idle_with_rows": ([0, 1, 1], [0, 1, 0]),
}


def ingest_ctrl(has, reset):
    ready = [0] * len(has)           # not read by the ingest kernels
    return torch.tensor([has, ready, reset], dtype=torch.int32)


def ingest_buffer(seqn, S, hr, seed=0):
    """Window buffer filled with small non-zero counts, so that a shift, a
    reset and an untouched stream all look different."""
    g = torch.Generator().manual_seed(100 + seed)
    return torch.randint(1, 5, (seqn, S, 2, *hr), generator=g).float()


def check_ingest_structure(got, buf0, has, reset, scale):
    """What each has_window / reset combination must leave behind,
    stated without an oracle."""
    for s in range(got.size(1)):
        if not has[s] and not reset[s]:
            assert torch.equal(got[:, s], buf0[:, s])       # untouched
            continue
        if not has[s]:
            assert not got[:, s].any()                      # reset, idle
        elif reset[s]:
            assert not got[:-1, s].any()                    # only the splat
        else:
            assert torch.equal(got[:-1, s], buf0[1:, s])    # shifted
        # only pixels on the scale grid can receive events
        last = got[-1, s].clone()
        last[..., ::scale, ::scale] = 0
        assert not last.any()
