"""Shared cases for the multi-recording (lanes) super-resolution tests: a
set of recordings of unequal length, exact batch-row-local stateful stubs,
and the single-path reference runs."""

import numpy as np
import torch
from torch import nn

from esr_amd.data.store import EventStoreWriter
from esr_amd.engine.superresolve import (super_resolve_store,
                                         super_resolve_stores)

import superresolve_helpers as S

GROUP, OUT_GROUP = "down2", "ori"
# window counts of the recording set; with seqn 3 the recordings run for
# 10, 3, 7, 1 and 5 steps, so two lanes hand over three times, once onto the
# 1-step recording
WINDOW_COUNTS = (12, 5, 9, 3, 7)
# events the single path writes per recording (seqn 3, WINDOW 32):
# MidFrame emits every window's 32 events, RunningSum 32 * (k + 1) at step k
MIDFRAME_EVENTS = (320, 96, 224, 32, 160)
MIDFRAME_CAP20_EVENTS = (200, 60, 140, 20, 100)
RUNNING_SUM_EVENTS = (2080, 288, 1120, 64, 640)


def write_lr_store(path, n_windows, seed, t_start, span=0.05, tail=S.TAIL):
    """A 'down2' recording on a 24 x 40 sensor like
    `superresolve_helpers.write_lr_store`: `n_windows` windows of S.WINDOW
    events plus `tail` more over `span` seconds from `t_start`; with six
    windows or more, one run of equal timestamps across a window boundary
    and one whole window on a single timestamp."""
    rng = np.random.default_rng(seed)
    W = S.WINDOW
    n = n_windows * W + tail
    ts = t_start + np.sort(rng.random(n)) * span
    if n_windows >= 7:
        ts[3 * W - 4:3 * W + 3] = ts[3 * W - 4]
        ts[5 * W:6 * W + 1] = ts[5 * W]
        ts = np.sort(ts)
    xs = np.clip(rng.normal(8, 3, n), 0, S.LR[1] - 1).astype(np.int64)
    ys = np.clip(rng.normal(5, 2, n), 0, S.LR[0] - 1).astype(np.int64)
    ps = rng.integers(0, 2, n) * 2 - 1
    with EventStoreWriter(path, S.HR) as w:
        w.add_group(GROUP, xs, ys, ts, ps)
    return str(path)


def write_recording_set(root, counts=WINDOW_COUNTS):
    """The recording set under `root`: Unix-epoch clocks an hour apart."""
    return [write_lr_store(root / f"rec{i}.evs", n, seed=10 + i,
                           t_start=1.7e9 + 3600.0 * i)
            for i, n in enumerate(counts)]


class _State(nn.Module):
    """The holder `state_holder` finds: `.state` carries the recurrence."""

    def __init__(self):
        super().__init__()
        self.state = None


class RunningSum(nn.Module):
    """state [B, 2, kH, kW] = the sum of the mid frames so far; output =
    mid + state.  Small integers, exact in fp32, and row b of the output
    depends on row b of the input and the state alone."""

    def __init__(self):
        super().__init__()
        self.time_propagate = _State()

    def reset_states(self):
        self.time_propagate.state = None

    def forward(self, x):
        mid = x[:, (x.size(1) - 1) // 2]
        old = self.time_propagate.state
        new = mid.clone() if old is None else old + mid
        self.time_propagate.state = new
        return mid + new


class TwoRowSum(RunningSum):
    """state [2B, 2, kH, kW]: rows [:B] accumulate mid, rows [B:] accumulate
    2 * mid; output = mid + both.  Sample b owns state rows b and B + b."""

    def forward(self, x):
        mid = x[:, (x.size(1) - 1) // 2]
        step = torch.cat([mid, 2 * mid])
        old = self.time_propagate.state
        new = step if old is None else old + step
        self.time_propagate.state = new
        B = mid.size(0)
        return mid + new[:B] + new[B:]


class TupleState(RunningSum):
    """A ConvLSTM-like pair as the state."""

    def forward(self, x):
        mid = x[:, (x.size(1) - 1) // 2]
        self.time_propagate.state = (mid.clone(), mid.clone())
        return mid


class OddRows(RunningSum):
    """A state of B + 1 rows: no whole number of rows per lane."""

    def forward(self, x):
        mid = x[:, (x.size(1) - 1) // 2]
        self.time_propagate.state = torch.cat([mid, mid[:1]])
        return mid


MODELS = {"midframe": S.MidFrame, "running_sum": RunningSum,
          "two_row": TwoRowSum}

_DROP = ("seconds",)


def sans_seconds(summary):
    return {k: v for k, v in summary.items() if k not in _DROP}


def run_args(**kw):
    args = dict(group=GROUP, scale=S.SCALE, seqn=3, window=S.WINDOW,
                device="cpu")
    args.update(kw)
    return args


def run_single(model_cls, srcs, root, **kw):
    """`super_resolve_store` on every recording alone: the reference.
    Returns [(dst, result)]."""
    root.mkdir(parents=True, exist_ok=True)
    out = []
    for i, src in enumerate(srcs):
        dst = str(root / f"out{i}.evs")
        out.append((dst, super_resolve_store(model_cls(), src, dst,
                                             **run_args(**kw))))
    return out


def run_lanes(model_cls, srcs, root, lanes, **kw):
    """`super_resolve_stores` on the whole list.  Returns [(dst, result)] in
    list order."""
    root.mkdir(parents=True, exist_ok=True)
    pairs = [(src, str(root / f"out{i}.evs")) for i, src in enumerate(srcs)]
    res = super_resolve_stores(model_cls(), pairs, lanes=lanes,
                               **run_args(**kw))
    assert list(res) == [dst for _, dst in pairs]
    return [(dst, res[dst]) for _, dst in pairs]


def assert_same_runs(got, want, keep=False):
    """Files byte-equal and summaries equal minus `seconds` (and minus the
    paths, which differ by construction)."""
    assert len(got) == len(want)
    for (dg, rg), (dw, rw) in zip(got, want):
        S.assert_same_files(dg, dw, OUT_GROUP)
        sg, sw = (rg[0], rw[0]) if keep else (rg, rw)
        assert sans_seconds(sg) == sans_seconds(sw), (dg, dw)
