"""Shared cases for the offline super-resolution tests (CPU and GPU)."""

import numpy as np
import torch
from torch import nn

from esr_amd.data.store import EventStore, EventStoreWriter
from esr_amd.ops import events as E

Q = 1 << 20
NAN, INF = float("nan"), float("inf")
COLS = ("xs", "ys", "ts", "ps")

# 2 x 3 x 4, cell_cap 5: counts 2, 4, 1 in channel 0 and 5, 2 in channel 1
HAND_CAP = 5
HAND = torch.tensor([[[2.5, 0.0, 3.5, 0.0],
                      [0.0, 1.0, 0.0, 0.0],
                      [-3.0, NAN, 0.4, 0.0]],
                     [[0.0, 0.0, 0.0, 0.0],
                      [0.0, INF, 0.0, 0.0],
                      [0.0, 0.0, 0.0, 2.0]]])
HAND_COUNTS = torch.tensor([[[2, 0, 4, 0], [0, 1, 0, 0], [0, 0, 0, 0]],
                            [[0, 0, 0, 0], [0, 5, 0, 0], [0, 0, 0, 2]]])
# (x, y, p, q) in file order: by phase, ties in cell order then j
HAND_ROWS = [
    (0, 0, 1, 0), (2, 0, 1, 0), (1, 1, 1, 0), (1, 1, -1, 0), (3, 2, -1, 0),
    (1, 1, -1, Q // 4), (2, 0, 1, Q // 3), (1, 1, -1, Q // 2),
    (2, 0, 1, 2 * Q // 3), (1, 1, -1, 3 * Q // 4),
    (0, 0, 1, Q), (2, 0, 1, Q), (1, 1, -1, Q), (3, 2, -1, Q)]


def timestamps(t0, t1, q):
    """The timestamp rule in numpy float64, one rounding per operation."""
    q = np.asarray(q, dtype=np.int64)
    frac = (Q + 99 * q).astype(np.float64) / np.float64(100 * Q)
    ts = np.float64(t0) + (np.float64(t1) - np.float64(t0)) * frac
    return np.minimum(np.maximum(ts, np.float64(t0)), np.float64(t1))


def splat_rows(xs, ys, ps, hw):
    """[2, H, W] int64 count map of event columns."""
    out = E.events_to_channels(torch.as_tensor(xs.astype(np.int64)),
                               torch.as_tensor(ys.astype(np.int64)),
                               torch.as_tensor(ps.astype(np.float32)), hw)
    return out.abs().round().long()


class MidFrame(nn.Module):
    """Returns its mid input frame; no state."""

    def forward(self, x):
        return x[:, (x.size(1) - 1) // 2]


class Lifted(nn.Module):
    """ESRNet plus 1.5 x its mid input frame, so that cells hold events even
    with untrained weights; the recurrent state is the net's."""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.time_propagate = net.time_propagate

    def reset_states(self):
        self.net.reset_states()

    def forward(self, x):
        return self.net(x) + 1.5 * x[:, (x.size(1) - 1) // 2]


LR = (12, 20)
SCALE = 2
HR = (LR[0] * SCALE, LR[1] * SCALE)
WINDOW = 32
N_WINDOWS = 12
TAIL = 7


def write_lr_store(path, t_start=1.7e9, seed=3, duplicates=True):
    """A 'down2' recording on a 24 x 40 sensor: N_WINDOWS windows of WINDOW
    events plus TAIL more, Unix-epoch timestamps, one run of equal
    timestamps across a window boundary."""
    rng = np.random.default_rng(seed)
    n = N_WINDOWS * WINDOW + TAIL
    ts = t_start + np.sort(rng.random(n)) * 0.05
    if duplicates:
        ts[3 * WINDOW - 4:3 * WINDOW + 3] = ts[3 * WINDOW - 4]
        # a whole window, and its right edge, on one timestamp
        ts[5 * WINDOW:6 * WINDOW + 1] = ts[5 * WINDOW]
        ts = np.sort(ts)
    # clustered so that HR cells hold several events
    xs = np.clip(rng.normal(8, 3, n), 0, LR[1] - 1).astype(np.int64)
    ys = np.clip(rng.normal(5, 2, n), 0, LR[0] - 1).astype(np.int64)
    ps = rng.integers(0, 2, n) * 2 - 1
    with EventStoreWriter(path, HR) as w:
        w.add_group("down2", xs, ys, ts, ps)
    return str(path)


def read_group(path, group):
    st = EventStore(path)
    n = st.num_events(group)
    return {f: np.load(st.path / f"{group}_{f}.npy") for f in COLS}, n


def inp_scaled_cnt(path, group, begin, end, lr, hr):
    """The training loader's input map of source rows [begin, end)."""
    ev = torch.from_numpy(EventStore(path).events(group, begin, end))
    return E.scaled_count_encoding(E.normalize_events(ev, lr), hr, "cnt")


def window_row_ranges(stats):
    """Row range of each emitted window, from the stats table."""
    emitted = np.asarray(stats)[:, 1]
    stop = np.cumsum(emitted)
    return list(zip((stop - emitted).tolist(), stop.tolist()))


def assert_same_files(a, b, group_a, group_b=None):
    ca, na = read_group(a, group_a)
    cb, nb = read_group(b, group_b or group_a)
    assert na == nb
    for f in COLS:
        assert ca[f].dtype == cb[f].dtype, f
        assert ca[f].tobytes() == cb[f].tobytes(), f"column {f} differs"
