"""Shared cases for the event-simulator tests (CPU and GPU)."""

import math

import numpy as np

from esr_amd.data.store import EventStore

CP, CN = 0.11, 0.07
COLS = ("xs", "ys", "ts", "ps")


def _smooth(a, sigma):
    r = int(3 * sigma) + 1
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), ax, a)
    return a


def texture(h, w, seed=0, sigma=1.5):
    tex = _smooth(np.random.default_rng(seed).random((h, w)), sigma)
    return (tex - tex.min()) / np.ptp(tex)


def panned(T, H, W, dy=1, dx=2, seed=0, sigma=1.5):
    """Frame t is the crop of a smooth random texture at (dy*t, dx*t)."""
    tex = texture(H + dy * T, W + dx * T, seed, sigma)
    return np.stack([tex[dy * t:dy * t + H, dx * t:dx * t + W]
                     for t in range(T)])


def case():
    """frames [7, 9, 13] in [0, 1] and their timestamps: a panned texture, a
    flat block that ramps (many equal timestamps) and a block that steps
    from 0 to 1 (dozens of crossings in one interval)."""
    T, H, W = 7, 9, 13
    frames = panned(T, H, W)
    frames[:, :3, :4] = np.linspace(0.1, 0.9, T)[:, None, None]
    frames[:3, 6:, 9:] = 0.0
    frames[3:, 6:, 9:] = 1.0
    return frames, np.linspace(0, 0.03, T)


def case_log():
    frames, ts = case()
    return np.log(frames + 1e-3), ts


def smooth_pan_log(H, W, shift=8):
    """Two analytic log frames of a smooth pattern moved by `shift` pixels."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    fr = [0.5 + 0.25 * np.sin((x + s) / 17.0) + 0.2 * np.cos((y + s) / 23.0)
          for s in (0, shift)]
    return np.log(np.stack(fr) + 1e-3), np.array([0.0, 1.0 / 240])


def brute_force(logf, ts, cp, cn, refractory=0.0):
    """The model of simulate_events_log pixel by pixel in Python floats, and
    the stated order by an explicit sort.  Returns ([4, N], k per event)."""
    T, H, W = logf.shape
    rows = []
    for y in range(H):
        for x in range(W):
            ref = float(logf[0, y, x])
            t_last = None
            for k in range(1, T):
                l0, l1 = float(logf[k - 1, y, x]), float(logf[k, y, x])
                t0, t1 = float(ts[k - 1]), float(ts[k])
                dl = l1 - ref
                n_pos = math.floor(max(dl, 0.0) / cp)
                n_neg = math.floor(max(-dl, 0.0) / cn)
                for n, C, pol in ((n_pos, cp, 1.0), (n_neg, cn, -1.0)):
                    for i in range(1, n + 1):
                        target = ref + (pol * C) * i
                        frac = ((target - l0) / (l1 - l0)
                                if abs(l1 - l0) > 1e-12 else 0.5)
                        frac = min(max(frac, 0.0), 1.0)
                        t = t0 + frac * (t1 - t0)
                        if (refractory > 0 and t_last is not None
                                and not t - t_last >= refractory):
                            continue
                        t_last = t
                        rows.append((t, k, 0 if pol > 0 else 1, i, y, x))
                ref = (ref + n_pos * cp) - n_neg * cn
    rows.sort()
    ev = np.array([[r[5], r[4], r[0], 1.0 if r[2] == 0 else -1.0]
                   for r in rows], dtype=np.float64).reshape(-1, 4).T
    return ev, np.array([r[1] for r in rows], dtype=np.int64)


def assert_case_conditions(ev, suppressed=None):
    """What the case must exercise: ties, both polarities, suppression."""
    assert (np.diff(ev[2]) == 0).sum() > 0
    assert (ev[3] > 0).any() and (ev[3] < 0).any()
    if suppressed is not None:
        assert 0 < suppressed < ev.shape[1]


def assert_events_equal(got, want):
    assert got.shape == want.shape
    for i, name in enumerate(COLS):
        assert np.array_equal(got[i], want[i]), name


def group_events(path, group):
    s = EventStore(path)
    return s.events(group, 0, s.num_events(group))


def stores_identical(a, b):
    sa, sb = EventStore(a), EventStore(b)
    assert sa.meta == sb.meta
    for g in sa.groups:
        for c in COLS:
            assert np.array_equal(sa._arr(f"{g}_{c}"), sb._arr(f"{g}_{c}")), \
                (g, c)
    if sa.num_images:
        assert np.array_equal(sa._arr("images"), sb._arr("images"))
        assert np.array_equal(sa.image_ts(), sb.image_ts())


def dataset_config():
    return {"scale": 2, "ori_scale": "down4", "time_bins": 1,
            "need_gt_frame": False, "need_gt_events": True,
            "mode": "events", "window": 64, "sliding_window": 16,
            "data_augment": {"enabled": False, "augment": [],
                             "augment_prob": []},
            "hot_filter": {"enabled": False},
            "sequence": {"sequence_length": 2, "seqn": 2, "step_size": None,
                         "pause": {"enabled": False,
                                   "proba_pause_when_running": 0,
                                   "proba_pause_when_paused": 0}}}
