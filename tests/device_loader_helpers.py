"""Shared fixture of the device-resident loader tests: two small EVS
sequences on a (40, 86) sensor, so the input group is 20x43 and the
fp32 divide-then-multiply of the CPU dataset does not reduce to x * scale
(column 15 lands on 29, column 30 on 59)."""

import copy

import numpy as np

from esr_amd.data import EventStoreWriter

SENSOR = (40, 86)
N_ORI, N_DOWN2 = 12_000, 3_000
# rows of every group that hold an out-of-range event: x = W at the first of
# each pair, y = H + 3 at the second
OUT_OF_RANGE_ROWS = (5, 6, 300, 301, 1500, 1501)


def _group(rng, n, res):
    H, W = res
    xs = rng.integers(0, W, n)
    ys = rng.integers(0, H, n)
    ps = rng.choice(np.array([-1, 1]), n)
    ts = np.sort(rng.random(n))
    # the columns whose fp32 mapping differs from x * 2 at width 43
    xs[10:14] = (15, 30, 15, 30)
    for k, row in enumerate(OUT_OF_RANGE_ROWS):
        if k % 2 == 0:
            xs[row] = W
        else:
            ys[row] = H + 3
    return xs, ys, ts, ps


def write_sequence(path, seed, mutate=None):
    """One sequence directory; `mutate(group, xs, ys, ts, ps)` may edit the
    arrays of a group in place before they are written."""
    rng = np.random.default_rng(seed)
    with EventStoreWriter(path, SENSOR) as w:
        for group, n, res in (("ori", N_ORI, SENSOR),
                              ("down2", N_DOWN2, (SENSOR[0] // 2,
                                                  SENSOR[1] // 2))):
            xs, ys, ts, ps = _group(rng, n, res)
            if mutate is not None:
                mutate(group, xs, ys, ts, ps)
            w.add_group(group, xs, ys, ts, ps)
    return path


def make_datalist(root, mutate=None):
    """Write the 2-sequence fixture under `root`; returns the datalist."""
    paths = [write_sequence(root / f"seq{k}.evs", 100 + k, mutate)
             for k in range(2)]
    datalist = root / "datalist.txt"
    datalist.write_text("".join(f"{p}\n" for p in paths))
    return datalist


def dl_config(datalist, **dataset_overrides):
    ds = {
        "scale": 2, "ori_scale": "down2", "time_bins": 1,
        "need_gt_frame": False, "need_gt_events": True,
        "mode": "events", "window": 256, "sliding_window": 128,
        "data_augment": {"enabled": True,
                         "augment": ["Horizontal", "Vertical", "Polarity"],
                         "augment_prob": [0.5, 0.5, 0.5]},
        "hot_filter": {"enabled": False},
        "sequence": {"sequence_length": 4, "seqn": 3, "step_size": None,
                     "pause": {"enabled": False,
                               "proba_pause_when_running": 0.4,
                               "proba_pause_when_paused": 0.5}},
    }
    ds.update(copy.deepcopy(dataset_overrides))
    return {"use_ddp": False, "path_to_datalist_txt": str(datalist),
            "batch_size": 2, "shuffle": False, "num_workers": 0,
            "pin_memory": False, "drop_last": True, "dataset": ds}
