"""Offline super-resolution on the CPU: window tiling, the torch emission
oracle, the append writer, `super_resolve_store` end to end and the CLI."""

import copy
import json
import logging
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from esr_amd.data.device_loader import batch_splat_torch, pack_events
from esr_amd.data.store import EventStore, EventStoreWriter
from esr_amd.engine.superresolve import (PHASE_Q, cell_counts_torch,
                                         emit_window_torch, hash_phase_torch,
                                         super_resolve_store, tile_windows)
from esr_amd.models import build_model

import superresolve_helpers as S

REPO = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------
# tile_windows

def test_tile_events_boundaries_and_tail():
    ts = np.arange(23, dtype=np.float64) * 0.5 + 100.0
    t = tile_windows(ts, "events", 5)
    assert t["begin"].tolist() == [0, 5, 10, 15]
    assert t["end"].tolist() == [5, 10, 15, 20]
    assert t["t0"].tolist() == [100.0, 102.5, 105.0, 107.5]
    assert t["t1"].tolist() == [102.5, 105.0, 107.5, 110.0]
    assert t["tail_events"] == 3
    # no partial tail: the final window ends on the last timestamp
    t = tile_windows(ts[:20], "events", 5)
    assert t["end"].tolist()[-1] == 20 and t["tail_events"] == 0
    assert t["t1"][-1] == ts[19]
    t = tile_windows(ts[:4], "events", 5)
    assert t["begin"].size == 0 and t["tail_events"] == 4


def test_tile_events_equal_timestamps_across_boundary():
    ts = np.array([0.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 3.0])
    t = tile_windows(ts, "events", 3)
    assert t["t0"].tolist() == [0.0, 2.0, 2.0]
    assert t["t1"].tolist() == [2.0, 2.0, 3.0]          # window 1: t1 == t0
    assert t["tail_events"] == 1


def test_tile_time():
    ts = np.array([10.0, 10.1, 10.5, 11.0, 11.0, 11.9, 12.0, 12.3, 13.2])
    t = tile_windows(ts, "time", 1.0)
    assert t["t0"].tolist() == [10.0, 11.0, 12.0]
    assert t["t1"].tolist() == [11.0, 12.0, 13.0]
    # an event ON a boundary opens the next window
    assert t["begin"].tolist() == [0, 3, 6]
    assert t["end"].tolist() == [3, 6, 8]
    assert t["tail_events"] == 1
    for w in range(3):
        sel = ts[t["begin"][w]:t["end"][w]]
        assert np.all((sel >= t["t0"][w]) & (sel < t["t1"][w]))
    with pytest.raises(ValueError):
        tile_windows(ts, "frames", 1.0)


# ---------------------------------------------------------------------------
# emit_window_torch

def test_cell_counts_rounding_and_non_finite():
    v = torch.tensor([2.5, 3.5, 0.5, 1.5, -3.0, S.NAN, S.INF, -S.INF, 1e30,
                      -1e30, 7.0, 1023.4, 1023.6])
    assert cell_counts_torch(v, 1023).tolist() == \
        [2, 4, 0, 2, 0, 0, 1023, 0, 1023, 0, 7, 1023, 1023]
    assert cell_counts_torch(S.HAND, S.HAND_CAP).tolist() == \
        S.HAND_COUNTS.tolist()


def test_emit_hand_map_exact_rows():
    t0, t1 = 5.0, 5.25
    ev = emit_window_torch(S.HAND, t0, t1, capacity=100, cell_cap=S.HAND_CAP)
    assert (ev["total"], ev["emitted"], ev["dropped"]) == (14, 14, 0)
    assert torch.equal(ev["counts"], S.HAND_COUNTS)
    got = list(zip(ev["xs"].tolist(), ev["ys"].tolist(), ev["ps"].tolist(),
                   ev["q"].tolist()))
    assert got == S.HAND_ROWS
    assert (ev["xs"].dtype, ev["ys"].dtype, ev["ts"].dtype, ev["ps"].dtype) \
        == (np.uint16, np.uint16, np.float64, np.int8)
    want_ts = S.timestamps(t0, t1, [r[3] for r in S.HAND_ROWS])
    assert ev["ts"].tobytes() == want_ts.tobytes()
    assert np.all((ev["ts"] >= t0) & (ev["ts"] <= t1))
    assert np.all(np.diff(ev["ts"]) >= 0)
    # n_c == 1 -> q = 0, i.e. t0 + (t1 - t0) / 100
    assert ev["ts"][2] == t0 + (t1 - t0) * (PHASE_Q / (100.0 * PHASE_Q))
    # the last event of every multi-event cell sits on t1
    assert ev["ts"][-4:].tolist() == [t1] * 4


def test_emit_timestamps_epoch_and_degenerate_window():
    t0, t1 = 1.7e9, 1.7e9 + 1e-3
    ev = emit_window_torch(S.HAND, t0, t1, capacity=100, cell_cap=S.HAND_CAP)
    assert ev["ts"].tobytes() == S.timestamps(t0, t1, ev["q"]).tobytes()
    assert np.all((ev["ts"] >= t0) & (ev["ts"] <= t1))
    sel = (ev["xs"] == 1) & (ev["ys"] == 1) & (ev["ps"] == -1)
    assert sel.sum() == 5 and np.all(np.diff(ev["ts"][sel]) > 0)
    ev = emit_window_torch(S.HAND, t0, t0, capacity=100, cell_cap=S.HAND_CAP)
    assert ev["ts"].tolist() == [t0] * 14


def test_emit_round_trip():
    g = torch.Generator().manual_seed(5)
    pred = torch.rand(2, 9, 13, generator=g) * 6 - 1.5
    for mode in ("linear", "random"):
        ev = emit_window_torch(pred, 0.0, 1.0, capacity=10_000, mode=mode,
                               seed=4)
        assert torch.equal(S.splat_rows(ev["xs"], ev["ys"], ev["ps"], (9, 13)),
                           ev["counts"])
        assert torch.equal(ev["counts"], pred.round().clamp(min=0).long())
        assert np.all(np.diff(ev["ts"]) >= 0)


def test_emit_capacity_drops_last_slots():
    full = emit_window_torch(S.HAND, 0.0, 1.0, capacity=100,
                             cell_cap=S.HAND_CAP)
    ev = emit_window_torch(S.HAND, 0.0, 1.0, capacity=full["total"] - 3,
                           cell_cap=S.HAND_CAP)
    assert (ev["total"], ev["emitted"], ev["dropped"]) == (14, 11, 3)
    assert ev["emitted"] + ev["dropped"] == ev["total"]
    # the last three slots: event 4 of cell (ch 1, y 1, x 1), both of (3, 2)
    dropped = [(1, 1, -1, S.Q), (3, 2, -1, 0), (3, 2, -1, S.Q)]
    want = [r for r in S.HAND_ROWS if r not in dropped]
    assert len(want) == 11
    got = list(zip(ev["xs"].tolist(), ev["ys"].tolist(), ev["ps"].tolist(),
                   ev["q"].tolist()))
    assert got == want
    assert torch.equal(ev["counts"], S.HAND_COUNTS)     # counts stay the truth


def test_emit_random_mode():
    kw = dict(capacity=100, cell_cap=S.HAND_CAP, mode="random")
    a = emit_window_torch(S.HAND, 0.0, 1.0, seed=1, window_index=0, **kw)
    b = emit_window_torch(S.HAND, 0.0, 1.0, seed=1, window_index=0, **kw)
    for f in S.COLS:
        assert a[f].tobytes() == b[f].tobytes()
    c = emit_window_torch(S.HAND, 0.0, 1.0, seed=2, window_index=0, **kw)
    d = emit_window_torch(S.HAND, 0.0, 1.0, seed=1, window_index=1, **kw)
    assert sorted(a["q"].tolist()) != sorted(c["q"].tolist())
    assert sorted(a["q"].tolist()) != sorted(d["q"].tolist())
    for ev in (a, c, d):
        assert ev["q"].min() >= 0 and ev["q"].max() <= S.Q
        assert np.all(np.diff(ev["q"]) >= 0)
        assert torch.equal(S.splat_rows(ev["xs"], ev["ys"], ev["ps"], (3, 4)),
                           S.HAND_COUNTS)


def test_hash_phase_matches_uint32_arithmetic():
    """The int64-carried hash against plain Python integers modulo 2^32."""
    M = 0xFFFFFFFF

    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & M
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M
        return h ^ (h >> 16)

    def ref(seed, w, c, j):
        h = fmix((seed + w * 0x9E3779B9) & M)
        h = fmix(h ^ c)
        h = fmix((h + j * 0x9E3779B9) & M)
        return h % (S.Q + 1)

    cases = [(0, 0, 0, 0), (1, 2, 3, 4), (0xFFFFFFFF, 7, 2147352577, 1022),
             (12345, 4000000, 99999, 65534)]
    for seed, w, c, j in cases:
        got = hash_phase_torch(seed, w, torch.tensor([c]), torch.tensor([j]))
        assert got.tolist() == [ref(seed, w, c, j)]


# ---------------------------------------------------------------------------
# append writer

def _columns(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 40000, n).astype(np.uint16),
            rng.integers(0, 40000, n).astype(np.uint16),
            1.7e9 + np.sort(rng.random(n)),
            (rng.integers(0, 2, n) * 2 - 1).astype(np.int8))


@pytest.mark.parametrize("sizes", [[5, 0, 1200, 3], [0], []])
def test_append_writer_equals_add_group(tmp_path, sizes):
    n = sum(sizes)
    cols = _columns(n, seed=1)
    with EventStoreWriter(tmp_path / "a.evs", (4, 6)) as w:
        w.add_group("ori", *cols)
    with EventStoreWriter(tmp_path / "b.evs", (4, 6)) as w:
        g = w.open_group("ori")
        off = 0
        for s in sizes:
            g.append(*(c[off:off + s] for c in cols))
            off += s
        g.close()
    assert json.loads((tmp_path / "a.evs" / "meta.json").read_text()) == \
        json.loads((tmp_path / "b.evs" / "meta.json").read_text())
    assert EventStore(tmp_path / "b.evs").num_events("ori") == n
    for f in S.COLS:
        a = np.load(tmp_path / "a.evs" / f"ori_{f}.npy")
        b = np.load(tmp_path / "b.evs" / f"ori_{f}.npy")
        assert a.dtype == b.dtype and a.shape == b.shape == (n,)
        assert np.array_equal(a, b)
    if n:
        st = EventStore(tmp_path / "b.evs")
        assert np.array_equal(st.events("ori", 2, n - 1),
                              EventStore(tmp_path / "a.evs")
                              .events("ori", 2, n - 1))


# ---------------------------------------------------------------------------
# end to end

@pytest.fixture(scope="module")
def lr_store(tmp_path_factory):
    return S.write_lr_store(tmp_path_factory.mktemp("sr") / "lr.evs")


def _run(model, src, dst, **kw):
    args = dict(group="down2", scale=S.SCALE, seqn=3, window=S.WINDOW,
                device="cpu", keep=True)
    args.update(kw)
    return super_resolve_store(model, src, str(dst), **args)


def test_end_to_end_identity(lr_store, tmp_path):
    summary, kept = _run(S.MidFrame(), lr_store, tmp_path / "hr.evs")
    st = EventStore(tmp_path / "hr.evs")
    assert st.sensor_resolution == list(S.HR)
    assert list(st.groups) == ["ori"] and summary["output_group"] == "ori"
    cols, n = S.read_group(tmp_path / "hr.evs", "ori")
    assert np.all(np.diff(cols["ts"]) >= 0)
    assert kept["windows"] == list(range(1, S.N_WINDOWS - 1))
    ranges = S.window_row_ranges(kept["stats"])
    assert ranges[-1][1] == n == summary["events_out"]
    src_ts = np.load(Path(lr_store) / "down2_ts.npy")
    for (a, b), w, counts in zip(ranges, kept["windows"], kept["counts"]):
        want = S.inp_scaled_cnt(lr_store, "down2", w * S.WINDOW,
                                (w + 1) * S.WINDOW, S.LR, S.HR)
        got = S.splat_rows(cols["xs"][a:b], cols["ys"][a:b], cols["ps"][a:b],
                           S.HR)
        assert torch.equal(got, want.long()), f"window {w}"
        assert torch.equal(counts, want.long())
        assert b - a == S.WINDOW
        t0, t1 = src_ts[w * S.WINDOW], src_ts[(w + 1) * S.WINDOW]
        assert np.all((cols["ts"][a:b] >= t0) & (cols["ts"][a:b] <= t1))
    # window 5 sits on one timestamp
    a, b = ranges[4]
    assert np.all(cols["ts"][a:b] == src_ts[5 * S.WINDOW])

    meta = json.loads((tmp_path / "hr.evs" / "meta.json").read_text())
    sr = meta["sr"]
    assert sr == {k: v for k, v in summary.items() if k != "seconds"}
    assert sr["windows_tiled"] == S.N_WINDOWS
    assert sr["windows_emitted"] + sr["windows_skipped_edges"] == S.N_WINDOWS
    assert sr["windows_skipped_edges"] == 2
    assert sr["tail_events_dropped"] == S.TAIL
    assert sr["events_in"] == S.N_WINDOWS * S.WINDOW
    assert sr["events_out"] == (S.N_WINDOWS - 2) * S.WINDOW
    assert sr["events_dropped"] == 0 and sr["overflowed_windows"] == []
    assert sr["covered"] == [src_ts[S.WINDOW], src_ts[11 * S.WINDOW]]
    assert (sr["source"], sr["group"], sr["scale"], sr["seqn"], sr["window"],
            sr["mode"], sr["redistribute"], sr["seed"], sr["cell_cap"]) == \
        (lr_store, "down2", 2, 3, S.WINDOW, "events", "linear", 0, 1023)
    assert sr["capacity"] == max(1024, 4 * 4 * S.WINDOW)


def test_overflow_is_reported(lr_store, tmp_path, caplog):
    with caplog.at_level(logging.WARNING):
        summary, kept = _run(S.MidFrame(), lr_store, tmp_path / "hr.evs",
                             capacity=S.WINDOW - 5)
    n_emit = S.N_WINDOWS - 2
    assert summary["events_dropped"] == 5 * n_emit
    assert summary["events_out"] == (S.WINDOW - 5) * n_emit
    assert summary["windows_overflowed"] == n_emit
    assert summary["overflowed_windows"] == kept["windows"]
    assert any("overflowed" in r.getMessage() for r in caplog.records)
    assert EventStore(tmp_path / "hr.evs").num_events("ori") == \
        summary["events_out"]


@pytest.fixture(scope="module")
def tiny_model():
    torch.manual_seed(0)
    return build_model("ESRNet", inch=2, basech=8, num_frame=3).eval()


def _loop_oracle(model, src, seqn=3, gain=1.0):
    """The per-window loop written out: batch_splat_torch, model(inp) with
    the state carried by the model itself, emit_window_torch."""
    model = copy.deepcopy(model).eval()
    model.reset_states()
    st = EventStore(src)
    n = st.num_events("down2")
    packed = torch.from_numpy(pack_events(
        np.load(st.path / "down2_xs.npy"), np.load(st.path / "down2_ys.npy"),
        np.load(st.path / "down2_ps.npy")).copy())
    ts = np.load(st.path / "down2_ts.npy")
    W, mid = S.WINDOW, (seqn - 1) // 2
    preds, cols = [], {f: [] for f in S.COLS}
    with torch.no_grad():
        for k in range(n // W - seqn + 1):
            jobs = torch.tensor([[(k + l) * W, (k + l + 1) * W, 0, 0]
                                 for l in range(seqn)], dtype=torch.int32)
            inp = torch.zeros(seqn, 2, *S.HR)
            batch_splat_torch(packed, jobs, inp, *S.LR)
            pred = model(inp[None])[0]
            w = k + mid
            ev = emit_window_torch(pred, ts[w * W], ts[(w + 1) * W],
                                   capacity=max(1024, 16 * W),
                                   window_index=w)
            preds.append(pred)
            for f in S.COLS:
                cols[f].append(ev[f])
    return torch.stack(preds), {f: np.concatenate(v) for f, v in cols.items()}


def test_end_to_end_tiny_esrnet_against_loop(lr_store, tmp_path, tiny_model):
    model = S.Lifted(tiny_model)
    want_pred, want_cols = _loop_oracle(model, lr_store)
    summary, kept = _run(copy.deepcopy(model), lr_store, tmp_path / "hr.evs")
    assert torch.equal(kept["pred"], want_pred)
    cols, n = S.read_group(tmp_path / "hr.evs", "ori")
    assert n == summary["events_out"] > 0
    for f in S.COLS:
        assert cols[f].tobytes() == want_cols[f].tobytes(), f
    # the recurrence matters: the first window alone predicts differently
    assert not torch.equal(kept["pred"][3], kept["pred"][0])
    assert np.all(np.diff(cols["ts"]) >= 0)


def test_chunking_gives_identical_files(lr_store, tmp_path, tiny_model):
    model = S.Lifted(tiny_model)
    for mode in ("linear", "random"):
        a, _ = _run(copy.deepcopy(model), lr_store, tmp_path / f"a_{mode}.evs",
                    chunk_windows=2, redistribute=mode, seed=9)
        b, _ = _run(copy.deepcopy(model), lr_store, tmp_path / f"b_{mode}.evs",
                    chunk_windows=256, redistribute=mode, seed=9)
        S.assert_same_files(tmp_path / f"a_{mode}.evs",
                            tmp_path / f"b_{mode}.evs", "ori")
        assert a["events_out"] == b["events_out"] > 0


def test_time_mode_and_sr_group_name(tmp_path):
    src = S.write_lr_store(tmp_path / "lr.evs", t_start=50.0,
                           duplicates=False)
    summary = _run(S.MidFrame(), src, tmp_path / "hr.evs", mode="time",
                   window=0.005, scale=4, keep=False)
    # down2 at 4x has no named level
    assert summary["output_group"] == "sr"
    st = EventStore(tmp_path / "hr.evs")
    assert st.sensor_resolution == [48, 80]
    ts = np.load(tmp_path / "hr.evs" / "sr_ts.npy")
    assert ts.size == summary["events_out"] > 0
    assert np.all(np.diff(ts) >= 0)
    assert summary["covered"][0] <= ts[0] and ts[-1] <= summary["covered"][1]
    assert summary["window"] == 0.005 and summary["mode"] == "time"


# ---------------------------------------------------------------------------
# refusals

def test_refusals(lr_store, tmp_path):
    dst = tmp_path / "hr.evs"
    with pytest.raises(ValueError, match="scale"):
        _run(S.MidFrame(), lr_store, dst, scale=1.5)
    with pytest.raises(ValueError, match="fewer than"):
        _run(S.MidFrame(), lr_store, dst, window=200)
    with pytest.raises(ValueError, match="fewer than"):
        _run(S.MidFrame(), lr_store, dst, max_windows=2)
    with pytest.raises(ValueError, match="no group"):
        _run(S.MidFrame(), lr_store, dst, group="down4")
    with pytest.raises(ValueError, match="32767"):
        _run(S.MidFrame(), lr_store, dst, scale=2000)


def test_refuses_tuple_state(lr_store, tmp_path):
    class Holder:
        state = None

    class TupleState(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.time_propagate = Holder()

        def reset_states(self):
            self.time_propagate.state = None

        def forward(self, x):
            self.time_propagate.state = (x[:, 0], x[:, 1])
            return x[:, 1]

    with pytest.raises(NotImplementedError, match="tuple"):
        _run(TupleState(), lr_store, tmp_path / "hr.evs")


# ---------------------------------------------------------------------------
# CLI

def test_superresolve_cli(lr_store, tmp_path, tiny_model):
    from esr_amd.engine import save_checkpoint
    config = {"model": {"name": "ESRNet",
                        "args": {"inch": 2, "basech": 8, "num_frame": 3}},
              "lr_scheduler": {"name": "none"}, "optimizer": {"name": "none"},
              "SEQN": 3}
    ckpt = tmp_path / "ckpt.pth"
    save_checkpoint(ckpt, config, tiny_model)
    out = subprocess.run(
        [sys.executable, "superresolve.py", "--model_path", str(ckpt),
         "--input", lr_store, "--group", "down2", "--output",
         str(tmp_path / "hr.evs"), "--scale", "2", "--seqn", "3",
         "--window", str(S.WINDOW), "--device", "cpu", "--redistribute",
         "random", "--seed", "3"],
        capture_output=True, text=True, timeout=300, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-3000:]
    printed = yaml.safe_load(out.stdout)
    st = EventStore(tmp_path / "hr.evs")
    assert st.sensor_resolution == list(S.HR)
    assert st.num_events("ori") == printed["events_out"]
    assert st.meta["sr"]["checkpoint"] == str(ckpt)
    assert st.meta["sr"]["redistribute"] == "random"
    # the same run through the function gives the same file
    want = _run(copy.deepcopy(tiny_model), lr_store, tmp_path / "fn.evs",
                redistribute="random", seed=3, keep=False)
    assert want["events_out"] == printed["events_out"]
    if want["events_out"]:
        S.assert_same_files(tmp_path / "hr.evs", tmp_path / "fn.evs", "ori")
