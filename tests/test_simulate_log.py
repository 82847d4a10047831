"""The simulator's oracle `simulate_events_log`, its refractory rule and
order, the slab-by-slab CPU form of `DeviceEventSimulator`, the image
appender and tools/frames_to_evs.py (all on the CPU)."""

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from esr_amd.data import EventSRDataset
from esr_amd.data.simulate import simulate_events, simulate_events_log
from esr_amd.data.simulate_device import (DeviceEventSimulator,
                                          frames_to_event_store_device,
                                          simulate_events_device)
from esr_amd.data.store import EventStore, EventStoreWriter

import simulate_helpers as S

REPO = Path(__file__).resolve().parent.parent
PERIODS = (1e-4, 5e-4, 2e-3)


def _moving_bar(T=8, H=32, W=32):
    # tests/test_simulate.py's case
    frames = np.zeros((T, H, W))
    for t in range(T):
        x = 4 + t * 3
        frames[t, :, x:x + 4] = 1.0
    return frames, np.linspace(0, 0.1, T)


@pytest.fixture(scope="module")
def case_events():
    logf, ts = S.case_log()
    return simulate_events_log(logf, ts, S.CP, S.CN)


def test_log_form_equals_simulate_events(case_events):
    frames, ts = S.case()
    S.assert_events_equal(case_events, simulate_events(frames, ts, S.CP, S.CN))
    S.assert_case_conditions(case_events)
    frames, ts = _moving_bar()
    S.assert_events_equal(
        simulate_events_log(np.log(frames + 1e-3), ts, 0.3, 0.3),
        simulate_events(frames, ts, cp=0.3, cn=0.3))


@pytest.mark.parametrize("refractory", (0.0, 5e-4))
def test_stated_order_and_model(refractory):
    """Against the model written out pixel by pixel and sorted explicitly by
    (t, k, polarity with + first, i, y, x)."""
    logf, ts = S.case_log()
    want, _ = S.brute_force(logf, ts, S.CP, S.CN, refractory)
    S.assert_events_equal(
        simulate_events_log(logf, ts, S.CP, S.CN, refractory), want)


def test_refractory_rule(case_events):
    logf, ts = S.case_log()
    S.assert_events_equal(simulate_events_log(logf, ts, S.CP, S.CN, 0.0),
                          case_events)
    total = last = case_events.shape[1]
    for period in PERIODS:
        ev = simulate_events_log(logf, ts, S.CP, S.CN, period)
        assert ev.shape[1] <= last               # does not grow with it
        last = ev.shape[1]
        S.assert_case_conditions(case_events, suppressed=total - last)
        pix = ev[1].astype(np.int64) * logf.shape[2] + ev[0].astype(np.int64)
        for p in np.unique(pix):
            assert (np.diff(ev[2][pix == p]) >= period).all()


def test_cpu_simulator_slab_by_slab(case_events):
    logf, ts = S.case_log()
    for refractory in (0.0, 5e-4):
        want = simulate_events_log(logf, ts, S.CP, S.CN, refractory)
        sim = DeviceEventSimulator(9, 13, S.CP, S.CN, refractory, "cpu")
        assert not sim.native
        chunks = []
        for k in range(len(ts) - 1):             # slabs of 2 frames
            chunks += list(sim.feed(logf[k:k + 2], ts[k:k + 2]))
        got = np.stack([np.concatenate([c[i] for c in chunks])
                        .astype(np.float64) for i in range(4)])
        S.assert_events_equal(got, want)
        S.assert_events_equal(
            simulate_events_device(logf, ts, S.CP, S.CN, refractory,
                                   device="cpu"), want)
    # a slab that does not continue the last one
    with pytest.raises(ValueError):
        sim.feed(logf[:2], ts[:2])


def test_bad_timestamps_raise():
    logf, ts = S.case_log()
    for bad in (ts[::-1], np.where(np.arange(7) == 3, ts[2], ts),
                np.where(np.arange(7) == 3, np.nan, ts), ts[:-1]):
        with pytest.raises(ValueError):
            simulate_events_log(logf, bad, S.CP, S.CN)
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, 0.0, "cpu")
    with pytest.raises(ValueError):
        sim.feed(logf, ts[::-1])
    bad = logf.copy()
    bad[2, 4, 4] = np.nan
    with pytest.raises(ValueError):
        list(sim.feed(bad, ts))


def test_open_images_reads_back_as_add_images(tmp_path):
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (5, 6, 7), dtype=np.uint8)
    ts = np.linspace(0, 1, 5)
    with EventStoreWriter(tmp_path / "a.evs", (6, 7)) as w:
        w.add_images(images, ts)
    with EventStoreWriter(tmp_path / "b.evs", (6, 7)) as w:
        with w.open_images((6, 7)) as app:
            app.append(images[:2], ts[:2])
            app.append(images[2:], ts[2:])
            with pytest.raises(ValueError):
                app.append(images[:, :5], ts)
    a, b = EventStore(tmp_path / "a.evs"), EventStore(tmp_path / "b.evs")
    assert a.meta == b.meta and b.num_images == 5
    got = np.load(tmp_path / "b.evs" / "images.npy")
    assert got.dtype == np.uint8 and np.array_equal(got, images)
    assert np.array_equal(b.image_ts(), a.image_ts())
    assert np.array_equal(b.image(3), a.image(3))


def test_cpu_pipeline_against_oracle_on_its_log_frames(tmp_path):
    frames = S.panned(6, 48, 64, seed=3, sigma=2.0)
    ts = np.arange(6) / 240.0
    logs = {}

    def sink(level, k0, logf):
        logs.setdefault(level, {}).update(
            {k0 + j: logf[j].numpy().copy() for j in range(logf.shape[0])})

    a = frames_to_event_store_device(
        tmp_path / "a.evs", frames, ts, levels=(1, 2, 4), seed=1,
        refractory=1e-4, device="cpu", frame_chunk=2, log_sink=sink)
    b = frames_to_event_store_device(
        tmp_path / "b.evs", frames, ts, levels=(1, 2, 4), seed=1,
        refractory=1e-4, device="cpu", frame_chunk=6)
    S.stores_identical(a, b)
    st = EventStore(a)
    cp, cn = st.meta["contrast_thresholds"]
    for level, name in ((1, "ori"), (2, "down2"), (4, "down4")):
        logf = np.stack([logs[level][k] for k in range(6)])
        want = simulate_events_log(logf, ts, cp, cn, 1e-4)
        assert want.shape[1] > 0
        S.assert_events_equal(S.group_events(a, name), want)
    assert st.num_images == 6


def test_frames_to_evs_tool_on_a_png_folder(tmp_path):
    from PIL import Image
    frames = S.panned(5, 32, 48, seed=5, sigma=2.0)
    root = tmp_path / "clips" / "clip0"
    root.mkdir(parents=True)
    for i, fr in enumerate(frames):
        Image.fromarray(np.rint(fr * 255).astype(np.uint8)).save(
            root / f"{i:04d}.png")
    out = tmp_path / "clip0.evs"
    cmd = [sys.executable, str(REPO / "tools" / "frames_to_evs.py"),
           "--out", str(out), "--fps", "240", "--levels", "1", "2", "4",
           "--cp", "0.1", "--cn", "0.1", "--device", "cpu",
           "--frame_chunk", "3", "--frames", str(root)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "cp = 0.1" in r.stdout
    st = EventStore(out)
    assert set(st.groups) == {"ori", "down2", "down4"}
    assert st.num_events("ori") > st.num_events("down4") > 0
    assert st.meta["contrast_thresholds"] == [0.1, 0.1]
    assert st.meta["refractory"] == 1e-4
    assert (np.diff(st.ts("ori")) >= 0).all()
    assert np.array_equal(st.image(2), np.rint(frames[2] * 255))
    ds = EventSRDataset(str(out), S.dataset_config())
    assert len(ds) > 0
    item = ds[0]
    assert item is not None

    # --data_root: every sub-directory, its own thresholds, the datalists
    (tmp_path / "clips" / "clip1").mkdir()
    for i, fr in enumerate(frames[::-1]):
        Image.fromarray(np.rint(fr * 255).astype(np.uint8)).save(
            tmp_path / "clips" / "clip1" / f"{i:04d}.png")
    root_out = tmp_path / "stores"
    cmd = [sys.executable, str(REPO / "tools" / "frames_to_evs.py"),
           "--data_root", str(tmp_path / "clips"), "--out", str(root_out),
           "--fps", "240", "--levels", "1", "2", "--seed", "3",
           "--device", "cpu", "--no_images", "--split", "0.5"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a, b = EventStore(root_out / "clip0.evs"), EventStore(root_out / "clip1.evs")
    assert a.num_images == 0 and a.num_events("ori") > 0
    assert a.meta["contrast_thresholds"] != b.meta["contrast_thresholds"]
    assert (root_out / "train_datalist.txt").read_text().split() == \
        [str(root_out / "clip0.evs")]
    assert (root_out / "valid_datalist.txt").read_text().split() == \
        [str(root_out / "clip1.evs")]
