"""The device event simulator (ops/native/src/esim.hip through
data/simulate_device.py) against its numpy oracle `simulate_events_log`:
every row equal, in the oracle's order."""

import numpy as np
import pytest
import torch

from esr_amd.data import EventSRDataset
from esr_amd.data.simulate import simulate_events_log
from esr_amd.data.simulate_device import (DeviceEventSimulator,
                                          frames_to_event_store_device,
                                          simulate_events_device)
from esr_amd.data.store import EventStore

import simulate_helpers as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


def _run(sim, logf, ts):
    chunks = list(sim.feed(logf, ts))
    for c in chunks:
        assert [a.dtype for a in c] == [np.uint16, np.uint16, np.float64,
                                        np.int8]
    if not chunks:
        return np.zeros((4, 0)), 0
    return np.stack([np.concatenate([c[i] for c in chunks]).astype(np.float64)
                     for i in range(4)]), len(chunks)


@pytest.fixture(scope="module")
def oracle():
    logf, ts = S.case_log()
    out = {r: simulate_events_log(logf, ts, S.CP, S.CN, r)
           for r in (0.0, 5e-4)}
    S.assert_case_conditions(out[0.0],
                             out[0.0].shape[1] - out[5e-4].shape[1])
    return out


@pytest.mark.parametrize("refractory", (0.0, 5e-4))
def test_case_equals_oracle(oracle, refractory):
    _ext()
    logf, ts = S.case_log()
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, refractory, DEV)
    assert sim.native
    got, _ = _run(sim, logf, ts)
    S.assert_events_equal(got, oracle[refractory])
    S.assert_events_equal(
        simulate_events_device(logf, ts, S.CP, S.CN, refractory, device=DEV),
        oracle[refractory])


@pytest.mark.parametrize("refractory", (0.0, 5e-4))
def test_chunking_gives_one_result(oracle, refractory):
    _ext()
    logf, ts = S.case_log()
    want = oracle[refractory]
    for per_chunk, n_chunks in ((1, 6), (2, 3), (None, 1)):
        sim = DeviceEventSimulator(9, 13, S.CP, S.CN, refractory, DEV,
                                   intervals_per_chunk=per_chunk)
        got, chunks = _run(sim, logf, ts)
        S.assert_events_equal(got, want)
        assert 1 <= chunks <= n_chunks and sim.halvings == 0
        assert (chunks == 1) == (per_chunk is None)
    # slab by slab, the state carried on the device
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, refractory, DEV)
    parts = [_run(sim, logf[a:b + 1], ts[a:b + 1])[0]
             for a, b in ((0, 2), (2, 3), (3, 6))]
    S.assert_events_equal(np.concatenate(parts, axis=1), want)
    # a capacity that holds the busiest interval but not the recording
    _, k = S.brute_force(logf, ts, S.CP, S.CN, refractory)
    busiest = int(np.bincount(k).max())
    assert busiest < want.shape[1]
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, refractory, DEV,
                               max_chunk_events=busiest)
    got, chunks = _run(sim, logf, ts)
    assert sim.halvings > 0 and chunks > 1
    S.assert_events_equal(got, want)


def test_interval_larger_than_capacity(oracle):
    _ext()
    logf, ts = S.case_log()
    _, k = S.brute_force(logf, ts, S.CP, S.CN)
    per_interval = np.bincount(k, minlength=7)
    worst = int(per_interval.argmax())             # the step's interval
    cap = int(per_interval.max()) - 1
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, 0.0, DEV,
                               max_chunk_events=cap)
    with pytest.raises(ValueError, match="max_chunk_events"):
        list(sim.feed(logf, ts))
    # usable afterwards: a recording that fits, after a reset
    assert per_interval[:worst].sum() > 0 and per_interval[:worst].max() <= cap
    sim.reset()
    got, _ = _run(sim, logf[:worst], ts[:worst])
    S.assert_events_equal(
        got, simulate_events_log(logf[:worst], ts[:worst], S.CP, S.CN))
    # the failing chunk left the state alone: the slab before it, the
    # failing interval (error), then another frame pair from the same state
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, 0.0, DEV,
                               max_chunk_events=cap)
    head, _ = _run(sim, logf[:worst], ts[:worst])
    with pytest.raises(ValueError, match="max_chunk_events"):
        list(sim.feed(logf[worst - 1:worst + 1], ts[worst - 1:worst + 1]))
    assert worst >= 2
    detour = np.stack([*logf[:worst], logf[worst - 2]])
    tail, _ = _run(sim, detour[-2:], ts[worst - 1:worst + 1])
    S.assert_events_equal(
        np.concatenate([head, tail], axis=1),
        simulate_events_log(detour, ts[:worst + 1], S.CP, S.CN))


def test_bad_input_raises_from_the_stats(oracle):
    _ext()
    logf, ts = S.case_log()
    bad = logf.copy()
    bad[2, 4, 4] = np.nan
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, 0.0, DEV)
    with pytest.raises(ValueError, match="non-finite"):
        list(sim.feed(bad, ts))
    bad[2, 4, 4] = np.inf
    sim.reset()
    with pytest.raises(ValueError, match="non-finite"):
        list(sim.feed(bad, ts))
    # the step crosses 1e-5 more than 65535 times
    assert (logf[3] - logf[2]).max() / 1e-5 > 65535
    for refractory in (0.0, 5e-4):
        sim = DeviceEventSimulator(9, 13, 1e-5, S.CN, refractory, DEV)
        with pytest.raises(ValueError, match="65535"):
            list(sim.feed(logf[2:4], ts[2:4]))
    torch.cuda.synchronize()
    # and the device still works
    sim = DeviceEventSimulator(9, 13, S.CP, S.CN, 0.0, DEV)
    S.assert_events_equal(_run(sim, logf, ts)[0], oracle[0.0])


def test_grid_wrap():
    """More pixels than one grid of the walk covers."""
    cap = _ext().grid_cap()
    H = 724
    W = cap // H + 36
    assert cap < H * W < 1.1 * cap
    logf, ts = S.smooth_pan_log(H, W)
    want = simulate_events_log(logf, ts, S.CP, S.CN, 1e-4)
    assert (want[3] > 0).any() and (want[3] < 0).any()
    tail = want[1] * W + want[0] >= cap
    assert tail.any() and not tail.all()
    got = simulate_events_device(logf, ts, S.CP, S.CN, 1e-4, device=DEV)
    S.assert_events_equal(got, want)


def test_pipeline(tmp_path):
    _ext()
    frames = S.panned(6, 48, 64, seed=3, sigma=2.0)
    ts = np.arange(6) / 240.0
    logs = {}

    def sink(level, k0, logf):
        assert logf.is_cuda and logf.dtype == torch.float64
        logs.setdefault(level, {}).update(
            {k0 + j: logf[j].cpu().numpy() for j in range(logf.shape[0])})

    kw = dict(levels=(1, 2, 4), seed=1, refractory=1e-4, device=DEV)
    a = frames_to_event_store_device(tmp_path / "a.evs", frames, ts,
                                     frame_chunk=2, log_sink=sink, **kw)
    b = frames_to_event_store_device(tmp_path / "b.evs", frames, ts,
                                     frame_chunk=6, **kw)
    S.stores_identical(a, b)
    st = EventStore(a)
    cp, cn = st.meta["contrast_thresholds"]
    for level, name in ((1, "ori"), (2, "down2"), (4, "down4")):
        logf = np.stack([logs[level][k] for k in range(6)])
        assert logf.shape[1:] == (48 // level, 64 // level)
        want = simulate_events_log(logf, ts, cp, cn, 1e-4)
        assert want.shape[1] > 0
        S.assert_events_equal(S.group_events(a, name), want)
        assert (np.diff(st.ts(name)) >= 0).all()
    assert st.num_images == 6
    ds = EventSRDataset(str(a), S.dataset_config())
    assert len(ds) > 0 and ds[0] is not None
