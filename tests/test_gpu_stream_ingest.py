"""stream_ingest.hip kernels against the torch ingest (run on CPU copies)
and an independent per-event loop oracle.  Counts are small integers in
fp32, so every comparison is torch.equal."""

import pytest
import torch

from esr_amd.engine.multistream import (splat_ragged_torch,
                                        window_advance_torch)

import multistream_helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


def _kernels(buf0, ev, offsets, ctrl, scale):
    buf = buf0.to(DEV)
    ev_d, off_d, ctrl_d = ev.to(DEV), offsets.to(DEV), ctrl.to(DEV)
    ext = _ext()
    ext.stream_window_advance(buf, ctrl_d)
    ext.stream_splat_ragged(ev_d, off_d, ctrl_d, buf, scale)
    torch.cuda.synchronize()
    return buf.cpu()


def _torch(buf0, ev, offsets, ctrl, scale):
    buf = buf0.clone()
    window_advance_torch(buf, ctrl)
    splat_ragged_torch(ev, offsets, ctrl, buf, scale)
    return buf


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("case", sorted(H.INGEST_CTRL))
def test_main_case(case, scale):
    """S=3, seqn=3, LR 16x24, cap 512: segments [40, empty, 472] with
    offsets[S] == cap; out-of-range, fractional, padding and piled-up
    events; every has_window / reset combination."""
    hr = (H.LR[0] * scale, H.LR[1] * scale)
    ev, offsets = H.ingest_events(H.LR, [40, 0, 472], cap=512)
    assert int(offsets[-1]) == 512 == ev.size(0)
    has, reset = H.INGEST_CTRL[case]
    ctrl = H.ingest_ctrl(has, reset)
    buf0 = H.ingest_buffer(3, 3, hr)
    got = _kernels(buf0, ev, offsets, ctrl, scale)
    assert torch.equal(got, _torch(buf0, ev, offsets, ctrl, scale))
    assert torch.equal(got, H.ingest_loop_oracle(buf0, ev, offsets, ctrl,
                                                 scale))
    H.check_ingest_structure(got, buf0, has, reset, scale)


@pytest.mark.parametrize("seqn", [3, 1])
def test_scalar_path(seqn):
    """LR 5x7 at scale 1: 2*kH*kW = 70 is no multiple of 4, so the shift
    takes the scalar kernel."""
    lr = (5, 7)
    ev, offsets = H.ingest_events(lr, [30, 0, 60], cap=100, seed=3)
    ctrl = H.ingest_ctrl([1, 0, 1], [0, 0, 1])
    buf0 = H.ingest_buffer(seqn, 3, lr, seed=1)
    got = _kernels(buf0, ev, offsets, ctrl, 1)
    assert torch.equal(got, _torch(buf0, ev, offsets, ctrl, 1))
    assert torch.equal(got, H.ingest_loop_oracle(buf0, ev, offsets, ctrl, 1))


def test_garbage_rows_beyond_the_last_offset():
    """Rows past offsets[S] are never read as events, whatever they hold."""
    scale = 2
    hr = (H.LR[0] * scale, H.LR[1] * scale)
    ev, offsets = H.ingest_events(H.LR, [100, 0, 200], cap=512, seed=5)
    ctrl = H.ingest_ctrl([1, 1, 1], [0, 0, 0])
    buf0 = H.ingest_buffer(3, 3, hr, seed=2)
    clean = _kernels(buf0, ev, offsets, ctrl, scale)
    dirty = ev.clone()
    g = torch.Generator().manual_seed(9)
    dirty[300:, :2] = torch.rand(212, 2, generator=g) * 16
    dirty[300:, 3] = 1.0
    dirty[500:, 0] = float("nan")
    dirty[505:, 1] = float("inf")
    dirty[508:, 0] = 3e9
    got = _kernels(buf0, dirty, offsets, ctrl, scale)
    assert torch.equal(got, clean)
    assert torch.equal(got, _torch(buf0, ev, offsets, ctrl, scale))


def test_wild_coordinates_inside_a_segment():
    """NaN, inf and coordinates beyond the int range are dropped like any
    other out-of-range event."""
    scale = 4
    hr = (H.LR[0] * scale, H.LR[1] * scale)
    ev, offsets = H.ingest_events(H.LR, [20, 20, 24], cap=64, seed=6)
    ev[20:26, 0] = torch.tensor([float("nan"), float("inf"), -float("inf"),
                                 3e9, -3e9, 2.0 ** 30])
    ev[20:26, 3] = 1.0
    ctrl = H.ingest_ctrl([1, 1, 1], [0, 0, 0])
    buf0 = H.ingest_buffer(3, 3, hr, seed=3)
    got = _kernels(buf0, ev, offsets, ctrl, scale)
    assert torch.equal(got, _torch(buf0, ev, offsets, ctrl, scale))
    assert torch.equal(got, H.ingest_loop_oracle(buf0, ev, offsets, ctrl,
                                                 scale))


def test_grid_stride():
    """5 streams at 512x512: 655360 float4 columns, more than the grid cap
    of 2048 blocks x 256 threads, so threads take a second column."""
    lr, scale, S, seqn = (256, 256), 2, 5, 2
    ev, offsets = H.ingest_events(lr, [100, 0, 50, 300, 62], cap=512, seed=7)
    ctrl = H.ingest_ctrl([1, 1, 0, 1, 1], [0, 0, 0, 1, 0])
    buf0 = H.ingest_buffer(seqn, S, (512, 512), seed=4)
    got = _kernels(buf0, ev, offsets, ctrl, scale)
    assert torch.equal(got, _torch(buf0, ev, offsets, ctrl, scale))
