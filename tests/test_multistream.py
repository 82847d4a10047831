"""MultiStreamESR semantics on CPU (torch ingest, no graph): every stream
behaves as if it had a StreamingESR of its own."""

import copy

import pytest
import torch

from esr_amd.engine import MultiStreamESR
from esr_amd.models import build_model
from esr_amd.ops.events import events_to_channels

import multistream_helpers as H
from multistream_helpers import A, B, C

# Batch-3 and batch-1 CPU convolutions need not be bit-equal.  Measured on
# the parent commit for this model (ESRNet basech 8, 3 frames, 32x48 count
# maps, 12 seeds x 5 recurrent steps, 1/2/4/8/16 threads):
#   max |model(x3)[i] - model(x3[i:i+1])| = 4.47e-8
# (outputs are ~0.1, i.e. 3 ulp).  atol = 4 x that.
BATCH_DIFF_MEASURED = 4.47e-8
ATOL_VS_SINGLE = 4 * BATCH_DIFF_MEASURED
# same batch on both sides: the project's bound for streaming vs manual
# sliding windows (test_streaming_state_continuity_cpu)
ATOL_SAME_BATCH = 1e-5


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    return build_model("ESRNet", inch=2, basech=8, num_frame=3, **kw)


def _server(model, **kw):
    args = dict(scale=H.SCALE, seqn=H.SEQN, max_streams=H.MAX_STREAMS,
                max_events=4096, device="cpu", use_graphs=False,
                amp_dtype=None)
    args.update(kw)
    return MultiStreamESR(copy.deepcopy(model), H.LR, **args)


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def multi_outs(model):
    return H.run_multistream(_server(model))


def _compare(got, want, atol):
    assert len(got) == len(want) == len(H.PUSHES)
    for tick, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) == H.WARM[tick], (tick, set(g), set(w))
        for sid in w:
            assert g[sid].shape == (2, *H.HR)
            err = (g[sid] - w[sid]).abs().max().item()
            assert err <= atol, (tick, sid, err)


def test_schedule_keys_are_the_warm_streams(multi_outs):
    assert [set(o) for o in multi_outs] == H.WARM


def test_schedule_matches_single_stream_servers(model, multi_outs):
    _compare(multi_outs, H.run_single_servers(model), ATOL_VS_SINGLE)


def test_schedule_matches_batched_oracle(model, multi_outs):
    _compare(multi_outs, H.run_batched_oracle(model), ATOL_SAME_BATCH)


def test_outputs_are_clones(model):
    srv = _server(model)
    sid = srv.open()
    for t in range(3):
        out = srv.step({sid: H.window(A, t)})
    keep = out[sid].clone()
    srv.step({sid: H.window(A, 3)})
    assert torch.equal(out[sid], keep)


def test_idle_stream_is_untouched(model):
    srv = _server(model)
    a, b = srv.open(), srv.open()
    S = srv.max_streams
    for t in range(4):
        srv.step({a: H.window(A, t), b: H.window(B, t)})
    buf = srv._buf[:, b].clone()
    state = srv._state[[b, S + b]].clone()
    assert buf.abs().sum() > 0 and state.abs().sum() > 0
    out = srv.step({a: H.window(A, 4)})
    assert set(out) == {a}
    assert torch.equal(srv._buf[:, b], buf)
    assert torch.equal(srv._state[[b, S + b]], state)
    # a warming stream does not advance its state either
    c = srv.open()
    srv.step({a: H.window(A, 5), c: H.window(C, 5)})
    assert not srv._state[[c, S + c]].any()
    assert srv._buf[-1, c].sum() > 0


def test_overflow_raises_before_anything_is_written(model):
    srv = _server(model, max_events=300)
    a, b = srv.open(), srv.open()
    for t in range(3):
        srv.step({a: H.window(A, t), b: H.window(B, t)})
    buf, state = srv._buf.clone(), srv._state.clone()
    count, tick = list(srv._count), srv._tick
    big = H.window(A, 9)
    assert big.size(1) + H.window(B, 3).size(1) > 300
    with pytest.raises(ValueError):
        srv.step({a: big, b: H.window(B, 3)})
    assert torch.equal(srv._buf, buf) and torch.equal(srv._state, state)
    assert srv._count == count and srv._tick == tick
    # the server goes on as if the tick had not happened
    assert set(srv.step({a: H.window(A, 3)})) == {a}


def test_failed_copy_leaves_bookkeeping_alone(model):
    """A window that cannot be copied raises before counters, pending
    resets or the device-side window and state have moved."""
    srv = _server(model)
    a, b = srv.open(), srv.open()
    for t in range(2):
        srv.step({a: H.window(A, t), b: H.window(B, t)})
    srv.reset(b)
    buf, state = srv._buf.clone(), srv._state.clone()
    count, pending, tick = list(srv._count), list(srv._pending_reset), \
        srv._tick
    bad = H.window(B, 2).to_sparse()         # [4, n], but no dense copy
    with pytest.raises(RuntimeError):
        srv.step({a: H.window(A, 2), b: bad})
    assert torch.equal(srv._buf, buf) and torch.equal(srv._state, state)
    assert (srv._count, srv._pending_reset, srv._tick) == \
        (count, pending, tick)
    # the tick can be repeated: a becomes warm, b restarts from its reset
    assert set(srv.step({a: H.window(A, 2), b: H.window(B, 2)})) == {a}
    assert srv._count[b] == 1


def test_slots(model):
    srv = _server(model)
    sids = [srv.open() for _ in range(H.MAX_STREAMS)]
    assert sorted(sids) == list(range(H.MAX_STREAMS))
    with pytest.raises(RuntimeError):
        srv.open()
    srv.close(sids[1])
    with pytest.raises(KeyError):
        srv.step({sids[1]: H.window(A, 0)})
    with pytest.raises(KeyError):
        srv.close(sids[1])
    assert srv.open() == sids[1]


def test_convlstm_state_is_refused():
    m = _model(recurrent_block_type="convlstm")
    with pytest.raises(NotImplementedError):
        _server(m)


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("case", sorted(H.INGEST_CTRL))
def test_torch_ingest_matches_loop_oracle(case, scale):
    """The torch ingest (CPU path, and the oracle of the HIP kernels)
    against per-event python loops over the documented rule."""
    from esr_amd.engine.multistream import (splat_ragged_torch,
                                            window_advance_torch)
    hr = (H.LR[0] * scale, H.LR[1] * scale)
    ev, offsets = H.ingest_events(H.LR, [40, 0, 472], cap=512)
    ctrl = H.ingest_ctrl(*H.INGEST_CTRL[case])
    buf0 = H.ingest_buffer(3, 3, hr)
    want = H.ingest_loop_oracle(buf0, ev, offsets, ctrl, scale)
    got = buf0.clone()
    window_advance_torch(got, ctrl)
    splat_ragged_torch(ev, offsets, ctrl, got, scale)
    assert torch.equal(got, want)
    assert not torch.equal(got, buf0)
    H.check_ingest_structure(got, buf0, *H.INGEST_CTRL[case], scale)


def test_step_events_roundtrip(model):
    """A warm stream's emitted HR event stream splats back to the rounded,
    clamped count map."""
    srv_ev, srv_cnt = _server(model), _server(model)
    for srv in (srv_ev, srv_cnt):
        assert (srv.open(), srv.open()) == (0, 1)
    for t in range(4):
        wins = {0: H.window(A, t), 1: H.window(B, t)} if t != 1 \
            else {0: H.window(A, t)}
        evs = srv_ev.step_events(wins)
        cnts = srv_cnt.step(wins)
        assert set(evs) == set(cnts)
    assert set(evs) == {0, 1}       # stream 1 became warm at the last tick
    for sid, ev in evs.items():
        assert ev.shape[1] == 4
        assert (ev[1:, 2] >= ev[:-1, 2]).all()
        want = cnts[sid].float().round().clamp(min=0)
        back = events_to_channels(ev[:, 0], ev[:, 1], ev[:, 3], H.HR)
        assert torch.equal(back, want)
    # fixed capacity: fixed shape
    evs = srv_ev.step_events({0: H.window(A, 4)}, capacity=64)
    assert evs[0].shape == (64, 4)
