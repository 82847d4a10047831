"""MultiStreamESR on the GPU: one captured graph for all streams, against
the eager server, per-stream StreamingESR servers, and under bf16 autocast."""

import copy

import pytest
import torch

from esr_amd.engine import MultiStreamESR
from esr_amd.models import build_model

import multistream_helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# graphed vs eager, same batch and same kernels: the project's bound from
# test_streaming_graphed_matches_eager_gpu
ATOL_GRAPH_VS_EAGER = 1e-4

# Batch 3 vs batch 1 may pick different MIOpen solvers.  Measured on an
# MI355X on the parent commit for this model in fp32 with the suite's
# MIOPEN_FIND_MODE=FAST (ESRNet basech 8, 3 frames, 32x48 count maps,
# 12 seeds x 5 recurrent steps, outputs ~0.1):
#   max |model(x3)[i] - model(x3[i:i+1])| = 0.0
# i.e. the fp32 path is bit-equal across these batch sizes, and the eager
# server measured 0.0 against the per-stream servers on every tick of the
# schedule.  atol = 4 x the measured value = 0.0: the maps must be equal.
# That is stricter than the semantics need: it holds only while MIOpen picks
# solvers that give bit-identical fp32 results at batch 1 and batch 3.  If
# this test alone fails after a ROCm, MIOpen or find-db update while
# test_graphed_matches_eager still passes, re-measure the line above before
# suspecting the server.
BATCH_DIFF_MEASURED = 0.0
ATOL_VS_SINGLE = 4 * BATCH_DIFF_MEASURED


def _model(seed=0):
    torch.manual_seed(seed)
    return build_model("ESRNet", inch=2, basech=8, num_frame=3)


def _server(model, **kw):
    args = dict(scale=H.SCALE, seqn=H.SEQN, max_streams=H.MAX_STREAMS,
                max_events=4096, device=DEV, use_graphs=True, amp_dtype=None)
    args.update(kw)
    return MultiStreamESR(copy.deepcopy(model), H.LR, **args)


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def eager_outs(model):
    srv = _server(model, use_graphs=False)
    assert srv._ext is not None, "native ingest kernels are not built"
    outs = H.run_multistream(srv)
    assert srv._graph is None
    return outs


def _compare(got, want, atol):
    assert len(got) == len(want) == len(H.PUSHES)
    for tick, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) == H.WARM[tick], (tick, set(g), set(w))
        for sid in w:
            assert g[sid].shape == (2, *H.HR)
            err = (g[sid] - w[sid]).abs().max().item()
            assert err <= atol, (tick, sid, err)


def test_graphed_matches_eager(model, eager_outs):
    srv = _server(model, use_graphs=True)
    outs = H.run_multistream(srv)
    assert srv._graph is not None, "graph was not captured"
    _compare(outs, eager_outs, ATOL_GRAPH_VS_EAGER)


def test_eager_matches_single_stream_servers(model, eager_outs):
    _compare(eager_outs, H.run_single_servers(model, device=DEV),
             ATOL_VS_SINGLE)


def test_missing_kernels_warn_and_fall_back(model, monkeypatch):
    """Without the native ingest kernels the server still works on the
    torch ingest, uncaptured, and says so."""
    import esr_amd.engine.multistream as ms
    monkeypatch.setattr(ms, "get_ext", lambda: None)
    with pytest.warns(RuntimeWarning, match="stream_ingest"):
        srv = _server(model, use_graphs=True)
    assert srv._ext is None and not srv.use_graphs
    a = srv.open()
    for t in range(3):
        out = srv.step({a: H.window(H.A, t)})
    assert srv._graph is None
    assert set(out) == {a} and torch.isfinite(out[a]).all()


def test_idle_stream_is_untouched_graphed(model):
    srv = _server(model)
    a, b = srv.open(), srv.open()
    S = srv.max_streams
    for t in range(4):
        srv.step({a: H.window(H.A, t), b: H.window(H.B, t)})
    buf = srv._buf[:, b].clone()
    state = srv._state[[b, S + b]].clone()
    assert buf.abs().sum() > 0 and state.abs().sum() > 0
    assert set(srv.step({a: H.window(H.A, 4)})) == {a}
    assert torch.equal(srv._buf[:, b], buf)
    assert torch.equal(srv._state[[b, S + b]], state)


def test_bf16_autocast_graphed_runs_on_the_native_stack(model):
    from esr_amd.ops import conv
    srv = _server(model, amp_dtype=torch.bfloat16)
    before = conv.stats["native_calls"]
    srv._capture()                  # step() would do this at its first tick
    assert srv._graph is not None, "graph was not captured"
    assert conv.stats["native_calls"] > before
    graph = srv._graph
    outs = H.run_multistream(srv)
    assert srv._graph is graph
    assert [set(o) for o in outs] == H.WARM
    for o in outs:
        for out in o.values():
            assert out.shape == (2, *H.HR) and out.dtype == torch.float32
            assert torch.isfinite(out).all()
