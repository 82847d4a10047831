"""FlatAdam's HIP kernels (flat_adam.hip) against its own CPU torch path and
the fp64 torch.optim.Adam reference, inside a captured graph, and through
the graphed trainer."""

import functools
import math
from pathlib import Path

import pytest
import torch

from flat_adam_helpers import (HYPER_CASES, assert_close_by_rule,
                               assert_untouched, feed_grads, flat, hyper_id,
                               make_case, make_flat_adam, reference_and_bound,
                               run_flat_adam, run_torch_adam, snapshot,
                               split_sizes)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# scalar tail only / n < 4 / no tail / partial final block / tail + second
# block / one float4 past a full 2048-block grid (grid-stride wrap) + tail
SIZES = [1, 3, 4, 1023, 1027, 256 * 4 * 2048 + 5]
STEPS = 5
PLAIN = (False, 0.0, False)


@functools.lru_cache(maxsize=None)
def _case(n, hyper, steps=STEPS):
    """Inputs, fp64 reference + bound and the CPU torch path, computed once
    per (n, hyper) and left unchanged."""
    init, grads = make_case(split_sizes(n), steps, seed=n % 1000 + 1)
    p64, bound = reference_and_bound(init, grads, hyper)
    cpu, cpu_opt, _ = run_flat_adam(init, grads, hyper)
    return init, grads, p64, bound, cpu, cpu_opt.device_state.clone()


# ---- 8. kernel against the torch path and the fp64 reference ----

@pytest.mark.parametrize("hyper", HYPER_CASES, ids=hyper_id)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_torch_path_and_fp64(n, hyper):
    init, grads, p64, bound, cpu, cpu_state = _case(n, hyper)
    got, opt, params = run_flat_adam(init, grads, hyper, device=DEV)
    assert_close_by_rule(got, p64, bound, f"n={n} kernel vs fp64")
    assert_close_by_rule(got, cpu, bound, f"n={n} kernel vs torch path")
    assert opt.step_count == STEPS and opt.skipped_steps == 0
    # scale, tracker, found_inf, step, lr, skipped are exact; the two bias
    # corrections are fp64 results rounded to fp32 on either side
    st = opt.device_state.cpu()
    assert torch.equal(st[:6], cpu_state[:6])
    assert torch.allclose(st[6:], cpu_state[6:], rtol=2 ** -22, atol=0)


@pytest.mark.parametrize("hyper", [PLAIN, (True, 1e-4, True)], ids=hyper_id)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_unscaling_is_bitwise_exact(n, hyper):
    init, grads = _case(n, hyper)[:2]
    plain, _, _ = run_flat_adam(init, grads, hyper, device=DEV)
    scaled, opt, _ = run_flat_adam(init, grads, hyper, device=DEV,
                                   mult=65536.0,
                                   loss_scale={"init_scale": 65536.0})
    assert opt.loss_scale_value == 65536.0 and opt.growth_tracker == STEPS
    assert torch.equal(plain, scaled)


def _overflow_step(n, bad, index):
    hyper = (True, 1e-4, False)
    init, grads = _case(n, hyper)[:2]
    opt, params = make_flat_adam(init, hyper, device=DEV, loss_scale={})
    feed_grads(opt, params, grads[0], 65536.0)
    opt.step()
    snap = snapshot(opt)
    feed_grads(opt, params, grads[1], 65536.0)
    opt.flat_grad[index] = bad
    opt.step()
    assert_untouched(opt, snap)
    assert opt.loss_scale_value == 32768.0
    assert opt.skipped_steps == 1
    assert opt.growth_tracker == 0
    assert opt.step_count == 1
    # the flag is left cleared and the next clean step is taken
    feed_grads(opt, params, grads[1], 32768.0)
    opt.step()
    assert opt.step_count == 2 and opt.skipped_steps == 1
    init, grads, p64, bound, _, _ = _case(n, hyper, 2)
    assert_close_by_rule(flat(params), p64, bound, f"n={n} after skip")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")],
                         ids=["inf", "nan"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_overflow_skips_step(n, bad):
    _overflow_step(n, bad, n // 2)


# ---- 9. position of the non-finite element ----

def _positions(n):
    """index 0, n-1 (inside the scalar tail) and a body element owned by the
    last block of the launch grid."""
    assert n % 4 != 0
    grid = min(-(-n // 1024), 2048)
    first_vec_of_last_block = (grid - 1) * 256
    assert first_vec_of_last_block < n // 4
    return [0, n - 1, first_vec_of_last_block * 4 + 2]


@pytest.mark.parametrize("which", [0, 1, 2],
                         ids=["first", "tail", "last-block"])
@pytest.mark.parametrize("n", [3003, 256 * 4 * 2048 + 5])
def test_kernel_nonfinite_position(n, which):
    _overflow_step(n, float("-inf") if which else float("nan"),
                   _positions(n)[which])


def test_kernel_growth():
    init, grads = _case(1027, PLAIN)[:2]
    ls = {"init_scale": 1024.0, "growth_interval": 2}
    opt, params = make_flat_adam(init, PLAIN, device=DEV, loss_scale=ls)
    cpu, cpu_params = make_flat_adam(init, PLAIN, loss_scale=ls)
    # clean, clean (grow), clean, overflow (back off), clean, clean (grow)
    expect = [(1024.0, 1), (2048.0, 0), (2048.0, 1), (1024.0, 0),
              (1024.0, 1), (2048.0, 0)]
    for k, (scale, tracker) in enumerate(expect):
        for o, ps in ((opt, params), (cpu, cpu_params)):
            feed_grads(o, ps, grads[k % STEPS], o.loss_scale_value)
            if k == 3:
                o.flat_grad[1026] = float("inf")
            o.step()
            assert (o.loss_scale_value, o.growth_tracker) == (scale, tracker)
    assert opt.step_count == 5 and opt.skipped_steps == 1
    assert torch.equal(opt.device_state.cpu()[:6], cpu.device_state[:6])


def test_missing_extension_is_an_error(monkeypatch):
    """No eager GPU fall-back: without the extension a GPU step raises."""
    import esr_amd.ops.native as native
    opt, params = make_flat_adam([torch.ones(5)], PLAIN, device=DEV)
    monkeypatch.setattr(native, "_EXT", None)
    monkeypatch.setattr(native, "_TRIED", True)
    with pytest.raises(RuntimeError, match="not built"):
        opt.step()


# ---- 10. captured step honours lr and skips inside the graph ----

def test_captured_step_reads_lr_from_device():
    hyper = (False, 1e-4, False)
    shapes = [(3,), (2, 5), (1027,)]
    n = 3 + 10 + 1027
    lrs = [1e-3, 5e-4, 2.5e-4, 2.5e-4]
    init, grads = make_case(shapes, len(lrs), seed=10)
    p64, bound = reference_and_bound(init, grads, hyper, lrs)

    opt, params = make_flat_adam(init, hyper, device=DEV, lr=lrs[0],
                                 loss_scale={"init_scale": 1024.0})
    src = torch.zeros(n, device=DEV)  # static source of the scaled grads

    def body():  # one stream, no parallel branches
        opt.zero_grad()
        opt.flat_grad.add_(src)
        opt.step()

    before = snapshot(opt)
    state0 = opt.device_state.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()  # warm-up: zero grads, so only moments/step would move
    torch.cuda.current_stream().wait_stream(side)
    opt.device_state.copy_(state0)
    for buf, saved in zip((opt.flat_param, opt.exp_avg, opt.exp_avg_sq),
                          before[0]):
        buf.copy_(saved)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    # capture records, it does not run
    assert opt.step_count == 0

    def replay(k, scale):
        opt.param_groups[0]["lr"] = lrs[k]
        opt.sync_lr()
        src.copy_(flat(grads[k]) * scale)
        graph.replay()

    for k in range(3):
        replay(k, 1024.0)
    assert opt.step_count == 3 and opt.skipped_steps == 0
    p3, bound3 = reference_and_bound(init, grads[:3], hyper, lrs[:3])
    assert_close_by_rule(flat(params), p3, bound3, "3 replays")
    # a fixed lr of 1e-3 (what a baked-in scalar would give) is far outside
    baked, _, _ = run_torch_adam(init, grads[:3], hyper, torch.float64,
                                 [lrs[0]] * 3)
    assert (baked - p3).abs().max().item() > 100 * bound

    # overflow inside the graph: skip, back off, nothing else moves
    snap = snapshot(opt)
    src.copy_(flat(grads[3]) * 1024.0)
    src[5] = float("inf")
    graph.replay()
    assert_untouched(opt, snap)
    assert opt.loss_scale_value == 512.0 and opt.skipped_steps == 1
    # and the next replay, at the backed-off scale, is step 4
    replay(3, 512.0)
    assert opt.step_count == 4
    assert_close_by_rule(flat(params), p64, bound, "4 steps + 1 skip")


# ---- 11. trainer end to end: fp16 + FlatAdam + loss scaling, graphed ----

ITERS = 3


def _train_config(datalist, out_dir, loss_scale, iterations=ITERS):
    from test_gpu_trainer import _train_config as base
    cfg = base(datalist, out_dir, iterations=iterations, hip_graphs=True)
    cfg["precision"] = "fp16"
    cfg["optimizer"] = {"name": "FlatAdam", "args": {"lr": 1e-3}}
    if loss_scale:
        cfg["loss_scale"] = {"enabled": True}
    return cfg


def _run(tmp_path, datalist, run_id, loss_scale, iterations=ITERS,
         resume=None):
    """Train; returns (parser, trainer, per-iteration losses, optimizer
    scalars seen right after graph capture, before the first replay)."""
    from esr_amd.config import ConfigParser
    from esr_amd.engine import build_training
    from esr_amd.utils.logging import setup_logging
    cfg = _train_config(datalist, tmp_path / f"out_{run_id}", loss_scale,
                        iterations)
    parser = ConfigParser(cfg, run_id=run_id)
    torch.manual_seed(7)
    trainer = build_training(parser, torch.device(DEV),
                             setup_logging(f"gpu-flat-{run_id}", None),
                             resume=resume)
    at_resume = (trainer.optimizer.loss_scale_value,
                 trainer.optimizer.step_count,
                 trainer.optimizer.skipped_steps)
    losses, after_capture = [], []
    graphed = trainer.graphed_bptt_step

    def recording_step(inputs_seq):
        if not after_capture:
            trainer._get_graph_step(inputs_seq)  # captures, cached for below
            o = trainer.optimizer
            after_capture.append((o.loss_scale_value, o.step_count,
                                  o.skipped_steps))
        out = graphed(inputs_seq)
        losses.append(out[0].item())
        return out

    trainer.graphed_bptt_step = recording_step
    trainer.train()
    return parser, trainer, losses, after_capture[0], at_resume


@pytest.fixture(scope="module")
def datalist(tmp_path_factory):
    from esr_amd.data import make_synthetic_dataset
    root = tmp_path_factory.mktemp("gpusynth_flat")
    return make_synthetic_dataset(root, num_sequences=1,
                                  resolution=(64, 64), num_events=60_000,
                                  seed=11)


@pytest.fixture(scope="module")
def scaled_run(tmp_path_factory, datalist):
    return _run(tmp_path_factory.mktemp("scaled"), datalist, "s1", True)


def test_trainer_graphed_fp16_with_loss_scaling(scaled_run):
    parser, trainer, losses, after_capture, _ = scaled_run
    assert trainer.use_graphs, "graph path fell back to eager"
    assert trainer._graph_step is not None
    assert trainer._graph_step[1].flat_grad is trainer.optimizer.flat_grad
    avg = trainer.train_metrics.avg("train_loss")
    assert math.isfinite(avg) and avg > 0
    assert len(losses) == ITERS and all(math.isfinite(v) for v in losses)
    # warm-up steps were rolled back: iteration 0 starts from a fresh scaler
    assert after_capture == (65536.0, 0, 0)
    opt = trainer.optimizer
    assert opt.step_count + opt.skipped_steps == ITERS
    assert opt.step_count >= 1
    assert opt.loss_scale_value == 65536.0 * 0.5 ** opt.skipped_steps


def test_trainer_checkpoint_and_resume_keep_scaler_state(
        scaled_run, tmp_path, datalist):
    parser, trainer = scaled_run[:2]
    ckpt = sorted(Path(parser.save_dir).glob("checkpoint-iteration*.pth"))[-1]
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    states = saved["optimizer"]["states"]
    opt = trainer.optimizer
    assert states["loss_scale"] == {
        "enabled": True, "scale": opt.loss_scale_value,
        "growth_tracker": opt.growth_tracker,
        "skipped_steps": opt.skipped_steps}
    assert int(states["state"][0]["step"]) == opt.step_count
    # one resumed iteration; the capture's warm-up roll-back must hand the
    # restored scale and step back, not a fresh scaler
    _, resumed, losses, after_capture, at_resume = _run(
        tmp_path, datalist, "s2", True, iterations=ITERS + 1,
        resume=str(ckpt))
    want = (opt.loss_scale_value, opt.step_count, opt.skipped_steps)
    assert at_resume == want
    assert after_capture == want
    assert len(losses) == 1 and math.isfinite(losses[0])
    ropt = resumed.optimizer
    assert ropt.step_count + ropt.skipped_steps == ITERS + 1


def test_trainer_first_step_loss_matches_unscaled_run(scaled_run, tmp_path,
                                                      datalist):
    """Scaling only touches the backward: the first-step loss equals a
    loss_scale-off FlatAdam run within the project's 0.1 relative bound
    (test_trainer_eager_vs_graph_losses_close)."""
    a = scaled_run[2][0]
    _, _, losses, _, _ = _run(tmp_path, datalist, "u1", False, iterations=1)
    b = losses[0]
    print(f"first-step loss: scaled {a:.6e}  un-scaled {b:.6e}")
    assert abs(a - b) / max(abs(a), 1e-6) < 0.1, (a, b)
