"""Gradient-norm clipping on FlatAdam's pure-torch path (CPU), in the config,
in `backward_and_step` and across two ranks.  Yardstick, tolerance and
inputs: grad_clip_helpers."""

import math

import pytest
import torch

from flat_adam_helpers import (HYPER_CASES, LR, assert_close_by_rule,
                               assert_untouched, flat, hyper_id,
                               make_flat_adam, run_flat_adam, run_torch_adam,
                               snapshot)
from grad_clip_helpers import (CPU_SIZES, STEPS, assert_clipping_matters,
                               assert_within_one_ulp, bits, clip_reference,
                               feed, make_clipped, run_clipped)

PLAIN = (False, 0.0, False)
GRAD_NORM, CLIP_COEF, CLIPPED = range(3)


# ---- 1. parameters, norm and counter against the fp64 yardstick ----

@pytest.mark.parametrize("hyper", HYPER_CASES, ids=hyper_id)
@pytest.mark.parametrize("n", CPU_SIZES)
def test_matches_fp64_clip_then_adam(n, hyper):
    init, grads, max_norm, p64, bound, norms64, unclipped = \
        clip_reference(n, hyper)
    assert_clipping_matters(p64, unclipped, bound)
    got, opt, _, clips = run_clipped(init, grads, hyper, max_norm)
    assert_close_by_rule(got, p64, bound, f"n={n} {hyper_id(hyper)}")
    assert opt.step_count == STEPS and opt.skipped_steps == 0
    # no norm sits near the threshold, where a last-bit difference in the
    # norm would flip the decision
    assert all(abs(v / max_norm - 1.0) > 0.2 for v in norms64)
    expected = 0
    for k, (c, v) in enumerate(zip(clips, norms64)):
        want = torch.tensor(v, dtype=torch.float32).item()
        assert_within_one_ulp(c[GRAD_NORM], want, f"norm of step {k}")
        expected += v > max_norm
        assert int(c[CLIPPED]) == expected
        if v > max_norm:
            assert c[CLIP_COEF] < 1.0
        else:
            assert c[CLIP_COEF] == 1.0
    assert opt.clipped_steps == expected
    assert expected == (3 if n == 1 else 4)  # step 3 never clips
    assert opt.grad_norm_value == clips[-1][GRAD_NORM].item()
    assert opt.clip_coef_value == clips[-1][CLIP_COEF].item()


# ---- 2. bitwise cases ----

@pytest.mark.parametrize("hyper", [PLAIN, (True, 1e-4, True)], ids=hyper_id)
def test_large_max_norm_is_bitwise_the_unclipped_optimizer(hyper):
    init, grads = clip_reference(1027, hyper)[:2]
    _, plain, _ = run_flat_adam(init, grads, hyper)
    _, opt, _, clips = run_clipped(init, grads, hyper, 1e30)
    for a, b in ((plain.flat_param, opt.flat_param),
                 (plain.exp_avg, opt.exp_avg),
                 (plain.exp_avg_sq, opt.exp_avg_sq)):
        assert torch.equal(bits(a), bits(b))
    assert opt.clipped_steps == 0
    assert all(c[CLIP_COEF] == 1.0 for c in clips)
    assert torch.equal(plain.device_state, opt.device_state)


@pytest.mark.parametrize("hyper", [PLAIN, (True, 1e-4, True)], ids=hyper_id)
def test_unscaling_stays_bitwise_exact_under_clipping(hyper):
    init, grads, max_norm = clip_reference(1027, hyper)[:3]
    plain, popt, _, pclips = run_clipped(init, grads, hyper, max_norm)
    scaled, opt, _, sclips = run_clipped(
        init, grads, hyper, max_norm, mult=65536.0,
        loss_scale={"init_scale": 65536.0})
    assert opt.loss_scale_value == 65536.0
    assert torch.equal(plain, scaled)
    assert torch.equal(bits(popt.exp_avg_sq), bits(opt.exp_avg_sq))
    # the reported norm is the un-scaled one, the coefficient the same
    for a, b in zip(pclips, sclips):
        assert torch.equal(a, b)


# ---- 3. a non-finite gradient skips the step ----

@pytest.mark.parametrize("bad", [float("inf"), float("nan")],
                         ids=["inf", "nan"])
@pytest.mark.parametrize("scaling", [False, True], ids=["unscaled", "scaled"])
def test_nonfinite_gradient_skips_step(scaling, bad):
    hyper = (True, 1e-4, False)
    init, grads, max_norm, _, _, _, _ = clip_reference(1027, hyper)
    ls = {"init_scale": 1024.0} if scaling else None
    mult = 1024.0 if scaling else 1.0
    opt, params = make_clipped(init, hyper, max_norm, loss_scale=ls)
    feed(opt, params, grads[0], mult)
    opt.step()
    snap = snapshot(opt)
    clipped = opt.clipped_steps
    feed(opt, params, grads[1], mult)
    opt.flat_grad[517] = bad
    opt.step()
    assert_untouched(opt, snap)
    assert opt.skipped_steps == 1 and opt.step_count == 1
    assert opt.clipped_steps == clipped
    assert opt.loss_scale_value == (512.0 if scaling else 1.0)
    # the flag is left cleared and the next clean step is taken
    feed(opt, params, grads[1], 512.0 if scaling else 1.0)
    opt.step()
    assert opt.step_count == 2 and opt.skipped_steps == 1
    assert opt.clipped_steps == clipped + 1
    init, grads, max_norm, p64, bound, _, unclipped = \
        clip_reference(1027, hyper, 2)
    assert_clipping_matters(p64, unclipped, bound)
    assert_close_by_rule(flat(params), p64, bound, "after skip")


# ---- 4. constructor ----

@pytest.mark.parametrize("bad", [0, -1.0, float("inf"), float("nan")])
def test_bad_max_grad_norm_raises(bad):
    from esr_amd.optim import FlatAdam, FlatAdamW
    for cls in (FlatAdam, FlatAdamW):
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls([torch.nn.Parameter(torch.ones(3))], max_grad_norm=bad)


def test_clipping_off_is_todays_optimizer():
    from esr_amd.optim import FlatAdamW, grad_clip_stats
    opt, _ = make_flat_adam([torch.ones(5)], PLAIN)
    assert opt.max_grad_norm is None and opt.clip_state is None
    assert opt.grad_norm_value is None and opt.clipped_steps is None
    assert len(opt.state_buffers()) == 3
    assert "grad_clip" not in opt.state_dict()
    assert grad_clip_stats(opt) is None
    assert grad_clip_stats(torch.optim.SGD(
        [torch.nn.Parameter(torch.ones(2))], lr=0.1)) is None
    optw = FlatAdamW([torch.nn.Parameter(torch.ones(5))], max_grad_norm=2.0)
    assert optw.max_grad_norm == 2.0
    assert optw.param_groups[0]["decoupled_weight_decay"]
    assert grad_clip_stats(optw) == (0.0, 0)


# ---- 5. state dict ----

def test_state_dict_round_trip_keeps_clipped_steps():
    init, grads, max_norm = clip_reference(1027, PLAIN)[:3]
    _, opt, params, _ = run_clipped(init, grads[:2], PLAIN, max_norm)
    sd = opt.state_dict()
    assert sd["grad_clip"] == {"max_norm": max_norm, "clipped_steps": 2}
    opt2, params2 = make_clipped([p.detach() for p in params], PLAIN,
                                 max_norm)
    opt2.load_state_dict(sd)
    assert opt2.clipped_steps == 2 and opt2.step_count == 2
    for o in (opt, opt2):
        feed(o, o._params, grads[3])
        o.step()
    assert torch.equal(flat(params), flat(params2))
    assert opt2.clipped_steps == 3


def test_clipped_flat_adam_state_dict_loads_into_adam():
    from flat_adam_helpers import make_torch_adam
    init, grads, max_norm = clip_reference(1027, PLAIN)[:3]
    _, opt, params, _ = run_clipped(init, grads[:2], PLAIN, max_norm)
    adam_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    adam = make_torch_adam(adam_params, PLAIN, lr=0.5)
    adam.load_state_dict(opt.state_dict())
    assert adam.param_groups[0]["lr"] == LR
    for p, g in zip(adam_params, grads[2]):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(adam_params, max_norm)
    adam.step()
    p64, bound, _, unclipped = clip_reference(1027, PLAIN, 3)[3:]
    assert_clipping_matters(p64, unclipped, bound)
    assert_close_by_rule(flat(adam_params), p64, bound, "flat->adam")


def test_adam_state_dict_loads_into_clipped_flat_adam():
    init, grads, max_norm = clip_reference(1027, PLAIN)[:3]
    _, adam, adam_params = run_torch_adam(init, grads[:1], PLAIN,
                                          torch.float32)
    opt, params = make_clipped([p.detach() for p in adam_params], PLAIN,
                               max_norm)
    feed(opt, params, grads[1])
    opt.step()  # the counter is not zero when the checkpoint arrives
    assert opt.clipped_steps == 1
    opt.load_state_dict(adam.state_dict())
    assert opt.clipped_steps == 0 and opt.step_count == 1
    assert opt.max_grad_norm == max_norm


# ---- 6. graph warm-up roll-back ----

def test_snapshot_and_restore_hand_the_clip_scalars_back():
    from esr_amd.optim import restore_optimizer, snapshot_optimizer
    init, grads, max_norm = clip_reference(1027, PLAIN)[:3]
    _, opt, params, clips = run_clipped(init, grads[:2], PLAIN, max_norm)
    assert any(t is opt.clip_state for t in opt.state_buffers())
    before = (flat(params).clone(), opt.device_state.clone())
    snap = snapshot_optimizer(opt)
    feed(opt, params, grads[3])
    opt.step()
    assert opt.clipped_steps == 3
    assert not torch.equal(opt.clip_state, clips[-1])
    restore_optimizer(opt, snap)
    assert torch.equal(bits(opt.clip_state), bits(clips[-1]))
    assert torch.equal(flat(params), before[0])
    assert torch.equal(opt.device_state, before[1])


# ---- 7. config ----

def test_grad_clip_plan():
    from esr_amd.engine.trainer import grad_clip_plan
    cfg = lambda name, gc: {"optimizer": {"name": name},  # noqa: E731
                            **({"grad_clip": gc} if gc is not None else {})}
    on = {"enabled": True, "max_norm": 2}
    assert grad_clip_plan(cfg("Adam", None)) == ("off", None)
    assert grad_clip_plan(cfg("FlatAdam", {"enabled": False,
                                           "max_norm": 1.0})) == ("off", None)
    assert grad_clip_plan(cfg("FlatAdam", {"max_norm": 1.0})) == ("off", None)
    assert grad_clip_plan(cfg("FlatAdam", on)) == ("flat", 2.0)
    assert grad_clip_plan(cfg("FlatAdamW", on)) == ("flat", 2.0)
    assert grad_clip_plan(cfg("Adam", on)) == ("torch", 2.0)
    with pytest.raises(ValueError, match="unknown grad_clip"):
        grad_clip_plan(cfg("FlatAdam", {"enabled": True, "max_norm": 1.0,
                                        "norm_type": 2}))
    for bad in (0, -1.0, float("inf"), float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="max_norm"):
            grad_clip_plan(cfg("FlatAdam", {"enabled": True,
                                            "max_norm": bad}))
    with pytest.raises(ValueError, match="max_norm"):
        grad_clip_plan(cfg("Adam", {"enabled": True}))


def test_build_training_passes_max_grad_norm(tmp_path, synth_datalist):
    from test_engine import _train_config
    from esr_amd.config import ConfigParser
    from esr_amd.engine import build_training
    from esr_amd.utils.logging import setup_logging

    def build(run_id, opt_name):
        cfg = _train_config(synth_datalist, tmp_path / f"out_{run_id}")
        cfg["optimizer"] = {"name": opt_name, "args": {"lr": 1e-3}}
        cfg["grad_clip"] = {"enabled": True, "max_norm": 1e-3}
        cfg["valid_dataloader"] = None
        cfg["trainer"]["monitor"] = "off"
        parser = ConfigParser(cfg, run_id=run_id)
        return parser, build_training(parser, torch.device("cpu"),
                                      setup_logging(f"gc-{run_id}", None))

    import json
    for run_id, name in (("f", "FlatAdam"), ("t", "Adam")):
        parser, trainer = build(run_id, name)
        flat_opt = name == "FlatAdam"
        assert getattr(trainer.optimizer, "max_grad_norm", None) == \
            (1e-3 if flat_opt else None)
        assert trainer.max_grad_norm == (None if flat_opt else 1e-3)
        trainer.train()
        norm, clipped = trainer.grad_clip_stats()
        assert math.isfinite(norm) and norm > 0
        assert (clipped is not None) == flat_opt
        tags = {}
        with open(parser.log_dir / "scalars.jsonl") as f:
            for line in f:
                rec = json.loads(line)
                tags.setdefault(rec["tag"], []).append(rec["value"])
        assert all(math.isfinite(v) and v > 0 for v in tags["grad_norm"])
        assert ("clipped_steps" in tags) == flat_opt


# ---- 8. backward_and_step for optimizers that do not clip on their own ----

def _tiny():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Tanh(),
                              torch.nn.Linear(3, 2))
    x = torch.randn(5, 4)
    return net, x


def _variants():
    """(flat buffer, GradScaler device): per-tensor and flat-buffer
    clipping, and per-tensor under a GradScaler where this torch build has
    one on the CPU (the graphed, flat-buffer step never runs with one)."""
    out = [(False, None), (True, None)]
    try:
        torch.amp.GradScaler("cpu", init_scale=1024.0)
        out.append((False, "cpu"))
    except Exception:
        pass
    return out


@pytest.mark.parametrize("flat_buffer,scaler", _variants(),
                         ids=lambda v: str(v))
def test_backward_and_step_clips_like_clip_grad_norm(flat_buffer, scaler):
    from esr_amd.engine.graph_runner import flatten_grads
    from esr_amd.engine.step import backward_and_step
    max_norm = 1e-2
    net, x = _tiny()
    ref, _ = _tiny()
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    ref_opt = torch.optim.Adam(ref.parameters(), lr=LR)
    flat_grad = flatten_grads(list(net.parameters()), "cpu") \
        if flat_buffer else None
    synced = []
    for k, mult in enumerate([1.0, 1e-4, 100.0]):
        ref_opt.zero_grad()
        (ref(x).square().sum() * mult).backward()
        want = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
        ref_opt.step()

        if flat_grad is not None:
            flat_grad.zero_()
        else:
            opt.zero_grad()
        gs = torch.amp.GradScaler("cpu", init_scale=1024.0) if scaler \
            else None
        norm = backward_and_step(net(x).square().sum() * mult, opt,
                                 lambda: synced.append(k), gs,
                                 max_grad_norm=max_norm, flat_grad=flat_grad)
        assert synced[-1] == k
        assert torch.allclose(norm, want, rtol=1e-6, atol=0)
        # the middle step does not clip, the other two do
        assert (want > max_norm) == (k != 1)
        for a, b in zip(net.parameters(), ref.parameters()):
            # same fp32 formula; only the order of the norm's sum differs
            assert torch.allclose(a, b, rtol=0, atol=LR * 1e-5), k
    # and without max_grad_norm nothing is clipped and None comes back
    assert backward_and_step(net(x).square().sum(), opt, lambda: None) is None


# ---- 9. two ranks ----

def _run_clip_sync(rank, port, q):
    """Un-wrapped model + clipping FlatAdam on two ranks: after the flat
    all-reduce both ranks see the same norm and take the same step."""
    import torch.distributed as dist
    from test_distributed import _init
    try:
        _init(rank, port)
        from esr_amd.engine.trainer import Trainer
        from esr_amd.optim import FlatAdam
        w = torch.nn.Parameter(torch.linspace(-1, 1, 6))
        opt = FlatAdam([w], lr=LR, max_grad_norm=1.0,
                       loss_scale={"init_scale": 4.0})

        class _T:  # minimal Trainer stand-in
            pass
        t = _T()
        t.model, t.optimizer = torch.nn.ParameterList([w]), opt
        # different gradients per rank, scaled by the loss scale
        opt.flat_grad.copy_(torch.arange(6.0) * (rank + 1) * 4.0)
        Trainer._sync_grads_if_needed(t)
        opt.step()
        q.put((rank, (opt.grad_norm_value, opt.clip_coef_value,
                      opt.clipped_steps, bits(w).tolist())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(400)
def test_ranks_clip_the_all_reduced_gradient_identically():
    from test_distributed import _spawn
    res = _spawn(_run_clip_sync, 29541)
    assert res[0] == res[1]
    norm, coef, clipped, _ = res[0][0]
    # mean gradient 1.5 * arange(6): norm 1.5 * sqrt(55)
    want = torch.tensor(1.5 * math.sqrt(55.0), dtype=torch.float32).item()
    assert_within_one_ulp(norm, want)
    assert clipped == 1 and coef < 1.0
