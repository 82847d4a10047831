"""FlatAdam on its pure-torch path (CPU): Adam/AdamW math against an fp64
reference, GradScaler semantics, checkpoint interchange with
torch.optim.Adam, and the config/trainer wiring."""

import math

import pytest
import torch

from flat_adam_helpers import (HYPER_CASES, LR, assert_close_by_rule,
                               assert_untouched, feed_grads, flat, fp32_ulp,
                               hyper_id, make_case, make_flat_adam,
                               reference_and_bound, run_flat_adam,
                               run_torch_adam, snapshot)

SHAPES = [(3,), (2, 5), (1027,)]
STEPS = 5
PLAIN = (False, 0.0, False)


# ---- 1. reference match against fp64 Adam ----

@pytest.mark.parametrize("hyper", HYPER_CASES, ids=hyper_id)
def test_matches_fp64_adam(hyper):
    init, grads = make_case(SHAPES, STEPS, seed=1)
    p64, bound = reference_and_bound(init, grads, hyper)
    got, opt, params = run_flat_adam(init, grads, hyper)
    assert_close_by_rule(got, p64, bound, hyper_id(hyper))
    assert opt.step_count == STEPS and opt.skipped_steps == 0
    # the step really moved the parameters, by about lr per step
    assert (got - flat(init).double()).abs().max().item() > LR


# ---- 2. un-scaling is exact ----

@pytest.mark.parametrize("hyper", [PLAIN, (True, 1e-4, True)], ids=hyper_id)
def test_unscaling_by_power_of_two_is_bitwise_exact(hyper):
    init, grads = make_case(SHAPES, STEPS, seed=2)
    plain, _, _ = run_flat_adam(init, grads, hyper)
    scaled, opt, _ = run_flat_adam(init, grads, hyper, mult=65536.0,
                                   loss_scale={"init_scale": 65536.0})
    assert opt.loss_scale_value == 65536.0
    assert torch.equal(plain, scaled)


# ---- 3. overflow skip ----

@pytest.mark.parametrize("bad", [float("inf"), float("nan")],
                         ids=["inf", "nan"])
def test_overflow_skips_step_and_backs_off(bad):
    hyper = (True, 1e-4, False)
    init, grads = make_case(SHAPES, 2, seed=3)
    opt, params = make_flat_adam(init, hyper, loss_scale={})
    feed_grads(opt, params, grads[0])
    opt.step()
    snap = snapshot(opt)
    feed_grads(opt, params, grads[1])
    opt.flat_grad[517] = bad
    opt.step()
    assert_untouched(opt, snap)
    assert opt.loss_scale_value == 32768.0
    assert opt.skipped_steps == 1
    assert opt.growth_tracker == 0
    assert opt.step_count == 1


# ---- 4. growth ----

def test_scale_grows_after_exactly_growth_interval_clean_steps():
    init, grads = make_case(SHAPES, 1, seed=4)
    ls = {"init_scale": 1024.0, "growth_interval": 2}
    opt, params = make_flat_adam(init, PLAIN, loss_scale=ls)

    def clean():
        feed_grads(opt, params, grads[0])
        opt.step()

    def overflow():
        feed_grads(opt, params, grads[0])
        opt.flat_grad[0] = float("inf")
        opt.step()

    clean()
    assert opt.loss_scale_value == 1024.0 and opt.growth_tracker == 1
    clean()
    assert opt.loss_scale_value == 2048.0 and opt.growth_tracker == 0
    # an overflow between two clean steps resets the count
    clean()
    overflow()
    assert opt.loss_scale_value == 1024.0 and opt.growth_tracker == 0
    clean()
    assert opt.loss_scale_value == 1024.0 and opt.growth_tracker == 1
    clean()
    assert opt.loss_scale_value == 2048.0
    assert opt.step_count == 5 and opt.skipped_steps == 1


# ---- 5. the fp16 underflow case loss scaling exists for ----

def _toy_backward(opt, w, x):
    opt.zero_grad()
    y = w.half() * x.half()
    loss = (y.float() * 1e-9).sum()
    opt.scale_loss(loss).backward()


def test_fp16_underflow_toy_case():
    x = torch.tensor([0.5, 1.0, 1.5, 2.0])
    w0 = torch.tensor([0.3, -0.7, 1.1, 0.9])
    true_grad = x.double() * 1e-9

    # un-scaled: dL/dy = 1e-9 is below fp16's smallest subnormal (6e-8),
    # the gradient is exactly zero and Adam does not move w at all
    w = torch.nn.Parameter(w0.clone())
    from esr_amd.optim import FlatAdam
    opt = FlatAdam([w], lr=LR)
    _toy_backward(opt, w, x)
    assert torch.equal(opt.flat_grad, torch.zeros(4))
    opt.step()
    assert torch.equal(w.detach(), w0)

    # scaled by 65536: the gradient survives the fp16 backward
    w = torch.nn.Parameter(w0.clone())
    opt = FlatAdam([w], lr=LR, loss_scale={"init_scale": 65536.0})
    _toy_backward(opt, w, x)
    unscaled = opt.flat_grad.double() / 65536.0
    assert (unscaled != 0).all()
    # fp16 error budget of the scaled backward: 2^-11 relative for rounding
    # dL/dy = 6.5536e-5 to fp16, plus half a subnormal spacing (2^-25) on the
    # product with x, whose smallest value is 0.5 * 6.5536e-5
    budget = 2.0 ** -11 + 2.0 ** -25 / (0.5 * 6.5536e-5)
    rel = ((unscaled - true_grad).abs() / true_grad).max().item()
    print(f"un-scaled fp16 gradient: rel err {rel:.3e}, budget {budget:.3e}")
    assert rel <= budget
    opt.step()

    # the optimizer step on these ~1e-9 gradients, by the rule of test 1;
    # the reference consumes the gradient the fp16 backward delivered
    g32 = [(opt.flat_grad.double() / 65536.0).float()]
    p64, bound = reference_and_bound([w0], [g32], PLAIN)
    assert_close_by_rule(w.detach(), p64, bound, "toy scaled")
    # ... and lands within fp16's error of the step the true gradient gives
    # (first Adam step = lr * g / (|g| + eps): a relative error r in g moves
    # it by at most lr * r)
    p_true, _, _ = run_torch_adam([w0], [[true_grad.float()]], PLAIN,
                                  torch.float64)
    moved = (p_true - w0.double()).abs().min().item()
    assert moved > 1e-2 * LR
    slack = LR * budget + bound
    assert (w.detach().double() - p_true).abs().max().item() <= slack


# ---- 6. state dict interchange with torch.optim.Adam ----

@pytest.mark.parametrize("hyper", [PLAIN, (True, 1e-4, False),
                                   (False, 1e-4, True)], ids=hyper_id)
def test_adam_state_dict_loads_into_flat_adam(hyper):
    init, grads = make_case(SHAPES, 3, seed=6)
    p64, bound = reference_and_bound(init, grads, hyper)
    _, adam, adam_params = run_torch_adam(init, grads[:2], hyper,
                                          torch.float32)
    opt, params = make_flat_adam([p.detach() for p in adam_params], hyper,
                                 lr=0.5)  # lr comes from the checkpoint
    opt.load_state_dict(adam.state_dict())
    assert opt.step_count == 2
    assert opt.param_groups[0]["lr"] == LR
    lo = opt.flat_param.data_ptr()
    hi = lo + opt.flat_param.numel() * 4
    for p in params:
        assert lo <= p.data.data_ptr() < hi
        assert lo <= p.data_ptr() < hi
    feed_grads(opt, params, grads[2])
    opt.step()
    assert_close_by_rule(flat(params), p64, bound, "adam->flat")


@pytest.mark.parametrize("hyper", [PLAIN, (True, 1e-4, False),
                                   (False, 1e-4, True)], ids=hyper_id)
def test_flat_adam_state_dict_loads_into_adam(hyper):
    from flat_adam_helpers import make_torch_adam
    init, grads = make_case(SHAPES, 3, seed=7)
    p64, bound = reference_and_bound(init, grads, hyper)
    _, opt, params = run_flat_adam(init, grads[:2], hyper, loss_scale={},
                                   mult=65536.0)
    sd = opt.state_dict()
    assert sd["loss_scale"] == {"enabled": True, "scale": 65536.0,
                                "growth_tracker": 2, "skipped_steps": 0}
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} | (
        {"max_exp_avg_sq"} if hyper[0] else set())
    adam_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    adam = make_torch_adam(adam_params, hyper, lr=0.5)
    adam.load_state_dict(sd)
    for p, g in zip(adam_params, grads[2]):
        p.grad = g.clone()
    adam.step()
    assert_close_by_rule(flat(adam_params), p64, bound, "flat->adam")


def test_flat_adam_state_dict_round_trip_keeps_scaler_state():
    init, grads = make_case(SHAPES, 2, seed=8)
    ls = {"init_scale": 256.0, "growth_interval": 5}
    opt, params = make_flat_adam(init, PLAIN, loss_scale=ls)
    feed_grads(opt, params, grads[0])
    opt.step()
    feed_grads(opt, params, grads[1])
    opt.flat_grad[3] = float("nan")
    opt.step()
    sd = opt.state_dict()
    opt2, params2 = make_flat_adam([p.detach() for p in params], PLAIN,
                                   loss_scale=ls)
    opt2.load_state_dict(sd)
    assert (opt2.loss_scale_value, opt2.growth_tracker, opt2.skipped_steps,
            opt2.step_count) == (128.0, 0, 1, 1)
    for o in (opt, opt2):
        feed_grads(o, o._params, grads[1])
        o.step()
    assert torch.equal(flat(params), flat(params2))


def _save_tiny_checkpoint(path, opt_name, optimizer):
    from esr_amd.engine.checkpoint import save_checkpoint
    cfg = {"model": {"name": "Tiny"}, "lr_scheduler": {"name": "StepLR"},
           "optimizer": {"name": opt_name}}
    save_checkpoint(path, cfg, torch.nn.Linear(2, 2), optimizer)


def test_resumer_treats_adam_and_flat_adam_as_one_component(tmp_path):
    from esr_amd.engine.checkpoint import Resumer
    init, grads = make_case(SHAPES, 1, seed=9)
    _, adam, adam_params = run_torch_adam(init, grads, PLAIN, torch.float32)
    _, fl, _ = run_flat_adam(init, grads, PLAIN)
    _save_tiny_checkpoint(tmp_path / "adam.pth", "Adam", adam)
    _save_tiny_checkpoint(tmp_path / "flat.pth", "FlatAdam", fl)

    opt, _ = make_flat_adam(init, PLAIN)
    Resumer(tmp_path / "adam.pth", config={"optimizer": {"name": "FlatAdam"}}
            ).resume_optimizer(opt)
    assert opt.step_count == 1
    adam2 = torch.optim.Adam([torch.nn.Parameter(t.clone()) for t in init])
    Resumer(tmp_path / "flat.pth", config={"optimizer": {"name": "Adam"}}
            ).resume_optimizer(adam2)
    assert len(adam2.state) == len(init)

    for ckpt, name in [("adam.pth", "SGD"), ("flat.pth", "SGD"),
                       ("adam.pth", "FlatAdamW"), ("flat.pth", "AdamW")]:
        with pytest.raises(ValueError):
            Resumer(tmp_path / ckpt, config={"optimizer": {"name": name}}
                    ).resume_optimizer(opt)


# ---- 7. config wiring ----

def test_build_optimizer_knows_flat_adam():
    from esr_amd.config import build_optimizer
    from esr_amd.optim import FlatAdam, FlatAdamW
    p = [torch.nn.Parameter(torch.ones(5))]
    opt = build_optimizer("FlatAdam", p, lr=1e-3,
                          loss_scale={"init_scale": 128.0})
    assert isinstance(opt, FlatAdam) and opt.loss_scale_value == 128.0
    assert not opt.param_groups[0]["decoupled_weight_decay"]
    optw = build_optimizer("FlatAdamW", [torch.nn.Parameter(torch.ones(5))],
                           lr=1e-3)
    assert isinstance(optw, FlatAdamW)
    assert optw.param_groups[0]["decoupled_weight_decay"]
    assert optw.param_groups[0]["weight_decay"] == 1e-2
    assert not optw.loss_scaling
    loss = torch.tensor(2.0)
    assert optw.scale_loss(loss) is loss
    assert opt.scale_loss(loss).item() == 256.0


def test_differing_param_groups_raise():
    from esr_amd.optim import FlatAdam
    a = torch.nn.Parameter(torch.ones(3))
    b = torch.nn.Parameter(torch.ones(4))
    with pytest.raises(ValueError, match="lr"):
        FlatAdam([{"params": [a]}, {"params": [b], "lr": 1e-4}], lr=1e-3)
    opt = FlatAdam([{"params": [a]}, {"params": [b]}], lr=1e-3)
    assert opt.flat_param.numel() == 7


def test_zero_grad_never_drops_the_views():
    opt, params = make_flat_adam([torch.ones(3), torch.ones(2, 2)], PLAIN)
    ptrs = [p.grad.data_ptr() for p in params]
    params[0].grad.fill_(3.0)
    opt.zero_grad(set_to_none=True)
    assert [p.grad.data_ptr() for p in params] == ptrs
    assert not opt.flat_grad.any()
    (params[0].sum() * 2 + params[1].sum()).backward()
    assert opt.flat_grad.tolist() == [2.0] * 3 + [1.0] * 4
    params[1].grad = None
    with pytest.raises(RuntimeError, match="flat_grad"):
        opt.step()


def test_loss_scale_plan():
    from esr_amd.engine.trainer import loss_scale_plan
    on = {"enabled": True, "init_scale": 1024.0}
    cfg = lambda name, ls: {"optimizer": {"name": name},  # noqa: E731
                            **({"loss_scale": ls} if ls is not None else {})}
    assert loss_scale_plan(cfg("Adam", None), True) == ("off", None)
    assert loss_scale_plan(cfg("FlatAdam", {"enabled": False}), True) \
        == ("off", None)
    assert loss_scale_plan(cfg("FlatAdam", on), True) \
        == ("flat", {"init_scale": 1024.0})
    assert loss_scale_plan(cfg("FlatAdamW", on), False)[0] == "flat"
    assert loss_scale_plan(cfg("Adam", on), False) \
        == ("grad_scaler", {"init_scale": 1024.0})
    with pytest.raises(ValueError, match="FlatAdam"):
        loss_scale_plan(cfg("Adam", on), True)
    with pytest.raises(ValueError, match="unknown loss_scale"):
        loss_scale_plan(cfg("FlatAdam", {"enabled": True, "bogus": 1}), True)


def _cpu_train(tmp_path, synth_datalist, run_id, opt_name, resume=None):
    from test_engine import _train_config
    from esr_amd.config import ConfigParser
    from esr_amd.engine import build_training
    from esr_amd.utils.logging import setup_logging
    cfg = _train_config(synth_datalist, tmp_path / f"out_{run_id}")
    cfg["optimizer"] = {"name": opt_name, "args": {"lr": 1e-3}}
    cfg["loss_scale"] = {"enabled": True, "init_scale": 1024.0}
    cfg["valid_dataloader"] = None
    cfg["trainer"]["monitor"] = "off"
    parser = ConfigParser(cfg, run_id=run_id)
    trainer = build_training(parser, torch.device("cpu"),
                             setup_logging(f"ls-{run_id}", None),
                             resume=resume)
    return parser, trainer


@pytest.mark.parametrize("opt_name", ["FlatAdam", "Adam"])
def test_trainer_eager_loss_scaling_and_resume(tmp_path, synth_datalist,
                                               opt_name):
    """Eager trainer: FlatAdam scales on its own, any other optimizer goes
    through torch.amp.GradScaler; both checkpoint the scaler state."""
    parser, trainer = _cpu_train(tmp_path, synth_datalist, "a", opt_name)
    assert (trainer.grad_scaler is None) == (opt_name == "FlatAdam")
    trainer.train()
    avg = trainer.train_metrics.avg("train_loss")
    assert math.isfinite(avg) and avg > 0
    scale, skipped = trainer.loss_scale_stats()
    assert scale == 1024.0
    ckpt = sorted(parser.save_dir.glob("checkpoint-iteration*.pth"))[-1]
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    if opt_name == "FlatAdam":
        assert skipped == 0 and trainer.optimizer.step_count == 2
        assert saved["optimizer"]["states"]["loss_scale"]["scale"] == 1024.0
        saved["optimizer"]["states"]["loss_scale"]["scale"] = 512.0
    else:
        assert saved["optimizer"]["grad_scaler"]["scale"] == 1024.0
        saved["optimizer"]["grad_scaler"]["scale"] = 512.0
    torch.save(saved, ckpt)
    _, resumed = _cpu_train(tmp_path, synth_datalist, "b", opt_name,
                            resume=str(ckpt))
    assert resumed.loss_scale_stats()[0] == 512.0
    if opt_name == "FlatAdam":
        assert resumed.optimizer.step_count == 2


def _run_flat_sync(rank, port, q):
    """Un-wrapped model + FlatAdam on two ranks: the flat gradient is
    averaged, and one rank's inf makes BOTH ranks skip the step."""
    import torch.distributed as dist
    from test_distributed import _init
    try:
        _init(rank, port)
        from esr_amd.engine.trainer import Trainer
        from esr_amd.optim import FlatAdam
        w = torch.nn.Parameter(torch.ones(6))
        opt = FlatAdam([w], lr=LR, loss_scale={"init_scale": 4.0})

        class _T:  # minimal Trainer stand-in
            pass
        t = _T()
        t.model, t.optimizer = torch.nn.ParameterList([w]), opt
        opt.flat_grad.fill_(float(rank + 1))
        Trainer._sync_grads_if_needed(t)
        mean = opt.flat_grad.tolist()
        if rank == 1:
            opt.flat_grad[2] = float("inf")
        Trainer._sync_grads_if_needed(t)
        opt.step()
        q.put((rank, (mean, opt.skipped_steps, opt.step_count,
                      opt.loss_scale_value)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(400)
def test_flat_grad_sync_and_joint_skip_across_ranks():
    from test_distributed import _spawn
    res = _spawn(_run_flat_sync, 29533)
    for rank in (0, 1):
        assert res[rank][0] == ([1.5] * 6, 1, 0, 2.0)
