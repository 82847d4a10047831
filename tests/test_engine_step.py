"""The shared BPTT step body (engine/step.py) against a spelled-out loop, and
the warm-up roll-back rule of esr_amd.optim (CPU)."""

import pytest
import torch
import torch.nn.functional as F

from esr_amd.optim import FlatAdam, restore_optimizer, snapshot_optimizer

MODEL_ARGS = {"inch": 2, "basech": 4, "num_frame": 3}
SEQN, FRAMES, SIZE, STEPS = 3, 4, 32, 3
MID = (SEQN - 1) // 2


# ---- 1./2. step body ----

def _data(kind, gt_size=SIZE, steps=STEPS):
    """`steps` batches of one 4-frame sequence, as the per-window list or
    the shared dict the two collate modes hand the trainer."""
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(steps):
        frames = torch.rand(1, FRAMES, 2, SIZE, SIZE, generator=g)
        gt = torch.rand(1, FRAMES, 2, gt_size, gt_size, generator=g)
        if kind == "shared":
            batches.append({"frames": frames, "seqn": SEQN,
                            "gt_mids": gt[:, MID:MID + FRAMES - SEQN + 1]})
        else:
            batches.append([{"inp_scaled_cnt": frames[:, w:w + SEQN],
                             "gt_cnt": gt[:, w:w + SEQN]}
                            for w in range(FRAMES - SEQN + 1)])
    return batches


def _trainer(tmp_path, synth_datalist, opt_name):
    from test_engine import _train_config
    from esr_amd.config import ConfigParser
    from esr_amd.engine import build_training
    from esr_amd.utils.logging import setup_logging
    cfg = _train_config(synth_datalist, tmp_path / "out")
    cfg["model"]["args"] = dict(MODEL_ARGS)
    cfg["optimizer"] = {"name": opt_name, "args": {"lr": 1e-3}}
    if opt_name == "FlatAdam":
        cfg["loss_scale"] = {"enabled": True, "init_scale": 1024}
    cfg["valid_dataloader"] = None
    cfg["trainer"]["monitor"] = "off"
    torch.manual_seed(0)
    return build_training(ConfigParser(cfg, run_id="step"),
                          torch.device("cpu"), setup_logging("step", None))


def _plain_twin(trainer, opt_name):
    """A second model with the trainer's initial weights and an optimizer
    of its own, built by hand."""
    from esr_amd.models import build_model
    model = build_model("ESRNet", **MODEL_ARGS)
    model.load_state_dict(trainer.model.state_dict())
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    if opt_name == "FlatAdam":
        return model, FlatAdam(params, lr=1e-3,
                               loss_scale={"init_scale": 1024})
    return model, torch.optim.Adam(params, lr=1e-3)


def _plain_list_step(model, opt, windows, scaled):
    opt.zero_grad(set_to_none=True)
    model.reset_states()
    loss = 0
    for win in windows:
        pred = model(win["inp_scaled_cnt"])
        gt = win["gt_cnt"][:, MID]
        if pred.shape[-2:] != gt.shape[-2:]:
            pred = F.interpolate(pred, size=gt.shape[-2:], mode="bicubic",
                                 align_corners=False)
        mse = F.mse_loss(pred, gt)
        loss = loss + mse
    (opt.scale_loss(loss) if scaled else loss).backward()
    opt.step()
    return loss.detach(), mse.detach()


def _plain_shared_step(model, opt, batch, scaled):
    opt.zero_grad(set_to_none=True)
    model.reset_states()
    loss = 0
    preds = model.forward_sequence(batch["frames"], batch["seqn"])
    for w, pred in enumerate(preds):
        mse = F.mse_loss(pred, batch["gt_mids"][:, w])
        loss = loss + mse
    (opt.scale_loss(loss) if scaled else loss).backward()
    opt.step()
    return loss.detach(), mse.detach()


def _compare(trainer, opt_name, kind, batches):
    model, opt = _plain_twin(trainer, opt_name)
    plain = _plain_shared_step if kind == "shared" else _plain_list_step
    trainer.model.train()
    for batch in batches:
        loss, mse, _ = trainer.bptt_step(batch, train=True)
        want_loss, want_mse = plain(model, opt, batch, opt_name == "FlatAdam")
        assert torch.isfinite(loss)
        assert torch.equal(loss, want_loss)
        assert torch.equal(mse, want_mse)
    got = list(trainer.model.parameters())
    want = list(model.parameters())
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a.detach(), b.detach())
    if opt_name == "FlatAdam":
        assert trainer.optimizer.step_count == len(batches) == opt.step_count
        assert trainer.loss_scale_stats() == (1024.0, 0)


@pytest.mark.parametrize("opt_name", ["Adam", "FlatAdam"])
@pytest.mark.parametrize("kind", ["list", "shared"])
def test_bptt_step_equals_spelled_out_loop(tmp_path, synth_datalist, kind,
                                           opt_name):
    trainer = _trainer(tmp_path, synth_datalist, opt_name)
    before = [p.detach().clone() for p in trainer.model.parameters()]
    _compare(trainer, opt_name, kind, _data(kind))
    assert any(not torch.equal(p.detach(), b)
               for p, b in zip(trainer.model.parameters(), before))


def test_validation_runs_the_loss_only(tmp_path, synth_datalist):
    trainer = _trainer(tmp_path, synth_datalist, "Adam")
    before = [p.detach().clone() for p in trainer.model.parameters()]
    batch = _data("list", steps=1)[0]
    with torch.no_grad():
        loss, mse, pred = trainer.bptt_step(batch, train=False)
    assert torch.isfinite(loss) and pred.shape == (1, 2, SIZE, SIZE)
    assert not trainer.optimizer.state
    for p, b in zip(trainer.model.parameters(), before):
        assert torch.equal(p.detach(), b)


def test_per_window_path_resizes_pred_to_gt(tmp_path, synth_datalist):
    """A ground truth 2 pixels larger than the prediction: bicubic resize,
    as the spelled-out loop does it."""
    trainer = _trainer(tmp_path, synth_datalist, "Adam")
    batches = _data("list", gt_size=SIZE + 2)
    assert batches[0][0]["gt_cnt"].shape[-1] == SIZE + 2
    trainer.model.reset_states()
    with torch.no_grad():
        assert trainer.model(batches[0][0]["inp_scaled_cnt"]).shape[-1] == SIZE
    _compare(trainer, "Adam", "list", batches)


# ---- 3. roll-back rule ----

SHAPES = [(3,), (2, 5), (67,)]


def _optimizer(name):
    g = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(s, generator=g))
              for s in SHAPES]
    if name == "Adam":
        opt = torch.optim.Adam(params, lr=1e-2, amsgrad=True)
    else:
        opt = FlatAdam(params, lr=1e-2, amsgrad=True,
                       loss_scale={"init_scale": 1024})
    return opt, params, g


def _step(opt, params, g, n, overflow=False):
    for k in range(n):
        for p in params:
            grad = torch.randn(p.shape, generator=g)
            if isinstance(opt, FlatAdam):
                p.grad.copy_(grad)
            else:
                p.grad = grad
        if overflow and k == 1 and isinstance(opt, FlatAdam):
            opt.flat_grad[4] = float("inf")     # backs the scale off
        opt.step()


def _state(opt):
    if isinstance(opt, FlatAdam):
        return opt.state_buffers()
    return [v for s in opt.state.values() for v in s.values()
            if torch.is_tensor(v)]


def _bits(tensors):
    return [t.detach().clone() for t in tensors]


def _assert_bit_equal(now, then):
    assert len(now) == len(then)
    for a, b in zip(now, then):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("name", ["Adam", "FlatAdam"])
def test_rollback_of_a_fresh_optimizer(name):
    opt, params, g = _optimizer(name)
    params0, state0 = _bits(params), _bits(_state(opt))
    snap = snapshot_optimizer(opt)
    _step(opt, params, g, 3, overflow=True)
    assert any(not torch.equal(p.detach(), b) for p, b in zip(params, params0))
    restore_optimizer(opt, snap)
    _assert_bit_equal(params, params0)
    if name == "Adam":
        # created by the warm-up: zeroed, i.e. never stepped
        assert len(_state(opt)) == 4 * len(SHAPES)
        assert not any(t.any() for t in _state(opt))
    else:
        _assert_bit_equal(_state(opt), state0)
        assert (opt.loss_scale_value, opt.step_count, opt.skipped_steps) \
            == (1024.0, 0, 0)


@pytest.mark.parametrize("name", ["Adam", "FlatAdam"])
def test_rollback_keeps_the_state_of_a_stepped_optimizer(name):
    """Two steps first, as a run resumed from a checkpoint would bring:
    moments, step and parameters come back as they were after them."""
    opt, params, g = _optimizer(name)
    _step(opt, params, g, 2)
    params2, state2 = _bits(params), _bits(_state(opt))
    assert any(t.any() for t in state2)
    snap = snapshot_optimizer(opt)
    _step(opt, params, g, 3, overflow=True)
    assert any(not torch.equal(a, b) for a, b in zip(_state(opt), state2))
    restore_optimizer(opt, snap)
    _assert_bit_equal(params, params2)
    _assert_bit_equal(_state(opt), state2)
    if name == "Adam":
        assert all(float(s["step"]) == 2 for s in opt.state.values())
    else:
        assert opt.step_count == 2 and opt.skipped_steps == 0


@pytest.mark.parametrize("name", ["Adam", "FlatAdam"])
@pytest.mark.parametrize("pre_steps", [0, 2])
def test_rollback_keeps_every_address(name, pre_steps):
    opt, params, g = _optimizer(name)
    _step(opt, params, g, pre_steps)
    snap = snapshot_optimizer(opt)
    _step(opt, params, g, 3)
    ptrs = [t.data_ptr() for t in _state(opt) + params]
    restore_optimizer(opt, snap)
    assert [t.data_ptr() for t in _state(opt) + params] == ptrs
