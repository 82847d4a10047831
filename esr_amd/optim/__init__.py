"""Optimizers, and what the engine may ask of any optimizer.

The engine works with every ``torch.optim.Optimizer``.  An optimizer opts
in to more by offering an attribute; the functions below are the only
places that look for one.
"""

import torch

from .flat_adam import LOSS_SCALE_DEFAULTS, FlatAdam, FlatAdamW

__all__ = ["FlatAdam", "FlatAdamW", "LOSS_SCALE_DEFAULTS", "flat_grad_of",
           "scale_loss", "sync_lr", "loss_scale_stats", "grad_clip_stats",
           "snapshot_optimizer",
           "restore_optimizer"]


def flat_grad_of(opt):
    """``opt.flat_grad``: the one buffer every ``p.grad`` is a view of, for
    a single all-reduce; None when the optimizer has no such buffer."""
    return getattr(opt, "flat_grad", None)


def scale_loss(opt, loss):
    """``opt.scale_loss(loss)``: the loss to run backward on when the
    optimizer scales (and un-scales) on its own; otherwise `loss`."""
    fn = getattr(opt, "scale_loss", None)
    return fn(loss) if fn is not None else loss


def sync_lr(opt):
    """``opt.sync_lr()``: refresh a device-side learning rate before a graph
    replay; nothing for optimizers that read ``lr`` on the host."""
    fn = getattr(opt, "sync_lr", None)
    if fn is not None:
        fn()


def loss_scale_stats(opt, grad_scaler=None):
    """(loss scale, skipped steps or None) from ``opt.loss_scaling`` with
    ``loss_scale_value`` / ``skipped_steps``, else from `grad_scaler`; None
    when nobody scales.  Reading synchronizes with the device."""
    if getattr(opt, "loss_scaling", False):
        return opt.loss_scale_value, opt.skipped_steps
    if grad_scaler is not None:
        return grad_scaler.get_scale(), None
    return None


def grad_clip_stats(opt):
    """(un-scaled gradient norm of the last step, clipped steps) from
    ``opt.max_grad_norm`` with ``grad_norm_value`` / ``clipped_steps``; None
    when the optimizer does not clip.  Reading synchronizes with the
    device."""
    if getattr(opt, "max_grad_norm", None) is None:
        return None
    return opt.grad_norm_value, opt.clipped_steps


def _state_tensors(opt):
    """``opt.state_buffers()`` where state lives outside ``opt.state``,
    else the tensors in ``opt.state``."""
    buffers = getattr(opt, "state_buffers", None)
    if buffers is not None:
        return list(buffers())
    return [v for s in opt.state.values() for v in s.values()
            if torch.is_tensor(v)]


def snapshot_optimizer(opt):
    """Copies of the parameters and of every state tensor that exists now,
    each paired with the live tensor, for `restore_optimizer`."""
    params = [p for g in opt.param_groups for p in g["params"]]
    return [(t, t.detach().clone()) for t in params + _state_tensors(opt)]


@torch.no_grad()
def restore_optimizer(opt, snap):
    """Undo the steps taken since `snapshot_optimizer`, in place so every
    tensor keeps its address: snapshotted tensors get their values back,
    state tensors created since are zeroed (= never stepped)."""
    known = set()
    for t, saved in snap:
        t.copy_(saved)
        known.add(id(t))
    for t in _state_tensors(opt):
        if id(t) not in known:
            t.zero_()
