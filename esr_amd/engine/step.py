"""The BPTT optimizer step, written once.

`Trainer.bptt_step` runs it eagerly on a batch it has moved to the device;
`GraphedBPTTStep` records the same two calls on its static buffers.
Everything here is capture-safe: the only branches are on host-side shapes.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from ..optim import scale_loss
from .capture import unwrap

__all__ = ["bptt_loss", "backward_and_step", "clip_flat_grad_"]


def bptt_loss(model, inputs, gts, *, sequence, seqn, autocast, loss_fn):
    """Loss summed over the sliding windows of one sequence, through the
    persistent recurrent state (parity: ESR:train_ours_cnt_seq.py:210-235).

    ``sequence=True`` is the shared-encoder path: `inputs` is one frames
    tensor [B, L, C, H, W] and `gts` one [B, n_windows, C, kH, kW] tensor;
    it calls ``forward_sequence`` on the module under any DDP wrapper.
    Otherwise `inputs` and `gts` are per-window lists and `model` itself
    (the wrapper, if there is one) is called.  The forward runs under the
    `autocast` context, the MSE in fp32.

    Returns ``(loss, last window's mse, last window's prediction)``.
    """
    inner = unwrap(model)
    inner.reset_states()
    loss = 0
    mse = pred = None
    if sequence:
        with autocast:
            preds = inner.forward_sequence(inputs, seqn)
        for w, pred in enumerate(preds):
            mse = loss_fn(pred.float(), gts[:, w].float())
            loss = loss + mse
    else:
        for inp, gt in zip(inputs, gts):
            with autocast:
                pred = model(inp)
                if pred.shape[-2:] != gt.shape[-2:]:
                    pred = F.interpolate(pred, size=gt.shape[-2:],
                                         mode="bicubic", align_corners=False)
            mse = loss_fn(pred.float(), gt.float())
            loss = loss + mse
    return loss, mse, pred


def clip_flat_grad_(flat_grad, max_norm):
    """``clip_grad_norm_`` on one flat gradient buffer as three
    capture-safe ops (norm, coefficient clamped to 1, multiply) instead of
    the per-tensor foreach chain.  Returns the norm before clipping."""
    norm = torch.linalg.vector_norm(flat_grad)
    coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
    flat_grad.mul_(coef)
    return norm


def backward_and_step(loss, optimizer, sync, grad_scaler=None,
                      max_grad_norm=None, flat_grad=None):
    """Backward on the scaled loss, `sync()` the gradients across ranks,
    optimizer step.  The scaled loss only drives the backward; callers log
    and return the un-scaled one.  `sync` stays in front of the optimizer:
    an inf/NaN survives the sum, so every rank takes the same skip
    decision.

    `max_grad_norm` clips the synchronized (and, with a `grad_scaler`,
    un-scaled) gradient for optimizers that do not clip on their own:
    `flat_grad`, when the caller owns one buffer all the ``.grad`` are views
    of, with `clip_flat_grad_`, otherwise with
    ``torch.nn.utils.clip_grad_norm_``.  Every rank clips the same
    all-reduced gradient, so no further communication is needed.  Returns
    the norm before clipping (a tensor), None when nothing was clipped
    here."""
    def clip():
        if max_grad_norm is None:
            return None
        if flat_grad is not None:
            return clip_flat_grad_(flat_grad, max_grad_norm)
        params = [p for g in optimizer.param_groups for p in g["params"]]
        return torch.nn.utils.clip_grad_norm_(params, max_grad_norm)

    if grad_scaler is not None:
        grad_scaler.scale(loss).backward()
        sync()
        if max_grad_norm is not None:
            grad_scaler.unscale_(optimizer)
        norm = clip()
        grad_scaler.step(optimizer)
        grad_scaler.update()
    else:
        scale_loss(optimizer, loss).backward()
        sync()
        norm = clip()
        optimizer.step()
    return norm
