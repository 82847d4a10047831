"""hipGraph-captured BPTT training step.

The flagship model is launch-latency-bound on MI355X (1.8 M params,
~130 kernels per window); capturing the whole BPTT optimizer step (all
sliding windows forward + one backward + gradient all-reduce + Adam) in a
hipGraph and replaying it cuts the step time ~2x (see profiles/README.md).

Used by the Trainer when ``trainer.hip_graphs`` is enabled (GPU, fixed
shapes) and by bench.py.  In distributed mode the model must NOT be
DDP-wrapped — gradients live in one flat buffer that is all-reduced with a
single RCCL call inside the graph (xGMI collectives on this model's few-MB
gradients are latency-bound, so one fused call is the right shape —
SURVEY §2.4).

With FlatAdam/FlatAdamW (esr_amd/optim) the optimizer's own flat gradient is
the all-reduced buffer, the backward runs on ``optimizer.scale_loss(loss)``
and the overflow skip / scale update are device-side parts of the captured
step; the learning rate is a device scalar refreshed before each replay.
Gradient-norm clipping is part of FlatAdam's step too; for any other
optimizer `max_grad_norm` clips the flat gradient with three torch ops
inside the captured step (step.py: `clip_flat_grad_`).

The step body itself is step.py's, shared with the eager trainer; the
warm-up / roll-back / capture sequence is capture.py's `capture_graph`, and
the roll-back rule (esr_amd.optim.restore_optimizer) is the same for every
optimizer: what existed before warm-up gets its values back, what warm-up
created is zeroed.
"""

from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn.functional as F

from ..optim import restore_optimizer, snapshot_optimizer, sync_lr
from .capture import amp_autocast, capture_graph
from .step import backward_and_step, bptt_loss

__all__ = ["GraphedBPTTStep", "flatten_grads"]


def flatten_grads(params, device, dtype=torch.float32):
    """Point every param's .grad into one flat buffer; returns the buffer."""
    total = sum(p.numel() for p in params)
    flat = torch.zeros(total, device=device, dtype=dtype)
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return flat


class GraphedBPTTStep:
    """Records one BPTT optimizer step (step.py: `bptt_loss` over all
    windows, then `backward_and_step` with the flat-gradient all-reduce as
    its sync) on static I/O buffers into a replayable hipGraph."""

    def __init__(self, model, optimizer, flat_grad, n_windows,
                 inp_shape, gt_shape, device, amp_dtype=None,
                 world_size: int = 1, warmup: int = 3,
                 sequence: bool = False, seqn: int = 3,
                 max_grad_norm=None):
        self.model = model
        self.optimizer = optimizer
        self.flat_grad = flat_grad
        self.device = device
        self.amp_dtype = amp_dtype
        self.world = world_size
        self.sequence = sequence
        self.seqn = seqn
        # only for optimizers that do not clip on their own
        self.max_grad_norm = max_grad_norm
        self.static_grad_norm = None
        # sequence: one inp_shape = [B, L, C, H, W] frames tensor and one
        # gt_shape = [B, n_windows, C, H, W]; otherwise one pair per window
        n_bufs = 1 if sequence else n_windows
        self.static_in = [torch.zeros(inp_shape, device=device)
                          for _ in range(n_bufs)]
        self.static_gt = [torch.zeros(gt_shape, device=device)
                          for _ in range(n_bufs)]
        self.graph = None
        self.static_loss = None
        self._warmup = warmup

    def _all_reduce(self):
        if self.world > 1:
            dist.all_reduce(self.flat_grad)
            self.flat_grad.div_(self.world)

    def _body(self):
        self.flat_grad.zero_()
        inputs, gts = (self.static_in[0], self.static_gt[0]) \
            if self.sequence else (self.static_in, self.static_gt)
        loss, mse, _ = bptt_loss(
            self.model, inputs, gts, sequence=self.sequence, seqn=self.seqn,
            autocast=amp_autocast(self.amp_dtype, self.device,
                                  cache_enabled=False),
            loss_fn=F.mse_loss)
        # the last assignment is the capture's: the replays' static output
        self.static_grad_norm = backward_and_step(
            loss, self.optimizer, self._all_reduce,
            max_grad_norm=self.max_grad_norm, flat_grad=self.flat_grad)
        return loss, mse

    def capture(self):
        # the warm-up runs initialize MIOpen plans, autograd allocations and
        # the capturable optimizer's state TENSORS, but their optimizer
        # steps on garbage data are real (and may overflow and back a loss
        # scale off): snapshot first, roll back before recording
        snap = snapshot_optimizer(self.optimizer)
        self.graph, (self.static_loss, self.static_mse) = capture_graph(
            self._body, warmup=self._warmup,
            after_warmup=lambda: restore_optimizer(self.optimizer, snap))
        return self

    def run(self, window_inputs, window_gts):
        """Copy inputs into the static buffers (H2D if needed) and replay."""
        for si, sg, inp, gt in zip(self.static_in, self.static_gt,
                                   window_inputs, window_gts):
            si.copy_(inp, non_blocking=True)
            sg.copy_(gt, non_blocking=True)
        # FlatAdam's lr is a device scalar read by the captured step
        sync_lr(self.optimizer)
        self.graph.replay()
        return self.static_loss, self.static_mse
