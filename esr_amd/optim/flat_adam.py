"""FlatAdam: Adam/AdamW over one flat fp32 buffer with capture-safe dynamic
loss scaling.

Parameters, gradients and the Adam moments live in flat contiguous fp32
buffers; every ``p.data`` / ``p.grad`` is a view into them.  One optimizer
step is at most three HIP launches (esr_amd/ops/native/src/flat_adam.hip)
independent of the number of parameter tensors:

    flat_grad_finite_check   (only with loss scaling)
    flat_adam_step           un-scale + Adam/AdamW, no-op on overflow
    flat_scale_update        GradScaler scale/tracker + step counter

With ``max_grad_norm`` the gradient's global L2 norm is clipped as
``torch.nn.utils.clip_grad_norm_`` would, on the un-scaled gradient and
inside the same phase (four launches): ``flat_grad_stats`` replaces the
finite check (it does both jobs in one pass over the gradient and then
finishes the norm in one block), and the step kernel multiplies by the
coefficient.

The skip decision, the loss scale, the clip coefficient, the step count and
the learning rate are device scalars, so the whole step records into a
hipGraph and a replay honours ``param_groups[0]['lr']`` changes made by an
lr scheduler (the host writes the device scalar outside the captured region,
see ``sync_lr``).

On CPU tensors ``step()`` runs a pure-torch implementation of the same
semantics (the CPU oracle, as elsewhere in ``ops/``).  On GPU tensors the
HIP extension is required.

Call ``model.to(device)`` BEFORE constructing the optimizer: moving the
model afterwards re-allocates the parameters and detaches them from the
flat buffers.
"""

from __future__ import annotations

import math

import torch
from torch.optim import Optimizer

__all__ = ["FlatAdam", "FlatAdamW", "LOSS_SCALE_DEFAULTS", "STATE_SIZE",
           "CLIP_SIZE"]

# torch.amp.GradScaler's defaults
LOSS_SCALE_DEFAULTS = {"init_scale": 65536.0, "growth_factor": 2.0,
                       "backoff_factor": 0.5, "growth_interval": 2000}

# device state layout (fp32; must match flat_adam.hip)
SCALE, TRACKER, FOUND_INF, STEP, LR, SKIPPED, BC1, BC2_SQRT = range(8)
STATE_SIZE = 8
# clip scalars, a tensor of their own (fp32; must match flat_adam.hip)
GRAD_NORM, CLIP_COEF, CLIPPED = range(3)
CLIP_SIZE = 3
# launch geometry of the flat kernels (esr_common.h): 256 threads x float4,
# at most 2048 blocks; the stats pass leaves one fp64 partial per block
_ELEMS_PER_BLOCK, _MAX_BLOCKS = 1024, 2048

_HYPER_KEYS = ("lr", "betas", "eps", "weight_decay", "amsgrad",
               "decoupled_weight_decay")


def _resolve_loss_scale(loss_scale):
    """None / {'enabled': False} -> None; otherwise the four GradScaler
    knobs with defaults filled in."""
    if loss_scale is None:
        return None
    cfg = dict(loss_scale)
    if not cfg.pop("enabled", True):
        return None
    unknown = set(cfg) - set(LOSS_SCALE_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown loss_scale keys {sorted(unknown)}; "
                         f"known: {sorted(LOSS_SCALE_DEFAULTS)}")
    out = dict(LOSS_SCALE_DEFAULTS)
    out.update(cfg)
    out["init_scale"] = float(out["init_scale"])
    out["growth_factor"] = float(out["growth_factor"])
    out["backoff_factor"] = float(out["backoff_factor"])
    out["growth_interval"] = int(out["growth_interval"])
    if out["init_scale"] <= 0 or out["growth_factor"] < 1.0 \
            or not 0.0 < out["backoff_factor"] <= 1.0 \
            or out["growth_interval"] < 1:
        raise ValueError(f"invalid loss_scale settings {out}")
    return out


class FlatAdam(Optimizer):
    """torch.optim.Adam semantics (``decoupled=True``: AdamW) on flat
    buffers, with optional device-side dynamic loss scaling.

    ``loss_scale`` is None (off) or a dict with any of ``init_scale``,
    ``growth_factor``, ``backoff_factor``, ``growth_interval``.
    One set of hyper-parameters applies to all params.

    ``max_grad_norm`` is None (off) or the L2 norm the un-scaled gradient is
    clipped to before each step (``clip_grad_norm_``'s formula; weight decay
    is added after clipping).  It is fixed at construction and baked into a
    captured graph.  With clipping on, a non-finite gradient skips the step
    whether or not the loss is scaled.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, amsgrad=False, decoupled=False,
                 loss_scale=None, max_grad_norm=None):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
                raise ValueError(f"max_grad_norm must be positive and "
                                 f"finite, got {max_grad_norm}")
        if lr < 0 or eps < 0 or weight_decay < 0 \
                or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("invalid FlatAdam hyper-parameters")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps,
                        weight_decay=weight_decay, amsgrad=bool(amsgrad),
                        decoupled_weight_decay=bool(decoupled))
        super().__init__(params, defaults)
        g0 = self.param_groups[0]
        for g in self.param_groups[1:]:
            for k in _HYPER_KEYS:
                if g[k] != g0[k]:
                    raise ValueError(
                        f"FlatAdam applies one set of hyper-parameters to "
                        f"all params; param groups disagree on '{k}' "
                        f"({g0[k]} vs {g[k]})")
        self._params = [p for g in self.param_groups for p in g["params"]]
        if not self._params:
            raise ValueError("FlatAdam got an empty parameter list")
        device = self._params[0].device
        for p in self._params:
            if p.device != device or p.dtype != torch.float32:
                raise ValueError("FlatAdam needs fp32 params on one device")
        self._ls = _resolve_loss_scale(loss_scale)

        self._offsets = []
        total = 0
        for p in self._params:
            self._offsets.append(total)
            total += p.numel()
        self._numel = total
        z = lambda: torch.zeros(total, device=device,  # noqa: E731
                                dtype=torch.float32)
        self.flat_param, self.flat_grad = z(), z()
        self.exp_avg, self.exp_avg_sq = z(), z()
        self.max_exp_avg_sq = z() if g0["amsgrad"] else None
        with torch.no_grad():
            for p, v in zip(self._params, self._views(self.flat_param)):
                v.copy_(p.data)
                p.data = v
            for p, v in zip(self._params, self._views(self.flat_grad)):
                if p.grad is not None:
                    v.copy_(p.grad)
                p.grad = v
        self._grad_ptrs = [p.grad.data_ptr() for p in self._params]

        self._state = torch.zeros(STATE_SIZE, device=device,
                                  dtype=torch.float32)
        self._max_norm = max_grad_norm
        self._clip = self._partials = None
        if max_grad_norm is not None:
            self._clip = torch.zeros(CLIP_SIZE, device=device,
                                     dtype=torch.float32)
            if device.type == "cuda":  # scratch of the stats pass
                blocks = min(-(-total // _ELEMS_PER_BLOCK), _MAX_BLOCKS)
                self._partials = torch.zeros(max(blocks, 1), device=device,
                                             dtype=torch.float64)
        self._lr_written = None
        self._write_state(scale=self._ls["init_scale"] if self._ls else 1.0,
                          tracker=0, step=0, skipped=0)
        self.sync_lr()

    # ---------------- buffers / device state ----------------

    def _views(self, flat):
        return [flat[o:o + p.numel()].view_as(p)
                for p, o in zip(self._params, self._offsets)]

    def _bias_corrections(self, next_step: int):
        b1, b2 = self.param_groups[0]["betas"]
        return 1.0 - b1 ** next_step, math.sqrt(1.0 - b2 ** next_step)

    def _write_state(self, scale, tracker, step, skipped):
        """Host-side (re)initialisation of the device scalars, in place."""
        bc1, bc2s = self._bias_corrections(int(step) + 1)
        lr = float(self.param_groups[0]["lr"])
        vals = [0.0] * STATE_SIZE
        vals[SCALE], vals[TRACKER], vals[STEP] = scale, tracker, step
        vals[LR], vals[SKIPPED], vals[BC1], vals[BC2_SQRT] = \
            lr, skipped, bc1, bc2s
        self._state.copy_(torch.tensor(vals, dtype=torch.float32))
        self._lr_written = lr

    def sync_lr(self):
        """Write ``param_groups[0]['lr']`` into the device scalar if it
        changed since the last write.  A tiny host-ordered write that must
        stay outside a captured region (GraphedBPTTStep.run calls it before
        each replay)."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_written:
            self._state[LR].fill_(lr)
            self._lr_written = lr

    @property
    def loss_scaling(self) -> bool:
        return self._ls is not None

    @property
    def device_state(self) -> torch.Tensor:
        """The fp32 device scalars (scale, tracker, found_inf, step, lr,
        skipped, bias corrections); snapshot/restore with clone()/copy_()."""
        return self._state

    def state_buffers(self):
        """Every tensor a step writes besides the parameters: the device
        scalars, the moments and, with clipping, the clip scalars
        (esr_amd.optim.snapshot_optimizer)."""
        bufs = [self._state, self.exp_avg, self.exp_avg_sq]
        if self.max_exp_avg_sq is not None:
            bufs.append(self.max_exp_avg_sq)
        if self._clip is not None:
            bufs.append(self._clip)
        return bufs

    @property
    def max_grad_norm(self):
        """The clipping threshold, None when clipping is off."""
        return self._max_norm

    @property
    def clip_state(self):
        """The fp32 clip scalars (grad norm, clip coefficient, clipped
        steps) on the device; None when clipping is off."""
        return self._clip

    # reading these synchronizes: logging cadence only
    @property
    def loss_scale_value(self) -> float:
        return float(self._state[SCALE])

    @property
    def skipped_steps(self) -> int:
        return int(self._state[SKIPPED])

    @property
    def step_count(self) -> int:
        return int(self._state[STEP])

    @property
    def growth_tracker(self) -> int:
        return int(self._state[TRACKER])

    # the clip scalars; None when clipping is off
    @property
    def grad_norm_value(self):
        """Un-scaled L2 norm of the last step's gradient."""
        return None if self._clip is None else float(self._clip[GRAD_NORM])

    @property
    def clip_coef_value(self):
        return None if self._clip is None else float(self._clip[CLIP_COEF])

    @property
    def clipped_steps(self):
        return None if self._clip is None else int(self._clip[CLIPPED])

    def scale_loss(self, loss):
        """loss * scale as a device-scalar multiply (capture-safe); the loss
        itself when scaling is off."""
        if self._ls is None:
            return loss
        return loss * self._state[SCALE]

    def zero_grad(self, set_to_none: bool = False):
        """Always zeroes the flat gradient in place; the .grad views are
        never dropped (captured graphs hold their addresses)."""
        self.flat_grad.zero_()

    # ---------------- step ----------------

    def _check_grad_views(self):
        for p, ptr in zip(self._params, self._grad_ptrs):
            if p.grad is None or p.grad.data_ptr() != ptr:
                raise RuntimeError(
                    "FlatAdam: a parameter's .grad no longer points into "
                    "flat_grad (was it set to None or re-assigned?)")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_grad_views()
        if self.flat_param.is_cuda:
            if not torch.cuda.is_current_stream_capturing():
                self.sync_lr()
            self._step_native()
        else:
            self.sync_lr()
            self._step_torch()
        return loss

    def _step_native(self):
        from ..ops.native import require_ext
        ext = require_ext()
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        ls = self._ls
        if self._clip is not None:
            # finite check and norm in one pass, with or without scaling
            ext.flat_grad_stats(self.flat_grad, self._state, self._partials,
                                self._clip, self._max_norm)
            ext.flat_adam_step_clipped(
                self.flat_param, self.flat_grad, self.exp_avg,
                self.exp_avg_sq, self.max_exp_avg_sq, self._state,
                self._clip, b1, b2, g["eps"], g["weight_decay"],
                g["decoupled_weight_decay"])
        else:
            if ls is not None:
                ext.flat_grad_finite_check(self.flat_grad, self._state)
            ext.flat_adam_step(self.flat_param, self.flat_grad, self.exp_avg,
                               self.exp_avg_sq, self.max_exp_avg_sq,
                               self._state, b1, b2, g["eps"],
                               g["weight_decay"],
                               g["decoupled_weight_decay"])
        ext.flat_scale_update(
            self._state, ls is not None,
            ls["growth_factor"] if ls else 1.0,
            ls["backoff_factor"] if ls else 1.0,
            ls["growth_interval"] if ls else 1, b1, b2)

    def _step_torch(self):
        """Same semantics as the kernels in plain torch ops (fp32, same
        operation order; the norm in fp64)."""
        st = self._state
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        f32 = lambda x: torch.tensor(x, dtype=torch.float32,  # noqa: E731
                                     device=st.device)
        ls = self._ls
        clip = self._clip
        found = (ls is not None or clip is not None) and \
            not bool(torch.isfinite(self.flat_grad).all())
        if clip is not None:
            total = float(self.flat_grad.double().square().sum())
            norm = math.sqrt(total) / float(st[SCALE])
            coef = self._max_norm / (norm + 1e-6)
            clips = coef < 1.0  # False for a NaN norm
            clip[GRAD_NORM] = f32(norm)
            clip[CLIP_COEF] = f32(coef) if clips else 1.0
            if clips and not found:
                clip[CLIPPED] += 1.0
        if found:
            if ls is not None:
                st[SCALE] *= f32(ls["backoff_factor"])
            st[TRACKER] = 0.0
            st[SKIPPED] += 1.0
            return
        p, m, v = self.flat_param, self.exp_avg, self.exp_avg_sq
        lr = st[LR]
        grad = self.flat_grad * (1.0 / st[SCALE])
        if clip is not None:  # a second multiply: un-scaling stays exact
            grad = grad * clip[CLIP_COEF]
        wd = g0["weight_decay"]
        if wd != 0:
            if g0["decoupled_weight_decay"]:
                p.mul_(1.0 - lr * f32(wd))
            else:
                grad = grad + f32(wd) * p
        # 1 - beta in fp64, rounded once (1.0f - 0.999f is off by 6e-5)
        m.add_((grad - m) * f32(1.0 - b1))
        v.mul_(f32(b2)).add_(f32(1.0 - b2) * grad * grad)
        vv = v
        if g0["amsgrad"]:
            torch.maximum(self.max_exp_avg_sq, v, out=self.max_exp_avg_sq)
            vv = self.max_exp_avg_sq
        denom = vv.sqrt() / st[BC2_SQRT] + f32(g0["eps"])
        p.sub_((lr / st[BC1]) * (m / denom))

        step = int(st[STEP]) + 1
        st[STEP] = float(step)
        bc1, bc2s = self._bias_corrections(step + 1)
        st[BC1], st[BC2_SQRT] = bc1, bc2s
        if ls is not None:
            tracker = int(st[TRACKER]) + 1
            if tracker >= ls["growth_interval"]:
                grown = st[SCALE] * f32(ls["growth_factor"])
                if bool(torch.isfinite(grown)):
                    st[SCALE] = grown
                tracker = 0
            st[TRACKER] = float(tracker)

    # ---------------- checkpointing (torch.optim.Adam layout) -----------

    def state_dict(self):
        """torch.optim.Adam's layout (per-param step / exp_avg / exp_avg_sq
        [/ max_exp_avg_sq] + param_groups), so checkpoints interchange with
        Adam/AdamW, plus a top-level ``loss_scale`` entry and, with
        clipping on, a top-level ``grad_clip`` entry."""
        st = self._state.detach().cpu()
        step = float(st[STEP])
        state = {}
        cols = [self._views(self.exp_avg), self._views(self.exp_avg_sq)]
        if self.max_exp_avg_sq is not None:
            cols.append(self._views(self.max_exp_avg_sq))
        for i in range(len(self._params)):
            s = {"step": torch.tensor(step, dtype=torch.float32),
                 "exp_avg": cols[0][i].clone(),
                 "exp_avg_sq": cols[1][i].clone()}
            if self.max_exp_avg_sq is not None:
                s["max_exp_avg_sq"] = cols[2][i].clone()
            state[i] = s
        groups, start = [], 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(start, start + len(g["params"])))
            start += len(g["params"])
            groups.append(packed)
        out = {"state": state, "param_groups": groups,
               "loss_scale": {"enabled": self._ls is not None,
                              "scale": float(st[SCALE]),
                              "growth_tracker": int(st[TRACKER]),
                              "skipped_steps": int(st[SKIPPED])}}
        if self._clip is not None:
            out["grad_clip"] = {"max_norm": self._max_norm,
                                "clipped_steps": self.clipped_steps}
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts FlatAdam and torch.optim.Adam/AdamW state dicts.  Copies
        IN PLACE: the p.data / p.grad views and any captured addresses
        survive."""
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(
                len(sg["params"]) != len(g["params"])
                for sg, g in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict has different param groups")
        for sg in groups:
            if bool(sg.get("amsgrad", False)) != \
                    (self.max_exp_avg_sq is not None):
                raise ValueError("loaded state dict disagrees on amsgrad")
            if sg.get("maximize", False):
                raise ValueError("FlatAdam does not support maximize")
        for sg, g in zip(groups, self.param_groups):
            for k, v in sg.items():
                if k in _HYPER_KEYS or k == "initial_lr":
                    g[k] = tuple(v) if k == "betas" else v
        g0 = self.param_groups[0]
        for g in self.param_groups[1:]:
            if any(g[k] != g0[k] for k in _HYPER_KEYS):
                raise ValueError(
                    "loaded param groups disagree on hyper-parameters")

        ids = [i for sg in groups for i in sg["params"]]
        saved = state_dict["state"]
        steps = set()
        cols = [(self._views(self.exp_avg), "exp_avg"),
                (self._views(self.exp_avg_sq), "exp_avg_sq")]
        if self.max_exp_avg_sq is not None:
            cols.append((self._views(self.max_exp_avg_sq), "max_exp_avg_sq"))
        for n, i in enumerate(ids):
            s = saved.get(i)
            if not s:  # Adam never stepped this param
                for views, _ in cols:
                    views[n].zero_()
                continue
            steps.add(int(float(s["step"])))
            for views, key in cols:
                views[n].copy_(s[key])
        if len(steps) > 1:
            raise ValueError(f"per-param step counts differ: {sorted(steps)}")
        step = steps.pop() if steps else 0

        ls = state_dict.get("loss_scale")
        if self._ls is None:
            scale, tracker, skipped = 1.0, 0, 0
            if ls:
                skipped = ls.get("skipped_steps", 0)
        elif ls and ls.get("enabled", True):
            scale, tracker, skipped = (ls["scale"], ls["growth_tracker"],
                                       ls["skipped_steps"])
        else:  # e.g. a plain Adam checkpoint: start scaling afresh
            scale, tracker, skipped = self._ls["init_scale"], 0, 0
        self._write_state(scale=scale, tracker=tracker, step=step,
                          skipped=skipped)
        if self._clip is not None:
            # the threshold stays the constructor's; only the counter moves
            gc = state_dict.get("grad_clip") or {}
            self._clip.zero_()
            self._clip[CLIPPED] = float(gc.get("clipped_steps", 0))


class FlatAdamW(FlatAdam):
    """FlatAdam with decoupled weight decay and torch.optim.AdamW's
    default ``weight_decay``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, amsgrad=False, loss_scale=None,
                 max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps,
                         weight_decay=weight_decay, amsgrad=amsgrad,
                         decoupled=True, loss_scale=loss_scale,
                         max_grad_norm=max_grad_norm)
