"""Shared helpers for the gradient-norm clipping tests (CPU torch path and
HIP kernels).

The yardstick is ``clip_grad_norm_(params, max_norm)`` followed by
torch.optim.Adam/AdamW ``step()`` in float64 on the same inputs, and the
tolerance is flat_adam_helpers' rule, with stock fp32 torch running the same
clip-then-step sequence:

    bound = 2 * max|p_torch_fp32 - p_fp64| + one fp32 ulp of max|p|

Adam is nearly invariant to a constant gradient scale, so equal-sized steps
would pass with clipping silently missing.  The per-step gradient
multipliers below make the clipped and the unclipped trajectories differ by
orders of magnitude more than the bound, and every parameter comparison
asserts that (`assert_clipping_matters`).
"""

import functools
import math

import torch

from flat_adam_helpers import (flat, fp32_ulp, make_case, make_torch_adam,
                               split_sizes)

MULTS = [1.0, 30.0, 0.03, 1000.0, 1.0]
STEPS = len(MULTS)
# scalar tail only / n < 4 / no tail / partial final block / tail + second
# block / several blocks + tail
CPU_SIZES = [1, 3, 4, 1023, 1027, 3003]


def max_norm_for(n):
    return 0.5 * math.sqrt(n)


def make_clip_case(n, steps=STEPS):
    """Seeded fp32 initial params and per-step grads, the grads multiplied
    by MULTS (in fp32: the products are the inputs of every path)."""
    init, grads = make_case(split_sizes(n), steps, seed=n % 1000 + 1)
    grads = [[g * m for g in gs] for gs, m in zip(grads, MULTS)]
    return init, grads


def run_torch_clipped(init, grads, hyper, dtype, max_norm):
    """clip_grad_norm_ + stock torch Adam/AdamW step in `dtype` on CPU;
    `max_norm` None leaves the clipping out.  Returns (flat params in fp64,
    the total norm of every step as a float, optimizer, params)."""
    params = [torch.nn.Parameter(t.detach().clone().to(dtype)) for t in init]
    opt = make_torch_adam(params, hyper)
    norms = []
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.detach().clone().to(dtype)
        if max_norm is not None:
            norms.append(float(
                torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
    return flat(params).double(), norms, opt, params


@functools.lru_cache(maxsize=None)
def clip_reference(n, hyper, steps=STEPS):
    """Inputs, the fp64 yardstick, the derived bound, the yardstick's norms
    and the UNCLIPPED fp64 run; computed once per case and left unchanged."""
    init, grads = make_clip_case(n, steps)
    max_norm = max_norm_for(n)
    p64, norms64, _, _ = run_torch_clipped(init, grads, hyper, torch.float64,
                                           max_norm)
    p32, _, _, _ = run_torch_clipped(init, grads, hyper, torch.float32,
                                     max_norm)
    bound = 2.0 * (p32 - p64).abs().max().item() \
        + fp32_ulp(p64.abs().max().item())
    unclipped, _, _, _ = run_torch_clipped(init, grads, hyper, torch.float64,
                                           None)
    return init, grads, max_norm, p64, bound, norms64, unclipped


def assert_clipping_matters(p64, unclipped, bound):
    gap = (unclipped - p64).abs().max().item()
    print(f"unclipped fp64 reference is {gap / bound:.3g} bounds away")
    assert gap > 100 * bound, (gap, bound)


def make_clipped(init, hyper, max_norm, device="cpu", loss_scale=None,
                 lr=1e-2):
    from esr_amd.optim import FlatAdam
    amsgrad, wd, decoupled = hyper
    params = [torch.nn.Parameter(t.detach().clone().to(device)) for t in init]
    opt = FlatAdam(params, lr=lr, weight_decay=wd, amsgrad=amsgrad,
                   decoupled=decoupled, loss_scale=loss_scale,
                   max_grad_norm=max_norm)
    return opt, params


def feed(opt, params, gs, mult=1.0):
    opt.zero_grad()
    with torch.no_grad():
        for p, g in zip(params, gs):
            p.grad.add_(g.to(p.device) * mult)


def run_clipped(init, grads, hyper, max_norm, device="cpu", loss_scale=None,
                mult=1.0):
    """FlatAdam with clipping over `grads`; returns (flat params in fp64,
    optimizer, params, the clip scalars after every step as CPU tensors)."""
    opt, params = make_clipped(init, hyper, max_norm, device, loss_scale)
    clips = []
    for gs in grads:
        feed(opt, params, gs, mult)
        opt.step()
        clips.append(opt.clip_state.detach().cpu().clone())
    return flat(params).double(), opt, params, clips


def assert_within_one_ulp(a, b, what=""):
    """fp32 values a and b are equal or neighbours."""
    a, b = float(a), float(b)
    assert abs(a - b) <= fp32_ulp(max(abs(a), abs(b))), (what, a, b)


def bits(t):
    return t.detach().cpu().view(torch.int32)
