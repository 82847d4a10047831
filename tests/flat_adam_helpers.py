"""Shared helpers for the FlatAdam tests (CPU torch path and HIP kernels).

The yardstick everywhere is torch.optim.Adam/AdamW run in float64 on the
same inputs.  The tolerance is not fixed in advance: it is derived from the
error stock fp32 torch Adam makes on the very same inputs,

    bound = 2 * max|p_torch_fp32 - p_fp64| + one fp32 ulp of max|p|

(factor 2: a different but equally valid fp32 operation order; anything
larger is a formula error).
"""

import math

import torch

HYPER_CASES = [
    # (amsgrad, weight_decay, decoupled)
    (False, 0.0, False), (True, 0.0, False),
    (False, 1e-4, False), (True, 1e-4, False),
    (False, 0.0, True), (True, 0.0, True),
    (False, 1e-4, True), (True, 1e-4, True),
]
LR = 1e-2


def hyper_id(h):
    return f"{'ams' if h[0] else 'noams'}-wd{h[1]:g}-{'adamw' if h[2] else 'adam'}"


def split_sizes(n):
    """Up to three param shapes with n elements in total."""
    if n < 3:
        return [(n,)]
    a = 1
    b = (n - 1) // 2
    return [(a,), (b,), (n - a - b,)]


def make_case(shapes, steps, seed=0):
    """Seeded fp32 initial params and per-step grads (CPU)."""
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes]
             for _ in range(steps)]
    return init, grads


def flat(tensors):
    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors])


def fp32_ulp(x: float) -> float:
    """Spacing of fp32 numbers at magnitude x."""
    if x == 0:
        return 2.0 ** -149
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23)


def make_torch_adam(params, hyper, lr=LR):
    amsgrad, wd, decoupled = hyper
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    return cls(params, lr=lr, weight_decay=wd, amsgrad=amsgrad)


def run_torch_adam(init, grads, hyper, dtype, lrs=None, opt_hook=None):
    """Stock torch Adam/AdamW in `dtype` on CPU; returns (flat params in
    fp64, optimizer, params)."""
    params = [torch.nn.Parameter(t.detach().clone().to(dtype)) for t in init]
    opt = make_torch_adam(params, hyper)
    if opt_hook is not None:
        opt_hook(opt, params)
    for k, gs in enumerate(grads):
        if lrs is not None:
            for grp in opt.param_groups:
                grp["lr"] = lrs[k]
        for p, g in zip(params, gs):
            p.grad = g.detach().clone().to(dtype)
        opt.step()
    return flat(params).double(), opt, params


def make_flat_adam(init, hyper, device="cpu", loss_scale=None, lr=LR):
    from esr_amd.optim import FlatAdam
    amsgrad, wd, decoupled = hyper
    params = [torch.nn.Parameter(t.detach().clone().to(device)) for t in init]
    opt = FlatAdam(params, lr=lr, weight_decay=wd, amsgrad=amsgrad,
                   decoupled=decoupled, loss_scale=loss_scale)
    return opt, params


def feed_grads(opt, params, gs, mult=1.0):
    """Write one step's grads through the .grad views (as autograd would)."""
    opt.zero_grad()
    with torch.no_grad():
        for p, g in zip(params, gs):
            p.grad.add_(g.to(p.device) * mult)


def run_flat_adam(init, grads, hyper, device="cpu", loss_scale=None,
                  mult=1.0, lrs=None):
    opt, params = make_flat_adam(init, hyper, device, loss_scale)
    for k, gs in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        feed_grads(opt, params, gs, mult)
        opt.step()
    return flat(params).double(), opt, params


def reference_and_bound(init, grads, hyper, lrs=None):
    """fp64 reference params and the derived tolerance (module docstring)."""
    p64, _, _ = run_torch_adam(init, grads, hyper, torch.float64, lrs)
    p32, _, _ = run_torch_adam(init, grads, hyper, torch.float32, lrs)
    e_ref = (p32 - p64).abs().max().item()
    bound = 2.0 * e_ref + fp32_ulp(p64.abs().max().item())
    return p64, bound


def assert_close_by_rule(got, p64, bound, what=""):
    err = (got.double().cpu() - p64).abs().max().item()
    print(f"{what} max|p - p_fp64| = {err:.3e}  bound = {bound:.3e}")
    assert err <= bound, (what, err, bound)


def snapshot(opt):
    """Bitwise-comparable copies of everything an overflow must not touch."""
    bufs = [opt.flat_param, opt.exp_avg, opt.exp_avg_sq]
    if opt.max_exp_avg_sq is not None:
        bufs.append(opt.max_exp_avg_sq)
    return [b.detach().clone() for b in bufs], opt.step_count


def assert_untouched(opt, snap):
    bufs, step = snap
    now, step_now = snapshot(opt)
    for a, b in zip(bufs, now):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert step_now == step
