"""GPU tests for the fp16 instantiations of the fused GRU gate kernels and
the deformable-conv kernels."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H16 = torch.float16


@pytest.fixture(autouse=True)
def _fp16_path_on(monkeypatch):
    monkeypatch.setenv("ESR_NATIVE_FP16", "1")
    monkeypatch.setenv("ESR_NATIVE_CONV", "1")


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def _assert_once_rounded(got, ref, what):
    """One elementwise fp32 expression rounded once to fp16:
    |got - ref| <= 2^-10 * |ref| + 2^-10."""
    assert got.dtype == H16, f"{what}: dtype {got.dtype}"
    diff = (got.float() - ref).abs()
    bound = 2.0 ** -10 * ref.abs() + 2.0 ** -10
    n_bad = int((~(diff <= bound)).sum().item())
    assert n_bad == 0, (f"{what}: {n_bad}/{diff.numel()} over bound "
                        f"(max diff {diff.max().item():.4g})")


# ------------------------------------------------------------- GRU gates

def test_gru_gates_fp16_forward_backward():
    from esr_amd.ops.convgru import gru_gates_out, gru_gates_ur
    C = 16
    ur16 = _rand(2, 2 * C, 24, 24, seed=1).to(H16)
    h16 = _rand(2, C, 24, 24, seed=2).to(H16)
    o16 = _rand(2, C, 24, 24, seed=3).to(H16)
    gu, gr, ghr, gh = [_rand(2, C, 24, 24, seed=s).to(H16)
                       for s in (4, 5, 6, 7)]

    # ---- pass 1: (ur_pre, h) -> u, r, h*r
    ur = ur16.clone().requires_grad_(True)
    h = h16.clone().requires_grad_(True)
    u, r, hr = gru_gates_ur(ur, h)
    assert type(u.grad_fn).__name__.startswith("_GatesUR"), u.grad_fn
    torch.autograd.backward([u, r, hr], [gu, gr, ghr])

    urf = ur16.float().requires_grad_(True)
    hf = h16.float().requires_grad_(True)
    uf = torch.sigmoid(urf[:, :C])
    rf = torch.sigmoid(urf[:, C:])
    hrf = hf * rf
    _assert_once_rounded(u, uf.detach(), "u")
    _assert_once_rounded(r, rf.detach(), "r")
    _assert_once_rounded(hr, hrf.detach(), "h*r")
    # the backward kernel starts from the fp16-ROUNDED saved u, r: evaluate
    # the torch formulas on those same rounded values
    u_s, r_s = u.detach().float(), r.detach().float()
    d_ur_ref = torch.cat([
        gu.float() * u_s * (1 - u_s),
        (gr.float() + ghr.float() * h16.float()) * r_s * (1 - r_s)], dim=1)
    dh_ref = ghr.float() * r_s
    _assert_once_rounded(ur.grad, d_ur_ref, "d ur_pre")
    _assert_once_rounded(h.grad, dh_ref, "dh (pass 1)")

    # ---- pass 2: h_new = h*(1-u) + tanh(o_pre)*u
    o = o16.clone().requires_grad_(True)
    u2 = u.detach().clone().requires_grad_(True)
    h2 = h16.clone().requires_grad_(True)
    h_new = gru_gates_out(o, u2, h2)
    assert type(h_new.grad_fn).__name__.startswith("_GatesOut"), h_new.grad_fn
    t_saved = h_new.grad_fn.saved_tensors[2]   # tanh(o_pre), fp16-rounded
    h_new.backward(gh)
    t = torch.tanh(o16.float())
    _assert_once_rounded(h_new, h16.float() * (1 - u_s) + t * u_s, "h_new")
    _assert_once_rounded(t_saved, t, "tanh(o_pre)")
    t_s = t_saved.float()
    _assert_once_rounded(o.grad, gh.float() * u_s * (1 - t_s * t_s),
                         "d o_pre")
    _assert_once_rounded(u2.grad, gh.float() * (t_s - h16.float()), "du")
    _assert_once_rounded(h2.grad, gh.float() * (1 - u_s), "dh (pass 2)")


# ------------------------------------------------------------------- DCN

def _dcn_problem(seed):
    B, C, Hh, W, dg = 2, 16, 24, 24, 4
    return (_rand(B, C, Hh, W, seed=seed),
            _rand(B, dg * 18, Hh, W, seed=seed + 1, scale=2.0),
            torch.rand(B, dg * 9, Hh, W, device=DEV,
                       generator=torch.Generator(device=DEV)
                       .manual_seed(seed + 2)),
            _rand(16, C, 3, 3, seed=seed + 3, scale=0.2),
            _rand(16, seed=seed + 4))


def _dcn_errors(dtype, seed=11):
    """Max-abs error of the 16-bit DCN path (forward + five grads) against
    the fp32 kernels on the same `dtype`-rounded inputs."""
    from esr_amd.ops.dcn import modulated_deform_conv2d
    prob = [t.to(dtype) for t in _dcn_problem(seed)]
    gout = _rand(2, 16, 24, 24, seed=seed + 9).to(dtype)

    def run(cast):
        leaves = [cast(t).clone().requires_grad_(True) for t in prob]
        out = modulated_deform_conv2d(*leaves, stride=1, padding=1,
                                      dilation=1, deformable_groups=4)
        out.backward(cast(gout))
        return [out.detach()] + [t.grad for t in leaves]

    got = run(lambda t: t)
    ref = run(lambda t: t.float())
    assert all(g.dtype == dtype for g in got)
    assert all(r.dtype == torch.float32 for r in ref)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    return [(g.float() - r).abs().max().item() for g, r in zip(got, ref)]


def test_dcn_fp16_no_worse_than_bf16():
    """Yardstick: the existing bf16 path.  fp16 carries three more mantissa
    bits, so per output and per grad its max error must not exceed the bf16
    path's error against its own oracle."""
    names = ["out", "grad_input", "grad_offset", "grad_mask", "grad_weight",
             "grad_bias"]
    e16 = _dcn_errors(H16)
    ebf = _dcn_errors(torch.bfloat16)
    report = ", ".join(f"{n}: fp16 {a:.4g} / bf16 {b:.4g}"
                       for n, a, b in zip(names, e16, ebf))
    print("DCN max-abs errors —", report)
    bad = [n for n, a, b in zip(names, e16, ebf) if not a <= b]
    assert not bad, f"fp16 worse than bf16 on {bad} — {report}"


def test_dcn_fp16_zero_offset_is_conv():
    from esr_amd.ops.dcn import modulated_deform_conv2d
    inp, _, _, weight, bias = [t.to(H16) for t in _dcn_problem(21)]
    offset = torch.zeros(2, 4 * 18, 24, 24, device=DEV, dtype=H16)
    mask = torch.ones(2, 4 * 9, 24, 24, device=DEV, dtype=H16)
    out = modulated_deform_conv2d(inp, offset, mask, weight, bias, stride=1,
                                  padding=1, dilation=1, deformable_groups=4)
    ref = F.conv2d(inp.float(), weight.float(), bias.float(), 1, 1)
    S = F.conv2d(inp.float().abs(), weight.float().abs(), bias.float().abs(),
                 1, 1)
    assert out.dtype == H16
    diff = (out.float() - ref).abs()
    bound = 2.0 ** -10 * ref.abs() + 2.0 ** -12 * S + 2.0 ** -24
    n_bad = int((~(diff <= bound)).sum().item())
    assert n_bad == 0, (f"{n_bad}/{diff.numel()} over the fp16 forward bound "
                        f"(worst diff/bound {(diff / bound).max().item():.3f})")


def test_deform_align_fp16_autocast_stays_fp16():
    from esr_amd.ops.dcn import DeformAlign2d
    torch.manual_seed(7)
    m = DeformAlign2d(16, 16, 3, stride=1, padding=1,
                      deformable_groups=4).to(DEV)
    x = _rand(2, 16, 24, 24, seed=31).to(H16).requires_grad_(True)
    f = _rand(2, 16, 24, 24, seed=32).to(H16)
    with torch.autocast("cuda", dtype=H16):
        out = m(x, f)
    assert out.dtype == H16
    node = out.grad_fn
    assert type(node).__name__.startswith("_DeformConvHIP"), node
    saved_input = node.saved_tensors[0]
    assert saved_input.dtype == H16, \
        f"input was up-cast to {saved_input.dtype} for the deformable conv"
    out.float().square().mean().backward()
    assert x.grad is not None and x.grad.dtype == H16
    assert bool(torch.isfinite(x.grad).all())
    assert m.weight.grad is not None and m.weight.grad.dtype == torch.float32
