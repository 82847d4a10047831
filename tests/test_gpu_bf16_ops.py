"""GPU tests for the bf16 instantiation of the fused GRU gate kernels (both
passes, every output and grad), for act_grad called directly in bf16 and
fp16, and for the 16-bit deformable-conv forward, against float64 torch
formulas on the same 16-bit-rounded operands (rules: tests/bound_rules.py).
"""

import pytest
import torch

from bound_rules import UNIT_ROUNDOFF, assert_within, once_rounded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, H16 = torch.bfloat16, torch.float16
SHAPE = (2, 16, 24, 24)


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def check_gates(dtype, shape):
    """Both gate passes, forward and backward, on `dtype` tensors of `shape`
    [B, C, H, W]; shared with the grid-wrap test."""
    from esr_amd.ops.convgru import gru_gates_out, gru_gates_ur
    B, C, Hh, W = shape
    ur_in = _rand(B, 2 * C, Hh, W, seed=1).to(dtype)
    h_in = _rand(*shape, seed=2).to(dtype)
    o_in = _rand(*shape, seed=3).to(dtype)
    gu, gr, ghr, gh = [_rand(*shape, seed=s).to(dtype).double()
                       for s in (4, 5, 6, 7)]
    ur64, h64, o64 = ur_in.double(), h_in.double(), o_in.double()

    def chk(got, ref64, what):
        once_rounded(got, ref64, dtype, f"gates {dtype} {what}")

    # ---- pass 1: (ur_pre, h) -> u, r, h*r
    ur = ur_in.clone().requires_grad_(True)
    h = h_in.clone().requires_grad_(True)
    u, r, hr = gru_gates_ur(ur, h)
    assert type(u.grad_fn).__name__.startswith("_GatesUR"), u.grad_fn
    torch.autograd.backward([u, r, hr],
                            [gu.to(dtype), gr.to(dtype), ghr.to(dtype)])
    r64 = torch.sigmoid(ur64[:, C:])
    chk(u, torch.sigmoid(ur64[:, :C]), "u")
    chk(r, r64, "r")
    chk(hr, h64 * r64, "h*r")
    # the backward kernel starts from the 16-bit-ROUNDED saved u, r:
    # evaluate the formulas on those same rounded values
    u_s, r_s = u.detach().double(), r.detach().double()
    chk(ur.grad, torch.cat([gu * u_s * (1 - u_s),
                            (gr + ghr * h64) * r_s * (1 - r_s)], dim=1),
        "d ur_pre")
    chk(h.grad, ghr * r_s, "dh (pass 1)")

    # ---- pass 2: h_new = h*(1-u) + tanh(o_pre)*u
    o = o_in.clone().requires_grad_(True)
    u2 = u.detach().clone().requires_grad_(True)
    h2 = h_in.clone().requires_grad_(True)
    h_new = gru_gates_out(o, u2, h2)
    assert type(h_new.grad_fn).__name__.startswith("_GatesOut"), h_new.grad_fn
    t_saved = h_new.grad_fn.saved_tensors[2]   # tanh(o_pre), rounded
    h_new.backward(gh.to(dtype))
    t64 = torch.tanh(o64)
    chk(h_new, h64 * (1 - u_s) + t64 * u_s, "h_new")
    chk(t_saved, t64, "tanh(o_pre)")
    t_s = t_saved.double()
    chk(o.grad, gh * u_s * (1 - t_s * t_s), "d o_pre")
    chk(u2.grad, gh * (t_s - h64), "du")
    chk(h2.grad, gh * (1 - u_s), "dh (pass 2)")


def test_gru_gates_bf16_forward_backward():
    check_gates(BF16, SHAPE)


def check_act_grad(act, dtype, shape):
    """ext.act_grad against dy * act'(y) in float64; y is a genuine
    activation output rounded to `dtype`.  Shared with the grid-wrap test."""
    from esr_amd.ops.conv import ACT_IDS
    pre = _rand(*shape, seed=11, scale=2.0)
    y = {"relu": torch.relu, "sigmoid": torch.sigmoid,
         "tanh": torch.tanh}[act](pre).to(dtype)
    dy = _rand(*shape, seed=12).to(dtype)
    got = _ext().act_grad(dy, y, ACT_IDS[act])
    assert got.dtype == dtype and got.shape == dy.shape
    y64, dy64 = y.double(), dy.double()
    if act == "relu":
        want = torch.where(y > 0, dy, torch.zeros_like(dy))
        n_diff = int((got != want).sum().item())
        assert n_diff == 0, f"relu grad: {n_diff} elements not bit-equal"
        assert int((y > 0).sum()) > 0 and int((y == 0).sum()) > 0
        return
    ref = dy64 * y64 * (1 - y64) if act == "sigmoid" \
        else dy64 * (1 - y64 * y64)
    once_rounded(got, ref, dtype, f"act_grad {act} {dtype}")


@pytest.mark.parametrize("dtype", [BF16, H16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", ["relu", "sigmoid", "tanh"])
def test_act_grad_direct(act, dtype):
    check_act_grad(act, dtype, SHAPE)


# ------------------------------------------------------------------- DCN

@pytest.mark.parametrize("dtype", [BF16, H16], ids=["bf16", "fp16"])
def test_dcn_16bit_forward_matches_fp64_oracle(dtype, monkeypatch):
    """The 16-bit deformable-conv forward against the independent float64
    oracle (_deform_conv2d_torch) on the same 16-bit-rounded operands - the
    other 16-bit DCN tests compare with the fp32 instantiation of the same
    kernel template.

    Bound: 2*2u*|ref| + 2u*S + 2^-24, with S the oracle run on |input|,
    offset, mask, |weight|, |bias| (mask and bilinear weights are >= 0, so S
    bounds the sum of the magnitudes of all terms).  Derivation:
      * the im2col columns are rounded once to 16 bits: <= u*S;
      * the GEMM output is rounded once and the bias add rounds it again:
        <= u*(2*|ref| + |b|);
      * fp32 accumulation over C*K + 1 = 145 terms: < 2^-13*S;
      * the factor 2 on each term is slack.
    """
    from esr_amd.ops.dcn import _deform_conv2d_torch, modulated_deform_conv2d
    monkeypatch.setenv("ESR_NATIVE_FP16", "1")
    B, C, Hh, W, dg, Cout = 2, 16, 24, 24, 4, 16
    prob = [_rand(B, C, Hh, W, seed=41),
            _rand(B, dg * 18, Hh, W, seed=42, scale=2.0),
            torch.rand(B, dg * 9, Hh, W, device=DEV,
                       generator=torch.Generator(device=DEV).manual_seed(43)),
            _rand(Cout, C, 3, 3, seed=44, scale=0.2),
            _rand(Cout, seed=45)]
    prob = [t.to(dtype) for t in prob]
    out = modulated_deform_conv2d(*prob, stride=1, padding=1, dilation=1,
                                  deformable_groups=dg)
    assert out.dtype == dtype
    inp, off, msk, wgt, bias = [t.cpu().double() for t in prob]
    geom = ((1, 1), (1, 1), (1, 1), dg)
    ref = _deform_conv2d_torch(inp, off, msk, wgt, bias, *geom)
    S = _deform_conv2d_torch(inp.abs(), off, msk, wgt.abs(), bias.abs(),
                             *geom)
    u = UNIT_ROUNDOFF[dtype]
    bound = 2 * 2 * u * ref.abs() + 2 * u * S + 2.0 ** -24
    assert_within(out.cpu(), ref, bound, f"dcn forward {dtype} vs fp64")
