"""GPU numerics tests for the fp16 instantiation of the gfx950 conv kernels.

Oracle: plain-PyTorch fp32 on the SAME fp16-rounded operands, so the only
allowed divergence is fp32 accumulation order plus the single fp16 rounding
of the output.  The forward bound is derived, not tuned.  With
S = conv2d(|x|, |w|) + |b| (fp32, elementwise):
  * fp32 accumulation over K <= 9*192+1 terms errs by <= K * 2^-24 * S
    < 2^-13 * S;
  * the output rounding adds <= 2^-11 * |ref|;
  * a factor 2 of slack covers the MFMA-internal summation order.
A single wrong or missing tap moves an element by ~0.2 at these input
scales, about ten times the bound.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H16 = torch.float16


@pytest.fixture(autouse=True)
def _fp16_path_on(monkeypatch):
    # the tests hold under either default of the switch
    monkeypatch.setenv("ESR_NATIVE_FP16", "1")
    monkeypatch.setenv("ESR_NATIVE_CONV", "1")


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


def _rand_f16(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(H16)


def _act(ref, act):
    if act == "relu":
        return F.relu(ref)
    if act == "sigmoid":
        return torch.sigmoid(ref)
    if act == "tanh":
        return torch.tanh(ref)
    return ref


def _assert_close(got, want, rtol=2e-2, atol=None, what=""):
    got = got.float()
    want = want.float()
    if atol is None:
        atol = 2e-2 * max(want.abs().max().item(), 1.0)
    diff = (got - want).abs()
    denom = want.abs().clamp_min(1.0)
    ok = (diff <= atol) | (diff / denom <= rtol)
    n_bad = int((~ok).sum().item())
    assert n_bad == 0, (
        f"{what}: {n_bad}/{ok.numel()} elements off "
        f"(max abs diff {diff.max().item():.4g}, atol {atol:.3g})")


def test_gemm16_probe_fragment_layout_fp16():
    """A=I with ASYMMETRIC B: the f16 MFMA has the bf16 form's lane maps
    and C/D layout.  All values are small multiples of 0.25 -> exact."""
    ext = _ext()
    A = torch.zeros(16, 32, device=DEV, dtype=H16)
    for i in range(16):
        A[i, i] = 1.0
    B = (torch.arange(32 * 16, device=DEV).reshape(32, 16) % 23).to(H16) * 0.25
    C = ext.gemm16_probe(A, B)
    want = A.float() @ B.float()
    assert C.dtype == torch.float32
    assert torch.equal(C, want), \
        f"identity-A fp16 probe failed, max {((C - want).abs()).max()}"


CASES = [
    # (Cin, Cout, H, W, ks, stride, act) — the rows of test_gpu_conv.CASES
    (2, 8, 64, 64, 3, 1, "relu"),        # head conv (VALU)
    (8, 16, 64, 64, 3, 2, "relu"),       # encoder s2 (VALU)
    (32, 64, 32, 32, 3, 2, "relu"),      # encoder s2 (MFMA)
    (64, 64, 32, 32, 3, 1, "relu"),      # deep conv (MFMA)
    (192, 64, 32, 32, 3, 1, "relu"),     # dense fusion (MFMA, 6 K-chunks)
    (192, 192, 16, 16, 3, 1, None),      # residual block width
    (128, 64, 32, 32, 1, 1, "relu"),     # 1x1 fusion (MFMA)
    (64, 2, 32, 32, 1, 1, "sigmoid"),    # kernel conv (VALU)
    (64, 1, 32, 32, 3, 1, "sigmoid"),    # attention map (VALU)
    (40, 48, 30, 30, 3, 1, "tanh"),      # unaligned channels + odd spatial
    (16, 33, 20, 44, 3, 1, None),        # Cout one past tile edge
    (64, 128, 32, 32, 3, 1, None),       # pixel-shuffle pre-conv
    (8, 2, 62, 32, 3, 1, "relu"),        # tail class, COCH=2, odd H
    (8, 2, 62, 30, 3, 1, "relu"),        # odd W -> routed to the v1 kernel
    (2, 8, 64, 64, 3, 2, None),          # tiny s2 (valu2 strided segs)
    (64, 216, 32, 32, 3, 1, None),       # flagship offset/mask conv: 224
                                         # packed rows, last cout block clamps
    (32, 64, 18, 70, 3, 2, "relu"),      # MFMA s2: Wo=35 two x-tiles (2nd
                                         # partial), Ho=9 partial row tile
    (64, 80, 10, 40, 1, 1, None),        # Cout_p=80, MREP=1, third block
                                         # half past Cout_p
    (2, 8, 24, 40, 3, 2, None),          # valu2 s2: Wo=20, 4-wide last strip,
                                         # misaligned rows
]


@pytest.mark.parametrize("cin,cout,h,w,ks,stride,act", CASES)
def test_conv_forward_fp16_matches_oracle(cin, cout, h, w, ks, stride, act):
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    x = _rand_f16(3, cin, h, w, seed=cin * 7 + cout)
    wt = _rand_f16(cout, cin, ks, ks, seed=cin + cout, scale=0.3)
    b = _rand_f16(cout, seed=5)

    y = _NativeConv2dFn.apply(x, wt, b, stride, ACT_IDS[act])
    pre = F.conv2d(x.float(), wt.float(), b.float(), stride=stride,
                   padding=ks // 2)
    ref = _act(pre, act)
    S = F.conv2d(x.float().abs(), wt.float().abs(), b.float().abs(),
                 stride=stride, padding=ks // 2)
    assert y.dtype == H16 and y.shape == ref.shape
    if act == "sigmoid":
        bound = 2.0 ** -10 + 2.0 ** -12 * S / 4
    elif act == "tanh":
        bound = 2.0 ** -10 + 2.0 ** -12 * S
    else:
        bound = 2.0 ** -10 * ref.abs() + 2.0 ** -12 * S + 2.0 ** -24
    diff = (y.float() - ref).abs()
    n_bad = int((~(diff <= bound)).sum().item())   # NaN counts as bad
    worst = (diff / bound).max().item()
    print(f"fwd fp16 {cin}->{cout} k{ks}s{stride} {act}: "
          f"max diff/bound {worst:.3f}, max abs diff {diff.max().item():.3g}")
    assert n_bad == 0, (
        f"fwd fp16 {cin}->{cout} k{ks}s{stride} {act}: {n_bad}/{diff.numel()}"
        f" elements over the derived bound (worst diff/bound {worst:.3f})")


def test_conv_fp16_overflow_saturates_like_torch():
    """fp32 results past 65504 must become inf exactly as torch's cast does;
    bf16 never had this range edge."""
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    x = torch.full((2, 64, 16, 16), 200.0, device=DEV, dtype=H16)
    wt = torch.ones(32, 64, 3, 3, device=DEV, dtype=H16)
    y = _NativeConv2dFn.apply(x, wt, None, 1, ACT_IDS[None])
    ref = F.conv2d(x.float(), wt.float(), None, stride=1, padding=1)
    assert ref.max().item() > 65504 and ref.min().item() < 65504
    want = ref.half()
    assert torch.isinf(want).any() and torch.isfinite(want).any()
    assert y.dtype == H16 and torch.equal(y, want), \
        f"{int((y != want).sum())} elements differ from ref.half()"

    y0 = _NativeConv2dFn.apply(x, -wt, None, 1, ACT_IDS["relu"])
    assert y0.dtype == H16
    assert int((y0 != 0).sum().item()) == 0, "relu(-overflow) must be 0"


def test_conv_fp16_underflow_keeps_subnormals():
    """Results in the fp16 subnormal range match ref.half() within one
    subnormal step (2^-24) — not flushed to zero."""
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    g = torch.Generator(device=DEV).manual_seed(17)
    x = ((torch.rand(2, 64, 16, 16, device=DEV, generator=g) * 2 - 1)
         * 2.0 ** -10).to(H16)
    wt = ((torch.rand(32, 64, 3, 3, device=DEV, generator=g) * 2 - 1)
          * 2.0 ** -11).to(H16)
    y = _NativeConv2dFn.apply(x, wt, None, 1, ACT_IDS[None])
    ref = F.conv2d(x.float(), wt.float(), None, stride=1, padding=1)
    # every result is subnormal in fp16 (< 2^-14) and most are not zero
    assert ref.abs().max().item() < 2.0 ** -14
    assert ref.abs().median().item() > 2.0 ** -22
    want = ref.half()
    diff = (y.float() - want.float()).abs()
    n_bad = int((~(diff <= 2.0 ** -24)).sum().item())
    assert n_bad == 0, (f"{n_bad}/{diff.numel()} subnormal results off by "
                        f"more than 2^-24 (max {diff.max().item():.3g})")
    assert int((y != 0).sum().item()) > y.numel() // 2, "subnormals flushed"


def test_conv_mixed_16bit_dtypes_raise():
    from esr_amd.ops.conv import _pack
    ext = _ext()
    x = _rand_f16(1, 64, 16, 16, seed=1)
    wp_bf16 = _pack(_rand_f16(64, 64, 3, 3, seed=2).to(torch.bfloat16))
    with pytest.raises(RuntimeError, match=r"(?s)Half.*BFloat16"):
        ext.conv2d_fwd_mfma(x, wp_bf16, None, 64, 3, 1, 0)
    # backward-only kernels stay bf16-only and must refuse fp16 cleanly
    dy = _rand_f16(1, 64, 16, 16, seed=3)
    with pytest.raises(RuntimeError, match=r"(?s)bf16.*Half"):
        ext.conv2d_wgrad_mfma(x, dy, 3, 1, 64, 64)


BWD_CASES = [
    (64, 64, 32, 32, 3, 1, "relu"),
    (32, 64, 32, 32, 3, 2, "relu"),
    (64, 1, 32, 32, 3, 1, "sigmoid"),
]


@pytest.mark.parametrize("cin,cout,h,w,ks,stride,act", BWD_CASES)
def test_conv_backward_fp16_matches_oracle(cin, cout, h, w, ks, stride, act,
                                           monkeypatch):
    """fp16 backward = native act_grad + aten.convolution_backward under
    BOTH settings of ESR_CONV_BWD (the native wgrad/dgrad are bf16-only)."""
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    # MIOpen's fp16 weight-grad solvers may reduce with atomics, so two
    # identical calls need not agree bitwise; ask for its deterministic
    # solvers so the bit-for-bit aten/native comparison below tests routing
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    x = _rand_f16(3, cin, h, w, seed=cin * 3 + cout)
    wt = _rand_f16(cout, cin, ks, ks, seed=cin + 2 * cout, scale=0.3)
    b = _rand_f16(cout, seed=9)
    ho = (h + 2 * (ks // 2) - ks) // stride + 1
    wo = (w + 2 * (ks // 2) - ks) // stride + 1
    gy = _rand_f16(3, cout, ho, wo, seed=31)

    xr = x.float().clone().requires_grad_(True)
    wr = wt.float().clone().requires_grad_(True)
    br = b.float().clone().requires_grad_(True)
    ref = _act(F.conv2d(xr, wr, br, stride=stride, padding=ks // 2), act)
    ref.backward(gy.float())

    got = {}
    for mode in ("aten", "native"):
        monkeypatch.setenv("ESR_CONV_BWD", mode)
        xg = x.clone().requires_grad_(True)
        wg = wt.clone().requires_grad_(True)
        bg = b.clone().requires_grad_(True)
        y = _NativeConv2dFn.apply(xg, wg, bg, stride, ACT_IDS[act])
        y.backward(gy)
        for name, t, r in (("dgrad", xg, xr), ("wgrad", wg, wr),
                           ("bgrad", bg, br)):
            assert t.grad.dtype == H16
            assert bool(torch.isfinite(t.grad).all()), f"{mode} {name} inf/nan"
            _assert_close(t.grad, r.grad, rtol=5e-2,
                          what=f"{mode} {name} {cin}->{cout} k{ks}s{stride}")
        got[mode] = (xg.grad, wg.grad, bg.grad)
    for a, n, name in zip(got["aten"], got["native"],
                          ("dgrad", "wgrad", "bgrad")):
        assert torch.equal(a, n), \
            f"{name}: ESR_CONV_BWD=native differs from aten for fp16"


def _model(seed):
    from esr_amd.models import build_model
    torch.manual_seed(seed)
    return build_model("ESRNet", inch=2, basech=8, num_frame=3,
                       upsampler="pixelshuffle").to(DEV)


def _model_input(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(1, 3, 2, 64, 64, device=DEV, generator=g).abs()


def test_esrnet_fp16_autocast_uses_native_convs(monkeypatch):
    from esr_amd.ops import conv as conv_mod
    model = _model(0).eval()
    x = _model_input(41)

    def run():
        conv_mod.stats["native_calls_fp16"] = 0
        with torch.no_grad(), torch.autocast("cuda", dtype=H16):
            model.reset_states()
            y = model(x)
        return y, conv_mod.stats["native_calls_fp16"]

    y, n = run()
    assert y.dtype == H16
    assert n >= 20, f"only {n} native fp16 conv dispatches"
    monkeypatch.setenv("ESR_NATIVE_FP16", "0")
    _, n_off = run()
    assert n_off == 0, f"{n_off} native fp16 dispatches with the switch off"


def test_esrnet_fp16_native_error_vs_miopen_error(monkeypatch):
    """Both fp16 forwards are rounding chains of the same depth: the native
    path's max-abs error against fp32 eager must be within 2x of the MIOpen
    fp16 path's (summation order + the fast __expf sigmoid)."""
    model = _model(1).eval()
    x = _model_input(21)
    with torch.no_grad():
        model.reset_states()
        y32 = model(x).float()
        with torch.autocast("cuda", dtype=H16):
            model.reset_states()
            y_native = model(x).float()
            monkeypatch.setenv("ESR_NATIVE_CONV", "0")
            model.reset_states()
            y_miopen = model(x).float()
    assert bool(torch.isfinite(y_native).all())
    e_native = (y_native - y32).abs().max().item()
    e_miopen = (y_miopen - y32).abs().max().item()
    print(f"whole-model fp16 max-abs error vs fp32: native {e_native:.4g}, "
          f"MIOpen {e_miopen:.4g} (|y32| max {y32.abs().max().item():.4g})")
    assert e_native <= 2 * e_miopen, (
        f"native fp16 error {e_native:.4g} > 2x MIOpen fp16 error "
        f"{e_miopen:.4g}")


def test_esrnet_fp16_train_step_native():
    from esr_amd.ops import conv as conv_mod
    model = _model(2).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    x = _model_input(33)
    gt = _model_input(34)[:, 0]
    before = [p.detach().clone() for p in model.parameters()]
    conv_mod.stats["native_calls_fp16"] = 0
    model.reset_states()
    with torch.autocast("cuda", dtype=H16):
        pred = model(x)
    assert conv_mod.stats["native_calls_fp16"] >= 20
    loss = F.mse_loss(pred.float(), gt.float())
    loss.backward()
    assert bool(torch.isfinite(loss))
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    opt.step()
    changed = sum(int(not torch.equal(a, p.detach()))
                  for a, p in zip(before, model.parameters()))
    assert changed > 0, "no weight changed after the step"
