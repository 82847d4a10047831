"""GPU numerics tests for the hand-written gfx950 conv kernels.

Oracle methodology: every native kernel is compared against a
plain-PyTorch reference computed from the SAME bf16-rounded inputs, so the
only allowed divergence is fp32 accumulation order + the final bf16
rounding of the output.  The forward (conv_bound) and the backward
(conv_bwd_bound), native and aten, are held to the derived per-element
bounds of tests/bound_rules.py against a float64 reference; the
whole-model tests keep the looser _assert_close rule.
"""

import os

import pytest
import torch
import torch.nn.functional as F

from bound_rules import (assert_within, conv_bound, conv_bwd_bound,
                         conv_bwd_ref64, conv_ref64, count_over)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


def _rand_bf16(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale) \
        .to(torch.bfloat16)


def _assert_close(got, want, rtol=2e-2, atol=None, what=""):
    got = got.float()
    want = want.float()
    if atol is None:
        atol = 2e-2 * max(want.abs().max().item(), 1.0)
    diff = (got - want).abs()
    denom = want.abs().clamp_min(1.0)
    ok = (diff <= atol) | (diff / denom <= rtol)
    # integer count, not a fp32 mean: a float mean of N ones can read
    # 1 - 2^-24 on GPU reductions and fake a failure
    n_bad = int((~ok).sum().item())
    assert n_bad == 0, (
        f"{what}: {n_bad}/{ok.numel()} elements off "
        f"(max abs diff {diff.max().item():.4g}, atol {atol:.3g})")


def test_gemm16_probe_fragment_layout():
    """A=I with ASYMMETRIC B catches transposed C-writes (guide §3)."""
    ext = _ext()
    A = torch.zeros(16, 32, device=DEV, dtype=torch.bfloat16)
    for i in range(16):
        A[i, i] = 1.0
    B = (torch.arange(32 * 16, device=DEV).reshape(32, 16) % 23).to(
        torch.bfloat16) * 0.25
    C = ext.gemm16_probe(A, B)
    want = A.float() @ B.float()
    assert torch.allclose(C, want, atol=1e-3), \
        f"identity-A probe failed, max {((C - want).abs()).max()}"
    # random full-rank check
    A2 = _rand_bf16(16, 32, seed=3)
    B2 = _rand_bf16(32, 16, seed=4)
    C2 = ext.gemm16_probe(A2, B2)
    _assert_close(C2, A2.float() @ B2.float(), what="gemm16 random")


CASES = [
    # (Cin, Cout, H, W, ks, stride, act) — covers MFMA + VALU dispatch,
    # channel-padding edges, non-multiple-of-tile spatial sizes
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
def test_conv_forward_matches_oracle(cin, cout, h, w, ks, stride, act):
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    x = _rand_bf16(3, cin, h, w, seed=cin * 7 + cout)
    wt = _rand_bf16(cout, cin, ks, ks, seed=cin + cout, scale=0.3)
    b = _rand_bf16(cout, seed=5).float().to(torch.bfloat16)

    y = _NativeConv2dFn.apply(x, wt, b, stride, ACT_IDS[act])
    ref64, S64 = conv_ref64(x, wt, b, stride, act)
    assert y.dtype == torch.bfloat16 and y.shape == ref64.shape
    assert_within(y.cpu(), ref64, conv_bound(ref64, S64, act, torch.bfloat16),
                  f"fwd bf16 {cin}->{cout} k{ks}s{stride} {act}")


@pytest.mark.parametrize("bwd", ["aten", "native"])
@pytest.mark.parametrize("cin,cout,h,w,ks,stride,act", [
    (2, 8, 64, 64, 3, 1, "relu"),
    (32, 64, 32, 32, 3, 2, "relu"),
    (64, 64, 32, 32, 3, 1, "relu"),
    (192, 64, 32, 32, 3, 1, None),
    (128, 64, 32, 32, 1, 1, "relu"),
    (64, 1, 32, 32, 3, 1, "sigmoid"),
    (40, 48, 30, 30, 3, 1, "tanh"),
    (8, 16, 64, 64, 3, 2, "relu"),
])
def test_conv_backward_matches_oracle(cin, cout, h, w, ks, stride, act, bwd,
                                      monkeypatch):
    monkeypatch.setenv("ESR_CONV_BWD", bwd)
    loose_dx = bwd == "aten" and \
        (cin, cout, h, w, ks, stride, act) in MIOPEN_DX_OVER
    _backward_vs_oracle(3, cin, cout, h, w, ks, stride, act, bwd, loose_dx)


# aten cases whose input grad MIOpen (the library's code, not this
# project's) returns outside conv_bwd_bound; their dx keeps the looser
# _assert_close rule, dW and db the bound.  Measured on MI355X: 192->64
# 32x32 k3 s1, act None: 29347 of 589824 dx elements over, worst diff/bound
# 7.47 (the native dgrad on the same case: 0 over, 0.47).  The cause was
# not investigated; supposed only: with act None the bound has no u*S term,
# which an algorithm that rounds an intermediate to bf16 could not meet.
MIOPEN_DX_OVER = {(192, 64, 32, 32, 3, 1, None)}


# native only, chosen from the kernels' tiling: (B, Cin, Cout, H, W, ks,
# stride, act)
NATIVE_BWD_EDGES = [
    # Cin_p 48 = 1.5 ci-blocks, Cout_p 80 = 1.25 co-blocks of
    # conv2d_wgrad_s1_kernel, uw 2 with an 8-wide last chunk, H 7 = 4 + 3 rows
    (3, 48, 80, 7, 40, 3, 1, None),
    # fpb = 2 with an odd batch: the last block holds one frame
    # (b0 + bf < B)
    (33, 128, 128, 6, 256, 3, 1, None),
    # conv2d_wgrad_s1_kernel<1> and the 1x1 dgrad, W one past a chunk
    (3, 40, 48, 5, 33, 1, 1, "relu"),
    # conv2d_dgrad_s2 and the stride-2 wgrad at odd H and W: Ho 9 / Wo 18,
    # the last input row and column are reached by one tap only
    (3, 32, 64, 17, 35, 3, 2, None),
    # Ho 17 = 16 + 1 rows: a second, one-row slab of rows_per_blk 16; uw 3
    (3, 32, 64, 34, 70, 3, 2, None),
    # Cout one past a tile; dgrad through conv2d_fwd_valu (Cin 16)
    (3, 16, 33, 20, 44, 3, 1, None),
]


@pytest.mark.parametrize("batch,cin,cout,h,w,ks,stride,act", NATIVE_BWD_EDGES)
def test_conv_backward_native_tiling_edges(batch, cin, cout, h, w, ks, stride,
                                           act, monkeypatch):
    monkeypatch.setenv("ESR_CONV_BWD", "native")
    _backward_vs_oracle(batch, cin, cout, h, w, ks, stride, act, "native")


def test_wgrad_multi_frame_blocks(monkeypatch):
    """conv2d_wgrad_s1_kernel with fpb = 2: B*uw*ciblks*coblks = 32*8*4*2 =
    2048 blocks, so each block sums two frames before its flush and restarts
    the rolling X window for the second.  H = 6 leaves a partial 4-row
    chunk."""
    monkeypatch.setenv("ESR_CONV_BWD", "native")
    _backward_vs_oracle(32, 128, 128, 6, 256, 3, 1, None, "native")


def _backward_vs_oracle(batch, cin, cout, h, w, ks, stride, act, bwd=None,
                        loose_dx=False):
    """dx, dW and db of _NativeConv2dFn under ESR_CONV_BWD = `bwd` (None: as
    the caller has set it) against float64 conv autograd on the same bf16
    operands, for the incoming gradient dy * act'(y) on the kernel's own
    forward output: every element within conv_bwd_bound.  `loose_dx`
    (MIOPEN_DX_OVER only) holds dx to _assert_close against the same
    reference instead."""
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    bwd = bwd or os.environ["ESR_CONV_BWD"]
    assert os.environ["ESR_CONV_BWD"] == bwd
    x = _rand_bf16(batch, cin, h, w, seed=cin * 3 + cout)
    wt = _rand_bf16(cout, cin, ks, ks, seed=cin - cout, scale=0.3)
    b = _rand_bf16(cout, seed=9)

    xg = x.clone().requires_grad_(True)
    wg = wt.clone().requires_grad_(True)
    bg = b.clone().requires_grad_(True)
    y = _NativeConv2dFn.apply(xg, wg, bg, stride, ACT_IDS[act])
    gy = _rand_bf16(*y.shape, seed=31)
    y.backward(gy)

    refs, Ss = conv_bwd_ref64(x, wt, gy, y.detach(), stride, act)
    n_w = batch * y.shape[2] * y.shape[3]
    over = {}
    for name, got, r, S, n in zip(("dx", "dW", "db"),
                                  (xg.grad, wg.grad, bg.grad), refs, Ss,
                                  (9 * cout, n_w, n_w)):
        assert got.dtype == torch.bfloat16, (name, got.dtype)
        over[name], worst = count_over(
            got.cpu(), r, conv_bwd_bound(r, S, n, act, torch.bfloat16))
        print(f"{bwd} B{batch} {cin}->{cout} {h}x{w} k{ks}s{stride} {act} "
              f"{name}: {over[name]}/{r.numel()} over, "
              f"max diff/bound {worst:.3f}")
    if loose_dx:
        del over["dx"]
        _assert_close(xg.grad.cpu(), refs[0], rtol=5e-2,
                      what=f"dgrad {cin}->{cout} k{ks}s{stride}")
    assert not any(over.values()), f"elements over the bound: {over}"


def test_convlayer_native_vs_fallback():
    """ConvLayer on GPU bf16: native path output == torch fallback path."""
    from esr_amd.models.blocks import ConvLayer
    torch.manual_seed(0)
    layer = ConvLayer(64, 64, 3, 1, 1, activation="relu").to(DEV) \
        .to(torch.bfloat16)
    x = _rand_bf16(2, 64, 32, 32, seed=11)
    y_native = layer(x)
    os.environ["ESR_NATIVE_CONV"] = "0"
    try:
        y_torch = layer(x)
    finally:
        os.environ["ESR_NATIVE_CONV"] = "1"
    _assert_close(y_native, y_torch, what="ConvLayer native vs torch")


def test_esrnet_forward_native_vs_fallback():
    """Whole-model bf16 forward: native conv path vs MIOpen fallback."""
    from esr_amd.models import build_model
    torch.manual_seed(1)
    model = build_model("ESRNet", inch=2, basech=8, num_frame=3,
                        upsampler="pixelshuffle").to(DEV).to(torch.bfloat16)
    model.eval()
    x = _rand_bf16(2, 3, 2, 64, 64, seed=21, scale=2.0).abs()
    with torch.no_grad():
        model.reset_states()
        y_native = model(x)
        os.environ["ESR_NATIVE_CONV"] = "0"
        try:
            model.reset_states()
            y_torch = model(x)
        finally:
            os.environ["ESR_NATIVE_CONV"] = "1"
    # both paths are bf16 with fp32 accumulation; small drift through the
    # 20-conv stack is expected, gross layout/tap errors are not
    _assert_close(y_native, y_torch, rtol=8e-2,
                  atol=8e-2 * max(y_torch.float().abs().max().item(), 1.0),
                  what="ESRNet native vs torch")


def test_esrnet_train_step_native():
    """One bf16 training step through the native conv path updates weights
    and produces finite grads."""
    from esr_amd.models import build_model
    torch.manual_seed(2)
    model = build_model("ESRNet", inch=2, basech=8, num_frame=3,
                        upsampler="pixelshuffle").to(DEV).to(torch.bfloat16)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    x = _rand_bf16(2, 3, 2, 64, 64, seed=33).abs()
    gt = _rand_bf16(2, 2, 64, 64, seed=34).abs()
    model.reset_states()
    pred = model(x)
    loss = F.mse_loss(pred.float(), gt.float())
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g.float()).all() for g in grads)
    opt.step()
    assert torch.isfinite(loss)


def test_esrnet_forward_uses_native_convs():
    """The bf16 model forward must actually dispatch to the native conv
    kernels (guards against silent fallback to MIOpen)."""
    from esr_amd.models import build_model
    from esr_amd.ops import conv as conv_mod
    model = build_model("ESRNet", inch=2, basech=8, num_frame=3,
                        upsampler="pixelshuffle").to(DEV).to(torch.bfloat16)
    x = _rand_bf16(1, 3, 2, 64, 64, seed=41).abs()
    conv_mod.stats["native_calls"] = 0
    with torch.no_grad():
        model.reset_states()
        model(x)
    # ESRNet at basech 8 runs ~30 convs per forward; all the deep ones
    # (Cout>=32 or Cin>=32) must go native
    assert conv_mod.stats["native_calls"] >= 20, \
        f"only {conv_mod.stats['native_calls']} native conv dispatches"


def test_wgrad_deterministic_across_runs():
    """The two-stage wgrad reduction has a FIXED summation order (no fp32
    atomics): identical inputs give bitwise-identical dW across runs —
    the reference's atomic col2im cannot promise this (SURVEY §5 race
    detection)."""
    from esr_amd.ops.native import require_ext
    ext = require_ext()
    x = _rand_bf16(16, 64, 32, 32, seed=3)
    dy = _rand_bf16(16, 64, 32, 32, seed=4)
    ref = ext.conv2d_wgrad_mfma(x, dy, 3, 1, 64, 64).clone()
    for _ in range(3):
        again = ext.conv2d_wgrad_mfma(x, dy, 3, 1, 64, 64)
        assert torch.equal(ref, again), "wgrad not bitwise deterministic"
