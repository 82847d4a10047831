"""Native bf16/fp16 NCHW convolution dispatch (hand-written gfx950 kernels).

Replaces MIOpen + NCHW<->NHWC transposes + autocast casts on the conv
shapes ESRNet runs (reference ConvLayer ESR:models/submodules.py:159-200,
ConvGRU convs :474-514): 3x3 stride-1/2 pad-1 and 1x1 convs, bias and
ReLU/sigmoid/tanh fused into the conv epilogue.

Dispatch (see conv2d.hip; thresholds from tools/bench_conv.py measured on
MI355X, profiles/README.md):
  * MFMA implicit-GEMM kernel for Cout >= 32 — measured 1.0-2.0x MIOpen
    bf16 on the deep/mid shapes;
  * direct VALU kernel for Cin >= 32 with tiny Cout (attention/kernel
    convs, 1.2-1.3x);
  * register-strip VALU v2 for the tiny-channel class (Cin and Cout both
    < 32): 8-wide output strips x all cout per thread, weights broadcast
    from LDS — head 2.7x, tail 1.3x vs MIOpen; the stride-2 enc1 shape
    (0.67x) stays on MIOpen.
Backward defaults to torch's aten.convolution_backward (MIOpen bf16).
The native backward kernels are implemented, oracle-tested and measured
(tools/bench_conv.py --wgrad / --bwd, MI355X):
  * weight-grad (conv2d_wgrad_s1: 4-row MFMA chunks, rolling X window,
    DETERMINISTIC two-stage reduction — no fp32 atomics) reaches
    0.9-1.1x MIOpen wrw on the wide 32x32 shapes (resblock 1.07x,
    192->64 1.05x, dense 1.03x) after a 7x optimization ladder driven by
    ablation (the original per-address atomic flush was 70-87% of the
    kernel; ESR_WGRAD_ABL still exposes the ablation arms);
  * stride-1 input-grad reuses the forward kernels with packed
    flipped/transposed weights; stride-2 dgrad is a VALU gather kernel.
End-to-end the native backward composition still measures 0.8x of
MIOpen's fused bwd on the whole shape set, so aten stays the default;
ESR_CONV_BWD=native forces all-native, =auto uses native for deep
stride-1 shapes.  fp32 falls back to torch everywhere (the CPU oracle of
the parity tests).

Bias grad: both backward branches take db from the native kernels, not
from aten.  With an activation, act_grad_bias writes dpre (act_grad's
arithmetic, bit-equal) and sums the rounded values per channel in the same
pass; without one, bias_grad is a read-only pass over dy.  Both reduce in
two stages in a fixed order (no atomics, two runs bit-equal; chain length in
conv2d.hip; a gradient with B*H*W >= 2^31 - 4096 per channel, or a chain
above 2^11, is an error there, not a fall-back to torch's sum, and the DCN
bias shares that), and aten.convolution_backward is called with
output_mask[2] = False, which drops ATen's strided NCHW sum((0,2,3)) over
dpre (8.15 ms, 6.3 % of the flagship step's kernel time; the native bias
grads take 1.23 ms — profiles/README.md, "conv bias gradient").

fp16 (fp16 autocast, or plain fp16 tensors): the three forward kernels,
act_grad, act_grad_bias and bias_grad have an fp16 instantiation
(mfma_f32_16x16x32_f16, same tiles and LDS layout, fp32 accumulate, one
round-to-nearest-even on store; overflow saturates to +/-inf like torch's
cast).  The native weight-grad and input-grad kernels are bf16-only, so the
fp16 backward is ALWAYS native act_grad(_bias) + aten.convolution_backward
(MIOpen fp16), whatever ESR_CONV_BWD says.  Nothing here scales the loss:
fp16 gradients below 6e-8 flush to zero unless the trainer's opt-in
`loss_scale` config key is set (device-side in esr_amd/optim FlatAdam,
torch.amp.GradScaler otherwise).

Env: ESR_NATIVE_CONV=0 disables the native path (A/B benching);
     ESR_CONV_BWD=native routes the bf16 backward to the native kernels;
     ESR_BIAS_GRAD=aten takes the bias grad from aten.convolution_backward
     again (A/B; default native, see _BIAS_GRAD_DEFAULT);
     ESR_NATIVE_FP16=0 restores the MIOpen fall-back (and the fp32-island
     deformable conv) for fp16 only; default on (see _FP16_DEFAULT).
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from .native import get_ext

__all__ = ["conv2d_act", "native_conv_supported", "ACT_IDS"]

ACT_IDS = {None: 0, "none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}

# dispatch telemetry: tests / profiling assert the native path really runs
# ("native_calls_fp16" counts the fp16 subset, in addition to native_calls)
# "native_bias_grad" counts backward calls whose bias grad came from
# act_grad_bias / bias_grad
stats = {"native_calls": 0, "native_calls_fp16": 0, "native_bias_grad": 0}

_MFMA_MIN_COUT = 32   # below this the MFMA M-tile would idle; use VALU
_CIK = 32             # K-chunk of the MFMA kernel (pad Cin up to this)


# Default of ESR_NATIVE_FP16.  The bf16 dispatch thresholds were measured
# against MIOpen bf16, so the fp16 default rests on its own measurement:
# config 5 (4x DVS 180x240, fp16 autocast) end to end, 3 alternating runs,
# 261.1 frames/s with the path on vs 255.8 on MIOpen (+2.0%; run-to-run
# range 1.0 / 2.7 frames/s, no overlap) — profiles/README.md, "fp16".
_FP16_DEFAULT = "1"


# Default of ESR_BIAS_GRAD: "native" = act_grad_bias / bias_grad, "aten" =
# the bias output of aten.convolution_backward (a strided NCHW reduce_kernel
# pass over dpre).  Flagship step end to end, parent and tree alternated
# three times: 130.82 / 130.86 / 130.71 ms on aten, 124.13 / 124.02 /
# 123.61 ms native (-6.9 ms, 5.3 %; ranges 0.15 / 0.52 ms, no overlap) —
# profiles/README.md, "conv bias gradient".
_BIAS_GRAD_DEFAULT = "native"


def _enabled() -> bool:
    return os.environ.get("ESR_NATIVE_CONV", "1") != "0"


def _native_bias_grad() -> bool:
    return os.environ.get("ESR_BIAS_GRAD", _BIAS_GRAD_DEFAULT) != "aten"


def native_fp16_enabled() -> bool:
    return os.environ.get("ESR_NATIVE_FP16", _FP16_DEFAULT) != "0"


def compute_dtype(autocast_on: bool, autocast_dtype, x_dtype,
                  fp16_enabled: bool | None = None):
    """Dtype half of the dispatch predicate (pure, CPU-testable).

    Takes the autocast state and the input dtype; returns the 16-bit dtype
    the native kernels should run in, or None for "fall back to torch".
    Under autocast the autocast dtype decides (operands are cast to it);
    outside autocast a plain bf16/fp16 tensor is taken as it is.
    """
    dt = autocast_dtype if autocast_on else x_dtype
    if dt == torch.bfloat16:
        return torch.bfloat16
    if dt == torch.float16:
        if fp16_enabled is None:
            fp16_enabled = native_fp16_enabled()
        return torch.float16 if fp16_enabled else None
    return None


def _ceil(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _pack(w: torch.Tensor) -> torch.Tensor:
    """[O, I, k, k] -> [k*k, O_p, I_p], O_p = ceil16(O), I_p = ceil32(I);
    keeps w's dtype (bf16 or fp16).

    Matches the A-fragment addressing of conv2d_fwd_mfma_kernel: row = cout,
    contiguous 8-channel groups along ci.
    """
    O, I, k, _ = w.shape
    t = w.permute(2, 3, 0, 1).reshape(k * k, O, I)
    op, ip = _ceil(O, 16), _ceil(I, _CIK)
    if op != O or ip != I:
        t = F.pad(t, (0, ip - I, 0, op - O))
    return t.contiguous()


class _NativeConv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, act_id):
        ext = get_ext()
        ks = w.shape[2]
        cout, cin = w.shape[0], w.shape[1]
        bias_f = bias.float() if bias is not None else None
        if cout >= _MFMA_MIN_COUT:
            y = ext.conv2d_fwd_mfma(x, _pack(w), bias_f, cout, ks, stride,
                                    act_id)
        elif cin < _MFMA_MIN_COUT and x.shape[-1] % 8 == 0:
            # tiny-channel head/tail class: register-strip kernel
            # (2.7x / 1.3x MIOpen on head/tail, bench_conv --valu2).
            # Widths not divisible by 8 conservatively take the v1 kernel
            # (their strip stores are row-misaligned; the suspected odd-W
            # failure later turned out to be a test-harness fp32-mean
            # artifact, but v2 at odd W is GPU-unverified) — every real
            # model shape is /8-padded anyway (ESRNet.DOWN_SCALE).
            y = ext.conv2d_fwd_valu2(x, w.contiguous(), bias_f, stride,
                                     act_id)
        else:
            y = ext.conv2d_fwd_valu(x, w.contiguous(), bias_f, stride, act_id)
        ctx.save_for_backward(x, w, y)
        ctx.stride_ = stride
        ctx.act_id = act_id
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = get_ext()
        x, w, y = ctx.saved_tensors
        stride, act_id = ctx.stride_, ctx.act_id
        ks = w.shape[2]
        cout, cin = w.shape[0], w.shape[1]
        dy = dy.contiguous()
        # bias grad: per-channel sum of the rounded dpre, produced by the
        # pass that writes dpre (act_grad_bias), or by a read-only pass over
        # dy when there is no activation (bias_grad)
        fused_db = ctx.has_bias and _native_bias_grad()
        db = None
        if fused_db:
            stats["native_bias_grad"] += 1
            if act_id:
                dpre, db = ext.act_grad_bias(dy, y, act_id)[:2]
            else:
                dpre, db = dy, ext.bias_grad(dy)[0]
        else:
            dpre = ext.act_grad(dy, y, act_id) if act_id else dy
        aten_db = ctx.has_bias and not fused_db

        # default aten: the native backward kernels (v2) are oracle-correct
        # but still measured behind MIOpen's wrw/bwd igemm on the deep
        # shapes (tools/bench_conv.py --bwd); "auto" switches stride-1
        # deep shapes native once they win
        mode = os.environ.get("ESR_CONV_BWD", "aten")
        native_bwd = mode == "native" or (
            mode == "auto" and stride == 1 and cin >= _MFMA_MIN_COUT)
        if x.dtype != torch.bfloat16:
            # wgrad/dgrad kernels are bf16-only: fp16 always takes aten
            native_bwd = False
        if not native_bwd:
            dx, dw, db_aten = torch.ops.aten.convolution_backward(
                dpre, x, w, [cout] if aten_db else None,
                [stride, stride], [ks // 2, ks // 2], [1, 1], False, [0, 0],
                1, [True, True, aten_db])
            return dx, dw, db_aten if aten_db else db, None, None

        # --- native backward path (ESR_CONV_BWD=native) ---
        # input grad: stride-1 is this conv with flipped/transposed weights
        if stride == 1:
            wt = w.transpose(0, 1)
            if ks == 3:
                wt = wt.flip((2, 3))
            if cin >= _MFMA_MIN_COUT:
                dx = ext.conv2d_fwd_mfma(dpre, _pack(wt), None, cin, ks, 1, 0)
            else:
                dx = ext.conv2d_fwd_valu(dpre, wt.contiguous(), None, 1, 0)
        else:
            dx = ext.conv2d_dgrad_s2(dpre, w.contiguous(),
                                     x.shape[2], x.shape[3])

        # weight grad: MFMA split-K into padded fp32 (transposed
        # [Cin_p, Cout_p] scratch for line-parallel atomics), then slice
        dwp = ext.conv2d_wgrad_mfma(x, dpre, ks, stride,
                                    _ceil(cin, 16), _ceil(cout, 16))
        dw = dwp.permute(1, 0, 2, 3)[:cout, :cin].to(w.dtype)
        if aten_db:
            db = dpre.sum(dim=(0, 2, 3), dtype=torch.float32).to(w.dtype)
        return dx, dw, db, None, None


def shape_supported(conv: torch.nn.Conv2d, dtype=None) -> bool:
    """Shape half of the dispatch predicate (CPU-testable).

    `dtype` is the compute dtype; None or bf16 gives the bf16 table, fp16
    may route further classes back to MIOpen (measured against MIOpen fp16).
    """
    if conv.out_channels < _MFMA_MIN_COUT and conv.in_channels < _MFMA_MIN_COUT:
        # tiny-channel class: the v2 register-strip kernel beats MIOpen at
        # stride 1 (head 2.7x, tail 1.3x); the stride-2 enc1 shape still
        # loses (0.67x) and stays on MIOpen (tools/bench_conv.py --valu2)
        if conv.stride[0] != 1:
            return False
    if dtype == torch.float16:
        # fp16 only — measured against MIOpen fp16, which is faster than
        # MIOpen bf16 on these classes (tools/bench_conv.py --dtype fp16,
        # two runs, run-to-run spread ~3%; profiles/README.md "fp16"):
        if conv.out_channels < _MFMA_MIN_COUT <= conv.in_channels:
            # v1 direct VALU class: attention map 64->1 3x3 0.79-0.80x
            # (the 1x1 64->2 member of the class: not measured)
            return False
        if conv.out_channels >= 128 and conv.kernel_size == (3, 3) \
                and conv.stride == (1, 1):
            # wide 3x3 stride-1: gru ur 128->128 0.73-0.75x, resblock
            # 192->192 0.87-0.88x, recon1 64->128 0.86-0.88x
            return False
    if conv.groups != 1 or conv.dilation != (1, 1):
        return False
    kh, kw = conv.kernel_size
    sh, sw = conv.stride
    ph, pw = conv.padding if isinstance(conv.padding, tuple) else \
        (conv.padding, conv.padding)
    if kh != kw or sh != sw or ph != pw:
        return False
    if (kh, sh) not in ((3, 1), (3, 2), (1, 1)):
        return False
    if ph != kh // 2:
        return False
    return True


def native_conv_supported(x: torch.Tensor, conv: torch.nn.Conv2d,
                          dtype=None) -> bool:
    if not (_enabled() and x.is_cuda and get_ext() is not None):
        return False
    return shape_supported(conv, dtype)


def conv2d_act(x: torch.Tensor, conv: torch.nn.Conv2d, act: str | None):
    """Fused conv+bias+act.  Returns the native-kernel result when the shape
    and dtype qualify, else None (caller falls back to torch)."""
    if act not in ACT_IDS or not (x.is_cuda and _enabled()):
        return None
    autocast_on = torch.is_autocast_enabled()
    dt = compute_dtype(
        autocast_on,
        torch.get_autocast_dtype("cuda") if autocast_on else None, x.dtype)
    if dt is None or not native_conv_supported(x, conv, dt):
        return None
    if x.dtype != dt:
        x = x.to(dt)
    w, b = conv.weight, conv.bias
    if w.dtype != dt:
        w = w.to(dt)                       # autograd records the cast:
        if b is not None:                  # grads flow back to fp32 masters
            b = b.to(dt)
    stats["native_calls"] += 1
    if dt == torch.float16:
        stats["native_calls_fp16"] += 1
    return _NativeConv2dFn.apply(x.contiguous(), w, b, conv.stride[0],
                                 ACT_IDS[act])
