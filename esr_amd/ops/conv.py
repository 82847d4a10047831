"""Native bf16/fp16 NCHW convolution dispatch (hand-written gfx950 kernels).

Replaces MIOpen + NCHW<->NHWC transposes + autocast casts on the conv
shapes ESRNet runs (reference ConvLayer ESR:models/submodules.py:159-200,
ConvGRU convs :474-514): 3x3 stride-1/2 pad-1 and 1x1 convs, bias and
ReLU/sigmoid/tanh fused into the conv epilogue.

Dispatch (see conv2d.hip; thresholds from tools/bench_conv.py measured on
MI355X, profiles/README.md):
  * stride-1 deep class (3x3 pad 1 / 1x1, Cin >= 32 and Cout >= 32, bf16):
    the 8x32-tile MFMA core conv2d_s1 (16-byte staging loads transposed in
    registers, patch staged once for all Cout, double-buffered, 16-byte
    stores) — 1.3-3.3x the older MFMA kernel on every shape, same bits
    (ESR_CONV_FWD=mfma keeps the older kernel);
  * MFMA implicit-GEMM kernel conv2d_fwd_mfma for the rest of Cout >= 32
    (stride 2, Cin < 32, fp16) — measured 1.0-2.0x MIOpen bf16;
  * direct VALU kernel for Cin >= 32 with tiny Cout (attention/kernel
    convs, 1.2-1.3x);
  * register-strip VALU v2 for the tiny-channel class (Cin and Cout both
    < 32): 8-wide output strips x all cout per thread, weights broadcast
    from LDS — head 2.7x, tail 1.3x vs MIOpen; the stride-2 enc1 shape
    (0.67x) stays on MIOpen.
Backward (bf16): ESR_CONV_BWD defaults to "auto", which routes per gradient
by measurement (tools/bench_conv.py --bwd-parts, table at _CONV_BWD_DEFAULT)
inside the stride-1 deep class and leaves every other class on
aten.convolution_backward (MIOpen bf16):
  * input grad, 3x3: conv2d_s1 with dgrad=True — the same core, its pack
    launch reading the weights flipped and transposed in place (no
    transpose/flip/permute/pad copies on the host side); 1.4-3.5x aten,
    whose time includes its NCHW<->NHWC transposes.  The 1x1 stays on aten;
  * weight grad: conv2d_wgrad_s1 (4-row MFMA chunks, rolling X window,
    DETERMINISTIC two-stage reduction — no fp32 atomics; the second stage
    writes [Cout, Cin, k, k] bf16, so no zero fill, permute, slice or cast
    follows) at Cin >= 192, where it wins by 3-7 %; elsewhere it is
    0.57-0.95x of MIOpen's wrw and aten is called with
    output_mask = [False, True, False].  ESR_WGRAD_ABL still exposes the
    ablation arms of its first stage;
  * stride-2 input grad is a VALU gather kernel, stride-2 weight grad the
    older atomic kernel: both only under ESR_CONV_BWD=native.
ESR_CONV_BWD=native forces every gradient native, =aten every gradient to
aten.  fp32 falls back to torch everywhere (the CPU oracle of the parity
tests).

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
     ESR_CONV_BWD=auto (default) | native | aten | dgrad (A/B: input grad
     native, weight grad aten): bf16 backward routing;
     ESR_CONV_FWD=auto (default) | core | mfma: forward kernel of the
     stride-1 deep class;
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


# Default of ESR_CONV_BWD, and what "auto" routes native inside the deep
# stride-1 class (bf16, 3x3 pad 1 / 1x1, Cin >= 32 and Cout >= 32); every
# other class stays on aten.  From tools/bench_conv.py --bwd-parts on MI355X
# at the flagship's per-call batches (profiles/README.md, "conv backward:
# native default"; ms, whole class summed unless a shape is named):
#   input grad, 3x3: conv2d_s1 1.4-3.5x aten on every shape (2.05 against
#     4.03 ms; the older native kernel 4.67) -> native;
#   input grad, 1x1 128->64: 0.061 against aten's 0.038 -> aten;
#   weight grad: conv2d_wgrad_s1 wins at Cin 192 only (resblock 0.950
#     against 1.017, 192->64 0.381 / 0.382 against 0.403 / 0.392) and is
#     0.57-0.95x elsewhere (gru 128->128 0.831 against 0.626) -> native at
#     Cin >= 192, 3x3;
#   whole backward of one conv, act and bias grad included: all aten 9.41,
#     all native 8.30, this routing 7.62 (put together from those columns).
_CONV_BWD_DEFAULT = "auto"
_AUTO_WGRAD_MIN_CIN = 192

# Default of ESR_CONV_FWD: the forward of the same class takes conv2d_s1,
# 2.03 against 4.91 ms for conv2d_fwd_mfma over the class (1.3-3.3x on every
# shape, the 1x1 0.039 against 0.061), same bits (same table).
_CONV_FWD_DEFAULT = "auto"


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
        if fwd_core_route(os.environ.get("ESR_CONV_FWD", _CONV_FWD_DEFAULT),
                          x.dtype == torch.bfloat16, ks, stride, cin, cout):
            y = ext.conv2d_s1(x, w.contiguous(), bias_f, act_id, False)
        elif cout >= _MFMA_MIN_COUT:
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

        dgrad_native, wgrad_native = bwd_route(
            os.environ.get("ESR_CONV_BWD", _CONV_BWD_DEFAULT),
            x.dtype == torch.bfloat16, ks, stride, cin, cout)
        pad = [ks // 2, ks // 2]
        if not (dgrad_native and wgrad_native):
            # aten computes whatever is not routed native; its bias output
            # only with ESR_BIAS_GRAD=aten
            dx, dw, db_aten = torch.ops.aten.convolution_backward(
                dpre, x, w, [cout] if aten_db else None,
                [stride, stride], pad, [1, 1], False, [0, 0], 1,
                [not dgrad_native, not wgrad_native, aten_db])
            if aten_db:
                db = db_aten
        elif aten_db:
            db = dpre.sum(dim=(0, 2, 3), dtype=torch.float32).to(w.dtype)

        if dgrad_native:
            if stride == 1 and cin >= _MFMA_MIN_COUT:
                # the 8x32-tile core with the weights indexed flipped and
                # transposed by its pack launch
                dx = ext.conv2d_s1(dpre, w.contiguous(), None, 0, True)
            elif stride == 1:
                wt = w.transpose(0, 1)
                if ks == 3:
                    wt = wt.flip((2, 3))
                dx = ext.conv2d_fwd_valu(dpre, wt.contiguous(), None, 1, 0)
            else:
                dx = ext.conv2d_dgrad_s2(dpre, w.contiguous(),
                                         x.shape[2], x.shape[3])
        if wgrad_native:
            if stride == 1:
                # two-stage deterministic reduction; the second stage writes
                # [Cout, Cin, k, k] bf16, rounded once from the fp32 sum
                dw = ext.conv2d_wgrad_s1(x, dpre, ks)
            else:
                # stride 2: split-K into padded transposed fp32, then slice
                dwp = ext.conv2d_wgrad_mfma(x, dpre, ks, stride,
                                            _ceil(cin, 16), _ceil(cout, 16))
                dw = dwp.permute(1, 0, 2, 3)[:cout, :cin].to(w.dtype)
        return dx, dw, db, None, None


def bwd_route(mode: str, is_bf16: bool, ks: int, stride: int, cin: int,
              cout: int) -> tuple[bool, bool]:
    """Backward half of the dispatch (pure, CPU-testable): (input grad
    native, weight grad native) for ESR_CONV_BWD = `mode`.

    "aten" and "native" route everything one way, "dgrad" sends only the
    input grad native (an A/B arm); anything else ("auto", the default)
    follows the measured table at _CONV_BWD_DEFAULT.  The
    native wgrad/dgrad kernels are bf16-only: fp16 always takes aten.
    """
    if not is_bf16 or mode == "aten":
        return False, False
    if mode == "native":
        return True, True
    if mode == "dgrad":
        # A/B arm of tools/bench_conv.py --bwd-parts: input grad native,
        # weight grad on aten, wherever "native" would apply
        return True, False
    deep_s1 = stride == 1 and ks in (1, 3) and \
        cin >= _MFMA_MIN_COUT and cout >= _MFMA_MIN_COUT
    if not deep_s1 or ks != 3:
        return False, False
    return True, cin >= _AUTO_WGRAD_MIN_CIN


def fwd_core_route(mode: str, is_bf16: bool, ks: int, stride: int, cin: int,
                   cout: int) -> bool:
    """Forward of the deep stride-1 class on the 8x32-tile core
    (conv2d_s1) instead of conv2d_fwd_mfma (pure, CPU-testable).
    ESR_CONV_FWD = "mfma" keeps every shape on the older kernel, "core"
    and "auto" take the core on the whole class, where it was measured
    faster on every shape (see _CONV_FWD_DEFAULT).  fp16 stays on the older kernel: the
    core's fp16 instantiation is built but was not measured."""
    if mode == "mfma" or not is_bf16:
        return False
    deep_s1 = stride == 1 and ks in (1, 3) and \
        cin >= _MFMA_MIN_COUT and cout >= _MFMA_MIN_COUT
    return deep_s1


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
