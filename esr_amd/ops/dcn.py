"""Modulated deformable convolution (DCNv2) for CDNA4.

The reference implements this as a CUDA extension
(ESR:models/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:125-327, host composition
ESR:models/DCNv2/src/cuda/dcn_v2_cuda.cu:20-216).  Here:

  * ``_deform_conv2d_torch`` — a fully vectorized pure-torch implementation
    (bilinear gather + GEMM).  Autograd-differentiable, runs on CPU and GPU;
    it is the oracle the HIP kernels are verified against and the fallback
    when the native extension is unavailable (CPU-only boxes).
  * The HIP path (esr_amd/ops/native/deform_conv.hip) does batched
    deformable im2col on gfx950 and a hipBLASLt GEMM through at::bmm, with a
    custom backward (col2im scatter + coordinate gradients).  Unlike the
    reference, the backward is batched — the reference loops per sample
    (ESR:models/DCNv2/src/cuda/dcn_v2_cuda.cu:150).  fp32, bf16 and fp16
    run natively (16-bit loads, fp32 compute); ESR_NATIVE_FP16=0 sends
    fp16 through fp32 islands instead.  The opt-in fused MFMA forward
    (ESR_DCN_FUSED=1) is fp32-only.
  * The backward has two paths for the input / offset / mask grads,
    chosen per call by ``dcn_bwd_path``: "fused" (one kernel, the group's
    input-grad planes summed in LDS; needs (C/dg)*H*W*4 B <= 64 KiB) and
    "split" (global-atomic col2im + cast + coordinate kernel).  The
    default takes the fused kernel wherever it applies; ESR_DCN_BWD=split
    restores the split path for A/B runs, and ``stats`` counts what ran.
  * The forward's im2col columns are saved for the weight-grad GEMM
    (B*C*K*Ho*Wo elements held until the backward); ESR_DCN_SAVE_COLS=0
    rebuilds them in the backward instead.

Layout conventions (identical to the reference kernels):
  offset: [B, dg*2*kh*kw, Ho, Wo] — per deformable group, per kernel index k
          channel 2k is the H offset and 2k+1 the W offset.
  mask:   [B, dg*kh*kw, Ho, Wo].
"""

from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

from .conv import native_fp16_enabled
from .native import get_ext, require_ext

__all__ = ["modulated_deform_conv2d", "DeformAlign2d",
           "deform_conv2d_backward", "dcn_bwd_fused_applicable",
           "dcn_bwd_path"]


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _deform_conv2d_torch(input, offset, mask, weight, bias,
                         stride, padding, dilation, deformable_groups):
    """Reference (oracle) implementation: bilinear gather + GEMM.

    Matches ESR:models/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:125-195 including
    zero-padded bilinear sampling outside the image.

    Boundary rule, the HIP kernels' (sample_in_range in deform_conv.hip) and
    the reference's: a sample at (h, w) counts only where -1 < h < H and
    -1 < w < W.  The constant mask below changes no value (at h = -1 the
    only corner inside the image has weight 0), but it fixes the offset
    gradient: at an integer coordinate it is the one-sided derivative of
    the cell [floor, floor + 1], and at h <= -1, w <= -1, h >= H or w >= W
    both components are zero.
    """
    B, C, H, W = input.shape
    Cout, Cin, kh, kw = weight.shape
    assert Cin == C, "grouped conv not supported (reference has groups=1)"
    sh, sw = stride
    ph, pw = padding
    dh, dw = dilation
    dg = deformable_groups
    K = kh * kw
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    dev, dt = input.device, input.dtype

    off = offset.view(B, dg, K, 2, Ho, Wo)
    msk = mask.view(B, dg, K, Ho, Wo)

    base_h = (torch.arange(Ho, device=dev, dtype=dt) * sh - ph).view(1, 1, 1, Ho, 1)
    base_w = (torch.arange(Wo, device=dev, dtype=dt) * sw - pw).view(1, 1, 1, 1, Wo)
    ker_h = (torch.arange(kh, device=dev, dtype=dt) * dh).repeat_interleave(kw).view(1, 1, K, 1, 1)
    ker_w = (torch.arange(kw, device=dev, dtype=dt) * dw).repeat(kh).view(1, 1, K, 1, 1)

    h_im = base_h + ker_h + off[:, :, :, 0]          # [B,dg,K,Ho,Wo]
    w_im = base_w + ker_w + off[:, :, :, 1]

    h0 = h_im.floor()
    w0 = w_im.floor()
    lh = h_im - h0
    lw = w_im - w0
    in_range = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)

    inp = input.view(B, dg, C // dg, H * W)
    cols = torch.zeros(B, dg, C // dg, K, Ho, Wo, device=dev, dtype=dt)
    for dy in (0, 1):
        for dx in (0, 1):
            hc = h0 + dy
            wc = w0 + dx
            valid = (hc >= 0) & (hc < H) & (wc >= 0) & (wc < W)
            wgt = ((lh if dy else 1 - lh) * (lw if dx else 1 - lw)) \
                * (valid & in_range)
            idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long()
            idx_f = idx.view(B, dg, 1, K * Ho * Wo).expand(-1, -1, C // dg, -1)
            gathered = torch.gather(inp, 3, idx_f).view(B, dg, C // dg, K, Ho, Wo)
            cols = cols + gathered * wgt.unsqueeze(2)
    cols = cols * msk.unsqueeze(2)
    # column order c_col = c_im * K + k (ESR:.../dcn_v2_im2col_cuda.cu:150)
    cols = cols.reshape(B, C * K, Ho * Wo)
    out = torch.bmm(weight.view(Cout, C * K).unsqueeze(0).expand(B, -1, -1), cols)
    out = out.view(B, Cout, Ho, Wo)
    if bias is not None:
        out = out + bias.view(1, Cout, 1, 1)
    return out


# The fused backward keeps one deformable group's input-grad planes in LDS
# as fp32; 64 KiB is what a block may ask for without opting in to more.
BWD_FUSED_LDS_MAX = 64 * 1024

# dispatch telemetry, as ops/conv.py's: which backward path each call took
# and whether it reused the forward's columns
stats = {"bwd_fused": 0, "bwd_split": 0, "bwd_cols_saved": 0}


def dcn_bwd_fused_applicable(C, dg, H, W):
    """Whether the fused backward kernel covers an input of C channels in dg
    deformable groups on an H x W image: the group's C/dg fp32 planes must
    fit in LDS.  deform_conv.hip checks the same rule (dcn_bwd_fused_fits)."""
    return C % dg == 0 and (C // dg) * H * W * 4 <= BWD_FUSED_LDS_MAX


def dcn_bwd_path(C, dg, H, W, path="auto"):
    """Resolve a backward path selector to "fused" or "split".  "auto"
    follows ESR_DCN_BWD (fused / split) when set, else takes the fused
    kernel wherever it applies; an explicit selector wins over the
    environment.  "fused" on a shape it does not cover is an error."""
    if path not in ("auto", "fused", "split"):
        raise ValueError(f"DCN backward path {path!r}: auto, fused or split")
    if path == "auto":
        path = os.environ.get("ESR_DCN_BWD", "auto")
        if path not in ("auto", "fused", "split"):
            raise ValueError(f"ESR_DCN_BWD={path!r}: auto, fused or split")
    fits = dcn_bwd_fused_applicable(C, dg, H, W)
    if path == "fused" and not fits:
        raise ValueError(
            f"DCN fused backward needs (C/dg)*H*W*4 B <= {BWD_FUSED_LDS_MAX}; "
            f"C={C} dg={dg} {H}x{W} needs {C // max(dg, 1) * H * W * 4}")
    if path == "auto":
        path = "fused" if fits else "split"
    return path


def save_cols_enabled():
    """ESR_DCN_SAVE_COLS=0: drop the forward's im2col columns and rebuild
    them in the backward (B*C*K*Ho*Wo elements less between the two)."""
    return os.environ.get("ESR_DCN_SAVE_COLS", "1") != "0"


def deform_conv2d_backward(input, offset, mask, weight, grad_out,
                           stride, padding, dilation, deformable_groups,
                           cols=None, path="auto"):
    """The native backward on contiguous GPU tensors: the five grads
    (input, offset, mask, weight, bias).  `cols` are the forward's columns
    if the caller kept them; `path` is auto / fused / split."""
    B, C, H, W = input.shape
    path = dcn_bwd_path(C, deformable_groups, H, W, path)
    stats["bwd_" + path] += 1
    if cols is not None:
        stats["bwd_cols_saved"] += 1
    return require_ext().deform_conv2d_backward_cols(
        input, offset, mask, weight, grad_out, cols,
        stride[0], stride[1], padding[0], padding[1],
        dilation[0], dilation[1], deformable_groups, path)


class _DeformConvHIP(torch.autograd.Function):
    """Autograd wrapper over the native HIP deformable-conv kernels."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias,
                stride, padding, dilation, deformable_groups):
        ext = get_ext()
        # save the CONTIGUOUS tensors: the HIP backward indexes its inputs
        # with contiguous strides (DeformAlign2d's offset is a channel slice
        # and non-contiguous for B>1 — saving the original silently corrupts
        # the backward)
        input = input.contiguous()
        offset = offset.contiguous()
        mask = mask.contiguous()
        weight = weight.contiguous()
        geom = (stride[0], stride[1], padding[0], padding[1],
                dilation[0], dilation[1], deformable_groups)
        # keep the im2col columns for the weight-grad GEMM unless switched
        # off; the opt-in fused MFMA forward never builds them
        if save_cols_enabled() and os.environ.get("ESR_DCN_FUSED") != "1":
            out, cols = ext.deform_conv2d_forward_cols(
                input, offset, mask, weight, bias, *geom)
            ctx.save_for_backward(input, offset, mask, weight, cols)
        else:
            out = ext.deform_conv2d_forward(
                input, offset, mask, weight, bias, *geom)
            ctx.save_for_backward(input, offset, mask, weight)
        ctx.conf = (stride, padding, dilation, deformable_groups)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        input, offset, mask, weight, *cols = ctx.saved_tensors
        stride, padding, dilation, dg = ctx.conf
        gi, go, gm, gw, gb = deform_conv2d_backward(
            input, offset, mask, weight, grad_out.contiguous(),
            stride, padding, dilation, dg, cols=cols[0] if cols else None)
        return (gi, go, gm, gw, gb if ctx.has_bias else None,
                None, None, None, None)


def modulated_deform_conv2d(input, offset, mask, weight, bias=None,
                            stride=1, padding=0, dilation=1,
                            deformable_groups=1):
    """Functional modulated deformable conv (DCNv2 semantics).

    Dispatches to the gfx950 HIP kernels on GPU tensors; raises if the
    native extension is missing on a GPU box (no silent eager fallback).
    """
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if input.is_cuda:
        ext = get_ext()
        if ext is None:
            raise RuntimeError(
                "esr_amd native extension not built - GPU deformable conv "
                "requires the HIP kernels (run __graft_entry__.build())")
        if input.dtype == torch.bfloat16 or (
                input.dtype == torch.float16 and native_fp16_enabled()):
            # 16-bit-native path: the HIP kernels load bf16/fp16 and compute
            # fp32 (the input grad is summed in fp32 and rounded once) —
            # halves the column-buffer/backward HBM traffic vs the r1
            # fp32-island design.
            dt = input.dtype
            w16 = weight.to(dt)
            b16 = None if bias is None else bias.to(dt)
            return _DeformConvHIP.apply(
                input, offset.to(dt), mask.to(dt),
                w16, b16, stride, padding, dilation, deformable_groups)
        if input.dtype == torch.float16:
            # ESR_NATIVE_FP16=0: the older fp32-island route
            out = _DeformConvHIP.apply(
                input.float(), offset.float(), mask.float(), weight.float(),
                None if bias is None else bias.float(),
                stride, padding, dilation, deformable_groups)
            return out.to(input.dtype)
        return _DeformConvHIP.apply(input, offset, mask, weight, bias,
                                    stride, padding, dilation, deformable_groups)
    return _deform_conv2d_torch(input, offset, mask, weight, bias,
                                stride, padding, dilation, deformable_groups)


class DeformAlign2d(nn.Module):
    """Deformable alignment layer: offsets/masks predicted from a *separate*
    feature map (the reference's ``DCN_sep``, ESR:models/DCNv2/dcn_v2.py:197-227).

    ``forward(input, feat)`` aligns `input` using offsets predicted from
    `feat`.  Offset/mask conv is zero-initialized so the layer starts as
    0.5 * standard conv (sigmoid(0) mask).
    """

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, dilation=1, deformable_groups=1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.deformable_groups = deformable_groups

        kh, kw = self.kernel_size
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kh, kw))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        n = in_channels * kh * kw
        stdv = 1.0 / math.sqrt(n)
        nn.init.uniform_(self.weight, -stdv, stdv)

        self.conv_offset_mask = nn.Conv2d(
            in_channels, deformable_groups * 3 * kh * kw,
            kernel_size=self.kernel_size, stride=self.stride,
            padding=self.padding, bias=True)
        nn.init.zeros_(self.conv_offset_mask.weight)
        nn.init.zeros_(self.conv_offset_mask.bias)

    def forward(self, input, feat):
        # The conv's output channels are interpreted directly as
        # [offset (2*dg*K) | mask (dg*K)] — the reference's chunk+cat
        # (ESR:models/DCNv2/dcn_v2.py:218-219) only permutes learned
        # channels, so skipping it is math-equivalent under training and
        # saves a concat launch per call.
        from .conv import conv2d_act
        om = conv2d_act(feat, self.conv_offset_mask, None)
        if om is None:
            om = self.conv_offset_mask(feat)
        kh, kw = self.kernel_size
        n_off = self.deformable_groups * 2 * kh * kw
        offset = om[:, :n_off]
        mask = torch.sigmoid(om[:, n_off:])
        return modulated_deform_conv2d(
            input, offset, mask, self.weight, self.bias,
            self.stride, self.padding, self.dilation, self.deformable_groups)
