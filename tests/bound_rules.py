"""Derived error bounds shared by the 16-bit kernel tests (bf16 and fp16).

The yardstick everywhere is a plain torch evaluation in float64 of the same
operation on the same 16-bit-rounded operands.  The kernels compute in fp32
and round once to the 16-bit type on store, so the bounds are built from

    u = unit roundoff of the output type: 2^-8 for bf16 (8 significand
        bits), 2^-11 for fp16 (11 bits);

and the fp32 evaluation error.  Every comparison counts the elements over
the bound as an integer over ALL elements (NaN counts as over); none is
sampled or masked.

once_rounded — one elementwise fp32 expression rounded once:
    |got - ref| <= 2u*|ref| + 2^-16
  u*|ref| is the store rounding, the factor 2 is slack; 2^-16 covers the fp32
  evaluation error of the six-operation gate formulas at |inputs| <= 8 (below
  2^-18, the fast-exp sigmoid included).

conv_bound — conv + bias + activation, fp32 accumulate, rounded once.  With
S = conv2d(|x|, |w|) + |b|:
    none / relu:  2u*|ref| + 2^-12*S + 2^-24
    sigmoid:      2u + 2^-12*S/4       (|sigmoid'| <= 1/4, output <= 1)
    tanh:         2u + 2^-12*S         (|tanh'| <= 1, output <= 1)
  fp32 accumulation over K <= 9*192+1 terms errs by <= K*2^-24*S < 2^-13*S;
  the factor 2 on it covers the MFMA-internal summation order.
"""

import torch
import torch.nn.functional as F

UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def count_over(got, ref64, bound):
    """(number of elements with |got - ref64| > bound or NaN, worst
    diff/bound).  `got` may be any float dtype; compared in float64."""
    assert ref64.dtype == torch.float64, ref64.dtype
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    diff = (got.double() - ref64).abs()
    n_bad = int((~(diff <= bound)).sum().item())   # NaN counts as bad
    worst = (diff / bound).max().item()
    return n_bad, worst


def assert_within(got, ref64, bound, what):
    """Assert zero elements over `bound`; prints and returns worst
    diff/bound."""
    n_bad, worst = count_over(got, ref64, bound)
    print(f"{what}: max diff/bound {worst:.3f}")
    assert n_bad == 0, (f"{what}: {n_bad}/{ref64.numel()} elements over the "
                        f"bound (worst diff/bound {worst:.3f})")
    return worst


def once_rounded_bound(ref64, dtype):
    return 2 * UNIT_ROUNDOFF[dtype] * ref64.abs() + 2.0 ** -16


def once_rounded(got, ref64, dtype, what="once_rounded"):
    """`got` (of `dtype`) is one fp32 expression rounded once; `ref64` is
    the same expression in float64."""
    assert got.dtype == dtype, f"{what}: dtype {got.dtype}, want {dtype}"
    return assert_within(got, ref64, once_rounded_bound(ref64, dtype), what)


def conv_bound(ref64, S64, act, dtype):
    """Per-element bound for conv + bias + `act` (None/"none", "relu",
    "sigmoid", "tanh") stored as `dtype`; `ref64` is the activated float64
    reference, `S64` = conv2d(|x|, |w|) + |b|."""
    u2 = 2 * UNIT_ROUNDOFF[dtype]
    if act == "sigmoid":
        return u2 + 2.0 ** -12 * S64 / 4
    if act == "tanh":
        return u2 + 2.0 ** -12 * S64
    assert act in (None, "none", "relu"), act
    return u2 * ref64.abs() + 2.0 ** -12 * S64 + 2.0 ** -24


def apply_act(pre, act):
    if act == "relu":
        return F.relu(pre)
    if act == "sigmoid":
        return torch.sigmoid(pre)
    if act == "tanh":
        return torch.tanh(pre)
    return pre


def conv_ref64(x, w, b, stride, act):
    """float64 reference and magnitude sum of a ks//2-padded conv on the
    (already 16-bit-rounded) operands, on the CPU: (ref64, S64)."""
    pad = w.shape[-1] // 2
    x64, w64 = x.detach().cpu().double(), w.detach().cpu().double()
    b64 = None if b is None else b.detach().cpu().double()
    pre = F.conv2d(x64, w64, b64, stride=stride, padding=pad)
    S = F.conv2d(x64.abs(), w64.abs(), None if b64 is None else b64.abs(),
                 stride=stride, padding=pad)
    return apply_act(pre, act), S
