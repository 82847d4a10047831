"""Derived error bounds shared by the kernel tests: bf16 and fp16, and fp32
for the DCN backward (where the u terms vanish).

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

dcn_bwd_bounds — the five grads of the deformable conv (input, offset, mask,
weight, bias) against float64 autograd of `_deform_conv2d_torch` on the
operands already rounded to the type under test.  Per element
    a*u*|ref| + b*u*S + 2*n*e*S + 2^-40,     e = 2^-24, u = 0 for fp32
  (a, b): input (2, 2), offset (2, 2), mask (2, 2), weight (2, 4),
  bias (2, 0).  u*|ref| is the one store rounding.  u*S on input, offset and
  mask: the kernels read col_grad, a GEMM output already rounded to the
  16-bit type.  2u*S on weight: the saved im2col columns are rounded to 16
  bits, and bmm(go2d, cols^T) is rounded per sample before .sum(0).  The
  factor 2 on each is slack, as in conv_bound.
  S is the sum of the magnitudes of all terms behind one element.  For
  input, mask, weight and bias it is the same float64 backward run on
  |input|, |weight|, |bias|, |gout| with offsets and mask unchanged (mask and
  bilinear weights are >= 0).  The coordinate derivative is a difference of
  corners, so for the offset grad
      S_off_h = mask * (GM(h -> floor h) + GM(h -> floor h + 1)),
  GM being the abs problem's mask grad re-evaluated with the h offset moved
  to the cell's two integer rows; S_off_w likewise along w.
  n is the longest fp32 summation behind one element: B*Ho*Wo + 8 for
  weight and bias, Cout + 4*cpg + 8 for offset and mask, Cout + 8 + the
  largest number of corner hits on one input element for the input grad.
  Every shape must keep 2*n*e <= 2^-12, so that the fp32 term cannot hide a
  structural error; offsets must be exact in the type, at least one sample
  must sit exactly on -1 and one on H-1 or W-1.

conv_bwd_bound — dx, dW, db of conv + bias + act.  The incoming gradient is
dpre64 = dy * act'(y) in float64 on the kernel's own rounded forward output
y (what act_grad sees); references are float64 conv2d autograd, S the same
backward on absolute values.
    2u*|ref| + c*u*S + 2*n*e*S + 2^-30
  c = 2 when an activation makes dpre a rounded intermediate, 0 for none;
  n = 9*Cout for dx, min(B*Ho*Wo, 2^11) for dW and db.  B*Ho*Wo is the
  number of terms behind a dW or db element, but n*e*S bounds a sum only
  by its longest chain of dependent fp32 additions, and no kernel here adds
  that many one after another: conv2d_wgrad_s1_kernel adds 32-term MFMA
  products, fpb*H of them per block, and the second stage adds one partial
  per block (32 + 12 + 136 = 180 at B33 128->128 6x256); the stride-2
  kernel 32-term products over 4 rows, 4 waves and one atomic per block;
  torch's sum is a tree.  Uncapped, 2*n*e at B32 6x256 is 2^-7.4, wider
  than u, and a dW with a whole frame left out passes.  The cap keeps
  2*n*e <= 2^-12 on every shape, the condition dcn_bwd_bounds asserts.
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


# ------------------------------------------------- backward rules
FP32_EPS = 2.0 ** -24


def unit_roundoff(dtype):
    """u of a 16-bit type; 0 for fp32, whose rounding the n*e terms carry."""
    return 0.0 if dtype == torch.float32 else UNIT_ROUNDOFF[dtype]


def _dcn_oracle():
    from esr_amd.ops.dcn import _deform_conv2d_torch
    return _deform_conv2d_torch


def dcn_bwd_ref64(args, gout, geom, fn=None):
    """float64 autograd of the torch DCN on the CPU.  `args` = (input,
    offset, mask, weight, bias), `geom` = (stride, pad, dilation, dg);
    returns the five grads.  `fn` replaces the oracle (self-tests only)."""
    s, p, d, dg = geom
    leaves = [t.detach().cpu().double().clone().requires_grad_(True)
              for t in args]
    out = (fn or _dcn_oracle())(*leaves, (s, s), (p, p), (d, d), dg)
    out.backward(gout.detach().cpu().double())
    return [t.grad for t in leaves]


def dcn_coords(offset, geom, kh, kw):
    """Sample coordinates (h_im, w_im), each [B, dg, K, Ho, Wo], float64."""
    s, p, d, dg = geom
    B, _, Ho, Wo = offset.shape
    K = kh * kw
    off = offset.detach().cpu().double().view(B, dg, K, 2, Ho, Wo)
    f64 = dict(dtype=torch.float64)
    base_h = (torch.arange(Ho, **f64) * s - p).view(1, 1, 1, Ho, 1)
    base_w = (torch.arange(Wo, **f64) * s - p).view(1, 1, 1, 1, Wo)
    ker_h = (torch.arange(kh, **f64) * d).repeat_interleave(kw) \
        .view(1, 1, K, 1, 1)
    ker_w = (torch.arange(kw, **f64) * d).repeat(kh).view(1, 1, K, 1, 1)
    return base_h + ker_h + off[:, :, :, 0], base_w + ker_w + off[:, :, :, 1]


def dcn_max_corner_hits(h_im, w_im, H, W):
    """Largest number of bilinear corners that land on one input pixel of
    one (sample, deformable group)."""
    B, dg = h_im.shape[:2]
    in_range = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    hits = torch.zeros(B * dg, H * W, dtype=torch.float64)
    rows = torch.arange(B * dg).view(B, dg, 1, 1, 1).expand_as(h_im)
    for dy in (0, 1):
        for dx in (0, 1):
            hc, wc = h_im.floor() + dy, w_im.floor() + dx
            ok = in_range & (hc >= 0) & (hc < H) & (wc >= 0) & (wc < W)
            flat = (rows * (H * W) + hc.clamp(0, H - 1) * W
                    + wc.clamp(0, W - 1)).long()
            hits.view(-1).index_add_(
                0, flat[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    return int(hits.max().item())


def dcn_bwd_bounds(args, gout, geom, ref, dtype):
    """Per-element bounds of the five DCN grads (see the module docstring)
    for kernels that store `dtype`; `ref` = dcn_bwd_ref64(args, gout, geom).
    Asserts the conditions under which the rule holds."""
    inp, off, msk, w, b = [t.detach().cpu().double() for t in args]
    g64 = gout.detach().cpu().double()
    s, p, d, dg = geom
    B, C, H, W = inp.shape
    Cout, _, kh, kw = w.shape
    K, cpg = kh * kw, C // dg
    Ho, Wo = g64.shape[2:]
    assert torch.equal(off.to(dtype).double(), off), \
        f"offsets are not exact in {dtype}"
    assert (msk >= 0).all(), "mask must be >= 0 for the abs problem"
    h_im, w_im = dcn_coords(off, geom, kh, kw)
    # exact in fp32 too, so the kernel floors as the float64 reference does
    assert torch.equal(h_im.float().double(), h_im)
    assert torch.equal(w_im.float().double(), w_im)
    assert ((h_im == -1) | (w_im == -1)).any(), "no sample on -1"
    assert ((h_im == H - 1) | (w_im == W - 1)).any(), "no sample on H-1 or W-1"

    def abs_grads(off_used):
        return dcn_bwd_ref64([inp.abs(), off_used, msk, w.abs(), b.abs()],
                             g64.abs(), geom)

    S_in, _, GM, S_w, S_b = abs_grads(off)
    o6 = off.view(B, dg, K, 2, Ho, Wo)
    m5 = msk.view(B, dg, K, Ho, Wo)
    S_off = torch.empty_like(o6)
    for comp in (0, 1):
        lo = o6.clone()
        lo[:, :, :, comp] = o6[:, :, :, comp].floor()   # base coords integer
        hi = lo.clone()
        hi[:, :, :, comp] += 1
        S_off[:, :, :, comp] = m5 * (
            abs_grads(lo.view_as(off))[2].view_as(m5)
            + abs_grads(hi.view_as(off))[2].view_as(m5))
    S_off = S_off.view_as(off)

    u = unit_roundoff(dtype)
    n_wb = B * Ho * Wo + 8
    n_om = Cout + 4 * cpg + 8
    n_in = Cout + 8 + dcn_max_corner_hits(h_im, w_im, H, W)
    rules = [(S_in, 2, 2, n_in), (S_off, 2, 2, n_om), (GM, 2, 2, n_om),
             (S_w, 2, 4, n_wb), (S_b, 2, 0, n_wb)]
    bounds = []
    for r, (S, a_, b_, n) in zip(ref, rules):
        assert 2 * n * FP32_EPS <= 2.0 ** -12, \
            f"n = {n}: the fp32 term could hide a structural error"
        # S is itself a float64 evaluation: allow its own roundoff
        assert (r.abs() <= S * (1 + 2.0 ** -40) + 2.0 ** -60).all(), \
            "magnitude sum below |ref|"
        bounds.append(a_ * u * r.abs() + b_ * u * S
                      + 2 * n * FP32_EPS * S + 2.0 ** -40)
    return bounds


def act_deriv64(y64, act):
    """act'(pre) written in the activated value y, as act_grad has it."""
    if act == "relu":
        return (y64 > 0).double()
    if act == "sigmoid":
        return y64 * (1 - y64)
    if act == "tanh":
        return 1 - y64 * y64
    assert act in (None, "none"), act
    return torch.ones_like(y64)


def conv_bwd_ref64(x, w, dy, y, stride, act):
    """float64 (dx, dW, db) of a ks//2-padded conv + bias + `act` on the
    16-bit-rounded operands, for the incoming gradient dy * act'(y) taken on
    the kernel's own forward output `y` (the bias acts through `y` alone),
    and the same backward on absolute values: (refs, Ss), three tensors
    each."""
    pad = w.shape[-1] // 2
    x64, w64, dy64, y64 = [t.detach().cpu().double() for t in (x, w, dy, y)]
    dpre = dy64 * act_deriv64(y64, act)

    def bwd(xs, ws, g):
        # conv2d's autograd without its forward pass
        return list(torch.ops.aten.convolution_backward(
            g, xs, ws, [ws.shape[0]], [stride, stride], [pad, pad], [1, 1],
            False, [0, 0], 1, [True, True, True]))

    return bwd(x64, w64, dpre), bwd(x64.abs(), w64.abs(), dpre.abs())


FP32_CHAIN_MAX = 2 ** 11


def conv_bwd_bound(ref64, S64, n, act, dtype):
    """Per-element bound of one conv grad; `n` is the number of fp32 terms
    behind an element, counted up to FP32_CHAIN_MAX (see the module
    docstring), so the fp32 term never exceeds 2^-12 * S."""
    u = unit_roundoff(dtype)
    n = min(n, FP32_CHAIN_MAX)
    c = 0 if act in (None, "none") else 2
    return (2 * u * ref64.abs() + c * u * S64 + 2 * n * FP32_EPS * S64
            + 2.0 ** -30)


def grid_offsets(shape, scale, dtype, generator, lattice=None):
    """DCN offsets that are exact in `dtype` and keep base + offset exact in
    fp32: randn * scale rounded to a binary grid (2^-10 for fp32, 2^-3 with
    |off| < 16 for bf16, 2^-4 for fp16).  `lattice` = "zero" gives all-zero
    offsets and "int" integers in {-2..2}."""
    if lattice == "zero":
        return torch.zeros(shape)
    if lattice == "int":
        return torch.randint(-2, 3, shape, generator=generator).float()
    assert lattice is None, lattice
    step = {torch.float32: 2.0 ** -10, torch.bfloat16: 2.0 ** -3,
            torch.float16: 2.0 ** -4}[dtype]
    off = torch.round(torch.randn(shape, generator=generator) * scale / step) \
        * step
    if dtype == torch.float32:
        # the 16-bit grids put 6-13 % of the coordinates on a pixel by
        # themselves; on the fine fp32 grid one offset in eight is made whole
        whole = torch.rand(shape, generator=generator) < 0.125
        off = torch.where(whole, off.round(), off)
    return off.clamp(-16 + step, 16 - step)


def dcn_torch_variant(input, offset, mask, weight, bias, stride, padding,
                      dilation, deformable_groups, in_range_rule=True,
                      clamp_corner=None):
    """The torch DCN oracle written out again with two switches, for the
    tests of the oracle and of the rules; with both at their defaults it
    is `_deform_conv2d_torch` to the bit.  `in_range_rule=False` is the
    oracle as it was before it took the kernels' boundary rule;
    `clamp_corner=(dy, dx)` drops that corner's `valid`, which clamps to the
    border pixel instead of zero-padding."""
    B, C, H, W = input.shape
    Cout, _, kh, kw = weight.shape
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    dg, K = deformable_groups, kh * kw
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    kwargs = dict(device=input.device, dtype=input.dtype)
    off = offset.view(B, dg, K, 2, Ho, Wo)
    base_h = (torch.arange(Ho, **kwargs) * sh - ph).view(1, 1, 1, Ho, 1)
    base_w = (torch.arange(Wo, **kwargs) * sw - pw).view(1, 1, 1, 1, Wo)
    ker_h = (torch.arange(kh, **kwargs) * dh).repeat_interleave(kw) \
        .view(1, 1, K, 1, 1)
    ker_w = (torch.arange(kw, **kwargs) * dw).repeat(kh).view(1, 1, K, 1, 1)
    h_im = base_h + ker_h + off[:, :, :, 0]
    w_im = base_w + ker_w + off[:, :, :, 1]
    h0, w0 = h_im.floor(), w_im.floor()
    lh, lw = h_im - h0, w_im - w0
    in_range = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    inp = input.view(B, dg, C // dg, H * W)
    cols = torch.zeros(B, dg, C // dg, K, Ho, Wo, **kwargs)
    for dy in (0, 1):
        for dx in (0, 1):
            hc, wc = h0 + dy, w0 + dx
            keep = (hc >= 0) & (hc < H) & (wc >= 0) & (wc < W)
            if clamp_corner == (dy, dx):
                keep = torch.ones_like(keep)
            if in_range_rule:
                keep = keep & in_range
            wgt = ((lh if dy else 1 - lh) * (lw if dx else 1 - lw)) * keep
            idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long()
            idx_f = idx.view(B, dg, 1, K * Ho * Wo).expand(-1, -1, C // dg, -1)
            gathered = torch.gather(inp, 3, idx_f) \
                .view(B, dg, C // dg, K, Ho, Wo)
            cols = cols + gathered * wgt.unsqueeze(2)
    cols = (cols * mask.view(B, dg, K, Ho, Wo).unsqueeze(2)) \
        .reshape(B, C * K, Ho * Wo)
    out = torch.bmm(weight.view(Cout, C * K).unsqueeze(0).expand(B, -1, -1),
                    cols).view(B, Cout, Ho, Wo)
    return out if bias is None else out + bias.view(1, Cout, 1, 1)


def dcn_grid_problem(B, C, H, W, Cout, dg, stride=1, pad=1, dil=1,
                     off_scale=2.0, seed=0, dtype=torch.float32,
                     lattice=None):
    """CPU tensors of a 3x3 DCN backward problem, ((input, offset, mask,
    weight, bias), grad_out), rounded to `dtype` but held in fp32, with
    offsets from grid_offsets."""
    g = torch.Generator().manual_seed(seed)
    Ho = (H + 2 * pad - (dil * 2 + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * 2 + 1)) // stride + 1
    args = [torch.randn(B, C, H, W, generator=g),
            grid_offsets((B, dg * 18, Ho, Wo), off_scale, dtype, g, lattice),
            torch.rand(B, dg * 9, Ho, Wo, generator=g),
            torch.randn(Cout, C, 3, 3, generator=g) * 0.2,
            torch.randn(Cout, generator=g)]
    gout = torch.randn(B, Cout, Ho, Wo, generator=g)
    return [t.to(dtype).float() for t in args], gout.to(dtype).float()
