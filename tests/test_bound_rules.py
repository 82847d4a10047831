"""CPU checks of tests/bound_rules.py: the rules pass torch's own fp32
evaluation rounded once (with room to spare) and fail small, realistic
kernel mistakes.  No GPU and no native extension involved."""

import pytest
import torch
import torch.nn.functional as F

import bound_rules as R

BF16, H16 = torch.bfloat16, torch.float16
# the clean fp32 evaluation must sit well inside a rule: store rounding is
# u*|ref| of a 2u*|ref| term, so ~0.5 is expected
CLEAN_MAX = 0.6


def _rand(*shape, seed, scale=1.0, dtype=BF16):
    """fp32 tensor holding `dtype`-rounded values."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).float()


@pytest.fixture(scope="module")
def conv216():
    """The flagship offset/mask conv 64 -> 216 3x3 on bf16-rounded operands:
    (x, w, b, ref64, S64).  Shared; not to be modified."""
    x = _rand(2, 64, 32, 32, seed=1)
    w = _rand(216, 64, 3, 3, seed=2, scale=0.3)
    b = _rand(216, seed=3)
    ref64, S64 = R.conv_ref64(x, w, b, 1, None)
    return x, w, b, ref64, S64


def _fp32_conv_rounded(x, w, b, stride, act, dtype):
    pre = F.conv2d(x, w, b, stride=stride, padding=w.shape[-1] // 2)
    return R.apply_act(pre, act).to(dtype)


@pytest.mark.parametrize("dtype", [BF16, H16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", [None, "relu", "sigmoid", "tanh"])
def test_conv_bound_passes_fp32_rounded_once(act, dtype):
    x = _rand(2, 192, 16, 16, seed=4, dtype=dtype)
    w = _rand(24, 192, 3, 3, seed=5, scale=0.3, dtype=dtype)
    b = _rand(24, seed=6, dtype=dtype)
    ref64, S64 = R.conv_ref64(x, w, b, 1, act)
    got = _fp32_conv_rounded(x, w, b, 1, act, dtype)
    worst = R.assert_within(got, ref64, R.conv_bound(ref64, S64, act, dtype),
                            f"clean conv {act} {dtype}")
    assert worst <= CLEAN_MAX, worst


def test_conv_bound_passes_clean_216(conv216):
    x, w, b, ref64, S64 = conv216
    got = _fp32_conv_rounded(x, w, b, 1, None, BF16)
    worst = R.assert_within(got, ref64, R.conv_bound(ref64, S64, None, BF16),
                            "clean conv 64->216")
    assert worst <= CLEAN_MAX, worst


def _mut_centre_tap(w):
    w[:, 5, 1, 1] *= 1.25          # one input channel's centre tap


def _mut_row_zeroed(w):
    w[100, :, 0, 2] = 0            # one (cout, tap) packed weight row


def _mut_group_zeroed(w):
    w[:, 8:16, 2, 1] = 0           # one 8-channel fragment group of one tap


@pytest.mark.parametrize("mutate", [_mut_centre_tap, _mut_row_zeroed,
                                    _mut_group_zeroed])
def test_conv_bound_fails_mutants(conv216, mutate):
    x, w, b, ref64, S64 = conv216
    wm = w.clone()
    mutate(wm)
    got = _fp32_conv_rounded(x, wm, b, 1, None, BF16)
    n_bad, worst = R.count_over(got, ref64,
                                R.conv_bound(ref64, S64, None, BF16))
    print(f"{mutate.__name__}: {n_bad}/{ref64.numel()} over the bound, "
          f"worst diff/bound {worst:.1f}")
    assert n_bad > 1000, n_bad


def _gate_inputs(dtype):
    return [_rand(2, 16, 24, 24, seed=s, dtype=dtype) for s in range(10, 17)]


def _gate_formulas(ur_u, ur_r, h, o, g1, g2, g3, saved):
    """Every expression the four gate kernels store, from fp32 or fp64
    inputs; `saved` are the 16-bit-rounded u, r, tanh the backward kernels
    (and the second forward) read back."""
    u, r, t = torch.sigmoid(ur_u), torch.sigmoid(ur_r), torch.tanh(o)
    us, rs, ts = [s.to(h.dtype) for s in saved]
    return {
        "u": u, "r": r, "hr": h * r, "tanh": t,
        "h_new": h * (1 - us) + t * us,
        "d_u_pre": g1 * us * (1 - us),
        "d_r_pre": (g2 + g3 * h) * rs * (1 - rs),
        "dh1": g3 * rs,
        "d_o_pre": g1 * us * (1 - ts * ts),
        "du": g1 * (ts - h),
        "dh2": g1 * (1 - us),
    }


@pytest.mark.parametrize("dtype", [BF16, H16], ids=["bf16", "fp16"])
def test_once_rounded_passes_fp32_gate_formulas(dtype):
    ins = _gate_inputs(dtype)
    saved = [torch.sigmoid(ins[0]).to(dtype), torch.sigmoid(ins[1]).to(dtype),
             torch.tanh(ins[3]).to(dtype)]
    got = _gate_formulas(*ins, saved=saved)
    ref = _gate_formulas(*[t.double() for t in ins], saved=saved)
    for name in got:
        worst = R.once_rounded(got[name].to(dtype), ref[name], dtype,
                               f"clean {name} {dtype}")
        assert worst <= CLEAN_MAX, (name, worst)


def test_once_rounded_fails_swapped_gate():
    """h*(1-u) + t*u written as h*u + t*u."""
    ur_u, _, h, o = _gate_inputs(BF16)[:4]
    u, t = torch.sigmoid(ur_u), torch.tanh(o)
    ref = h.double() * (1 - u.double()) + t.double() * u.double()
    wrong = (h * u + t * u).to(BF16)
    with pytest.raises(AssertionError, match="over the bound"):
        R.once_rounded(wrong, ref, BF16, "swapped gate")
    n_bad, _ = R.count_over(wrong, ref, R.once_rounded_bound(ref, BF16))
    assert n_bad > 1000, n_bad


def test_nan_counts_as_over_the_bound():
    ref = torch.ones(8, dtype=torch.float64)
    got = torch.ones(8).to(BF16)
    got[3] = float("nan")
    n_bad, _ = R.count_over(got, ref, R.once_rounded_bound(ref, BF16))
    assert n_bad == 1
    with pytest.raises(AssertionError):
        R.once_rounded(got, ref, BF16)
    with pytest.raises(AssertionError, match="dtype"):
        R.once_rounded(got.float(), ref, BF16)


# ------------------------------------------------------------ DCN backward
F32 = torch.float32
DCN_GEOM = (1, 1, 1, 4)                    # stride, pad, dilation, dg
DCN_NAMES = ["input", "offset", "mask", "weight", "bias"]


@pytest.fixture(scope="module", params=[
    (F32, 2.0), (BF16, 2.0), (BF16, 8.0), (H16, 2.0), (H16, 8.0)],
    ids=["fp32-s2", "bf16-s2", "bf16-s8", "fp16-s2", "fp16-s8"])
def dcn_case(request):
    """B2 C16 14x18 Cout12 dg4 on grid offsets: (dtype, args, gout, ref64,
    bounds).  Shared; not to be modified."""
    dtype, scale = request.param
    args, gout = R.dcn_grid_problem(2, 16, 14, 18, 12, 4, off_scale=scale,
                                    seed=3, dtype=dtype)
    ref = R.dcn_bwd_ref64(args, gout, DCN_GEOM)
    return dtype, args, gout, ref, R.dcn_bwd_bounds(args, gout, DCN_GEOM,
                                                    ref, dtype)


def _emulated_dcn_backward(args, gout, geom, dtype):
    """The five grads in float64, rounded to `dtype` exactly where the
    kernels round: col_grad, the im2col columns, the per-sample weight-grad
    products, and each output once.  col_grad is injected through the
    oracle itself: an identity weight of C*K outputs makes its output the
    columns and its incoming gradient col_grad."""
    from esr_amd.ops.dcn import _deform_conv2d_torch

    def rd(t):
        return t.to(dtype).double()

    inp, off, msk, w, _ = [t.double() for t in args]
    g64 = gout.double()
    s, p, d, dg = geom
    B, C = inp.shape[:2]
    Cout, CK = w.shape[0], C * 9
    go2d = g64.view(B, Cout, -1)
    col_grad = rd(torch.matmul(w.view(Cout, CK).t(), go2d))
    leaves = [t.clone().requires_grad_(True) for t in (inp, off, msk)]
    cols = _deform_conv2d_torch(*leaves, torch.eye(CK, dtype=torch.float64)
                                .view(CK, C, 3, 3), None,
                                (s, s), (p, p), (d, d), dg)
    cols.backward(col_grad.view_as(cols))
    cols_r = rd(cols.detach()).view(B, CK, -1)
    gw = rd(rd(torch.bmm(go2d, cols_r.transpose(1, 2))).sum(0)).view_as(w)
    return [rd(t.grad) for t in leaves] + [gw, rd(g64.sum((0, 2, 3)))]


def test_dcn_bwd_bounds_pass_emulated_kernel(dcn_case):
    dtype, args, gout, ref, bounds = dcn_case
    got = _emulated_dcn_backward(args, gout, DCN_GEOM, dtype)
    for n, g, r, bd in zip(DCN_NAMES, got, ref, bounds):
        R.assert_within(g, r, bd, f"emulated DCN grad_{n} {dtype}")


def test_dcn_bwd_bounds_pass_fp32_oracle():
    """torch's own fp32 evaluation of the oracle is inside the fp32 rule."""
    from esr_amd.ops.dcn import _deform_conv2d_torch
    args, gout = R.dcn_grid_problem(2, 16, 14, 18, 12, 4, off_scale=2.0,
                                    seed=3, dtype=F32)
    ref = R.dcn_bwd_ref64(args, gout, DCN_GEOM)
    bounds = R.dcn_bwd_bounds(args, gout, DCN_GEOM, ref, F32)
    leaves = [t.clone().requires_grad_(True) for t in args]
    _deform_conv2d_torch(*leaves, (1, 1), (1, 1), (1, 1), 4).backward(gout)
    for n, t, r, bd in zip(DCN_NAMES, leaves, ref, bounds):
        worst = R.assert_within(t.grad, r, bd, f"fp32 oracle grad_{n}")
        assert worst <= CLEAN_MAX, (n, worst)


def _mutant_old_oracle(args, gout):
    return R.dcn_bwd_ref64(args, gout, DCN_GEOM, fn=lambda *a: (
        R.dcn_torch_variant(*a, in_range_rule=False)))


def _mutant_clamped_corner(args, gout):
    return R.dcn_bwd_ref64(args, gout, DCN_GEOM, fn=lambda *a: (
        R.dcn_torch_variant(*a, clamp_corner=(0, 0))))


def _mutant_offsets_swapped(args, gout):
    def swap(t):
        B, _, Ho, Wo = t.shape
        return t.reshape(B, -1, 2, Ho, Wo).flip(2).reshape(t.shape)
    grads = R.dcn_bwd_ref64([args[0], swap(args[1])] + args[2:], gout,
                            DCN_GEOM)
    grads[1] = swap(grads[1])
    return grads


def _mutant_cpg_tail(args, gout):
    """Offset and mask grads reduced over all but the last channel of each
    group; the other grads untouched."""
    grads = R.dcn_bwd_ref64(args, gout, DCN_GEOM)
    inp = args[0].clone()
    cpg = inp.shape[1] // DCN_GEOM[3]
    inp[:, cpg - 1::cpg] = 0
    short = R.dcn_bwd_ref64([inp] + args[1:], gout, DCN_GEOM)
    grads[1], grads[2] = short[1], short[2]
    return grads


@pytest.mark.parametrize("mutant,hit", [
    (_mutant_old_oracle, ["offset"]),
    (_mutant_clamped_corner, ["input", "offset", "mask", "weight"]),
    (_mutant_offsets_swapped, ["input", "offset", "mask", "weight"]),
    (_mutant_cpg_tail, ["offset", "mask"])])
def test_dcn_bwd_bounds_fail_mutants(dcn_case, mutant, hit):
    """Exact float64 grads of a slightly wrong DCN are over the bound, in
    every grad the mistake reaches, even at bf16 width."""
    dtype, args, gout, ref, bounds = dcn_case
    got = mutant(args, gout)
    over = {}
    for n, g, r, bd in zip(DCN_NAMES, got, ref, bounds):
        over[n], worst = R.count_over(g, r, bd)
        print(f"{mutant.__name__} {dtype} grad_{n}: {over[n]}/{r.numel()} "
              f"over, worst diff/bound {worst:.1f}")
    for n in hit:
        assert over[n] >= 1, (n, over)
    assert all(over[n] == 0 for n in DCN_NAMES if n not in hit), over


def test_dcn_bwd_bounds_refuse_bad_problems():
    args, gout = R.dcn_grid_problem(1, 4, 6, 7, 3, 2, seed=1, dtype=BF16)
    ref = R.dcn_bwd_ref64(args, gout, (1, 1, 1, 2))
    bad = [args[0], args[1] + 2.0 ** -12] + args[2:]
    with pytest.raises(AssertionError, match="not exact"):
        R.dcn_bwd_bounds(bad, gout, (1, 1, 1, 2), ref, BF16)
    # B*Ho*Wo + 8 > 2^11: the fp32 term would be wider than 2^-12 * S
    args, gout = R.dcn_grid_problem(2, 2, 32, 32, 2, 1, seed=1, dtype=BF16)
    ref = R.dcn_bwd_ref64(args, gout, (1, 1, 1, 1))
    with pytest.raises(AssertionError, match="structural"):
        R.dcn_bwd_bounds(args, gout, (1, 1, 1, 1), ref, BF16)


# ----------------------------------------------------------- conv backward
def _conv_bwd_case(act, dtype=BF16):
    x = _rand(3, 40, 9, 13, seed=21, dtype=dtype)
    w = _rand(24, 40, 3, 3, seed=22, scale=0.3, dtype=dtype)
    b = _rand(24, seed=23, dtype=dtype)
    dy = _rand(3, 24, 9, 13, seed=24, dtype=dtype)
    y = _fp32_conv_rounded(x, w, b, 1, act, dtype).float()
    return x, w, b, dy, y


def _conv_bwd_bounds(refs, Ss, x, w, dy, act, dtype):
    n_dx, n_w = 9 * w.shape[0], dy.shape[0] * dy.shape[2] * dy.shape[3]
    return [R.conv_bwd_bound(r, S, n, act, dtype)
            for r, S, n in zip(refs, Ss, (n_dx, n_w, n_w))]


@pytest.mark.parametrize("act", [None, "relu", "sigmoid", "tanh"])
def test_conv_bwd_bound_passes_fp32_rounded(act):
    """fp32 act_grad rounded to bf16, then fp32 conv backward rounded once."""
    x, w, b, dy, y = _conv_bwd_case(act)
    refs, Ss = R.conv_bwd_ref64(x, w, dy, y, 1, act)
    dpre = dy * R.act_deriv64(y.double(), act).float()
    if act is not None:
        dpre = dpre.to(BF16).float()
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    F.conv2d(*leaves, padding=1).backward(dpre)
    for n, t, r, bd in zip(("dx", "dW", "db"), leaves, refs,
                           _conv_bwd_bounds(refs, Ss, x, w, dy, act, BF16)):
        worst = R.assert_within(t.grad.to(BF16), r, bd,
                                f"clean conv {n} {act}")
        assert worst <= CLEAN_MAX, (n, worst)


def test_conv_bwd_bound_fails_mutants():
    """Unflipped dgrad weights, one batch frame left out of dW and db."""
    x, w, b, dy, y = _conv_bwd_case(None)
    refs, Ss = R.conv_bwd_ref64(x, w, dy, y, 1, None)
    bounds = _conv_bwd_bounds(refs, Ss, x, w, dy, None, BF16)
    dx_wrong = F.conv2d(dy, w.transpose(0, 1), padding=1).to(BF16)
    short, _ = R.conv_bwd_ref64(x[:2], w, dy[:2], y[:2], 1, None)
    for got, r, bd in ((dx_wrong, refs[0], bounds[0]),
                       (short[1], refs[1], bounds[1]),
                       (short[2], refs[2], bounds[2])):
        n_bad, _ = R.count_over(got, r, bd)
        assert n_bad > r.numel() // 2, n_bad


@pytest.fixture(scope="module")
def conv_bwd_many_frames():
    """B33 16->16 6x256, act None: B*Ho*Wo = 50688 terms behind each dW and
    db element, the count of test_gpu_conv's fpb = 2 cases.  (x, w, dy,
    refs, bounds); shared, not to be modified."""
    x = _rand(33, 16, 6, 256, seed=31)
    w = _rand(16, 16, 3, 3, seed=32, scale=0.3)
    b = _rand(16, seed=33)
    dy = _rand(33, 16, 6, 256, seed=34)
    y = _fp32_conv_rounded(x, w, b, 1, None, BF16).float()
    refs, Ss = R.conv_bwd_ref64(x, w, dy, y, 1, None)
    return x, w, dy, refs, _conv_bwd_bounds(refs, Ss, x, w, dy, None, BF16)


def test_conv_bwd_bound_many_frames_passes_fp32(conv_bwd_many_frames):
    x, w, dy, refs, bounds = conv_bwd_many_frames
    leaves = [t.clone().requires_grad_(True)
              for t in (x, w, torch.zeros(16))]
    F.conv2d(*leaves, padding=1).backward(dy)
    for n, t, r, bd in zip(("dx", "dW", "db"), leaves, refs, bounds):
        worst = R.assert_within(t.grad.to(BF16), r, bd, f"B33 clean {n}")
        assert worst <= CLEAN_MAX, (n, worst)


@pytest.mark.parametrize("frames", [list(range(32)),
                                    list(range(33)) + [1]],
                         ids=["last-frame-lost", "frame-1-twice"])
def test_conv_bwd_bound_many_frames_fails_lost_frame(conv_bwd_many_frames,
                                                     frames):
    """What an fpb = 2 block of the wgrad kernel could get wrong: the odd
    batch's last frame left out, or a block's second frame summed twice.
    One frame in 33 must put most dW and db elements over."""
    x, w, dy, refs, bounds = conv_bwd_many_frames
    got, _ = R.conv_bwd_ref64(x[frames], w, dy[frames], dy[frames], 1, None)
    for n, g, r, bd in zip(("dW", "db"), got[1:], refs[1:], bounds[1:]):
        n_bad, worst = R.count_over(g.to(BF16), r, bd)
        print(f"{n}: {n_bad}/{r.numel()} over, worst diff/bound {worst:.1f}")
        assert n_bad > r.numel() // 2, (n, n_bad)
