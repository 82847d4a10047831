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
