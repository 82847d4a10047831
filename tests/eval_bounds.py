"""Derived error bounds for the restoration-metric sums (loss/device_metrics.py,
ops/native/src/eval_metrics.hip), in the manner of tests/bound_rules.py:
constants come from the arithmetic, never from what a kernel gives.

The yardstick is `metric_sums_torch`: the same five columns in float64 torch
ops.  The inputs are fp32, so p*p, t*t and p*t are exact in float64 (24 + 24
significand bits <= 53) and only additions, the scalings and the quotient
round.  u = 2^-53 is the float64 unit roundoff.

sums columns (sum |p-t|, sum (p-t)^2): relative (H*W + 2) * u.
  p - t rounds once, the square once, and a sum of H*W non-negative terms in
  ANY order errs by at most (H*W - 1) * u relative (every partial sum is at
  most the total).

max t, min t: exact.  No arithmetic is involved.

SSIM sum: a running error bound, per window position, then summed.
  Every 7-tap or 49-term float64 sum errs by at most 48 * u * sum|terms|,
  whatever the order (48 additions, each partial sum at most sum|terms|).  So
  the five window sums start as (value, 48 * u * box(|terms|)) with the
  absolute sums taken over the window itself, and the pair is carried through
  the formula of loss/metrics.py::_ssim_single by the textbook rules

      a*b : |a| eb + |b| ea + ea eb,  then + u * (|a*b| + that)
      a+b : ea + eb,                  then + u * (|a+b| + that)
      a/b : (ea + |a/b| eb) / (|b| - eb), then + u * (|a/b| + that)

  i.e. the propagated error plus one rounding of the result.  Constants that
  are not powers of two (1/49, 49/48, C1, C2) carry 4u relative: C = (K*R)^2
  is three roundings away from its decimal value.  The true denominators
  ux^2 + uy^2 + C1 and vx + vy + C2 are at least C1 and C2, so |b| - eb is
  floored there; the quotient rule needs nothing else.  The value is taken
  both as (A1*A2)/(B1*B2), which is what `_ssim_single` and the kernel
  compute, and as (A1/B1)*(A2/B2); the bound is the larger of the two.
  A fused multiply-add rounds once where the rules above count twice, so an
  evaluation that contracts stays inside (the kernel does not contract: it
  has to return exactly 1 per window for equal maps).
  Adding the N = (H-6)(W-6) values in any order costs at most
  N * u * sum|values| more.

The bound is the error of ONE evaluation against the exact value.  Two
float64 evaluations can differ by twice that in theory; the tests hold the
kernel to ONE times the bound against `metric_sums_torch`, which is tighter
than the theory needs and has room because worst-case rounding bounds exceed
what any summation order actually produces.  An fp32 evaluation is orders of
magnitude outside (tests/test_device_eval.py::test_bound_has_teeth).
"""

import torch
import torch.nn.functional as F

U = 2.0 ** -53
WIN = 7
SUM_TERMS = WIN * WIN - 1          # additions behind a 7x7 (or 7+7 tap) sum


def sums_rel_bound(H: int, W: int) -> float:
    return (H * W + 2) * U


# ---- (value, error) pairs ------------------------------------------------
def _rounded(v, e):
    return v, e + U * (v.abs() + e)


def _mul(a, b):
    (av, ae), (bv, be) = a, b
    return _rounded(av * bv, av.abs() * be + bv.abs() * ae + ae * be)


def _add(a, b):
    (av, ae), (bv, be) = a, b
    return _rounded(av + bv, ae + be)


def _sub(a, b):
    return _add(a, (-b[0], b[1]))


def _div(a, b, floor):
    (av, ae), (bv, be) = a, b
    lo = torch.clamp(bv.abs() - be, min=floor * (1 - 8 * U))
    v = av / bv
    return _rounded(v, (ae + v.abs() * be) / lo)


def _const(c: float, like, exact: bool = False):
    v = torch.full_like(like, c)
    return v, torch.zeros_like(like) if exact else 4 * U * v.abs()


def ssim_sum_bound(pred: torch.Tensor, tgt: torch.Tensor,
                   data_range: float = 2.0) -> torch.Tensor:
    """float64 [P]: bound on |computed - exact| of column 4 for fp32
    [P, H, W] maps, for any float64 evaluation of `_ssim_single`'s formula
    with direct window sums."""
    assert pred.dtype == torch.float32 and tgt.dtype == torch.float32, \
        "the products are exact in float64 only for fp32 inputs"
    p, t = pred.double().cpu(), tgt.double().cpu()

    def box(x):                       # window sum, valid border
        return F.avg_pool2d(x[:, None], WIN, stride=1)[:, 0] * (WIN * WIN)

    def wsum(x):
        return box(x), SUM_TERMS * U * box(x.abs())

    one = box(p)
    inv_n = _const(1.0 / (WIN * WIN), one)
    cov = _const((WIN * WIN) / (WIN * WIN - 1.0), one)
    two = _const(2.0, one, exact=True)
    c1v, c2v = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    C1, C2 = _const(c1v, one), _const(c2v, one)

    ux, uy = _mul(wsum(p), inv_n), _mul(wsum(t), inv_n)
    uxx, uyy = _mul(wsum(p * p), inv_n), _mul(wsum(t * t), inv_n)
    uxy = _mul(wsum(p * t), inv_n)
    vx = _mul(cov, _sub(uxx, _mul(ux, ux)))
    vy = _mul(cov, _sub(uyy, _mul(uy, uy)))
    vxy = _mul(cov, _sub(uxy, _mul(ux, uy)))
    A1 = _add(_mul(two, _mul(ux, uy)), C1)
    A2 = _add(_mul(two, vxy), C2)
    B1 = _add(_add(_mul(ux, ux), _mul(uy, uy)), C1)
    B2 = _add(_add(vx, vy), C2)
    s1 = _div(_mul(A1, A2), _mul(B1, B2), c1v * c2v)
    s2 = _mul(_div(A1, B1, c1v), _div(A2, B2, c2v))
    err = torch.maximum(s1[1], s2[1])
    n = err.size(1) * err.size(2)
    per_plane = err.sum((1, 2))
    return per_plane + n * U * (s1[0].abs().sum((1, 2)) + per_plane)


def assert_sums_within(got: torch.Tensor, ref: torch.Tensor,
                       pred: torch.Tensor, tgt: torch.Tensor, what: str,
                       data_range: float = 2.0) -> float:
    """`got` [P, 5] against the float64 oracle `ref` on fp32 maps [P, H, W];
    prints and returns the worst diff / bound over the bounded columns."""
    assert ref.dtype == torch.float64 and got.dtype == torch.float64
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape == (pred.size(0), 5), (got.shape, ref.shape)
    H, W = pred.shape[-2:]
    worst = 0.0
    rel = sums_rel_bound(H, W)
    for c in (0, 1):
        diff = (got[:, c] - ref[:, c]).abs()
        bound = rel * ref[:, c].abs()
        assert bool((diff <= bound).all()), \
            f"{what}: column {c} off by {diff.max().item():.3e}, bound " \
            f"{bound.max().item():.3e}"
        worst = max(worst, (diff / bound.clamp(min=1e-300)).max().item())
    for c in (2, 3):
        assert torch.equal(got[:, c], ref[:, c]), f"{what}: column {c}"
    bound = ssim_sum_bound(pred, tgt, data_range)
    diff = (got[:, 4] - ref[:, 4]).abs()
    assert bool((diff <= bound).all()), \
        f"{what}: SSIM sum off by {diff.max().item():.3e}, bound " \
        f"{bound.max().item():.3e}"
    worst = max(worst, (diff / bound).max().item())
    print(f"{what}: worst diff/bound {worst:.3f}, SSIM bound "
          f"{bound.max().item():.3e}")
    return worst
