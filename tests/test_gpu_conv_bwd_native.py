"""GPU tests of the stride-1 deep-class conv kernels: the 8x32-tile MFMA core
(conv2d_s1: forward and input grad) and the weight grad that writes dW in the
weight's layout (conv2d_wgrad_s1), under the default routing and under
ESR_CONV_BWD=native.

Every element of the forward is held to conv_bound and of dx, dW and db to
conv_bwd_bound (tests/bound_rules.py), against float64 references on the
same bf16 operands.  Shapes are the smallest that reach the kernels' edges;
what each one reaches is written beside it.
"""

import pytest
import torch

from bound_rules import (assert_within, conv_bound, conv_bwd_bound,
                         conv_bwd_ref64, conv_ref64, count_over)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rand_bf16(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale) \
        .to(torch.bfloat16)


# (B, Cin, Cout, H, W, ks, act)
CASES = [
    # the plain deep conv: four row tiles, one K chunk pair, MC 4 both ways
    (3, 64, 64, 32, 32, 3, "relu"),
    # W 33: rows not 16-byte aligned (element loads and stores), a second
    # x tile one pixel wide whose left halo is real; H 11 = 8 + 3 rows;
    # Cin 40 (K chunk 2 holds 8 channels; dgrad M 40 -> 3 fragments in MC 4);
    # Cout 72 (forward MC 6 with 24 padded rows; dgrad K 72 -> 96)
    (3, 40, 72, 11, 33, 3, "relu"),
    # W 8: narrower than a tile, aligned; H 5: one partial row tile;
    # Cout 216: forward split in two blocks of MC 8 (256 padded rows),
    # dgrad K 216 -> 7 chunks
    (3, 64, 216, 5, 8, 3, None),
    # 1x1; dgrad M 216 split over two blocks; W 40: a second x tile 8 wide
    (5, 216, 64, 12, 40, 1, "tanh"),
    # 1x1 on unaligned rows, with and without activation (act 0: dpre is
    # dy itself and db comes from bias_grad)
    (3, 40, 72, 5, 33, 1, "relu"),
    (3, 40, 72, 5, 33, 1, None),
    # MC 2 both ways; W 72: three x tiles, real halo columns on both sides,
    # the last tile 8 wide; H 9 = 8 + 1
    (3, 32, 32, 9, 72, 3, "sigmoid"),
    # wgrad with two frames per block and an odd batch (17*8*4*4 = 2176
    # blocks -> fpb 2, the last block holds one frame); Cout 256: forward
    # split MC 8 x 2, dgrad K 256; W 256: eight x tiles
    (17, 128, 256, 2, 256, 3, None),
    # Cout 192 / Cin 160: both directions split into two blocks of MC 6
    (3, 160, 192, 8, 16, 3, None),
]


def _run(batch, cin, cout, h, w, ks, act):
    """Forward and backward of _NativeConv2dFn as the environment routes
    them: (x, wt, b, gy, y, dx, dW, db)."""
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    x = _rand_bf16(batch, cin, h, w, seed=cin * 3 + cout)
    wt = _rand_bf16(cout, cin, ks, ks, seed=cin + 2 * cout, scale=0.3)
    b = _rand_bf16(cout, seed=9)
    xg = x.clone().requires_grad_(True)
    wg = wt.clone().requires_grad_(True)
    bg = b.clone().requires_grad_(True)
    y = _NativeConv2dFn.apply(xg, wg, bg, 1, ACT_IDS[act])
    gy = _rand_bf16(*y.shape, seed=31)
    y.backward(gy)
    return x, wt, b, gy, y.detach(), xg.grad, wg.grad, bg.grad


def _set_mode(monkeypatch, mode):
    if mode == "native":
        monkeypatch.setenv("ESR_CONV_BWD", "native")
        monkeypatch.setenv("ESR_CONV_FWD", "core")
    else:
        monkeypatch.delenv("ESR_CONV_BWD", raising=False)
        monkeypatch.delenv("ESR_CONV_FWD", raising=False)


@pytest.mark.parametrize("mode", ["default", "native"])
@pytest.mark.parametrize("batch,cin,cout,h,w,ks,act", CASES)
def test_deep_s1_forward_backward_within_bounds(batch, cin, cout, h, w, ks,
                                                act, mode, monkeypatch):
    _set_mode(monkeypatch, mode)
    x, wt, b, gy, y, dx, dw, db = _run(batch, cin, cout, h, w, ks, act)
    tag = f"{mode} B{batch} {cin}->{cout} {h}x{w} k{ks} {act}"

    ref64, S64 = conv_ref64(x, wt, b, 1, act)
    assert y.dtype == torch.bfloat16 and y.shape == ref64.shape
    assert_within(y.cpu(), ref64, conv_bound(ref64, S64, act, torch.bfloat16),
                  f"{tag} fwd")

    refs, Ss = conv_bwd_ref64(x, wt, gy, y, 1, act)
    n_w = batch * h * w
    over = {}
    for name, got, r, S, n in zip(("dx", "dW", "db"), (dx, dw, db), refs, Ss,
                                  (9 * cout, n_w, n_w)):
        assert got.dtype == torch.bfloat16, (name, got.dtype)
        assert got.shape == r.shape, (name, got.shape, r.shape)
        over[name], worst = count_over(
            got.cpu(), r, conv_bwd_bound(r, S, n, act, torch.bfloat16))
        print(f"{tag} {name}: {over[name]}/{r.numel()} over, "
              f"max diff/bound {worst:.3f}")
    assert not any(over.values()), f"elements over the bound: {over}"


@pytest.mark.parametrize("ks,h", [(3, 11), (1, 5)])
def test_core_kernels_called_directly(ks, h):
    """conv2d_s1 and conv2d_wgrad_s1 themselves (whatever the routing sends
    to them), on unaligned rows, 3x3 and 1x1: forward with bias and relu,
    then the input grad and the weight grad of a conv without activation."""
    from esr_amd.ops.native import require_ext
    ext = require_ext()
    batch, cin, cout, w, act = 3, 40, 72, 33, "relu"
    x = _rand_bf16(batch, cin, h, w, seed=1)
    wt = _rand_bf16(cout, cin, ks, ks, seed=2, scale=0.3)
    b = _rand_bf16(cout, seed=3)
    y = ext.conv2d_s1(x, wt, b.float(), 1, False)
    ref64, S64 = conv_ref64(x, wt, b, 1, act)
    assert_within(y.cpu(), ref64, conv_bound(ref64, S64, act, torch.bfloat16),
                  f"conv2d_s1 k{ks} fwd")
    gy = _rand_bf16(*y.shape, seed=4)
    dx = ext.conv2d_s1(gy, wt, None, 0, True)
    dw = ext.conv2d_wgrad_s1(x, gy, ks)
    # act None: gy is the pre-activation gradient itself
    refs, Ss = conv_bwd_ref64(x, wt, gy, y, 1, None)
    for name, got, r, S, n in (("dx", dx, refs[0], Ss[0], 9 * cout),
                               ("dW", dw, refs[1], Ss[1], batch * h * w)):
        assert got.dtype == torch.bfloat16 and got.shape == r.shape
        assert_within(got.cpu(), r,
                      conv_bwd_bound(r, S, n, None, torch.bfloat16),
                      f"direct k{ks} {name}")


def test_whole_backward_bit_equal_across_runs(monkeypatch):
    """No atomics anywhere in the native deep-class backward: two runs of the
    whole backward give the same bits.  (Under the default routing whatever
    stays on aten is MIOpen's, whose split-K weight grad adds with atomics.)"""
    _set_mode(monkeypatch, "native")
    first = _run(6, 64, 128, 16, 32, 3, "relu")
    again = _run(6, 64, 128, 16, 32, 3, "relu")
    for name, a, c in zip(("y", "dx", "dW", "db"), first[4:], again[4:]):
        assert torch.equal(a, c), f"{name} differs between two runs"
