"""Grid-stride wrap: every kernel launched through esr_grid's block cap, run
a little past one full grid, so the threads at the front take a SECOND loop
iteration and the per-iteration state (index decode, the accumulator
re-zero of the strip conv, the i / chw batch split of the gates) is
exercised beyond its first pass.

Sizes come from ext.grid_cap() (blocks x threads of one capped grid): the
shapes are written for the cap of 524 288 and one dimension of each scales
with the cap, and every test asserts cap < items < 1.1 * cap, so a changed
cap moves the coverage with it or fails here.

References are float64 torch on the same operands, bounds from
tests/bound_rules.py unless a test says otherwise.
"""

import pytest
import torch

from bound_rules import assert_within, conv_bound, conv_ref64
from test_gpu_bf16_ops import check_act_grad, check_gates
from test_gpu_conv import _backward_vs_oracle
from test_gpu_dcn_bwd import _check_oracle
from test_gpu_kernels import splat_problem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
CAP_WRITTEN_FOR = 524288


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


def _cap():
    return int(_ext().grid_cap())


def _scaled(dim):
    """`dim` at the cap the shapes were written for, in proportion else."""
    return max(1, round(dim * _cap() / CAP_WRITTEN_FOR))


def _assert_wraps(items, what):
    cap = _cap()
    print(f"{what}: {items} items, cap {cap}")
    assert cap < items < 1.1 * cap, f"{what}: {items} items vs cap {cap}"


def _rand_bf16(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(BF16)


def test_conv2d_fwd_valu_wraps():
    """8 -> 2 3x3 relu at W = 302 (W % 8 = 6, the v1 kernel's class)."""
    from esr_amd.ops.conv import ACT_IDS
    x = _rand_bf16(3, 8, _scaled(300), 302, seed=1)
    w = _rand_bf16(2, 8, 3, 3, seed=2, scale=0.3)
    b = _rand_bf16(2, seed=3)
    y = _ext().conv2d_fwd_valu(x, w, b.float(), 1, ACT_IDS["relu"])
    _assert_wraps(y.numel(), "conv2d_fwd_valu outputs")
    ref64, S64 = conv_ref64(x, w, b, 1, "relu")
    assert y.dtype == BF16 and y.shape == ref64.shape
    assert_within(y.cpu(), ref64, conv_bound(ref64, S64, "relu", BF16),
                  "conv2d_fwd_valu past one grid")


def test_conv2d_fwd_valu2_wraps():
    """2 -> 2 3x3: one work item is an 8-wide output strip."""
    from esr_amd.ops.conv import ACT_IDS
    x = _rand_bf16(3, 2, _scaled(704), 2048, seed=4)
    w = _rand_bf16(2, 2, 3, 3, seed=5, scale=0.3)
    b = _rand_bf16(2, seed=6)
    y = _ext().conv2d_fwd_valu2(x, w, b.float(), 1, ACT_IDS[None])
    _assert_wraps(x.shape[0] * x.shape[2] * (x.shape[3] // 8),
                  "conv2d_fwd_valu2 strips")
    ref64, S64 = conv_ref64(x, w, b, 1, None)
    assert y.dtype == BF16 and y.shape == ref64.shape
    assert_within(y.cpu(), ref64, conv_bound(ref64, S64, None, BF16),
                  "conv2d_fwd_valu2 past one grid")


def _gate_shape():
    # chw = 24*105*105 = 264 600 is no multiple of the block size: the batch
    # boundary of the i / chw split falls inside a block
    return (2, _scaled(24), 105, 105)


def test_act_grad_wraps():
    shape = _gate_shape()
    _assert_wraps(shape[0] * shape[1] * shape[2] * shape[3],
                  "act_grad elements")
    check_act_grad("tanh", BF16, shape)


def test_gru_gates_wrap():
    shape = _gate_shape()
    _assert_wraps(shape[0] * shape[1] * shape[2] * shape[3],
                  "gate kernels elements")
    check_gates(BF16, shape)


def test_dcn_split_kernels_wrap():
    """dcn_im2col, the untiled dcn_col2im and dcn_col2im_coord on one fp32
    problem: cpg*H*W*4 = 133 KB is past the fused backward's LDS limit and
    dilation 2 is outside the tiled col2im's shape, so path="auto" runs the
    three capped grid-stride kernels.  Forward atol 1e-4 as TestDeformConv,
    grads by test_gpu_dcn_bwd's rule, both against the float64 oracle."""
    from esr_amd.ops import dcn
    B, C, H, W, Cout, dg, K = 2, 64, _scaled(65), 64, 8, 8, 9
    pad = dil = 2
    Ho, Wo = H, W
    _assert_wraps(B * C * Ho * Wo, "dcn_im2col items")
    assert B * C * K * Ho * Wo > _cap() and B * dg * K * Ho * Wo > _cap()
    print(f"dcn_col2im items {B * C * K * Ho * Wo}, "
          f"dcn_col2im_coord items {B * dg * K * Ho * Wo}")
    assert not dcn.dcn_bwd_fused_applicable(C, dg, H, W)

    g = torch.Generator().manual_seed(17)
    args = [torch.randn(B, C, H, W, generator=g),
            torch.randn(B, dg * 2 * K, Ho, Wo, generator=g) * 2,
            torch.rand(B, dg * K, Ho, Wo, generator=g),
            torch.randn(Cout, C, 3, 3, generator=g) * 0.2,
            torch.randn(Cout, generator=g)]
    gout = torch.randn(B, Cout, Ho, Wo, generator=g)
    # Offsets on a 2^-16 grid: base + tap + offset then needs < 24 bits, so
    # the kernels' fp32 sample coordinates are exact and equal the float64
    # oracle's.  The offset grad is the one-sided derivative right of
    # floor(coordinate): with free fp32 offsets one of these 1.2 M
    # coordinates rounds onto an integer in fp32 and not in float64, the two
    # floors differ, and that element shows the kink (0.06 of max|grad|,
    # equally between the fp32 and the float64 run of the oracle itself).
    args[1] = (args[1] * 2.0 ** 16).round() / 2.0 ** 16
    # exactly on -1, H or W the kernels define the derivative as 0 and the
    # oracle as the inner one-sided slope: keep the data clear of it
    off = args[1].view(B, dg, 3, 3, 2, Ho, Wo).double()
    tap = torch.arange(3.0, dtype=torch.float64) * dil - pad
    h_im = off[:, :, :, :, 0] + tap.view(3, 1, 1, 1) \
        + torch.arange(Ho, dtype=torch.float64).view(Ho, 1)
    w_im = off[:, :, :, :, 1] + tap.view(1, 3, 1, 1) \
        + torch.arange(Wo, dtype=torch.float64)
    assert not bool(((h_im == -1) | (h_im == H) | (w_im == -1)
                     | (w_im == W)).any())

    ref_leaves = [t.double().requires_grad_(True) for t in args]
    ref_out = dcn._deform_conv2d_torch(*ref_leaves, (1, 1), (pad, pad),
                                       (dil, dil), dg)
    ref_out.backward(gout.double())

    leaves = [t.to(DEV).requires_grad_(True) for t in args]
    before = dict(dcn.stats)
    out = dcn.modulated_deform_conv2d(*leaves, stride=1, padding=pad,
                                      dilation=dil, deformable_groups=dg)
    out.backward(gout.to(DEV))
    assert dcn.stats["bwd_split"] == before["bwd_split"] + 1
    assert dcn.stats["bwd_fused"] == before["bwd_fused"]

    ref64 = ref_out.detach()
    diff = (out.detach().cpu().double() - ref64).abs()
    n_bad = int((~(diff <= 1e-4 + 1e-5 * ref64.abs())).sum().item())
    print(f"dcn forward past one grid: max abs diff {diff.max().item():.3g}")
    assert n_bad == 0, f"forward: {n_bad}/{diff.numel()} off by > 1e-4"
    _check_oracle([t.grad for t in leaves], [t.grad for t in ref_leaves])


def test_conv2d_dgrad_s2_wraps(monkeypatch):
    """32 -> 64 3x3 stride 2 through the all-native backward; dx, dW and db
    within conv_bwd_bound of tests/bound_rules.py (test_gpu_conv's rule)."""
    h = _scaled(74)
    _assert_wraps(3 * 32 * h * 74, "conv2d_dgrad_s2 items")
    monkeypatch.setenv("ESR_CONV_BWD", "native")
    _backward_vs_oracle(3, 32, 64, h, 74, 3, 2, "relu")


def test_splat_kernels_wrap():
    """Integer counts: exact."""
    ext = _ext()
    B, N, TB, H, W = 2, _scaled(270000), 4, 64, 64
    _assert_wraps(B * N, "splat events")
    ev, cnt, stack = splat_problem(B, N, TB, H, W, seed=23)
    ev = ev.to(DEV)
    out_c = ext.splat_count(ev, H, W).cpu()
    assert torch.equal(out_c, cnt.float()), \
        f"splat_count: {int((out_c != cnt.float()).sum())} cells differ"
    out_s = ext.splat_stack(ev, TB, H, W, 0.0, 1.0).cpu()
    assert torch.equal(out_s, stack.float()), \
        f"splat_stack: {int((out_s != stack.float()).sum())} cells differ"


def test_redistribute_wraps():
    """529 000 cells of 0 / 1 / 2 events, explicit capacity, against the CPU
    oracle as test_redistribute_gpu_matches_cpu_oracle compares."""
    from esr_amd.ops.events import redistribute_stack
    Y, X = _scaled(230), 230
    g = torch.Generator().manual_seed(29)
    stack = torch.randint(0, 3, (5, 2, 1, Y, X), generator=g).float()
    _assert_wraps(stack.numel(), "redistribute cells")
    cap = int(stack.sum(dim=(1, 2, 3, 4)).max().item())
    cpu = redistribute_stack(stack, mode="linear", capacity=cap)
    gpu = redistribute_stack(stack.to(DEV), mode="linear", capacity=cap).cpu()
    assert gpu.shape == cpu.shape == (5, cap, 4)
    n_bad = int((~((gpu[..., 2] - cpu[..., 2]).abs() <= 1e-5)).sum().item())
    assert n_bad == 0, f"{n_bad} timestamps differ"
    assert torch.equal(gpu[..., 3], cpu[..., 3]), "polarities differ"
    for b in range(stack.size(0)):
        hists = []
        for ev in (cpu[b], gpu[b]):
            live = ev[ev[:, 3] != 0]
            h = torch.zeros(Y, X, dtype=torch.int64)
            h.index_put_((live[:, 1].long(), live[:, 0].long()),
                         torch.ones(live.size(0), dtype=torch.int64),
                         accumulate=True)
            hists.append(h)
        assert torch.equal(hists[0], hists[1]), f"item {b}: histograms differ"
        assert torch.equal(hists[0], stack[b].sum(dim=(0, 1)).long())
