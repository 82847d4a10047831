"""DCN backward on the GPU: the fused kernel (input-grad planes summed in
LDS, offset / mask grads in the same pass), the saved im2col columns and
the path choice, against the CPU fp32 autograd oracle
(`_deform_conv2d_torch`).  Inputs as tests/test_gpu_kernels.py::_dcn_problem:
offsets randn * scale, mask rand.

The `*_within_bounds` tests hold all five grads, on both paths and in all
three types, to the per-element float64 bounds of tests/bound_rules.py
(dcn_bwd_bounds), on offsets drawn from a binary grid so that samples land
exactly on pixels, on -1 and on H-1 / W-1."""

import functools

import pytest
import torch

from bound_rules import (count_over, dcn_bwd_bounds, dcn_bwd_ref64,
                         dcn_grid_problem)

pytestmark = pytest.mark.gpu

NAMES = ["input", "offset", "mask", "weight", "bias"]
# run-to-run bound of test_dcn_backward_replay_determinism
RTOL = ATOL = 1e-5


@functools.lru_cache(maxsize=None)
def _problem(B, C, H, W, Cout, dg, stride=1, pad=1, dil=1, off_scale=2.0,
             seed=0, dtype=torch.float32):
    """CPU tensors (input, offset, mask, weight, bias, grad_out), already
    rounded to `dtype` but held in fp32, and the oracle's five grads.
    Cached: callers must not modify what they get."""
    from esr_amd.ops.dcn import _deform_conv2d_torch
    g = torch.Generator().manual_seed(seed)
    Ho = (H + 2 * pad - (dil * 2 + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * 2 + 1)) // stride + 1
    args = [torch.randn(B, C, H, W, generator=g),
            torch.randn(B, dg * 18, Ho, Wo, generator=g) * off_scale,
            torch.rand(B, dg * 9, Ho, Wo, generator=g),
            torch.randn(Cout, C, 3, 3, generator=g) * 0.2,
            torch.randn(Cout, generator=g)]
    gout = torch.randn(B, Cout, Ho, Wo, generator=g)
    args = [t.to(dtype).float() for t in args]
    gout = gout.to(dtype).float()
    leaves = [t.clone().requires_grad_(True) for t in args]
    out = _deform_conv2d_torch(*leaves, (stride, stride), (pad, pad),
                               (dil, dil), dg)
    out.backward(gout)
    return args + [gout], [t.grad for t in leaves]


def _run(tensors, dg, path, stride=1, pad=1, dil=1, dtype=torch.float32,
         cols=None):
    from esr_amd.ops.dcn import deform_conv2d_backward
    inp, off, msk, w, _, gout = [t.to("cuda", dtype).contiguous()
                                 for t in tensors]
    return deform_conv2d_backward(inp, off, msk, w, gout, (stride, stride),
                                  (pad, pad), (dil, dil), dg, cols=cols,
                                  path=path)


def _rel_errs(grads, ref):
    return [(g.float().cpu() - r).abs().max().item()
            / (r.abs().max().item() + 1e-6) for g, r in zip(grads, ref)]


def _check_oracle(grads, ref, which=NAMES):
    errs = dict(zip(NAMES, _rel_errs(grads, ref)))
    print("rel errs:", {n: f"{errs[n]:.3g}" for n in which})
    for n in which:
        assert errs[n] < 1e-3, f"grad_{n} rel err {errs[n]}"


@pytest.mark.parametrize("off_scale", [2.0, 8.0])
def test_fused_fp32_matches_oracle(off_scale):
    """Odd sizes (partial waves, rows that are no 16-B multiple).  Scale 8
    puts many samples outside the image or in the (-1, 0) / (H-1, H)
    border bands."""
    from esr_amd.ops import dcn
    tensors, ref = _problem(2, 16, 14, 18, 12, 4, off_scale=off_scale, seed=3)
    before = dict(dcn.stats)
    grads = _run(tensors, 4, "fused")
    assert dcn.stats["bwd_fused"] == before["bwd_fused"] + 1
    assert dcn.stats["bwd_split"] == before["bwd_split"]
    _check_oracle(grads, ref)


@pytest.mark.parametrize("C,dg,Cout", [(12, 2, 5), (16, 8, 5)],
                         ids=["cpg6", "cpg2"])
def test_fused_fp32_cpg_not_multiple_of_chunk(C, dg, Cout):
    """The fused kernel loads channels four at a time; with cpg = 6 the
    second chunk's tail, and with cpg = 2 half of the only chunk, lies past
    cpg: it re-reads the last channel and must not be added anywhere."""
    from esr_amd.ops import dcn
    tensors, ref = _problem(1, C, 9, 11, Cout, dg, off_scale=2.0, seed=13)
    before = dcn.stats["bwd_fused"]
    grads = _run(tensors, dg, "fused")
    assert dcn.stats["bwd_fused"] == before + 1
    _check_oracle(grads, ref)


@pytest.mark.parametrize("stride,pad,dil", [(2, 1, 1), (1, 2, 2)])
def test_fused_stride_and_dilation(stride, pad, dil):
    tensors, ref = _problem(1, 8, 16, 16, 4, 2, stride=stride, pad=pad,
                            dil=dil, off_scale=1.0, seed=9)
    grads = _run(tensors, 2, "fused", stride=stride, pad=pad, dil=dil)
    _check_oracle(grads, ref, ["input", "offset", "mask"])


def test_whole_group_edge():
    """cpg*H*W*4 of exactly 64 KiB runs fused; 73.7 KB does not: auto takes
    the split path there, fused is an error, auto still matches."""
    from esr_amd.ops import dcn
    from esr_amd.ops.native import require_ext
    tensors, ref = _problem(1, 8, 32, 64, 4, 1, seed=5)
    before = dcn.stats["bwd_fused"]
    _check_oracle(_run(tensors, 1, "auto"), ref)
    assert dcn.stats["bwd_fused"] == before + 1

    tensors, ref = _problem(1, 8, 48, 48, 4, 1, seed=6)
    before = dict(dcn.stats)
    _check_oracle(_run(tensors, 1, "auto"), ref)
    assert dcn.stats["bwd_split"] == before["bwd_split"] + 1
    assert dcn.stats["bwd_fused"] == before["bwd_fused"]
    with pytest.raises(ValueError, match="fused backward needs"):
        _run(tensors, 1, "fused")
    # the extension refuses it too, whoever calls
    inp, off, msk, w, _, gout = [t.cuda() for t in tensors]
    with pytest.raises(RuntimeError, match="fused path"):
        require_ext().deform_conv2d_backward_cols(
            inp, off, msk, w, gout, None, 1, 1, 1, 1, 1, 1, 1, "fused")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_16bit_no_worse_than_split(dtype):
    """Both paths keep an fp32 sum and round once, so only the add order
    differs: per grad the fused max-abs error against the fp32 oracle (on
    the same 16-bit-rounded inputs) is at most 2x the split path's.
    Beside it both paths are held to the float64 bounds, so they cannot be
    wrong in the same way; that problem has grid offsets and 30 rows, not
    32: the weight grad sums B*Ho*Wo + 8 terms in fp32 and the bound rule
    wants that below 2^11."""
    tensors, ref = _problem(2, 16, 32, 32, 16, 4, seed=11, dtype=dtype)
    fused = _run(tensors, 4, "fused", dtype=dtype)
    split = _run(tensors, 4, "split", dtype=dtype)
    assert all(g.dtype == dtype for g in fused)
    ef = [(g.float().cpu() - r).abs().max().item() for g, r in zip(fused, ref)]
    es = [(g.float().cpu() - r).abs().max().item() for g, r in zip(split, ref)]
    report = ", ".join(f"{n}: fused {a:.4g} / split {b:.4g}"
                       for n, a, b in zip(NAMES, ef, es))
    print(f"DCN backward max-abs errors ({dtype}) -", report)
    bad = [n for n, a, b in zip(NAMES, ef, es) if not a <= 2 * b]
    assert not bad, f"fused worse than 2x split on {bad} - {report}"

    tensors, ref, bounds = _bound_problem(2, 16, 30, 32, 16, 4, seed=11,
                                          dtype=dtype)
    for path in ("fused", "split"):
        _check_bounds(_run(tensors, 4, path, dtype=dtype), ref, bounds,
                      dtype, f"30x32 {path}")


def test_fused_run_to_run():
    tensors, _ = _problem(2, 16, 32, 32, 8, 4, seed=0)
    g1 = _run(tensors, 4, "fused")
    g2 = _run(tensors, 4, "fused")
    for a, b, n in zip(g1, g2, NAMES):
        print(f"grad_{n}: {(a != b).sum().item()} of {a.numel()} differ")
        assert torch.allclose(a, b, atol=ATOL, rtol=RTOL), n


@pytest.mark.parametrize("save", ["1", "0"])
def test_saved_columns_match_recompute(monkeypatch, save):
    """Grads through modulated_deform_conv2d against the 12-argument entry,
    which rebuilds the columns: weight and bias bitwise, the rest within
    the run-to-run bound; the same with saving switched off."""
    from esr_amd.ops import dcn
    from esr_amd.ops.native import require_ext
    monkeypatch.setenv("ESR_DCN_SAVE_COLS", save)
    tensors, _ = _problem(2, 16, 14, 18, 12, 4, seed=7)
    *args, gout = [t.cuda() for t in tensors]
    leaves = [t.clone().requires_grad_(True) for t in args]
    before = dcn.stats["bwd_cols_saved"]
    out = dcn.modulated_deform_conv2d(*leaves, stride=1, padding=1,
                                      dilation=1, deformable_groups=4)
    out.backward(gout)
    assert dcn.stats["bwd_cols_saved"] == before + (save == "1")
    ref = require_ext().deform_conv2d_backward(
        *args[:4], gout, 1, 1, 1, 1, 1, 1, 4)
    got = [t.grad for t in leaves]
    assert torch.equal(got[3], ref[3]), "grad_weight not bitwise"
    assert torch.equal(got[4], ref[4]), "grad_bias not bitwise"
    for i in range(3):
        assert torch.allclose(got[i], ref[i], atol=ATOL, rtol=RTOL), NAMES[i]


def test_graph_capture_replays():
    """Forward + backward of a DeformAlign2d in bf16 captured with the
    engine's helper: two replays give finite grads equal to the eager run.
    Capture fails on a synchronise or a host read, so this also shows the
    path has neither."""
    from esr_amd.engine.capture import capture_graph
    from esr_amd.ops import dcn
    torch.manual_seed(0)
    m = dcn.DeformAlign2d(16, 16, 3, padding=1, deformable_groups=4) \
        .cuda().to(torch.bfloat16)
    x = torch.randn(2, 16, 32, 32, device="cuda").to(torch.bfloat16) \
        .requires_grad_(True)
    f = torch.randn(2, 16, 32, 32, device="cuda").to(torch.bfloat16) \
        .requires_grad_(True)
    leaves = [x, f] + list(m.parameters())

    def body():
        out = m(x, f)
        return torch.autograd.grad(out.float().square().mean(), leaves)

    before = dcn.stats["bwd_fused"]
    eager = [g.clone() for g in body()]
    assert dcn.stats["bwd_fused"] == before + 1
    graph, static = capture_graph(body, warmup=2)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, eager):
            assert torch.isfinite(got).all()
            assert torch.allclose(got.float(), want.float(),
                                  atol=ATOL, rtol=RTOL)


# ------------------------------------------- per-element float64 bounds
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
PATHS = ["fused", "split"]


@functools.lru_cache(maxsize=None)
def _bound_problem(B, C, H, W, Cout, dg, stride=1, pad=1, dil=1,
                   off_scale=2.0, seed=0, dtype=torch.float32, lattice=None):
    """Grid-offset CPU tensors (input, offset, mask, weight, bias, grad_out)
    rounded to `dtype`, the float64 grads and their bounds.  Cached: callers
    must not modify what they get."""
    args, gout = dcn_grid_problem(B, C, H, W, Cout, dg, stride, pad, dil,
                                  off_scale, seed, dtype, lattice)
    geom = (stride, pad, dil, dg)
    ref = dcn_bwd_ref64(args, gout, geom)
    return args + [gout], ref, dcn_bwd_bounds(args, gout, geom, ref, dtype)


def _check_bounds(grads, ref, bounds, dtype, what):
    """All five grads, every element counted; prints each worst diff/bound
    before asserting."""
    over = {}
    for n, g, r, bd in zip(NAMES, grads, ref, bounds):
        assert g.dtype == dtype, (n, g.dtype)
        over[n], worst = count_over(g.cpu(), r, bd)
        print(f"{what} {str(dtype)[6:]} grad_{n}: {over[n]}/{r.numel()} "
              f"over, "
              f"max diff/bound {worst:.3f}")
    assert not any(over.values()), f"{what}: elements over the bound {over}"


def _run_counted(tensors, dg, path, **kw):
    """_run, and check that `path` is the one that ran."""
    from esr_amd.ops import dcn
    other = "split" if path == "fused" else "fused"
    before = dict(dcn.stats)
    grads = _run(tensors, dg, path, **kw)
    assert dcn.stats["bwd_" + path] == before["bwd_" + path] + 1
    assert dcn.stats["bwd_" + other] == before["bwd_" + other]
    return grads


@pytest.mark.parametrize("off_scale", [2.0, 8.0])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_main_shape_within_bounds(dtype, path, off_scale):
    """B2 C16 14x18 Cout12 dg4: partial waves, two x-tiles of the tiled
    col2im with the second partial.  On the split path fp32 takes
    dcn_col2im_tiled_kernel and the 16-bit types dcn_col2im_kernel
    (ESR_DCN_TILED is read once per process and left alone here).  Scale 8
    pushes samples beyond the tile's +-4 halo, so the tiled kernel's
    global-atomic fallback runs, and many outside the image."""
    tensors, ref, bounds = _bound_problem(2, 16, 14, 18, 12, 4,
                                          off_scale=off_scale, seed=3,
                                          dtype=dtype)
    grads = _run_counted(tensors, 4, path, dtype=dtype)
    _check_bounds(grads, ref, bounds, dtype, f"14x18 s{off_scale:g} {path}")


def test_tiled_grid_within_bounds():
    """18x34 in fp32 on the split path: 2x3 tiles of dcn_col2im_tiled_kernel,
    partial in both directions."""
    tensors, ref, bounds = _bound_problem(1, 8, 18, 34, 4, 2, off_scale=2.0,
                                          seed=17)
    grads = _run_counted(tensors, 2, "split")
    _check_bounds(grads, ref, bounds, torch.float32, "18x34 split")


@pytest.mark.parametrize("lattice", ["zero", "int"])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES[:2], ids=DT_IDS[:2])
def test_lattice_offsets_within_bounds(dtype, path, lattice):
    """All-zero offsets (DeformAlign2d's initial state: every top-row and
    left-column tap exactly on -1) and integer offsets in {-2..2}: every
    sample sits on a pixel, where the offset grad is the one-sided
    derivative of the cell [floor, floor + 1], and zero at <= -1."""
    tensors, ref, bounds = _bound_problem(2, 16, 14, 18, 12, 4, seed=19,
                                          dtype=dtype, lattice=lattice)
    grads = _run_counted(tensors, 4, path, dtype=dtype)
    _check_bounds(grads, ref, bounds, dtype, f"lattice {lattice} {path}")


@pytest.mark.parametrize("C,dg,Cout", [(12, 2, 5), (16, 8, 5)],
                         ids=["cpg6", "cpg2"])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES[:2], ids=DT_IDS[:2])
def test_cpg_tail_within_bounds(dtype, path, C, dg, Cout):
    """cpg 6 and 2 against the fused kernel's four-channel chunks, and the
    same through the split kernels."""
    tensors, ref, bounds = _bound_problem(1, C, 9, 11, Cout, dg, seed=13,
                                          dtype=dtype)
    grads = _run_counted(tensors, dg, path, dtype=dtype)
    _check_bounds(grads, ref, bounds, dtype, f"9x11 cpg{C // dg} {path}")


@pytest.mark.parametrize("stride,pad,dil", [(2, 1, 1), (1, 2, 2)])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES[:2], ids=DT_IDS[:2])
def test_stride_and_dilation_within_bounds(dtype, path, stride, pad, dil):
    tensors, ref, bounds = _bound_problem(1, 8, 16, 16, 4, 2, stride=stride,
                                          pad=pad, dil=dil, off_scale=1.0,
                                          seed=9, dtype=dtype)
    grads = _run_counted(tensors, 2, path, stride=stride, pad=pad, dil=dil,
                         dtype=dtype)
    _check_bounds(grads, ref, bounds, dtype,
                  f"16x16 s{stride}p{pad}d{dil} {path}")


@pytest.mark.parametrize("save", [None, "0"], ids=["saved", "rebuilt"])
def test_autograd_bf16_within_bounds(monkeypatch, save):
    """Grads through modulated_deform_conv2d in bf16, with the forward's
    columns saved (ESR_DCN_SAVE_COLS unset) and rebuilt in the backward."""
    from esr_amd.ops import dcn
    if save is None:
        monkeypatch.delenv("ESR_DCN_SAVE_COLS", raising=False)
    else:
        monkeypatch.setenv("ESR_DCN_SAVE_COLS", save)
    monkeypatch.delenv("ESR_DCN_BWD", raising=False)
    dtype = torch.bfloat16
    tensors, ref, bounds = _bound_problem(2, 16, 14, 18, 12, 4, seed=3,
                                          dtype=dtype)
    *args, gout = [t.to("cuda", dtype) for t in tensors]
    leaves = [t.clone().requires_grad_(True) for t in args]
    before = dict(dcn.stats)
    out = dcn.modulated_deform_conv2d(*leaves, stride=1, padding=1,
                                      dilation=1, deformable_groups=4)
    out.backward(gout)
    assert dcn.stats["bwd_fused"] == before["bwd_fused"] + 1
    assert dcn.stats["bwd_cols_saved"] == \
        before["bwd_cols_saved"] + (save is None)
    _check_bounds([t.grad for t in leaves], ref, bounds, dtype,
                  f"autograd cols {'saved' if save is None else 'rebuilt'}")
