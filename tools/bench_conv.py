#!/usr/bin/env python3
"""Microbenchmark: native gfx950 conv kernels vs torch/MIOpen per shape.

Runs the conv shapes ESRNet's flagship config actually executes (batch
sizes as in the batch-64 bench step) and prints native vs torch (bf16,
NCHW) forward and fwd+bwd times.

--dtype fp16 runs the same comparison with fp16 operands (native fp16
kernels vs MIOpen fp16); --wgrad stays bf16 (the native weight-grad kernel
is bf16-only).

--bias-grad times the conv bias gradient at the same call sites:
act_grad + dpre.sum((0,2,3)) against act_grad_bias (bias_grad where the conv
has no activation), with the bytes each must move over the kernel time.

Usage (GPU box): python tools/bench_conv.py [--iters 50] [--dtype fp16]
"""

import argparse
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

# (label, frames, Cin, Cout, H, W, ks, stride, act) — flagship step shapes
SHAPES = [
    ("head 2->8 @256", 512, 2, 8, 256, 256, 3, 1, "relu"),
    ("enc1 8->16 s2 @256", 512, 8, 16, 256, 256, 3, 2, "relu"),
    ("enc2 16->32 s2 @128", 512, 16, 32, 128, 128, 3, 2, "relu"),
    ("enc3 32->64 s2 @64", 512, 32, 64, 64, 64, 3, 2, "relu"),
    ("ltc predmap 128->64 @32", 768, 128, 64, 32, 32, 3, 1, "relu"),
    ("ltc predmap 64->1 @32", 768, 64, 1, 32, 32, 3, 1, "sigmoid"),
    ("ltc resblock 192->192 @32", 384, 192, 192, 32, 32, 3, 1, "relu"),
    ("ltc fuse 192->64 @32", 384, 192, 64, 32, 32, 3, 1, None),
    ("gru ur 128->128 @32", 768, 128, 128, 32, 32, 3, 1, None),
    ("gru out 128->64 @32", 768, 128, 64, 32, 32, 3, 1, None),
    ("gfuse 128->64 1x1 @32", 384, 128, 64, 32, 32, 1, 1, "relu"),
    ("fusion 128->64 @32", 768, 128, 64, 32, 32, 3, 1, "relu"),
    ("dense 192->64 @32", 384, 192, 64, 32, 32, 3, 1, "relu"),
    ("recon1 64->128 @32", 384, 64, 128, 32, 32, 3, 1, None),
    ("recon2 32->64 @64", 384, 32, 64, 64, 64, 3, 1, None),
    ("recon3 16->32 @128", 384, 16, 32, 128, 128, 3, 1, None),
    ("tail 8->2 @256", 384, 8, 2, 256, 256, 3, 1, "relu"),
]


DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def bench(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def valu2_component(args):
    """Tiny-channel shapes: v2 strip kernel vs v1 VALU vs torch/MIOpen."""
    from esr_amd.ops.conv import ACT_IDS
    from esr_amd.ops.native import require_ext
    ext = require_ext()
    dev = "cuda:0"
    dt = DTYPES[args.dtype]
    torch.manual_seed(0)
    tiny = [sh for sh in SHAPES if sh[2] < 32 and sh[3] < 32]
    print(f"{'shape':34s} {'v2 ms':>9s} {'v1 ms':>9s} {'torch':>9s} {'t/v2':>6s}")
    for label, B, cin, cout, h, w, ks, stride, act in tiny:
        x = torch.randn(B, cin, h, w, device=dev).to(dt)
        wt = (torch.randn(cout, cin, ks, ks, device=dev) * 0.2).to(dt)
        b = torch.randn(cout, device=dev).float()
        aid = ACT_IDS[act]
        act_fn = {None: lambda t: t, "relu": F.relu,
                  "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act]

        def v2():
            return ext.conv2d_fwd_valu2(x, wt, b, stride, aid)

        def v1():
            return ext.conv2d_fwd_valu(x, wt, b, stride, aid)

        def ref():
            return act_fn(F.conv2d(x, wt, b.to(dt),
                                   stride=stride, padding=ks // 2))
        # correctness spot check before timing
        got = v2().float()
        want = act_fn(F.conv2d(x.float(), wt.float(), b,
                               stride=stride, padding=ks // 2))
        err = (got - want).abs().max().item()
        scale = want.abs().max().item() + 1e-6
        assert err / scale < 2e-2, f"{label}: v2 wrong, rel {err / scale}"
        t2 = bench(v2, args.iters)
        t1 = bench(v1, args.iters)
        tt = bench(ref, args.iters)
        print(f"{label:34s} {t2:9.3f} {t1:9.3f} {tt:9.3f} {tt / t2:6.2f}")


def wgrad_component(args):
    """Isolated weight-grad: native conv2d_wgrad_mfma vs aten wgrad-only."""
    from esr_amd.ops.native import require_ext
    ext = require_ext()
    dev = "cuda:0"
    torch.manual_seed(0)
    if args.dtype != "bf16":
        print("--wgrad: the native weight-grad kernel is bf16-only; "
              "timing bf16")

    def ceil(v, m):
        return (v + m - 1) // m * m

    print(f"{'shape':34s} {'native ms':>10s} {'aten ms':>10s} {'x':>6s}")
    for label, B, cin, cout, h, w, ks, stride, _ in SHAPES:
        x = torch.randn(B, cin, h, w, device=dev).to(torch.bfloat16)
        dy_h = (h + 2 * (ks // 2) - ks) // stride + 1
        dy_w = (w + 2 * (ks // 2) - ks) // stride + 1
        dy = torch.randn(B, cout, dy_h, dy_w, device=dev).to(torch.bfloat16)
        wt = torch.randn(cout, cin, ks, ks, device=dev).to(torch.bfloat16)

        def native():
            return ext.conv2d_wgrad_mfma(x, dy, ks, stride,
                                         ceil(cin, 16), ceil(cout, 16))

        def aten():
            return torch.ops.aten.convolution_backward(
                dy, x, wt, None, [stride, stride], [ks // 2, ks // 2],
                [1, 1], False, [0, 0], 1, [False, True, False])[1]

        tn = bench(native, args.iters)
        tt = bench(aten, args.iters)
        print(f"{label:34s} {tn:10.3f} {tt:10.3f} {tt / tn:6.2f}")


# deep stride-1 shapes of the flagship that SHAPES does not list (frames as
# the step calls them)
DEEP_EXTRA = [
    ("lstm/convblock 64->64 @32", 384, 64, 64, 32, 32, 3, 1, "relu"),
    ("offset 128->64 @32", 192, 128, 64, 32, 32, 3, 1, "relu"),
    ("dcn offset/mask 64->216 @32", 128, 64, 216, 32, 32, 3, 1, None),
]


def bwd_parts_component(args):
    """Deep stride-1 class, bf16: the whole backward of one conv as
    _NativeConv2dFn.backward runs it (act grad + bias grad + dx + dW) under
    ESR_CONV_BWD = auto (the default routing) / dgrad (input grad native,
    weight grad aten) / native / aten, then input grad and weight grad
    alone, native against aten with only that output asked for (aten's time
    includes its layout transposes), and the forward on the 8x32-tile core
    against conv2d_fwd_mfma.  Times in ms."""
    import os
    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn, _pack
    from esr_amd.ops.native import require_ext
    ext = require_ext()
    dev = "cuda:0"
    bf = torch.bfloat16
    torch.manual_seed(0)
    deep = [sh for sh in SHAPES + DEEP_EXTRA
            if sh[7] == 1 and sh[2] >= 32 and sh[3] >= 32]
    print(f"{'shape':30s} {'B':>4s} | {'bwd auto':>8s} {'dgrad':>7s} "
          f"{'native':>7s} {'aten':>7s} | {'dx core':>7s} {'dx old':>7s} {'dx aten':>7s} | "
          f"{'dW nat':>7s} {'dW aten':>7s} | {'fwd core':>8s} {'fwd old':>7s}")
    tot = [0.0] * 11
    for label, B, cin, cout, h, w_, ks, stride, act in deep:
        x = torch.randn(B, cin, h, w_, device=dev).to(bf)
        wt = (torch.randn(cout, cin, ks, ks, device=dev) * 0.2).to(bf)
        b = torch.randn(cout, device=dev).to(bf)
        bias_f = b.float()
        aid = ACT_IDS[act]
        xg = x.clone().requires_grad_(True)
        wg = wt.clone().requires_grad_(True)
        bg = b.clone().requires_grad_(True)
        y = _NativeConv2dFn.apply(xg, wg, bg, stride, aid)
        gy = torch.randn_like(y)
        dpre = ext.act_grad(gy, y.detach(), aid) if aid else gy
        pad = [ks // 2, ks // 2]

        def whole():
            return torch.autograd.grad(y, (xg, wg, bg), gy, retain_graph=True)

        def aten_part(mask):
            return lambda: torch.ops.aten.convolution_backward(
                dpre, x, wt, None, [1, 1], pad, [1, 1], False, [0, 0], 1,
                mask)

        def dx_old():
            t = wt.transpose(0, 1)
            if ks == 3:
                t = t.flip((2, 3))
            return ext.conv2d_fwd_mfma(dpre, _pack(t), None, cin, ks, 1, 0)

        times = []
        for mode in ("auto", "dgrad", "native", "aten"):
            os.environ["ESR_CONV_BWD"] = mode
            times.append(bench(whole, args.iters))
        os.environ.pop("ESR_CONV_BWD")
        times.append(bench(
            lambda: ext.conv2d_s1(dpre, wt, None, 0, True), args.iters))
        times.append(bench(dx_old, args.iters))
        times.append(bench(aten_part([True, False, False]), args.iters))
        times.append(bench(
            lambda: ext.conv2d_wgrad_s1(x, dpre, ks), args.iters))
        times.append(bench(aten_part([False, True, False]), args.iters))
        times.append(bench(
            lambda: ext.conv2d_s1(x, wt, bias_f, aid, False), args.iters))
        times.append(bench(
            lambda: ext.conv2d_fwd_mfma(x, _pack(wt), bias_f, cout, ks, 1,
                                        aid), args.iters))
        # the two forward kernels add in the same order: compare bits
        same = torch.equal(ext.conv2d_s1(x, wt, bias_f, aid, False),
                           ext.conv2d_fwd_mfma(x, _pack(wt), bias_f, cout,
                                               ks, 1, aid))
        tot = [a + t for a, t in zip(tot, times)]
        t = times
        print(f"{label:30s} {B:4d} | {t[0]:8.3f} {t[1]:7.3f} {t[2]:7.3f} "
              f"{t[3]:7.3f} | {t[4]:7.3f} {t[5]:7.3f} {t[6]:7.3f} | "
              f"{t[7]:7.3f} {t[8]:7.3f} | {t[9]:8.3f} {t[10]:7.3f}"
              f"{'' if same else '  fwd bits differ'}", flush=True)
    t = tot
    print(f"{'TOTAL':30s} {'':4s} | {t[0]:8.3f} {t[1]:7.3f} {t[2]:7.3f} "
          f"{t[3]:7.3f} | {t[4]:7.3f} {t[5]:7.3f} {t[6]:7.3f} | {t[7]:7.3f} "
          f"{t[8]:7.3f} | {t[9]:8.3f} {t[10]:7.3f}")


HBM_PEAK_TBS = 8.0   # MI355X HBM3E peak


def bias_grad_component(args):
    """Bias gradient at the flagship call sites: today's two passes
    (act_grad, then torch's strided sum over dpre) against the fused pass.
    Bytes that must move: 3*|dpre| fused (read dy and y, write dpre),
    1*|dpre| for the read-only bias_grad of a conv without activation."""
    from esr_amd.ops.conv import ACT_IDS
    from esr_amd.ops.native import require_ext
    ext = require_ext()
    dev = "cuda:0"
    dt = DTYPES[args.dtype]
    torch.manual_seed(0)
    print(f"{'shape':34s} {'MB':>7s} {'old ms':>8s} {'new ms':>8s} "
          f"{'x':>6s} {'TB/s':>6s} {'of peak':>8s}")
    tot_o = tot_n = 0.0
    for label, B, cin, cout, h, w, ks, stride, act in SHAPES:
        ho = (h + 2 * (ks // 2) - ks) // stride + 1
        wo = (w + 2 * (ks // 2) - ks) // stride + 1
        dy = torch.randn(B, cout, ho, wo, device=dev).to(dt)
        y = None
        if act:
            act_fn = {"relu": torch.relu, "sigmoid": torch.sigmoid,
                      "tanh": torch.tanh}[act]
            y = act_fn(torch.randn_like(dy, dtype=torch.float32)).to(dt)
        aid = ACT_IDS[act]

        def old():
            dpre = ext.act_grad(dy, y, aid) if aid else dy
            return dpre.sum((0, 2, 3))

        def new():
            if aid:
                return ext.act_grad_bias(dy, y, aid)[1]
            return ext.bias_grad(dy)[0]

        ref = old().float()
        err = (new().float() - ref).abs().max().item()
        assert err <= 2.0 ** -6 * ref.abs().max().item() + 1e-3, (label, err)
        nbytes = dy.numel() * 2 * (3 if aid else 1)
        to = bench(old, args.iters)
        tn = bench(new, args.iters)
        tbs = nbytes / (tn * 1e-3) / 1e12
        tot_o += to
        tot_n += tn
        print(f"{label:34s} {nbytes / 1e6:7.1f} {to:8.3f} {tn:8.3f} "
              f"{to / tn:6.2f} {tbs:6.2f} {tbs / HBM_PEAK_TBS:8.1%}")
    print(f"{'TOTAL':34s} {'':7s} {tot_o:8.3f} {tot_n:8.3f} "
          f"{tot_o / tot_n:6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--bwd", action="store_true", help="also time fwd+bwd")
    ap.add_argument("--wgrad", action="store_true",
                    help="time the wgrad kernel alone vs aten wgrad-only")
    ap.add_argument("--valu2", action="store_true",
                    help="A/B the tiny-channel strip kernel vs v1 and torch")
    ap.add_argument("--bias-grad", action="store_true",
                    help="time act_grad + sum((0,2,3)) against "
                         "act_grad_bias / bias_grad, with achieved bytes/s")
    ap.add_argument("--bwd-parts", action="store_true",
                    help="deep stride-1 class: whole backward per conv under "
                         "ESR_CONV_BWD=auto/native/aten, dx and dW alone "
                         "against aten, forward core against the older kernel")
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="bf16",
                    help="operand dtype of the native kernels and of the "
                         "MIOpen comparison (--wgrad stays bf16)")
    args = ap.parse_args()

    if args.wgrad:
        return wgrad_component(args)
    if args.valu2:
        return valu2_component(args)
    if args.bias_grad:
        return bias_grad_component(args)
    if args.bwd_parts:
        return bwd_parts_component(args)

    from esr_amd.ops.conv import ACT_IDS, _NativeConv2dFn
    dev = "cuda:0"
    dt = DTYPES[args.dtype]
    torch.manual_seed(0)

    total_n, total_t = 0.0, 0.0
    print(f"{'shape':34s} {'native ms':>10s} {'torch ms':>10s} {'x':>6s}")
    for label, B, cin, cout, h, w, ks, stride, act in SHAPES:
        x = torch.randn(B, cin, h, w, device=dev).to(dt)
        wt = (torch.randn(cout, cin, ks, ks, device=dev) * 0.2).to(dt)
        b = torch.randn(cout, device=dev).to(dt)
        act_fn = {None: lambda t: t, "relu": F.relu,
                  "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act]

        def native():
            return _NativeConv2dFn.apply(x, wt, b, stride, ACT_IDS[act])

        def ref():
            return act_fn(F.conv2d(x, wt, b, stride=stride, padding=ks // 2))

        if args.bwd:
            xg = x.clone().requires_grad_(True)
            wg = wt.clone().requires_grad_(True)
            bgr = b.clone().requires_grad_(True)
            y0 = native()
            gy = torch.randn_like(y0)

            def native_b():
                y = _NativeConv2dFn.apply(xg, wg, bgr, stride, ACT_IDS[act])
                y.backward(gy)

            xr = x.clone().requires_grad_(True)
            wr = wt.clone().requires_grad_(True)
            br = b.clone().requires_grad_(True)

            def ref_b():
                y = act_fn(F.conv2d(xr, wr, br, stride=stride,
                                    padding=ks // 2))
                y.backward(gy)
            tn = bench(native_b, args.iters)
            tt = bench(ref_b, args.iters)
        else:
            tn = bench(native, args.iters)
            tt = bench(ref, args.iters)
        total_n += tn
        total_t += tt
        print(f"{label:34s} {tn:10.3f} {tt:10.3f} {tt / tn:6.2f}")
    print(f"{'TOTAL':34s} {total_n:10.3f} {total_t:10.3f} "
          f"{total_t / total_n:6.2f}")


if __name__ == "__main__":
    main()
