#!/usr/bin/env python3
"""Microbenchmark the DCN kernels at the flagship shape (GPU box).

  python tools/bench_dcn.py --batch 768 --dtype bf16   # what the step runs
  python tools/bench_dcn.py --bwd-path split           # one backward path
  ESR_DCN_TILED=0 python tools/bench_dcn.py --dtype fp32 --bwd-path split
                                   # split path, per-contribution col2im

The backward is timed per path (fused / split), with the im2col columns
rebuilt and with them handed over from the forward.
"""

import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from esr_amd.ops.dcn import deform_conv2d_backward  # noqa: E402
from esr_amd.ops.native import require_ext  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16,
          "fp16": torch.float16}


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--batch", type=int, default=128,
                   help="the flagship step runs 768")
    p.add_argument("--dtype", choices=sorted(DTYPES), default="fp32")
    p.add_argument("--bwd-path", choices=["both", "auto", "fused", "split"],
                   default="both")
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()

    ext = require_ext()
    dt = DTYPES[args.dtype]
    g = torch.Generator().manual_seed(0)
    B, C, H, W, Cout, dg = args.batch, 64, 32, 32, 64, 8  # dense_fuse shape

    def dev(t):
        return t.cuda().to(dt)

    input = dev(torch.randn(B, C, H, W, generator=g))
    offset = dev(torch.randn(B, dg * 18, H, W, generator=g) * 1.5)
    mask = dev(torch.rand(B, dg * 9, H, W, generator=g))
    weight = dev(torch.randn(Cout, C, 3, 3, generator=g) * 0.2)
    bias = dev(torch.randn(Cout, generator=g))
    gout = dev(torch.randn(B, Cout, H, W, generator=g))
    one = (1, 1)

    print(f"B={B} C={C} {H}x{W} dg={dg} {args.dtype} "
          f"ESR_DCN_TILED={os.environ.get('ESR_DCN_TILED', 'default')}")
    if dt == torch.float32:
        t_fwd_fused = timeit(lambda: ext.deform_conv2d_forward_fused(
            input, offset, mask, weight, bias, dg))
        print(f"fwd fused      : {t_fwd_fused:.3f} ms")
    cols_fn = lambda: ext.deform_im2col(input, offset, mask, 3, 3, 1, 1,  # noqa
                                        1, 1, 1, 1, dg)
    t_im2col = timeit(cols_fn)
    cols = cols_fn()
    t_gemm = timeit(lambda: torch.matmul(weight.reshape(Cout, -1), cols))
    print(f"fwd im2col     : {t_im2col:.3f} ms (+GEMM {t_gemm:.3f} ms)")

    paths = ["fused", "split"] if args.bwd_path == "both" else [args.bwd_path]
    for path in paths:
        for label, c in (("cols rebuilt", None), ("cols saved", cols)):
            t = timeit(lambda: deform_conv2d_backward(
                input, offset, mask, weight, gout, one, one, one, dg,
                cols=c, path=path), iters=args.iters, warmup=3)
            print(f"bwd {path:5s} ({label:12s}): {t:.3f} ms")


if __name__ == "__main__":
    main()
