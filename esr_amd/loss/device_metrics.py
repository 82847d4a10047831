"""Restoration metrics as per-plane sums, for evaluation on the device.

`loss/metrics.py` returns one Python float per metric and per call, each
through `.item()`.  Here one call gives five float64 columns per plane (one
plane is one (image, channel)):

    0  sum |p - t|      1  sum (p - t)^2      2  max t      3  min t
    4  sum of SSIM over the (H-6)(W-6) valid 7x7 window positions

and `finalize` turns a table of them into l1 / mse / rmse / psnr / ssim on the
host with the semantics of `loss/metrics.py`, once per evaluation instead of
once per window.

`metric_sums` runs the native kernel (ops/native/src/eval_metrics.hip) on CUDA
fp32 inputs; `metric_sums_torch` is the same thing in float64 torch ops on
any device: the CPU path and the kernel's oracle.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ..ops.native import get_ext

__all__ = ["metric_sums", "metric_sums_torch", "finalize", "COLUMNS"]

COLUMNS = ("abs_sum", "sq_sum", "tgt_max", "tgt_min", "ssim_sum")
_WIN, _K1, _K2 = 7, 0.01, 0.03


def _planes(pred: torch.Tensor, tgt: torch.Tensor):
    if pred.shape != tgt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and tgt "
                         f"{tuple(tgt.shape)} differ in shape")
    if pred.dim() < 2:
        raise ValueError("metric_sums needs [..., H, W] maps")
    H, W = pred.shape[-2:]
    if H < _WIN or W < _WIN:
        raise ValueError(f"metric_sums needs H, W >= {_WIN} for the SSIM "
                         f"window, got {H}x{W}")
    return pred.reshape(-1, H, W), tgt.reshape(-1, H, W)


def metric_sums_torch(pred: torch.Tensor, tgt: torch.Tensor,
                      data_range: float = 2.0) -> torch.Tensor:
    """[..., H, W] maps -> float64 [P, 5] on the inputs' device."""
    p, t = _planes(pred.detach(), tgt.detach())
    p, t = p.double(), t.double()
    d = p - t
    n = _WIN * _WIN
    cov_norm = n / (n - 1)

    def filt(x):                     # window mean, valid border
        return F.avg_pool2d(x[:, None], _WIN, stride=1)[:, 0]

    ux, uy = filt(p), filt(t)
    uxx, uyy, uxy = filt(p * p), filt(t * t), filt(p * t)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1 = (_K1 * data_range) ** 2
    C2 = (_K2 * data_range) ** 2
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) \
        / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return torch.stack([d.abs().sum((1, 2)), (d * d).sum((1, 2)),
                        t.amax((1, 2)), t.amin((1, 2)), s.sum((1, 2))], dim=1)


def metric_sums(pred: torch.Tensor, tgt: torch.Tensor,
                data_range: float = 2.0) -> torch.Tensor:
    """[..., H, W] maps -> float64 [P, 5].  No host synchronisation: safe
    inside a captured graph."""
    ext = get_ext() if pred.is_cuda else None
    if (ext is not None and hasattr(ext, "restoration_metrics")
            and pred.dtype == torch.float32 and tgt.dtype == torch.float32):
        p, t = _planes(pred.detach(), tgt.detach())
        return ext.restoration_metrics(p.contiguous(), t.contiguous(),
                                       float(data_range))
    return metric_sums_torch(pred, tgt, data_range)


def finalize(sums: torch.Tensor, C: int, H: int, W: int) -> dict:
    """float64 [N*C, 5] sums -> {"l1", "mse", "rmse", "psnr", "ssim"}, each a
    list of N Python floats (one per image), computed in float64 on the host.

    As in loss/metrics.py: l1 and mse are means over all C*H*W elements; ssim
    is the mean over channels of the per-channel mean; psnr is per channel
    with data_range = max(tgt[ch]) - min(tgt over ALL channels), a
    non-positive range taken as 1.0 and zero error as inf, then averaged."""
    rows = sums.detach().to("cpu", torch.float64).reshape(-1, C, 5).tolist()
    n_pix, n_win = H * W, (H - _WIN + 1) * (W - _WIN + 1)
    out = {k: [] for k in ("l1", "mse", "rmse", "psnr", "ssim")}
    for img in rows:
        mse = sum(ch[1] for ch in img) / (C * n_pix)
        out["l1"].append(sum(ch[0] for ch in img) / (C * n_pix))
        out["mse"].append(mse)
        out["rmse"].append(math.sqrt(mse))
        out["ssim"].append(sum(ch[4] / n_win for ch in img) / C)
        tmin = min(ch[3] for ch in img)
        total = 0.0
        for ch in img:
            err = ch[1] / n_pix
            if err == 0:
                total += float("inf")
                continue
            data_range = ch[2] - tmin
            data_range = data_range if data_range > 0 else 1.0
            total += 10.0 * math.log10(data_range ** 2 / err)
        out["psnr"].append(total / C)
    return out
