"""Shared inputs of the device-evaluation tests (tests/test_device_eval.py,
tests/test_gpu_device_eval.py): the map pairs, the evaluator's config on the
device-loader fixture and the seeded model."""

import torch

from esr_amd.models import build_model

import device_loader_helpers as H


def make_pair(shape, seed, rate=3.0):
    """Poisson-count target, prediction = target + noise (negatives
    included), fp32 [C, H, W]."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.poisson(torch.full(shape, rate), generator=g)
    pred = tgt + 0.7 * torch.randn(shape, generator=g)
    return pred, tgt


def eval_config(datalist, **dataset_overrides):
    cfg = H.dl_config(datalist, data_augment={"enabled": False,
                                              "augment": [],
                                              "augment_prob": []},
                      **dataset_overrides)
    cfg.update(batch_size=1, drop_last=False)
    return cfg


def seeded_model(device="cpu"):
    torch.manual_seed(0)
    return build_model("ESRNet", inch=2, basech=8, num_frame=3,
                       upsampler="pixelshuffle").to(device).eval()
