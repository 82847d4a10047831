"""CPU-side tests for the fp16 half of the native-conv dispatch layer:
the pure dtype-decision function, dtype-agnostic weight packing, the
optional dtype argument of shape_supported and the fused-gate dtype set."""

import inspect

import torch
import torch.nn as nn

from esr_amd.ops import conv as conv_mod
from esr_amd.ops.conv import _pack, compute_dtype, shape_supported
from esr_amd.ops.convgru import _FUSED_DTYPES


def test_compute_dtype_fp16_autocast(monkeypatch):
    monkeypatch.setenv("ESR_NATIVE_FP16", "1")
    assert compute_dtype(True, torch.float16, torch.float32) == torch.float16
    # the autocast dtype decides, whatever the tensor arrives as
    assert compute_dtype(True, torch.float16, torch.float16) == torch.float16
    assert compute_dtype(True, torch.float16, torch.bfloat16) == torch.float16


def test_compute_dtype_bf16_autocast(monkeypatch):
    for v in ("0", "1"):
        monkeypatch.setenv("ESR_NATIVE_FP16", v)
        assert compute_dtype(True, torch.bfloat16, torch.float32) \
            == torch.bfloat16
        assert compute_dtype(False, None, torch.bfloat16) == torch.bfloat16


def test_compute_dtype_fp32_without_autocast(monkeypatch):
    for v in ("0", "1"):
        monkeypatch.setenv("ESR_NATIVE_FP16", v)
        assert compute_dtype(False, None, torch.float32) is None
        assert compute_dtype(False, torch.float16, torch.float32) is None


def test_compute_dtype_plain_fp16_tensor(monkeypatch):
    monkeypatch.setenv("ESR_NATIVE_FP16", "1")
    assert compute_dtype(False, None, torch.float16) == torch.float16


def test_compute_dtype_fp16_switched_off(monkeypatch):
    monkeypatch.setenv("ESR_NATIVE_FP16", "0")
    assert compute_dtype(True, torch.float16, torch.float32) is None
    assert compute_dtype(False, None, torch.float16) is None
    # the explicit argument wins over the environment
    assert compute_dtype(True, torch.float16, torch.float32,
                         fp16_enabled=True) == torch.float16


def test_fp16_default_is_a_switch_value(monkeypatch):
    monkeypatch.delenv("ESR_NATIVE_FP16", raising=False)
    assert conv_mod._FP16_DEFAULT in ("0", "1")
    assert conv_mod.native_fp16_enabled() == (conv_mod._FP16_DEFAULT == "1")


def test_pack_fp16_keeps_dtype_and_padded_shape():
    g = torch.Generator().manual_seed(0)
    O, I, k = 33, 40, 3
    w = torch.randn(O, I, k, k, generator=g)
    p16 = _pack(w.to(torch.float16))
    pbf = _pack(w.to(torch.bfloat16))
    assert p16.dtype == torch.float16
    assert p16.shape == pbf.shape == (9, 48, 64)
    assert p16.is_contiguous()
    for tap in (0, 4, 8):
        ky, kx = tap // 3, tap % 3
        assert torch.equal(p16[tap, :O, :I], w.to(torch.float16)[:, :, ky, kx])
    assert not p16[:, O:, :].any() and not p16[:, :, I:].any()


def test_shape_supported_dtype_argument_is_optional():
    assert "dtype" in inspect.signature(shape_supported).parameters

    def conv(cin, cout, k, s):
        return nn.Conv2d(cin, cout, k, s, k // 2)

    table = [(conv(2, 8, 3, 1), True), (conv(8, 16, 3, 2), False),
             (conv(16, 32, 3, 2), True), (conv(192, 192, 3, 1), True),
             (conv(128, 64, 1, 1), True), (conv(64, 1, 3, 1), True),
             (conv(8, 2, 3, 1), True), (conv(64, 64, 5, 1), False)]
    for c, want in table:
        # left out == None == bf16: today's table
        assert shape_supported(c) is want
        assert shape_supported(c, None) is want
        assert shape_supported(c, torch.bfloat16) is want
        # fp16 may only route MORE shapes back to MIOpen, never fewer
        if not want:
            assert shape_supported(c, torch.float16) is False


def test_shape_dispatch_table_fp16():
    """fp16-only routing measured against MIOpen fp16
    (profiles/README.md, "fp16"); bf16 keeps these shapes native."""
    def conv(cin, cout, k, s):
        return nn.Conv2d(cin, cout, k, s, k // 2)

    f16 = torch.float16
    assert shape_supported(conv(2, 8, 3, 1), f16)         # head (valu2)
    assert shape_supported(conv(16, 32, 3, 2), f16)       # enc2 (MFMA)
    assert shape_supported(conv(128, 64, 3, 1), f16)      # fusion (MFMA)
    assert shape_supported(conv(128, 64, 1, 1), f16)      # 1x1 fusion
    assert shape_supported(conv(32, 128, 3, 2), f16)      # wide but stride 2
    assert shape_supported(conv(64, 128, 1, 1), f16)      # wide but 1x1
    # back to MIOpen for fp16 only
    for c in (conv(64, 1, 3, 1), conv(64, 2, 1, 1),        # v1 VALU class
              conv(128, 128, 3, 1), conv(192, 192, 3, 1),  # wide 3x3 s1
              conv(64, 128, 3, 1)):
        assert shape_supported(c, f16) is False
        assert shape_supported(c) is True


def test_stats_has_fp16_counter():
    assert conv_mod.stats["native_calls_fp16"] >= 0
    assert "native_calls" in conv_mod.stats


def test_fused_gate_dtypes_include_fp16():
    assert torch.float16 in _FUSED_DTYPES
    assert torch.float32 in _FUSED_DTYPES and torch.bfloat16 in _FUSED_DTYPES
