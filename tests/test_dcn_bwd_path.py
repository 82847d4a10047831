"""Path choice of the DCN backward (esr_amd/ops/dcn.py): a pure function of
(C, dg, H, W) plus the selector and ESR_DCN_BWD.  No GPU needed."""

import pytest

from esr_amd.ops.dcn import (BWD_FUSED_LDS_MAX, dcn_bwd_fused_applicable,
                             dcn_bwd_path, save_cols_enabled)


def test_applicability_rule():
    assert BWD_FUSED_LDS_MAX == 64 * 1024
    assert dcn_bwd_fused_applicable(64, 8, 32, 32)       # flagship: 32 KiB
    assert dcn_bwd_fused_applicable(8, 1, 32, 64)        # exactly 64 KiB
    assert not dcn_bwd_fused_applicable(8, 1, 48, 48)    # 73,728 B
    assert not dcn_bwd_fused_applicable(8, 1, 32, 65)    # one column over
    assert dcn_bwd_fused_applicable(16, 4, 14, 18)
    assert not dcn_bwd_fused_applicable(10, 4, 8, 8)     # C % dg != 0
    # more groups make smaller planes
    assert not dcn_bwd_fused_applicable(64, 1, 32, 32)
    assert dcn_bwd_fused_applicable(64, 4, 32, 32)


def test_path_selector(monkeypatch):
    monkeypatch.delenv("ESR_DCN_BWD", raising=False)
    assert dcn_bwd_path(64, 8, 32, 32) == "fused"
    assert dcn_bwd_path(64, 8, 32, 32, "split") == "split"
    assert dcn_bwd_path(8, 1, 48, 48) == "split"
    assert dcn_bwd_path(8, 1, 48, 48, "auto") == "split"
    with pytest.raises(ValueError, match="fused backward needs"):
        dcn_bwd_path(8, 1, 48, 48, "fused")
    with pytest.raises(ValueError, match="auto, fused or split"):
        dcn_bwd_path(64, 8, 32, 32, "tiled")


def test_path_env(monkeypatch):
    monkeypatch.setenv("ESR_DCN_BWD", "split")
    assert dcn_bwd_path(64, 8, 32, 32) == "split"
    # an explicit selector wins over the environment
    assert dcn_bwd_path(64, 8, 32, 32, "fused") == "fused"
    monkeypatch.setenv("ESR_DCN_BWD", "fused")
    assert dcn_bwd_path(64, 8, 32, 32) == "fused"
    with pytest.raises(ValueError, match="fused backward needs"):
        dcn_bwd_path(8, 1, 48, 48)
    monkeypatch.setenv("ESR_DCN_BWD", "nope")
    with pytest.raises(ValueError, match="ESR_DCN_BWD"):
        dcn_bwd_path(64, 8, 32, 32)


def test_save_cols_switch(monkeypatch):
    monkeypatch.delenv("ESR_DCN_SAVE_COLS", raising=False)
    assert save_cols_enabled()
    monkeypatch.setenv("ESR_DCN_SAVE_COLS", "0")
    assert not save_cols_enabled()
    monkeypatch.setenv("ESR_DCN_SAVE_COLS", "1")
    assert save_cols_enabled()
