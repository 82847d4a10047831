"""CPU tests of the pure routing predicates of esr_amd/ops/conv.py."""

from esr_amd.ops import conv as C


def test_aten_and_native_route_everything_one_way():
    for ks, stride, cin, cout in [(3, 1, 64, 64), (3, 2, 8, 16), (1, 1, 128, 64),
                                  (3, 1, 2, 8)]:
        assert C.bwd_route("aten", True, ks, stride, cin, cout) == \
            (False, False)
        assert C.bwd_route("native", True, ks, stride, cin, cout) == \
            (True, True)


def test_dgrad_arm_routes_only_the_input_grad():
    assert C.bwd_route("dgrad", True, 3, 1, 192, 192) == (True, False)
    assert C.bwd_route("dgrad", True, 1, 1, 128, 64) == (True, False)


def test_fp16_backward_always_aten():
    for mode in ("aten", "native", "auto", "dgrad"):
        assert C.bwd_route(mode, False, 3, 1, 64, 64) == (False, False)
    for mode in ("mfma", "core", "auto"):
        assert not C.fwd_core_route(mode, False, 3, 1, 64, 64)


def test_auto_touches_the_deep_stride1_class_only():
    outside = [(3, 2, 32, 64), (3, 1, 16, 32), (3, 1, 64, 1), (3, 1, 2, 8),
               (5, 1, 64, 64)]
    for ks, stride, cin, cout in outside:
        assert C.bwd_route("auto", True, ks, stride, cin, cout) == \
            (False, False)
        assert not C.fwd_core_route("auto", True, ks, stride, cin, cout)
        assert not C.fwd_core_route("core", True, ks, stride, cin, cout)
    for ks, cin, cout in [(3, 128, 64), (1, 128, 64), (3, 32, 64),
                          (3, 64, 216), (3, 192, 192)]:
        for mode in ("core", "auto"):
            assert C.fwd_core_route(mode, True, ks, 1, cin, cout)
        assert not C.fwd_core_route("mfma", True, ks, 1, cin, cout)


def test_auto_table():
    # 3x3: input grad native; weight grad native from Cin 192
    assert C.bwd_route("auto", True, 3, 1, 128, 64) == (True, False)
    assert C.bwd_route("auto", True, 3, 1, 32, 64) == (True, False)
    assert C.bwd_route("auto", True, 3, 1, 64, 216) == (True, False)
    assert C.bwd_route("auto", True, 3, 1, 192, 192) == (True, True)
    assert C.bwd_route("auto", True, 3, 1, 192, 64) == (True, True)
    # 1x1: aten keeps both
    assert C.bwd_route("auto", True, 1, 1, 128, 64) == (False, False)
    # an unknown value is the default routing, not a silent aten
    assert C.bwd_route("", True, 3, 1, 128, 64) == (True, False)


def test_default_is_auto():
    assert C._CONV_BWD_DEFAULT == "auto"
    assert C._CONV_FWD_DEFAULT == "auto"
