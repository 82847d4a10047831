"""eval_metrics.hip against `metric_sums_torch` (run on CPU copies) within
tests/eval_bounds.py, and `infer_sequence_device` on the GPU against itself
on the CPU, against its own eager run and against the oracle on its own maps.

GRAPH_TOL: use_graphs=True against use_graphs=False, fp32, on the MI355X.
Measured: 0.0 on every result key except `time`, and torch.equal prediction
maps, bicubic maps and sum tables (the replay launches the kernels the eager
run launches, in the same order, and the metrics kernel is deterministic).
4 x 0.0 = 0.0: the comparison is exact.
"""

import pytest
import torch

from esr_amd.engine.capture import capture_graph
from esr_amd.engine.device_inference import infer_sequence_device
from esr_amd.engine.inference import build_metrics
from esr_amd.loss.device_metrics import finalize, metric_sums, \
    metric_sums_torch
from esr_amd.ops.native import get_ext

import device_eval_helpers as T
import eval_bounds as EB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAPH_TOL = 4 * 0.0


def _tile():
    th, tw = get_ext().restoration_metrics_tile()
    return int(th), int(tw)


def _sizes():
    ext = get_ext()
    if ext is None or not hasattr(ext, "restoration_metrics_tile"):
        return [(7, 7)]               # the tests then fail on the missing op
    th, tw = _tile()
    return [(7, 7), (8, 9), (40, 86), (th, tw), (th + 1, tw + 1),
            (th + 6, tw + 6), (2 * th + 7, 2 * tw + 5)]


def test_extension_has_the_kernel():
    ext = get_ext()
    assert ext is not None and hasattr(ext, "restoration_metrics")
    th, tw = _tile()
    assert th >= 7 and tw >= 7


@pytest.fixture(scope="module")
def oracle():
    """(pred, tgt, float64 sums) per size, P = 6 distinct planes, computed
    once on the CPU and shared."""
    out = {}
    for k, (h, w) in enumerate(_sizes()):
        pred, tgt = T.make_pair((6, h, w), seed=900 + k)
        out[(h, w)] = (pred, tgt, metric_sums_torch(pred, tgt))
    return out


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_oracle(oracle, size):
    pred, tgt, ref = oracle[size]
    a = metric_sums(pred.to(DEV), tgt.to(DEV))
    b = metric_sums(pred.to(DEV), tgt.to(DEV))
    assert a.dtype == torch.float64 and a.shape == (6, 5) and a.is_cuda
    assert torch.equal(a, b), "two launches differ"
    assert torch.equal(a[:, 2].cpu(), tgt.amax((1, 2)).double())
    assert torch.equal(a[:, 3].cpu(), tgt.amin((1, 2)).double())
    EB.assert_sums_within(a, ref, pred, tgt, f"kernel {size}")
    # a plane mix-up would pass a per-plane bound only on equal planes
    assert len({round(v, 6) for v in ref[:, 4].tolist()}) == 6


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_maps_are_exact_on_the_device(oracle, size):
    _, tgt, _ = oracle[size]
    t = tgt.to(DEV)
    sums = metric_sums(t.clone(), t).cpu()
    h, w = size
    zero = torch.zeros(6, dtype=torch.float64)
    assert torch.equal(sums[:, 0], zero) and torch.equal(sums[:, 1], zero)
    assert sums[:, 4].tolist() == [float((h - 6) * (w - 6))] * 6
    fin = finalize(sums, 2, h, w)
    assert fin["psnr"] == [float("inf")] * 3 and fin["ssim"] == [1.0] * 3


def test_zero_range_and_small_maps_on_the_device():
    tgt = torch.full((2, 9, 11), 3.0, device=DEV)
    fin = finalize(metric_sums(tgt + 0.5, tgt), 2, 9, 11)
    assert fin["psnr"][0] == pytest.approx(10.0 * 0.6020599913279624,
                                           abs=1e-12)
    with pytest.raises(ValueError, match="H, W >= 7"):
        metric_sums(torch.zeros(2, 6, 40, device=DEV),
                    torch.zeros(2, 6, 40, device=DEV))
    with pytest.raises(RuntimeError, match="H, W >= 7"):
        get_ext().restoration_metrics(torch.zeros(2, 40, 6, device=DEV),
                                      torch.zeros(2, 40, 6, device=DEV), 2.0)


def test_kernel_replays_from_a_captured_graph(oracle):
    th, tw = _tile()
    size = (th + 6, tw + 6)
    sp = torch.zeros(6, *size, device=DEV)
    st = torch.zeros(6, *size, device=DEV)
    graph, out = capture_graph(lambda: metric_sums(sp, st), warmup=1,
                               device=torch.device(DEV))
    pred, tgt, ref = oracle[size]
    pred2, tgt2 = T.make_pair((6, *size), seed=77)
    for p, t, r in ((pred, tgt, ref),
                    (pred2, tgt2, metric_sums_torch(pred2, tgt2))):
        sp.copy_(p)
        st.copy_(t)
        graph.replay()
        EB.assert_sums_within(out.clone(), r, p, t, f"replay {size}")


# ---- the evaluator on cuda:0 ---------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    datalist = T.H.make_datalist(tmp_path_factory.mktemp("evs_eval_gpu"))
    path = datalist.read_text().split()[0]
    cfg = T.eval_config(datalist)
    out = {}
    _, out["cpu"] = infer_sequence_device(
        cfg, path, T.seeded_model(), "cpu", metrics=build_metrics("cpu"),
        save_images=False, return_maps=True)
    metrics = build_metrics(DEV)
    for name, kw in (("graph", {"use_graphs": True}),
                     ("eager", {"use_graphs": False})):
        out[name] = infer_sequence_device(
            cfg, path, T.seeded_model(DEV), DEV, metrics=metrics,
            save_images=False, return_maps=True, **kw)
    out["args"] = (cfg, path, metrics)
    return out


def test_device_splats_equal_the_cpu_evaluators(runs):
    for name in ("graph", "eager"):
        maps = runs[name][1]
        for key in ("inp", "gt", "lr"):
            assert torch.equal(maps[key].cpu(), runs["cpu"][key]), (name, key)
    assert runs["cpu"]["inp"].size(0) == 5


def test_graph_replay_equals_eager(runs):
    (res_g, maps_g), (res_e, maps_e) = runs["graph"], runs["eager"]
    assert set(res_g) == set(res_e)
    for key, value in res_e.items():
        if key == "time" or isinstance(value, str):
            continue
        diff = 0.0 if res_g[key] == value else abs(res_g[key] - value)
        print(f"graph vs eager {key}: |diff| {diff:.3e}")
        assert diff <= GRAPH_TOL, (key, res_g[key], value)
    for key in ("esr", "bicubic"):
        diff = (maps_g[key] - maps_e[key]).abs().max().item()
        print(f"graph vs eager {key} maps: max |diff| {diff:.3e}")
        assert diff <= GRAPH_TOL, key
    assert res_g["time"] > 0 and res_e["time"] > 0


def _self_consistent(result, maps, what):
    """The table equals the oracle on the run's own maps, and the result
    dict is finalize() of the table."""
    n, _, h, w = maps["gt"].shape
    pred = torch.stack([maps["esr"], maps["bicubic"]], 1).cpu() \
        .reshape(n * 4, h, w).contiguous()
    tgt = torch.stack([maps["gt"], maps["gt"]], 1).cpu() \
        .reshape(n * 4, h, w).contiguous()
    got = maps["table"][:, :20].reshape(n * 4, 5)
    EB.assert_sums_within(got.contiguous(), metric_sums_torch(pred, tgt),
                          pred, tgt, what)
    fin = finalize(got, 2, h, w)
    for j, name in enumerate(("esr", "bicubic")):
        for key in ("l1", "mse", "rmse", "ssim", "psnr"):
            assert result[f"{name}_{key}"] == sum(fin[key][j::2]) / n
    assert bool((maps["esr"] != 0).any())


def test_tables_match_the_oracle_on_their_own_maps(runs):
    for name in ("graph", "eager"):
        _self_consistent(*runs[name], what=f"{name} table")


def test_bf16_run_is_self_consistent_and_native(runs):
    from esr_amd.ops import conv
    cfg, path, metrics = runs["args"]
    before = conv.stats["native_calls"]
    result, maps = infer_sequence_device(
        cfg, path, T.seeded_model(DEV), DEV, metrics=metrics,
        save_images=False, return_maps=True, amp_dtype=torch.bfloat16)
    assert conv.stats["native_calls"] > before
    _self_consistent(result, maps, "bf16 table")
    for key in ("inp", "gt", "lr"):
        assert torch.equal(maps[key].cpu(), runs["cpu"][key])
