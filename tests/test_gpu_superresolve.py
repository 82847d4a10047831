"""Offline super-resolution on the GPU: `sr_emit_window` against its torch
oracle `emit_window_torch` (exact equality of every column, the cursor and
the counts), and `super_resolve_store` on the device against the CPU run.

CPU-vs-GPU bound of the fp32 predictions.  Measured once on an MI355X with
the suite's MIOPEN_FIND_MODE=FAST for the model and recording of
`test_tiny_esrnet_device` (ESRNet basech 8, 3 frames, plus 1.5 x the mid
input frame; 24 x 40 maps, 10 recurrent steps, predictions up to 4.6):
    max |GPU - CPU| over the kept fp32 predictions = 2.384e-07
(two fp32 ulps at the largest prediction, 4.6), and 0.0 between the graphed
and the eager device run.  The test asserts <= 4 x the measured value, the
CPU path being the reference.
"""

import copy

import numpy as np
import pytest
import torch

from esr_amd.engine.superresolve import (cell_counts_torch, emit_window_torch,
                                         super_resolve_store)
from esr_amd.models import build_model

import superresolve_helpers as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRED_DIFF_MEASURED = 2.384e-07


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


class Emitter:
    """Chunk columns, cursor and scratch for maps [2, kH, kW]."""

    def __init__(self, kH, kW, capacity, rows, cursor=0, window_index=0):
        self.ext = _ext()
        self.capacity = capacity
        self.cols = [torch.full((rows,), 0xFFFF, dtype=torch.uint16,
                                device=DEV),
                     torch.full((rows,), 0xFFFF, dtype=torch.uint16,
                                device=DEV),
                     torch.full((rows,), -1.0, dtype=torch.float64,
                                device=DEV),
                     torch.full((rows,), 7, dtype=torch.int8, device=DEV)]
        self.cs = torch.tensor([cursor, -1, -1, -1, window_index],
                               dtype=torch.int64, device=DEV)
        self.win = torch.zeros(2, dtype=torch.float64, device=DEV)
        self.scratch = self.ext.sr_emit_scratch(self.win, 2 * kH * kW,
                                                capacity)

    def emit(self, pred, t0=None, t1=None, cell_cap=1023, mode=0, seed=0):
        if t0 is not None:
            self.win.copy_(torch.tensor([t0, t1], dtype=torch.float64))
        self.ext.sr_emit_window(pred, self.win, self.cols, self.cs,
                                self.capacity, cell_cap, mode, seed,
                                self.scratch)

    def rows(self, a, b):
        return [c[a:b].cpu().numpy() for c in self.cols]

    def untouched(self, a, b):
        xs, ys, ts, ps = self.rows(a, b)
        return bool(np.all(xs == 0xFFFF) and np.all(ys == 0xFFFF)
                    and np.all(ts == -1.0) and np.all(ps == 7))


def _check_against_oracle(pred, t0, t1, *, capacity, cell_cap=1023,
                          mode="linear", seed=0, cursor=0, window_index=0):
    """One window on the device against the oracle: columns, cursor, stats,
    the counts stage, and nothing written outside the window's rows."""
    _, kH, kW = pred.shape
    want = emit_window_torch(pred, t0, t1, capacity=capacity,
                             cell_cap=cell_cap, mode=mode, seed=seed,
                             window_index=window_index)
    n = want["emitted"]
    rows = cursor + capacity + 8
    em = Emitter(kH, kW, capacity, rows, cursor, window_index)
    em.emit(pred.to(DEV).contiguous(), t0, t1, cell_cap,
            {"linear": 0, "random": 1}[mode], seed)
    assert em.cs.tolist() == [cursor + n, want["total"], n, want["dropped"],
                              window_index + 1]
    got = em.rows(cursor, cursor + n)
    for f, g in zip(S.COLS, got):
        assert g.dtype == want[f].dtype, f
        assert g.tobytes() == want[f].tobytes(), \
            f"column {f}: {int((g != want[f]).sum())} of {n} rows differ"
    assert em.untouched(0, cursor) and em.untouched(cursor + n, rows)
    counts = em.scratch[0].view(2, kH, kW).cpu().long()
    assert torch.equal(counts, want["counts"])
    return want, got


def _sparse(seed, shape, high):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, high + 1, shape, generator=g).float()
    return v * (torch.rand(shape, generator=g) < 0.3)


# ---------------------------------------------------------------------------
# sr_emit_window against emit_window_torch

@pytest.mark.parametrize("mode", ["linear", "random"])
def test_hand_map(mode):
    want, _ = _check_against_oracle(S.HAND, 5.0, 5.25, capacity=100,
                                    cell_cap=S.HAND_CAP, mode=mode, seed=11,
                                    window_index=3)
    assert want["total"] == 14
    if mode == "linear":
        got = list(zip(want["xs"].tolist(), want["ys"].tolist(),
                       want["ps"].tolist(), want["q"].tolist()))
        assert got == S.HAND_ROWS


@pytest.mark.parametrize("mode", ["linear", "random"])
def test_sparse_random_map(mode):
    pred = _sparse(1, (2, 32, 48), 5)
    want, _ = _check_against_oracle(pred, 2.0, 3.0, capacity=8192, mode=mode,
                                    seed=5, window_index=17)
    assert want["total"] > 1000 and want["dropped"] == 0


def test_half_integers():
    g = torch.Generator().manual_seed(2)
    pred = torch.randint(-3, 12, (2, 17, 23), generator=g).float() / 2
    want, _ = _check_against_oracle(pred, 0.0, 1.0, capacity=4096)
    # halves go to even
    assert torch.equal(want["counts"][pred == 2.5],
                       torch.full_like(want["counts"][pred == 2.5], 2))
    assert torch.equal(want["counts"][pred == 3.5],
                       torch.full_like(want["counts"][pred == 3.5], 4))


def test_one_cell_at_cell_cap():
    pred = torch.zeros(2, 5, 7)
    pred[1, 3, 4] = 5000.0
    pred[0, 0, 0] = 1.0
    want, got = _check_against_oracle(pred, 0.0, 1.0, capacity=2048)
    assert want["total"] == 1024 and int(want["counts"][1, 3, 4]) == 1023
    assert np.all(np.diff(got[2]) >= 0)


def test_all_zero_map_writes_nothing():
    want, _ = _check_against_oracle(torch.zeros(2, 6, 9), 1.0, 2.0,
                                    capacity=64, cursor=5)
    assert (want["total"], want["emitted"]) == (0, 0)


def test_capacity_total_minus_three():
    pred = _sparse(3, (2, 32, 48), 5)
    total = int(cell_counts_torch(pred).sum())
    want, _ = _check_against_oracle(pred, 0.0, 1.0, capacity=total - 3)
    assert (want["emitted"], want["dropped"]) == (total - 3, 3)
    assert want["emitted"] + want["dropped"] == want["total"] == total


def test_non_zero_starting_cursor():
    _check_against_oracle(_sparse(4, (2, 32, 48), 5), 0.0, 1.0,
                          capacity=4096, cursor=777)


def test_two_windows_back_to_back():
    a, b = _sparse(5, (2, 32, 48), 5), _sparse(6, (2, 32, 48), 5)
    cap = 2000        # below b's total or not, the oracle decides
    em = Emitter(32, 48, cap, 2 * cap + 8, cursor=3, window_index=40)
    wa = emit_window_torch(a, 10.0, 10.5, capacity=cap, mode="random",
                           seed=8, window_index=40)
    wb = emit_window_torch(b, 10.5, 10.5, capacity=cap, mode="random",
                           seed=8, window_index=41)
    em.emit(a.to(DEV), 10.0, 10.5, mode=1, seed=8)
    assert em.cs.tolist() == [3 + wa["emitted"], wa["total"], wa["emitted"],
                              wa["dropped"], 41]
    em.emit(b.to(DEV), 10.5, 10.5, mode=1, seed=8)
    n = wa["emitted"] + wb["emitted"]
    assert em.cs.tolist() == [3 + n, wb["total"], wb["emitted"],
                              wb["dropped"], 42]
    for f, g in zip(S.COLS, em.rows(3, 3 + n)):
        assert g.tobytes() == np.concatenate([wa[f], wb[f]]).tobytes(), f
    assert em.untouched(0, 3) and em.untouched(3 + n, 2 * cap + 8)


def test_wide_map_needs_15_bit_coordinates():
    pred = torch.zeros(2, 1, 5000)
    pred[0, 0, 4999] = 2.0
    pred[1, 0, 4096] = 1.0
    pred[0, 0, 903] = 1.0            # 4999 - 4096: where 12 bits would land
    want, got = _check_against_oracle(pred, 0.0, 1.0, capacity=16)
    assert sorted(got[0].tolist()) == [903, 4096, 4999, 4999]


def test_map_past_one_grid():
    """Cells AND events a little past one full grid of the capped kernels:
    the counts, emit and append loops all take a second iteration."""
    cap = int(_ext().grid_cap())
    kW = 512
    kH = cap // (2 * kW) + 3
    ncells = 2 * kH * kW
    print(f"sr_emit cells: {ncells}, cap {cap}")
    assert cap < ncells < 1.1 * cap
    g = torch.Generator().manual_seed(7)
    pred = torch.randint(0, 4, (2, kH, kW), generator=g).float()
    total = int(pred.sum())
    assert total > cap
    _check_against_oracle(pred, 100.0, 101.0, capacity=total + 100)


# ---------------------------------------------------------------------------
# timestamps

def test_timestamps_epoch_bit_equal_to_numpy():
    t0, t1 = 1.7e9, 1.7e9 + 1e-3
    pred = _sparse(9, (2, 32, 48), 40)
    want, got = _check_against_oracle(pred, t0, t1, capacity=40000)
    xs, ys, ts, ps = got
    assert ts.tobytes() == S.timestamps(t0, t1, want["q"]).tobytes()
    assert np.all((ts >= t0) & (ts <= t1)) and np.all(np.diff(ts) >= 0)
    # strictly increasing within a cell (file order is phase order)
    cell = (ps.astype(np.int64) < 0) * (32 * 48) + ys.astype(np.int64) * 48 \
        + xs
    order = np.argsort(cell, kind="stable")
    same = np.diff(cell[order]) == 0
    assert same.sum() > 1000
    assert np.all(np.diff(ts[order])[same] > 0)


def test_degenerate_window_all_on_t0():
    t0 = 1.7e9 + 0.123
    _, got = _check_against_oracle(_sparse(10, (2, 32, 48), 5), t0, t0,
                                   capacity=8192)
    assert got[2].size > 0 and np.all(got[2] == t0)


# ---------------------------------------------------------------------------
# non-finite and huge predictions
#
# The clamp, as sr_counts_kernel reads (ops/native/src/sr_emit.hip,
# sr_cell_count): NaN returns 0 before anything else; r = rintf(v) is
# compared AS A FLOAT, !(r > 0) -> 0 and r >= cell_cap -> cell_cap, and only a
# value strictly between is converted to int.  Every later kernel reads
# these int32 counts, never the prediction, and bounds its stores on
# capacity and rows.  The oracle's form of the same rule is
# tests/test_superresolve.py::test_cell_counts_rounding_and_non_finite.

def test_non_finite_and_huge_inputs():
    vals = [S.NAN, S.INF, -S.INF, 1e30, -1e30]
    v = torch.tensor(vals + [0.0] * 7).view(2, 2, 3)
    ext = _ext()
    for cell_cap in (1023, 9):
        counts = ext.sr_emit_counts(v.to(DEV), cell_cap).cpu()
        assert counts.dtype == torch.int32
        assert counts.view(-1)[:5].tolist() == [0, cell_cap, 0, cell_cap, 0]
        assert torch.equal(counts.long(), cell_counts_torch(v, cell_cap))
    want, _ = _check_against_oracle(v, 0.0, 1.0, capacity=4096)
    assert want["total"] == 2 * 1023
    # and with the capacity far below what the map asks for
    pred = torch.full((2, 8, 8), S.INF)
    pred[0, 0, :4] = torch.tensor([S.NAN, -S.INF, 1e30, -1e30])
    want, _ = _check_against_oracle(pred, 0.0, 1.0, capacity=300, cursor=2)
    assert want["dropped"] == want["total"] - 300 > 100000


# ---------------------------------------------------------------------------
# capture

def test_capture_replays_equal_eager_calls():
    preds = [_sparse(20, (2, 32, 48), 5), _sparse(21, (2, 32, 48), 5)]
    wins = [(50.0, 50.25), (50.25, 51.0)]
    cap = 4096
    eager = Emitter(32, 48, cap, 3 * cap, window_index=6)
    for p, (t0, t1) in zip(preds, wins):
        eager.emit(p.to(DEV), t0, t1, mode=1, seed=2)

    em = Emitter(32, 48, cap, 3 * cap, window_index=6)
    static = torch.zeros(2, 32, 48, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        em.emit(static, mode=1, seed=2)                 # warm-up, empty map
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        em.emit(static, mode=1, seed=2)
    em.cs.copy_(torch.tensor([0, -1, -1, -1, 6]))
    for p, (t0, t1) in zip(preds, wins):
        static.copy_(p)
        em.win.copy_(torch.tensor([t0, t1], dtype=torch.float64))
        graph.replay()
    torch.cuda.synchronize()
    assert em.cs.tolist() == eager.cs.tolist()
    n = int(em.cs[0])
    assert n > 1000
    for f, a, b in zip(S.COLS, em.rows(0, 3 * cap), eager.rows(0, 3 * cap)):
        assert a.tobytes() == b.tobytes(), f


# ---------------------------------------------------------------------------
# super_resolve_store on the device

@pytest.fixture(scope="module")
def lr_store(tmp_path_factory):
    return S.write_lr_store(tmp_path_factory.mktemp("sr_gpu") / "lr.evs")


def _run(model, src, dst, **kw):
    args = dict(group="down2", scale=S.SCALE, seqn=3, window=S.WINDOW,
                device=DEV, keep=True)
    args.update(kw)
    return super_resolve_store(model, src, str(dst), **args)


@pytest.mark.parametrize("redistribute", ["linear", "random"])
def test_identity_device_file_equals_cpu_file(lr_store, tmp_path,
                                              redistribute):
    kw = dict(redistribute=redistribute, seed=4)
    cpu, kc = _run(S.MidFrame(), lr_store, tmp_path / "cpu.evs", device="cpu",
                   **kw)
    gpu, kg = _run(S.MidFrame(), lr_store, tmp_path / "gpu.evs", **kw)
    S.assert_same_files(tmp_path / "cpu.evs", tmp_path / "gpu.evs", "ori")
    assert torch.equal(kg["pred"].cpu(), kc["pred"])
    assert torch.equal(kg["counts"].cpu(), kc["counts"])
    assert torch.equal(kg["stats"], kc["stats"])
    drop = ("seconds",)
    assert {k: v for k, v in gpu.items() if k not in drop} == \
        {k: v for k, v in cpu.items() if k not in drop}
    assert gpu["events_out"] == (S.N_WINDOWS - 2) * S.WINDOW


@pytest.fixture(scope="module")
def lifted():
    torch.manual_seed(0)
    return S.Lifted(build_model("ESRNet", inch=2, basech=8, num_frame=3)
                    .eval())


@pytest.fixture(scope="module")
def device_runs(lr_store, lifted, tmp_path_factory):
    """The graphed, the eager and the CPU run of the tiny model, once."""
    root = tmp_path_factory.mktemp("sr_runs")
    out = {}
    for name, kw in (("graph", dict(use_graphs=True)),
                     ("eager", dict(use_graphs=False)),
                     ("cpu", dict(device="cpu"))):
        model = copy.deepcopy(lifted).to(kw.get("device", DEV))
        out[name] = (root / f"{name}.evs",
                     *_run(model, lr_store, root / f"{name}.evs", **kw))
    return out


def test_tiny_esrnet_graphs_equal_eager(device_runs):
    (pg, sg, kg), (pe, se, ke) = device_runs["graph"], device_runs["eager"]
    diff = (kg["pred"] - ke["pred"]).abs().max().item()
    print(f"graph vs eager: max |diff| of the kept predictions {diff}")
    assert torch.equal(kg["counts"], ke["counts"])
    assert torch.equal(kg["stats"], ke["stats"])
    S.assert_same_files(pg, pe, "ori")
    assert sg["events_out"] == se["events_out"] > 0


def test_tiny_esrnet_windows_splat_back(device_runs):
    path, summary, kept = device_runs["graph"]
    cols, n = S.read_group(path, "ori")
    ranges = S.window_row_ranges(kept["stats"])
    assert ranges[-1][1] == n == summary["events_out"]
    assert np.all(np.diff(cols["ts"]) >= 0)
    for (a, b), counts in zip(ranges, kept["counts"].cpu()):
        got = S.splat_rows(cols["xs"][a:b], cols["ys"][a:b], cols["ps"][a:b],
                           S.HR)
        assert torch.equal(got, counts)
    assert torch.equal(kept["counts"].cpu(),
                       cell_counts_torch(kept["pred"].cpu()))


def test_tiny_esrnet_device_against_cpu(device_runs):
    _, _, kg = device_runs["graph"]
    _, _, kc = device_runs["cpu"]
    assert kg["pred"].shape == kc["pred"].shape == (S.N_WINDOWS - 2, 2, *S.HR)
    diff = (kg["pred"].cpu() - kc["pred"]).abs().max().item()
    print(f"device vs CPU: max |diff| of the kept fp32 predictions {diff:.3e}"
          f" (max |pred| {kc['pred'].abs().max().item():.3f})")
    assert diff <= 4 * PRED_DIFF_MEASURED


def test_chunking_on_device(lr_store, lifted, tmp_path, device_runs):
    model = copy.deepcopy(lifted).to(DEV)
    summary, kept = _run(model, lr_store, tmp_path / "c2.evs",
                         chunk_windows=2)
    S.assert_same_files(tmp_path / "c2.evs", device_runs["graph"][0], "ori")
    assert torch.equal(kept["stats"], device_runs["graph"][2]["stats"])
