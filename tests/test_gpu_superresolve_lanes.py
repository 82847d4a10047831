"""Several recordings at once on the GPU: `sr_emit_lanes` against its torch
oracle `emit_window_torch` lane by lane (exact equality of every column, the
cursors, the counts and the window indices), and `super_resolve_stores` on
the device against the device single path and the CPU lanes run.

Batch-3 vs batch-1 bound of the fp32 predictions.  Measured once on an
MI355X with the suite's MIOPEN_FIND_MODE=FAST for the model of
`test_tiny_esrnet_lanes_against_single_path` (ESRNet basech 8, 3 frames, plus
1.5 x the mid input frame; 24 x 40 maps, five recordings of 10, 3, 7, 1 and 5
recurrent steps in three lanes), against `super_resolve_store` on the device:
    max |lanes - single| over the kept fp32 predictions = 0.0
(and 0.0 between the graphed and the eager lanes run)
The test asserts <= 4 x the measured value, `super_resolve_store` being the
reference.  tests/test_gpu_multistream.py measured 0.0 for batch 3 against
batch 1 of this model as well.  With 0.0 the assertion is equality, and the
files must then be byte-equal too.  That is stricter than the semantics need:
it holds only while MIOpen picks solvers that give bit-identical fp32 results
at batch 1 and batch 3.  If `test_tiny_esrnet_lanes_against_single_path`
alone fails after a ROCm, MIOpen or find-db update while
`test_tiny_esrnet_lanes_graphs_equal_eager` and
`test_tiny_esrnet_kept_predictions_reproduce_the_files` still pass,
re-measure the line above before suspecting the scheduler.
"""

import copy

import numpy as np
import pytest
import torch

from esr_amd.engine.superresolve import (cell_counts_torch, emit_window_torch,
                                         super_resolve_store,
                                         super_resolve_stores)
from esr_amd.models import build_model

import superresolve_helpers as S
import superresolve_lanes_helpers as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRED_DIFF_MEASURED = 0.0
MODES = {"linear": 0, "random": 1}
SENTINEL = (0xFFFF, 0xFFFF, -1.0, 7)
DTYPES = (torch.uint16, torch.uint16, torch.float64, torch.int8)


def _ext():
    from esr_amd.ops.native import require_ext
    return require_ext()


class LaneEmitter:
    """Sentinel-filled chunk columns [S, rows], cursors, clocks, control and
    scratch for S maps [2, kH, kW]."""

    def __init__(self, S_, kH, kW, capacity_max, rows, cursors, windows):
        self.ext = _ext()
        self.S, self.capacity_max, self.n_rows = S_, capacity_max, rows
        self.cols = [torch.full((S_, rows), v, dtype=dt, device=DEV)
                     for v, dt in zip(SENTINEL, DTYPES)]
        self.cs0 = [[c, -1, -1, -1, w] for c, w in zip(cursors, windows)]
        self.cs = torch.tensor(self.cs0, dtype=torch.int64, device=DEV)
        self.win = torch.zeros(S_, 2, dtype=torch.float64, device=DEV)
        self.ctl = torch.zeros(S_, 2, dtype=torch.int64, device=DEV)
        self.scratch = self.ext.sr_emit_lanes_scratch(
            self.win, S_, 2 * kH * kW, capacity_max)

    def set(self, wins, active, caps):
        self.win.copy_(torch.tensor(wins, dtype=torch.float64))
        self.ctl.copy_(torch.tensor(list(zip(active, caps)),
                                    dtype=torch.int64))

    def emit(self, pred, cell_cap=1023, mode=0, seed=0):
        self.ext.sr_emit_lanes(pred, self.win, self.cols, self.cs, self.ctl,
                               self.capacity_max, cell_cap, mode, seed,
                               self.scratch)

    def rows(self, s, a, b):
        return [c[s, a:b].cpu().numpy() for c in self.cols]

    def untouched(self, s, a, b):
        return all(bool(np.all(col == v))
                   for col, v in zip(self.rows(s, a, b), SENTINEL))


def _check_lanes(preds, wins, caps, active, *, cursors=None, windows=None,
                 capacity_max=None, cell_cap=1023, mode="linear", seed=0):
    """One call on the device against the oracle, lane by lane: columns,
    cursor, counts, window index, the counts stage, nothing written outside
    a lane's rows and nothing at all in an inactive lane."""
    S_, _, kH, kW = preds.shape
    cursors = cursors or [0] * S_
    windows = windows or [0] * S_
    capacity_max = capacity_max or max(caps)
    rows = max(cursors) + capacity_max + 8
    em = LaneEmitter(S_, kH, kW, capacity_max, rows, cursors, windows)
    em.set(wins, active, caps)
    em.emit(preds.to(DEV).contiguous(), cell_cap, MODES[mode], seed)
    got_cs = em.cs.tolist()
    counts = em.scratch[0].view(S_, 2, kH, kW).cpu().long()
    wants = []
    for s in range(S_):
        if not active[s]:
            assert got_cs[s] == em.cs0[s], s
            assert em.untouched(s, 0, rows), s
            assert int(counts[s].sum()) == 0
            wants.append(None)
            continue
        want = emit_window_torch(preds[s], wins[s][0], wins[s][1],
                                 capacity=caps[s], cell_cap=cell_cap,
                                 mode=mode, seed=seed,
                                 window_index=windows[s])
        n, cur = want["emitted"], cursors[s]
        assert got_cs[s] == [cur + n, want["total"], n, want["dropped"],
                             windows[s] + 1], s
        for f, g in zip(S.COLS, em.rows(s, cur, cur + n)):
            assert g.dtype == want[f].dtype, f
            assert g.tobytes() == want[f].tobytes(), \
                f"lane {s} column {f}: {int((g != want[f]).sum())} of {n} " \
                f"rows differ"
        assert em.untouched(s, 0, cur) and em.untouched(s, cur + n, rows), s
        assert torch.equal(counts[s], want["counts"]), s
        wants.append(want)
    return wants, em


def _sparse(seed, shape, high, density=0.3):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, high + 1, shape, generator=g).float()
    return v * (torch.rand(shape, generator=g) < density)


# ---------------------------------------------------------------------------
# sr_emit_lanes against emit_window_torch

@pytest.mark.parametrize("mode", ["linear", "random"])
def test_three_lanes_one_idle_one_overflowing(mode):
    preds = torch.stack([_sparse(1, (2, 32, 48), 5),
                         _sparse(2, (2, 32, 48), 5),
                         _sparse(3, (2, 32, 48), 5)])
    preds[1, 0, 0, :4] = torch.tensor([S.NAN, S.INF, -S.INF, 1e30])
    preds[1, 1, 5] = S.NAN
    preds[1, 1, 6] = S.INF
    total2 = int(cell_counts_torch(preds[2]).sum())
    t0 = 1.7e9 + 0.123
    wants, _ = _check_lanes(
        preds, [(1.7e9, 1.7e9 + 1e-3), (3.0, 4.0), (t0, t0)],
        [8192, 8192, total2 - 3], [1, 0, 1], cursors=[777, 5, 31],
        windows=[17, 3, 40], capacity_max=8192, mode=mode, seed=5)
    assert wants[0]["total"] > 1000 and wants[0]["dropped"] == 0
    assert (wants[2]["emitted"], wants[2]["dropped"]) == (total2 - 3, 3)
    assert np.all(wants[2]["ts"] == t0)


@pytest.mark.parametrize("mode", ["linear", "random"])
def test_one_lane_equals_sr_emit_window(mode):
    ext = _ext()
    pred = _sparse(4, (2, 32, 48), 5)
    cap, rows = 2000, 2000 + 50
    em = LaneEmitter(1, 32, 48, cap, rows, [9], [6])
    em.set([(10.0, 10.5)], [1], [cap])
    em.emit(pred[None].to(DEV), mode=MODES[mode], seed=8)
    cols = [torch.full((rows,), v, dtype=dt, device=DEV)
            for v, dt in zip(SENTINEL, DTYPES)]
    cs = torch.tensor([9, -1, -1, -1, 6], dtype=torch.int64, device=DEV)
    win = torch.tensor([10.0, 10.5], dtype=torch.float64, device=DEV)
    ext.sr_emit_window(pred.to(DEV), win, cols, cs, cap, 1023, MODES[mode],
                       8, ext.sr_emit_scratch(win, 2 * 32 * 48, cap))
    assert em.cs[0].tolist() == cs.tolist()
    assert cs[3].item() > 0                 # the capacity cuts this window
    for f, a, b in zip(S.COLS, em.cols, cols):
        assert a[0].cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f


@pytest.mark.parametrize("zero_lane", [0, 2])
def test_all_zero_map_at_either_end(zero_lane):
    """The total-from-scan arithmetic at the first and at the last cell."""
    preds = torch.stack([_sparse(10 + s, (2, 32, 48), 5) for s in range(3)])
    preds[zero_lane] = 0
    preds[zero_lane, 0, 3, 3] = -2.0        # still no event
    wants, _ = _check_lanes(preds, [(0.0, 1.0), (1.0, 2.0), (2.0, 3.0)],
                            [8192] * 3, [1, 1, 1], cursors=[5, 6, 7],
                            windows=[1, 2, 3])
    assert wants[zero_lane]["total"] == 0
    assert all(w["total"] > 1000 for s, w in enumerate(wants)
               if s != zero_lane)


@pytest.mark.parametrize("mode", ["linear", "random"])
def test_full_lane_next_to_a_short_lane(mode):
    """Every cell of lane 0 holds cell_cap events, so q = Q occurs once per
    cell; lane 1 holds a few single events (q = 0) and a short total: pad
    keys and maximum phases must not cross the lane boundary."""
    cell_cap = 5
    preds = torch.zeros(3, 2, 32, 48)
    preds[0] = 1e30
    preds[1, 0, 4, ::7] = 1.0
    preds[1, 1, 31, 47] = 1.0
    preds[2, 1, 0, 0] = 3.0
    full = 2 * 32 * 48 * cell_cap
    wants, _ = _check_lanes(preds, [(0.0, 1.0), (5.0, 6.0), (7.0, 9.0)],
                            [full, full, full], [1, 1, 1], cell_cap=cell_cap,
                            mode=mode, seed=3, windows=[4, 5, 6])
    assert wants[0]["emitted"] == full
    assert wants[1]["emitted"] == 8 and wants[2]["emitted"] == 3
    if mode == "linear":
        assert int((wants[0]["q"] == S.Q).sum()) == 2 * 32 * 48
        assert np.all(wants[1]["q"] == 0)


def test_lanes_past_one_grid():
    """Two lanes, each a little past one full grid of the capped kernels:
    the lane boundary falls inside the second pass of the counts, emit and
    append loops."""
    cap = int(_ext().grid_cap())
    kW = 512
    kH = cap // (2 * kW) + 3
    ncells = 2 * kH * kW
    assert cap < ncells < 1.1 * cap
    g = torch.Generator().manual_seed(7)
    preds = torch.randint(0, 3, (2, 2, kH, kW), generator=g).float()
    preds[1] *= (torch.rand(2, kH, kW, generator=g) < 0.2)
    totals = [int(p.sum()) for p in preds]
    assert totals[0] > cap > totals[1] > 1000
    _check_lanes(preds, [(100.0, 101.0), (200.0, 200.5)],
                 [totals[0] + 100, totals[1] - 7], [1, 1], cursors=[3, 0],
                 windows=[8, 9])


def test_capture_replays_equal_eager_calls():
    calls = [
        (torch.stack([_sparse(20 + s, (2, 32, 48), 5) for s in range(3)]),
         [(50.0, 50.25), (1.0, 2.0), (7.0, 7.0)], [1, 1, 0],
         [4096, 1000, 4096]),
        (torch.stack([_sparse(30 + s, (2, 32, 48), 5) for s in range(3)]),
         [(50.25, 51.0), (2.0, 2.5), (7.0, 8.0)], [1, 0, 1],
         [4096, 1000, 900])]
    cap = 4096

    def emitter():
        return LaneEmitter(3, 32, 48, cap, 3 * cap, [0, 2, 4], [6, 7, 8])
    eager = emitter()
    for p, wins, active, caps in calls:
        eager.set(wins, active, caps)
        eager.emit(p.to(DEV), mode=1, seed=2)

    em = emitter()
    static = torch.zeros(3, 2, 32, 48, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        em.emit(static, mode=1, seed=2)     # warm-up: every lane idle
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        em.emit(static, mode=1, seed=2)
    assert em.cs.tolist() == em.cs0         # idle lanes: nothing moved
    for p, wins, active, caps in calls:
        static.copy_(p)
        em.set(wins, active, caps)
        graph.replay()
    torch.cuda.synchronize()
    assert em.cs.tolist() == eager.cs.tolist()
    assert all(int(n) > 500 for n in em.cs[:, 0])
    for f, a, b in zip(S.COLS, em.cols, eager.cols):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f


# ---------------------------------------------------------------------------
# super_resolve_stores on the device

@pytest.fixture(scope="module")
def srcs(tmp_path_factory):
    return L.write_recording_set(tmp_path_factory.mktemp("lanes_gpu_src"))


@pytest.mark.parametrize("name", list(L.MODELS))
def test_stub_models_equal_single_path_and_cpu(srcs, tmp_path, name):
    cls = L.MODELS[name]
    single = L.run_single(cls, srcs, tmp_path / "single", device=DEV)
    cpu = L.run_lanes(cls, srcs, tmp_path / "cpu", 3)
    for tag, kw in (("graph", dict(use_graphs=True)),
                    ("eager", dict(use_graphs=False))):
        got = L.run_lanes(cls, srcs, tmp_path / tag, 3, device=DEV, **kw)
        L.assert_same_runs(got, single)
        L.assert_same_runs(got, cpu)
    assert sum(r["events_out"] for _, r in single) > 0


@pytest.fixture(scope="module")
def lifted():
    torch.manual_seed(0)
    return S.Lifted(build_model("ESRNet", inch=2, basech=8, num_frame=3)
                    .eval())


def _lanes(model, srcs, root, **kw):
    root.mkdir(parents=True, exist_ok=True)
    pairs = [(src, str(root / f"out{i}.evs")) for i, src in enumerate(srcs)]
    res = super_resolve_stores(
        copy.deepcopy(model), pairs, lanes=3,
        **L.run_args(device=DEV, keep=True, **kw))
    return [(dst, *res[dst]) for _, dst in pairs]


@pytest.fixture(scope="module")
def esr_runs(srcs, lifted, tmp_path_factory):
    """The graphed and the eager lanes run and the device single path of the
    tiny model, once: [(dst, summary, kept)] per recording."""
    root = tmp_path_factory.mktemp("lanes_esr")
    out = {"graph": _lanes(lifted, srcs, root / "graph", use_graphs=True),
           "eager": _lanes(lifted, srcs, root / "eager", use_graphs=False),
           "single": []}
    (root / "single").mkdir()
    for i, src in enumerate(srcs):
        dst = str(root / "single" / f"out{i}.evs")
        out["single"].append((dst, *super_resolve_store(
            copy.deepcopy(lifted), src, dst,
            **L.run_args(device=DEV, keep=True))))
    return out


def test_tiny_esrnet_lanes_graphs_equal_eager(esr_runs):
    for (pg, sg, kg), (pe, se, ke) in zip(esr_runs["graph"],
                                          esr_runs["eager"]):
        diff = (kg["pred"] - ke["pred"]).abs().max().item()
        print(f"graph vs eager: max |diff| of the kept predictions {diff}")
        assert torch.equal(kg["counts"], ke["counts"])
        assert torch.equal(kg["stats"], ke["stats"])
        S.assert_same_files(pg, pe, L.OUT_GROUP)
        assert L.sans_seconds(sg) == L.sans_seconds(se)
        assert sg["events_out"] > 0


def test_tiny_esrnet_kept_predictions_reproduce_the_files(esr_runs, srcs):
    """Emission and scheduling, whatever the forward computed: the run's own
    kept predictions through the oracle give each file exactly."""
    from esr_amd.data.store import EventStore
    from esr_amd.engine.superresolve import tile_windows
    for src, (path, summary, kept) in zip(srcs, esr_runs["graph"]):
        st = EventStore(src)
        n = st.num_events(L.GROUP)
        tiles = tile_windows(np.asarray(st.ts(L.GROUP)[:n]), "events",
                             S.WINDOW)
        evs = [emit_window_torch(p.cpu(), tiles["t0"][w], tiles["t1"][w],
                                 capacity=summary["capacity"], window_index=w)
               for p, w in zip(kept["pred"], kept["windows"])]
        cols, n_out = S.read_group(path, L.OUT_GROUP)
        assert n_out == summary["events_out"] == sum(e["emitted"]
                                                     for e in evs)
        for f in S.COLS:
            assert cols[f][:n_out].tobytes() == \
                np.concatenate([e[f] for e in evs]).tobytes(), f
        assert kept["stats"].tolist() == \
            [[e["total"], e["emitted"], e["dropped"]] for e in evs]


def test_tiny_esrnet_lanes_against_single_path(esr_runs):
    worst = 0.0
    for (pl, sl, kl), (ps, ss, ks) in zip(esr_runs["graph"],
                                          esr_runs["single"]):
        assert kl["pred"].shape == ks["pred"].shape
        worst = max(worst, (kl["pred"] - ks["pred"]).abs().max().item())
    print(f"lanes vs single path: max |diff| of the kept fp32 predictions "
          f"{worst:.3e}")
    assert worst <= 4 * PRED_DIFF_MEASURED
    if PRED_DIFF_MEASURED == 0.0:
        for (pl, sl, kl), (ps, ss, ks) in zip(esr_runs["graph"],
                                              esr_runs["single"]):
            S.assert_same_files(pl, ps, L.OUT_GROUP)
            assert L.sans_seconds(sl) == L.sans_seconds(ss)


def test_bf16_autocast_lanes_run_on_the_native_stack(srcs, lifted, tmp_path):
    from esr_amd.ops import conv
    before = conv.stats["native_calls"]
    runs = _lanes(lifted, srcs, tmp_path, amp_dtype=torch.bfloat16)
    assert conv.stats["native_calls"] > before
    for path, summary, kept in runs:
        cols, n = S.read_group(path, L.OUT_GROUP)
        assert n == summary["events_out"] > 0
        assert np.all(np.diff(cols["ts"][:n]) >= 0)
        assert kept["pred"].dtype == torch.float32
