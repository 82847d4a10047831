"""`super_resolve_stores` on the CPU: several recordings in lanes of one
batched tick against `super_resolve_store` on each recording alone.  Every
output store must be byte for byte the single path's, and every summary equal
minus `seconds`: the stub models are exact in fp32 and batch-row local, so a
state leak between lanes or across a handover changes the files."""

from pathlib import Path

import pytest

from esr_amd.engine import super_resolve_stores

import superresolve_helpers as S
import superresolve_lanes_helpers as L


@pytest.fixture(scope="module")
def srcs(tmp_path_factory):
    return L.write_recording_set(tmp_path_factory.mktemp("lanes_src"))


@pytest.fixture(scope="module")
def singles(srcs, tmp_path_factory):
    """The single-path runs with default arguments, once per model."""
    root = tmp_path_factory.mktemp("lanes_single")
    return {name: L.run_single(cls, srcs, root / name)
            for name, cls in L.MODELS.items()}


def test_the_single_path_behaves_as_the_tests_assume(singles, srcs,
                                                     tmp_path):
    def events(runs):
        return tuple(r["events_out"] for _, r in runs)
    assert events(singles["midframe"]) == L.MIDFRAME_EVENTS
    assert events(singles["running_sum"]) == L.RUNNING_SUM_EVENTS
    assert all(r["windows_overflowed"] == 0
               for runs in singles.values() for _, r in runs)
    # the two-row state counts every mid frame three times
    assert events(singles["two_row"]) == tuple(
        3 * r - 2 * m for r, m in zip(L.RUNNING_SUM_EVENTS,
                                      L.MIDFRAME_EVENTS))
    cap20 = L.run_single(S.MidFrame, srcs, tmp_path, capacity=20)
    assert events(cap20) == L.MIDFRAME_CAP20_EVENTS
    for (_, r), n in zip(cap20, L.WINDOW_COUNTS):
        assert r["windows_overflowed"] == n - 2
        assert r["events_dropped"] == 12 * (n - 2)


@pytest.mark.parametrize("lanes", [1, 2, 3, 8])
@pytest.mark.parametrize("name", list(L.MODELS))
def test_lanes_equal_the_single_path(srcs, singles, tmp_path, name, lanes):
    got = L.run_lanes(L.MODELS[name], srcs, tmp_path, lanes)
    L.assert_same_runs(got, singles[name])


def test_capacity_overflow_in_every_window(srcs, tmp_path):
    want = L.run_single(S.MidFrame, srcs, tmp_path / "single", capacity=20)
    got = L.run_lanes(S.MidFrame, srcs, tmp_path / "lanes", 2, capacity=20)
    L.assert_same_runs(got, want)
    for (_, g), (_, w) in zip(got, want):
        assert g["overflowed_windows"] == w["overflowed_windows"] != []


def test_time_mode_capacity_is_per_recording(srcs, tmp_path):
    kw = dict(mode="time", window=0.01)
    want = L.run_single(L.RunningSum, srcs, tmp_path / "single", **kw)
    capacities = [r["capacity"] for _, r in want]
    assert len(set(capacities)) >= 3, capacities
    got = L.run_lanes(L.RunningSum, srcs, tmp_path / "lanes", 3, **kw)
    assert [r["capacity"] for _, r in got] == capacities
    L.assert_same_runs(got, want)


def test_random_phases_use_the_lanes_own_window_index(srcs, tmp_path):
    kw = dict(redistribute="random", seed=9)
    want = L.run_single(L.RunningSum, srcs, tmp_path / "single", **kw)
    got = L.run_lanes(L.RunningSum, srcs, tmp_path / "lanes", 2, **kw)
    L.assert_same_runs(got, want)
    # and the seed matters: the files are not the linear ones
    other = L.run_single(L.RunningSum, srcs[:1], tmp_path / "linear")
    with pytest.raises(AssertionError):
        S.assert_same_files(got[0][0], other[0][0], L.OUT_GROUP)


def test_chunk_windows_two(srcs, singles, tmp_path):
    got = L.run_lanes(L.TwoRowSum, srcs, tmp_path, 3, chunk_windows=2)
    L.assert_same_runs(got, singles["two_row"])


def test_keep_returns_the_single_paths_windows(srcs, tmp_path):
    import torch
    want = L.run_single(L.RunningSum, srcs, tmp_path / "single", keep=True)
    got = L.run_lanes(L.RunningSum, srcs, tmp_path / "lanes", 2, keep=True)
    L.assert_same_runs(got, want, keep=True)
    for (_, (_, kg)), (_, (_, kw)) in zip(got, want):
        assert kg["windows"] == kw["windows"]
        for f in ("pred", "counts", "stats"):
            assert torch.equal(kg[f], kw[f]), f


def _pairs(srcs, root):
    return [(s, str(root / f"out{i}.evs")) for i, s in enumerate(srcs)]


def test_too_short_recording_raises_before_anything_is_written(srcs,
                                                               tmp_path):
    short = L.write_lr_store(tmp_path / "short.evs", 2, seed=40,
                             t_start=1.7e9)
    pairs = _pairs([srcs[0], short, srcs[1]], tmp_path / "out")
    with pytest.raises(ValueError, match="short.evs"):
        super_resolve_stores(S.MidFrame(), pairs, lanes=2, **L.run_args())
    assert not any(Path(dst).exists() for _, dst in pairs)


def test_other_resolution_raises_before_anything_is_written(srcs, tmp_path):
    import numpy as np
    from esr_amd.data.store import EventStoreWriter
    n = 5 * S.WINDOW
    with EventStoreWriter(tmp_path / "wide.evs", (24, 48)) as w:
        w.add_group(L.GROUP, np.zeros(n, np.int64), np.zeros(n, np.int64),
                    np.arange(n) * 1e-4, np.ones(n, np.int64))
    pairs = _pairs([srcs[0], srcs[1], str(tmp_path / "wide.evs")],
                   tmp_path / "out")
    with pytest.raises(ValueError, match="wide.evs"):
        super_resolve_stores(S.MidFrame(), pairs, lanes=2, **L.run_args())
    assert not any(Path(dst).exists() for _, dst in pairs)


def test_missing_group_raises(srcs, tmp_path):
    pairs = _pairs(srcs[:2], tmp_path / "out")
    with pytest.raises(ValueError, match="rec0.evs"):
        super_resolve_stores(S.MidFrame(), pairs, lanes=2,
                             **L.run_args(group="down4"))
    assert not any(Path(dst).exists() for _, dst in pairs)


def test_tuple_state_is_not_supported(srcs, tmp_path):
    with pytest.raises(NotImplementedError, match="tuple state"):
        super_resolve_stores(L.TupleState(), _pairs(srcs[:2], tmp_path),
                             lanes=2, **L.run_args())


def test_state_rows_must_divide_into_lanes(srcs, tmp_path):
    with pytest.raises(ValueError, match="rows per lane"):
        super_resolve_stores(L.OddRows(), _pairs(srcs[:2], tmp_path),
                             lanes=2, **L.run_args())


def test_arena_limit_states_both_numbers(srcs, tmp_path):
    with pytest.raises(ValueError, match="max_bytes = 1000"):
        super_resolve_stores(S.MidFrame(), _pairs(srcs, tmp_path), lanes=2,
                             max_bytes=1000, **L.run_args())


# ---------------------------------------------------------------------------
# CLI

def test_cli_lanes_partitions_by_resolution(srcs, tmp_path):
    """`--lanes 2 --data_list` over two LR resolutions: each part goes
    through the lanes, the YAML keeps the list's order, and every store is
    what the function writes for that part."""
    import copy
    import subprocess
    import sys

    import numpy as np
    import torch
    import yaml

    from esr_amd.data.store import EventStoreWriter
    from esr_amd.engine import save_checkpoint
    from esr_amd.models import build_model

    repo = Path(__file__).resolve().parent.parent
    rng = np.random.default_rng(5)
    n = 4 * S.WINDOW
    with EventStoreWriter(tmp_path / "wide.evs", (24, 48)) as w:
        w.add_group(L.GROUP, rng.integers(0, 24, n), rng.integers(0, 12, n),
                    np.sort(rng.random(n)), rng.integers(0, 2, n) * 2 - 1)
    listed = [srcs[3], str(tmp_path / "wide.evs"), srcs[1]]
    (tmp_path / "list.txt").write_text("\n".join(listed) + "\n")
    torch.manual_seed(0)
    model = build_model("ESRNet", inch=2, basech=8, num_frame=3).eval()
    config = {"model": {"name": "ESRNet",
                        "args": {"inch": 2, "basech": 8, "num_frame": 3}},
              "lr_scheduler": {"name": "none"}, "optimizer": {"name": "none"},
              "SEQN": 3}
    ckpt = tmp_path / "ckpt.pth"
    save_checkpoint(ckpt, config, model)
    out = subprocess.run(
        [sys.executable, "superresolve.py", "--model_path", str(ckpt),
         "--data_list", str(tmp_path / "list.txt"), "--group", L.GROUP,
         "--output", str(tmp_path / "hr"), "--scale", "2", "--seqn", "3",
         "--window", str(S.WINDOW), "--device", "cpu", "--lanes", "2"],
        capture_output=True, text=True, timeout=300, cwd=str(repo))
    assert out.returncode == 0, out.stderr[-3000:]
    printed = yaml.safe_load(out.stdout)
    dsts = [str(tmp_path / "hr" / f"{Path(src).stem}.evs") for src in listed]
    assert list(printed) == dsts
    # the function on the same parts: two 24 x 40 recordings share the lanes,
    # the 24 x 48 one runs alone
    want = {}
    for part in ([0, 2], [1]):
        pairs = [(listed[i], str(tmp_path / f"fn{i}.evs")) for i in part]
        res = super_resolve_stores(copy.deepcopy(model), pairs, lanes=2,
                                   **L.run_args(checkpoint=str(ckpt)))
        want.update({i: res[pairs[k][1]] for k, i in enumerate(part)})
    for i, dst in enumerate(dsts):
        assert L.sans_seconds(printed[dst]) == L.sans_seconds(want[i])
        assert printed[dst]["source"] == listed[i]
        if want[i]["events_out"]:
            S.assert_same_files(dst, tmp_path / f"fn{i}.evs", L.OUT_GROUP)
