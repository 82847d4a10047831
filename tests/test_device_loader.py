"""DeviceSequenceLoader (torch form, CPU) against SequenceDataLoader with
collate='shared'.  Count maps hold small integers in fp32, so every
comparison is torch.equal."""

import copy

import pytest
import torch
from torch.utils.data.distributed import DistributedSampler

from esr_amd.data import SequenceDataLoader
from esr_amd.data.device_loader import (FLAG_HFLIP, FLAG_PFLIP, FLAG_VFLIP,
                                        DeviceSequenceLoader)
from esr_amd.ops import events as E

import device_loader_helpers as H

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def datalist(tmp_path_factory):
    return H.make_datalist(tmp_path_factory.mktemp("evs_device"))


def _oracle(cfg):
    cfg = copy.deepcopy(cfg)
    cfg["collate"] = "shared"
    return SequenceDataLoader(cfg)


def _assert_parity(oracle, loader, epochs=(0, 1)):
    """Every batch of both epochs equal; returns the loader's job tables."""
    tables = []
    for epoch in epochs:
        if epoch:
            oracle.set_epoch(epoch)
            loader.set_epoch(epoch)
        want = list(oracle)
        assert len(loader) == len(oracle) == len(want) > 0
        n = 0
        for ref, got in zip(want, loader):
            assert got["seqn"] == ref["seqn"]
            assert got["frames"].dtype == torch.float32
            assert got["frames"].shape == ref["frames"].shape
            assert got["gt_mids"].shape == ref["gt_mids"].shape
            assert torch.equal(got["frames"], ref["frames"])
            assert torch.equal(got["gt_mids"], ref["gt_mids"])
            assert ref["frames"].sum() > 0 and ref["gt_mids"].sum() > 0
            tables.append(loader.job_table(loader.last_indices))
            n += 1
        assert n == len(want)
    return tables


def test_parity_with_cpu_loader(datalist):
    cfg = H.dl_config(datalist)
    loader = DeviceSequenceLoader(cfg, CPU)
    assert loader.seqn == 3 and loader.scale == 2
    assert list(loader.inp_sensor_resolution) == [20, 43]
    assert list(loader.gt_sensor_resolution) == [40, 86]
    assert loader.dist_sampler is None
    # premise: over the two epochs every flip is both taken and not taken
    flags = set()
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        for idx in range(len(loader.dataset)):
            flags.add(int(loader.job_table([idx])[0, 2]))
    loader.set_epoch(0)
    for bit in (FLAG_HFLIP, FLAG_VFLIP, FLAG_PFLIP):
        assert any(f & bit for f in flags), f"flag {bit} never set"
        assert any(not f & bit for f in flags), f"flag {bit} never clear"
    _assert_parity(_oracle(cfg), loader)


def test_parity_with_pauses(datalist):
    cfg = H.dl_config(datalist)
    cfg["dataset"]["sequence"]["pause"]["enabled"] = True
    oracle = _oracle(cfg)
    loader = DeviceSequenceLoader(cfg, CPU)
    # premise: the oracle holds a paused step (zero input, GT still there)
    paused = 0
    for epoch in (0, 1):
        oracle.set_epoch(epoch)
        for batch in oracle:
            paused += int((batch["frames"].sum(dim=(2, 3, 4)) == 0).sum())
    assert paused > 0
    oracle.set_epoch(0)
    _assert_parity(oracle, loader)


def test_without_gt_events(datalist):
    cfg = H.dl_config(datalist, need_gt_events=False)
    loader = DeviceSequenceLoader(cfg, CPU)
    want = list(_oracle(cfg))
    for ref, got in zip(want, loader):
        assert torch.equal(got["frames"], ref["frames"])
        assert torch.equal(got["gt_mids"], ref["gt_mids"])
        assert got["gt_mids"].sum() == 0 and got["frames"].sum() > 0


def test_fp32_rounding_is_the_oracles(datalist):
    """At width 43 the oracle's x / 43 * 86 in fp32 is not x * 2."""
    cfg = H.dl_config(datalist)
    cfg["dataset"]["data_augment"]["enabled"] = False
    oracle = _oracle(cfg)
    loader = DeviceSequenceLoader(cfg, CPU)
    ref = next(iter(oracle))["frames"]
    # naive splat of the same windows: item b is sequence 0's item b
    ds = oracle.dataset.datasets[0].dataset
    naive = torch.zeros_like(ref)
    for b in range(ref.size(0)):
        for l in range(ref.size(1)):
            i0, i1 = ds.event_indices[b * 4 + l]
            ev = torch.from_numpy(ds.store.events("down2", i0, i1)).float()
            naive[b, l] = E.events_to_channels(ev[0] * 2, ev[1] * 2, ev[3],
                                               (40, 86))
    assert naive.sum() > 0
    assert not torch.equal(ref, naive)
    # the columns that show it: x = 15 -> 29 and x = 30 -> 59
    assert ref[0, 0, :, :, 29].sum() > 0 and naive[0, 0, :, :, 29].sum() == 0
    assert ref[0, 0, :, :, 59].sum() > 0 and naive[0, 0, :, :, 59].sum() == 0
    got = next(iter(loader))["frames"]
    assert torch.equal(got, ref)
    assert not torch.equal(got, naive)


@pytest.mark.parametrize("key,override", [
    ("add_noise", {"add_noise": {"enabled": True, "noise_level": 0.01}}),
    ("hot_filter", {"hot_filter": {"enabled": True}}),
    ("custom_resolution", {"custom_resolution": [32, 32]}),
    ("real_world_test", {"real_world_test": True}),
    ("inp_cnt", {"fields": ["inp_scaled_cnt", "gt_cnt", "inp_cnt"]}),
])
def test_unsupported_options_raise(datalist, key, override):
    with pytest.raises(ValueError, match=key):
        DeviceSequenceLoader(H.dl_config(datalist, **override), CPU)


def test_supported_fields_pass(datalist):
    cfg = H.dl_config(datalist, fields=["inp_scaled_cnt", "gt_cnt"])
    assert len(DeviceSequenceLoader(cfg, CPU)) == 5


def test_bad_store_and_budget_raise(datalist, tmp_path):
    def bad_polarity(group, xs, ys, ts, ps):
        if group == "down2":
            ps[77] = 0

    def bad_coordinate(group, xs, ys, ts, ps):
        if group == "ori":
            ys[123] = 1 << 15

    for k, mutate in enumerate((bad_polarity, bad_coordinate)):
        dl = H.make_datalist(tmp_path / f"bad{k}", mutate)
        with pytest.raises(ValueError, match=r"seq0\.evs"):
            DeviceSequenceLoader(H.dl_config(dl), CPU)

    cfg = H.dl_config(datalist)
    cfg["device_resident"] = {"max_bytes": 1}
    need = 4 * 2 * (H.N_ORI + H.N_DOWN2)
    with pytest.raises(ValueError, match=str(need)):
        DeviceSequenceLoader(cfg, CPU)
    cfg["device_resident"] = {"max_bytes": need}
    assert DeviceSequenceLoader(cfg, CPU).resident_bytes == need


def test_shuffle_and_sharding(datalist):
    torch.manual_seed(0)
    cfg = H.dl_config(datalist)
    cfg["shuffle"] = True
    loader = DeviceSequenceLoader(cfg, CPU)
    epochs = []
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        order = []
        for _ in loader:
            order += loader.last_indices
        assert sorted(order) == list(range(10))
        epochs.append(order)
    assert epochs[0] != epochs[1]

    seen = []
    for rank in (0, 1):
        probe = DeviceSequenceLoader(H.dl_config(datalist), CPU)
        sampler = DistributedSampler(probe.dataset, num_replicas=2,
                                     rank=rank, shuffle=True)
        sharded = DeviceSequenceLoader(cfg, CPU, sampler=sampler)
        assert sharded.dist_sampler is sampler
        sharded.set_epoch(3)
        assert sampler.epoch == 3
        mine = []
        for _ in sharded:
            mine += sharded.last_indices
        assert len(mine) == len(set(mine)) == 4   # 5 per rank, drop_last
        seen.append(set(mine))
    assert not seen[0] & seen[1]


def test_views_share_one_buffer(datalist):
    """The documented lifetime: the next batch overwrites the last one."""
    loader = DeviceSequenceLoader(H.dl_config(datalist), CPU)
    it = iter(loader)
    first = next(it)
    kept = first["frames"].clone()
    second = next(it)
    assert first["frames"].data_ptr() == second["frames"].data_ptr()
    assert not torch.equal(kept, second["frames"])


def _tiny_train_config(datalist, out_dir, device_resident):
    dl = H.dl_config(datalist)
    if device_resident:
        dl["device_resident"] = True
    else:
        dl["collate"] = "shared"
    return {
        "experiment": "test", "SEQN": 3,
        "model": {"name": "ESRNet",
                  "args": {"inch": 2, "basech": 4, "num_frame": 3}},
        "optimizer": {"name": "Adam", "args": {"lr": 1e-3}},
        "lr_scheduler": {"name": "ExponentialLR", "args": {"gamma": 0.95}},
        "trainer": {
            "output_path": str(out_dir),
            "epoch_based_train": {"enabled": False},
            "iteration_based_train": {
                "enabled": True, "iterations": 2, "save_period": 100,
                "train_log_step": 1, "valid_log_step": 1, "valid_step": 100,
                "lr_change_rate": 1000},
            "monitor": "min valid_loss", "early_stop": 10,
            "tensorboard": False, "vis": {"enabled": False},
        },
        "train_dataloader": dl,
        "valid_dataloader": copy.deepcopy(dl),
    }


def test_training_end_to_end_matches_cpu_loader(datalist, tmp_path):
    from esr_amd.config import ConfigParser
    from esr_amd.engine import build_training
    from esr_amd.utils.logging import setup_logging

    losses = {}
    for resident in (True, False):
        cfg = _tiny_train_config(datalist, tmp_path / f"out{resident}",
                                 resident)
        torch.manual_seed(11)
        trainer = build_training(ConfigParser(cfg, run_id=f"r{resident}"),
                                 CPU, setup_logging(f"dev{resident}", None))
        kind = type(trainer.train_dataloader)
        assert (kind is DeviceSequenceLoader) == resident
        assert (type(trainer.valid_dataloader) is DeviceSequenceLoader) \
            == resident
        trainer.model.train()
        trainer.train_dataloader.set_epoch(0)
        got = []
        for step, batch in enumerate(trainer.train_dataloader):
            if step == 2:
                break
            loss, _, _ = trainer.bptt_step(batch, train=True)
            got.append(loss.clone())
        assert len(got) == 2
        losses[resident] = got
    for a, b in zip(losses[True], losses[False]):
        assert torch.isfinite(a) and a > 0
        assert torch.equal(a, b)
