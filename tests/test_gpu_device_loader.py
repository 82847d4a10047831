"""batch_splat.hip against `batch_splat_torch` (run on CPU copies), and the
device-resident loader on the GPU against the same loader on the CPU.  Every
addend is 1.0, so every comparison is torch.equal."""

import numpy as np
import pytest
import torch

from esr_amd.data.device_loader import (FLAG_GT, DeviceSequenceLoader,
                                        batch_splat_torch)
from esr_amd.ops.native import get_ext

import device_loader_helpers as H

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not hasattr(get_ext(), "evs_batch_splat"),
                       reason="the native extension lacks evs_batch_splat "
                              "(run python -m esr_amd.ops.native.build)"),
]

DEV = "cuda:0"
LR, HR = (20, 43), (40, 86)


@pytest.fixture(scope="module")
def datalist(tmp_path_factory):
    return H.make_datalist(tmp_path_factory.mktemp("evs_device_gpu"))


@pytest.fixture(scope="module")
def resident(datalist):
    """The CPU loader (its packed events and group offsets) and the kernel's
    chunk size."""
    loader = DeviceSequenceLoader(H.dl_config(datalist), torch.device("cpu"))
    return loader, int(get_ext().evs_batch_splat_chunk())


def _job_table(loader, chunk):
    """All 8 flag combinations for both kinds over windows that hold the
    out-of-range rows, an empty job, and lengths 1, CHUNK-1, CHUNK,
    CHUNK+1."""
    inp, gt = loader._inp_base[0], loader._gt_base[0]
    inp1, gt1 = loader._inp_base[1], loader._gt_base[1]
    rows = []
    for flags in range(8):
        # rows 5, 6, 300, 301 of the group are out of range
        rows.append((inp + 0, inp + 400, flags))
        rows.append((gt + 0, gt + 400, flags | FLAG_GT))
        # rows 1500, 1501, in the second chunk of the job
        rows.append((inp1 + 200, inp1 + 1700, flags))
        rows.append((gt1 + 200, gt1 + 1700, flags | FLAG_GT))
    rows.append((inp + 50, inp + 50, 3))                    # empty
    rows.append((gt + 50, gt + 50, FLAG_GT))
    for n in (1, chunk - 1, chunk, chunk + 1):
        rows.append((inp + 7, inp + 7 + n, 5))
        rows.append((gt1 + 9, gt1 + 9 + n, 2 | FLAG_GT))
    table = np.zeros((len(rows), 4), dtype=np.int32)
    table[:, :3] = rows
    return torch.from_numpy(table)


def _oracle(packed, jobs):
    out = torch.zeros(jobs.size(0), 2, *HR)
    batch_splat_torch(packed, jobs, out, *LR)
    return out


@pytest.mark.parametrize("slack", [0, 3000])
def test_kernel_matches_torch_form(resident, slack):
    loader, chunk = resident
    assert chunk + 1 <= H.N_DOWN2
    jobs = _job_table(loader, chunk)
    longest = int((jobs[:, 1] - jobs[:, 0]).max())
    assert longest == 1500 > chunk
    want = _oracle(loader._packed, jobs)
    # the job table does what it is meant to: flips move mass, the empty
    # jobs add nothing, an n-event job adds at most n
    assert not torch.equal(want[0], want[4]) and want[32].sum() == 0 \
        and want[33].sum() == 0 and want[34].sum() == 1
    assert 0 < want[0].sum() < 400         # out-of-range rows were dropped
    out = torch.full((jobs.size(0), 2, *HR), 0.0, device=DEV)
    get_ext().evs_batch_splat(loader._packed.to(DEV), jobs.to(DEV), out,
                              LR[0], LR[1], longest + slack)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    # "adds into out in place": a second launch doubles every count
    get_ext().evs_batch_splat(loader._packed.to(DEV), jobs.to(DEV), out,
                              LR[0], LR[1], longest + slack)
    assert torch.equal(out.cpu(), 2 * want)


def test_loader_on_gpu_matches_cpu(datalist, resident):
    cfg = H.dl_config(datalist)
    cfg["dataset"]["sequence"]["pause"]["enabled"] = True
    cpu = DeviceSequenceLoader(cfg, torch.device("cpu"))
    gpu = DeviceSequenceLoader(cfg, torch.device(DEV))
    assert gpu._ext is not None
    for epoch in (0, 1):
        cpu.set_epoch(epoch)
        gpu.set_epoch(epoch)
        assert len(cpu) == len(gpu) == 5
        n = 0
        for ref, got in zip(cpu, gpu):
            assert got["frames"].device == torch.device(DEV)
            assert torch.equal(got["frames"].cpu(), ref["frames"])
            assert torch.equal(got["gt_mids"].cpu(), ref["gt_mids"])
            assert ref["frames"].sum() > 0 and ref["gt_mids"].sum() > 0
            n += 1
        assert n == 5


def _train_config(datalist, out_dir, resident_loader):
    # the 64x64 synthetic sequences: 16x16 input, 32x32 GT, the batch shape
    # [2, 4, 2, 32, 32] the captured step is exercised with elsewhere
    dl = H.dl_config(datalist, ori_scale="down4", window=1024,
                     sliding_window=512)
    dl["device_resident" if resident_loader else "collate"] = \
        True if resident_loader else "shared"
    return {
        "experiment": "gpu-device-loader", "SEQN": 3, "precision": "bf16",
        "model": {"name": "ESRNet",
                  "args": {"inch": 2, "basech": 8, "num_frame": 3,
                           "upsampler": "pixelshuffle"}},
        "optimizer": {"name": "Adam", "args": {"lr": 1e-3}},
        "lr_scheduler": {"name": "ExponentialLR", "args": {"gamma": 0.95}},
        "trainer": {
            "output_path": str(out_dir), "hip_graphs": True,
            "epoch_based_train": {"enabled": False},
            "iteration_based_train": {
                "enabled": True, "iterations": 1, "save_period": 100,
                "train_log_step": 1, "valid_log_step": 1, "valid_step": 100,
                "lr_change_rate": 1000},
            "monitor": "off", "tensorboard": False, "vis": {"enabled": False},
        },
        "train_dataloader": dl, "valid_dataloader": None,
    }


def test_graphed_trainer_takes_device_batches(synth_datalist, tmp_path):
    """The captured training step fed by the device loader: its first-step
    loss is that of the same trainer fed by the CPU loader.  The two get
    bit-equal inputs and the same seeded weights, so both run the same
    forward on the same numbers; 1e-5 relative leaves room only for an fp32
    reduction that is not order-stable."""
    from esr_amd.config import ConfigParser
    from esr_amd.engine import build_training
    from esr_amd.utils.logging import setup_logging

    loss = {}
    for resident_loader in (True, False):
        cfg = _train_config(synth_datalist,
                            tmp_path / f"out{resident_loader}",
                            resident_loader)
        torch.manual_seed(5)
        trainer = build_training(
            ConfigParser(cfg, run_id=f"d{resident_loader}"),
            torch.device(DEV), setup_logging(f"gdl{resident_loader}", None))
        assert isinstance(trainer.train_dataloader, DeviceSequenceLoader) \
            == resident_loader
        trainer.train()
        assert trainer.use_graphs, "graph path fell back to eager"
        loss[resident_loader] = trainer.train_metrics.avg("train_loss")
    print("first-step loss, device vs CPU loader:", loss[True], loss[False])
    assert loss[False] > 0
    assert abs(loss[True] - loss[False]) <= 1e-5 * abs(loss[False])


def test_graph_capture_and_replay(resident):
    loader, chunk = resident
    tables = [_job_table(loader, chunk)]
    # a second table: the same rows in reverse order, flips rotated
    second = tables[0].flip(0).clone()
    second[:, 2] = (second[:, 2] & FLAG_GT) | ((second[:, 2] + 3) & 7)
    tables.append(second)
    longest = int((tables[0][:, 1] - tables[0][:, 0]).max())
    ext = get_ext()
    packed = loader._packed.to(DEV)
    jobs = torch.zeros_like(tables[0], device=DEV)
    out = torch.ones(jobs.size(0), 2, *HR, device=DEV)

    def body():
        out.zero_()
        ext.evs_batch_splat(packed, jobs, out, LR[0], LR[1], longest)

    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    want = [_oracle(loader._packed, t) for t in tables]
    assert not torch.equal(want[0], want[1])
    for t, w in zip(tables, want):
        jobs.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), w)
