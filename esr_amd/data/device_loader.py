"""Device-resident training feed for stored EVS sequences.

The CPU loader re-splats every window in Python and torch CPU ops and ships
the count maps over PCIe; one worker core builds a few hundred items a
second while a rank at the flagship step rate consumes thousands
(docs/SCALING.md, "Input-feed budget").  The trainer reads only two count
maps per window, `inp_scaled_cnt` and `gt_cnt`, and neither looks at a
timestamp: windowing does, and the dataset works that out once at
construction.  So `DeviceSequenceLoader` keeps each sequence on the device at
one packed word per event and turns a batch into a table of
(begin, end, flags) jobs, one H2D copy of that table and one kernel launch
(ops/native/src/batch_splat.hip).

Parity with `SequenceDataLoader(collate='shared')` holds by construction:
the loader builds the very `SequenceDataset` objects the CPU loader builds
and takes the index tables, the per-item seed, the pause chain and the
augmentation draws from them; the splat arithmetic is the CPU dataset's bit
for bit.  The CPU loader stays and is the oracle
(tests/test_device_loader.py).

Limits: count maps only.  Noise injection, hot-pixel filtering, custom
resolutions, frames and the stack / voxel encodings are the CPU loader's;
asking for them here is a ValueError at construction.
"""

from __future__ import annotations

import bisect
import warnings

import numpy as np
import torch
from torch.utils.data import (BatchSampler, RandomSampler, SequentialSampler)
from torch.utils.data.distributed import DistributedSampler

from ..ops.native import get_ext
from ..parallel import is_distributed
from .loader import concatenate_datasets
from .sequence import SequenceDataset

__all__ = ["DeviceSequenceLoader", "batch_splat_torch", "pack_events",
           "FLAG_HFLIP", "FLAG_VFLIP", "FLAG_PFLIP", "FLAG_GT"]

FLAG_HFLIP, FLAG_VFLIP, FLAG_PFLIP, FLAG_GT = 1, 2, 4, 8

_COORD_BITS = 15
_COORD_MASK = (1 << _COORD_BITS) - 1
_SUPPORTED_FIELDS = {"inp_scaled_cnt", "gt_cnt"}
_DEFAULT_MAX_BYTES = 8 << 30


def pack_events(xs, ys, ps, name: str = "events") -> np.ndarray:
    """One int32 word per event: x in bits 0-14, y in bits 15-29, bit 31 set
    for polarity -1.  Raises ValueError naming `name` if a coordinate does
    not fit 15 bits or a polarity is not -1 or +1."""
    xs = np.asarray(xs)
    ys = np.asarray(ys)
    ps = np.asarray(ps)
    if xs.size and (int(xs.max()) > _COORD_MASK or int(ys.max()) > _COORD_MASK
                    or int(xs.min()) < 0 or int(ys.min()) < 0):
        raise ValueError(f"{name}: event coordinates must lie in "
                         f"[0, {1 << _COORD_BITS}) to be packed")
    if ps.size and not bool(np.all((ps == 1) | (ps == -1))):
        raise ValueError(f"{name}: event polarities must be -1 or +1")
    word = xs.astype(np.uint32) | (ys.astype(np.uint32) << _COORD_BITS) \
        | ((ps < 0).astype(np.uint32) << 31)
    return word.view(np.int32)


def batch_splat_torch(packed: torch.Tensor, jobs: torch.Tensor,
                      out: torch.Tensor, lrH: int, lrW: int) -> None:
    """Torch form of `evs_batch_splat`, same contract: for every row
    {begin, end, flags, reserved} of jobs int32 [J, 4], add the packed events
    begin..end into plane out[j] of out fp32 [J, 2, kH, kW], in place.

    An input job (flag bit 3 clear) is flipped on the (lrH, lrW) grid and
    mapped to the output grid by an fp32 divide and an fp32 multiply, as
    `normalize_events` and `scaled_count_encoding` do; a GT job (bit 3 set)
    is flipped on the output grid itself.  Pixels that fall outside the
    output grid are dropped.  Used on the CPU and when the extension is not
    built; it is the kernel's oracle."""
    J, kH, kW = out.size(0), out.size(2), out.size(3)
    E = packed.numel()
    rows = jobs.detach().cpu().tolist()
    begin = [min(max(r[0], 0), E) for r in rows]
    length = [max(min(r[1], E) - b, 0) for r, b in zip(rows, begin)]
    total = sum(length)
    if total == 0:
        return
    dev = packed.device
    lens = torch.tensor(length, device=dev)
    job = torch.repeat_interleave(torch.arange(J, device=dev), lens)
    starts = torch.cumsum(lens, 0) - lens
    idx = torch.arange(total, device=dev) - starts[job] \
        + torch.tensor(begin, device=dev)[job]
    word = packed[idx].long() & 0xFFFFFFFF
    flags = jobs[:, 2].to(dev).long()[job]
    gt = (flags & FLAG_GT) != 0
    x = word & _COORD_MASK
    y = (word >> _COORD_BITS) & _COORD_MASK
    neg = (word >> 31) != 0
    x = torch.where((flags & FLAG_HFLIP) != 0,
                    torch.where(gt, kW, lrW) - 1 - x, x)
    y = torch.where((flags & FLAG_VFLIP) != 0,
                    torch.where(gt, kH, lrH) - 1 - y, y)
    neg = neg ^ ((flags & FLAG_PFLIP) != 0)
    # two separately rounded fp32 operations, then truncation toward zero
    xs = (x.float() / lrW * kW).long()
    ys = (y.float() / lrH * kH).long()
    x = torch.where(gt, x, xs)
    y = torch.where(gt, y, ys)
    valid = (x >= 0) & (x < kW) & (y >= 0) & (y < kH)
    lin = ((job * 2 + neg.long()) * kH + y) * kW + x
    lin = lin[valid]
    out.view(-1).index_add_(0, lin, torch.ones(lin.numel(), device=dev))


def _unsupported(ds_cfg: dict) -> None:
    for key in ("add_noise", "hot_filter"):
        if (ds_cfg.get(key) or {}).get("enabled", False):
            raise ValueError(
                f"device_resident loader does not support dataset."
                f"{key}.enabled; use the CPU loader")
    if ds_cfg.get("custom_resolution") is not None:
        raise ValueError("device_resident loader does not support "
                         "dataset.custom_resolution; use the CPU loader")
    if ds_cfg.get("real_world_test", False):
        raise ValueError("device_resident loader does not support "
                         "dataset.real_world_test; use the CPU loader")
    fields = ds_cfg.get("fields")
    if fields is not None:
        extra = sorted(set(fields) - _SUPPORTED_FIELDS)
        if extra:
            raise ValueError(
                f"device_resident loader builds only "
                f"{sorted(_SUPPORTED_FIELDS)}; dataset.fields asks for "
                f"{extra}")


class DeviceSequenceLoader:
    """Iterable over training batches splatted on `device` from
    device-resident packed events.

    Each item is what `shared_sequence_collate` yields, minus `mid_step`:

        {"frames":  [B, L, 2, kH, kW] float32 on `device`,
         "gt_mids": [B, L-seqn+1, 2, kH, kW] float32 on `device`,
         "seqn": seqn}

    Both tensors are views of ONE static buffer that the next batch
    overwrites: they stay valid only until the next batch is requested.
    Clone what has to outlive that.

    `dataloader_config` is a `SequenceDataLoader` config; `num_workers`,
    `pin_memory` and `collate` are ignored.  `device_resident` may be a
    mapping with `max_bytes` (default 8 GiB), the most the packed events may
    take on the device.  `sampler` overrides the index sampler (any iterable
    of dataset indices with an optional `set_epoch`).
    """

    def __init__(self, dataloader_config: dict, device, sampler=None):
        cfg = dataloader_config
        ds_cfg = cfg["dataset"]
        _unsupported(ds_cfg)
        self.device = torch.device(device)
        self.dataset = concatenate_datasets(cfg["path_to_datalist_txt"],
                                            SequenceDataset, ds_cfg)
        seqs = self.dataset.datasets
        first = seqs[0]
        self.seqn = int(ds_cfg["sequence"]["seqn"])
        self.scale = ds_cfg["scale"]
        self.inp_sensor_resolution = first.inp_sensor_resolution
        self.gt_sensor_resolution = first.gt_sensor_resolution
        self.batch_size = int(cfg["batch_size"])
        self.L = first.L
        self.mid_idx = (self.seqn - 1) // 2
        self.n_windows = self.L - self.seqn + 1
        lrH, lrW = self.inp_sensor_resolution
        kH, kW = self.gt_sensor_resolution
        for s in seqs:
            if (s.L != self.L
                    or s.inp_sensor_resolution != self.inp_sensor_resolution
                    or s.gt_sensor_resolution != self.gt_sensor_resolution):
                raise ValueError(
                    f"{s.dataset.store.path}: sequence length or resolution "
                    f"differs from the first sequence's; a batch cannot mix "
                    f"them")
        if self.n_windows < 1:
            raise ValueError(f"sequence_length {self.L} is shorter than "
                             f"seqn {self.seqn}")
        if kH % lrH or kW % lrW or kH // lrH != kW // lrW:
            raise ValueError(
                f"device_resident loader needs the GT resolution {kH}x{kW} "
                f"to be a whole multiple of the input resolution "
                f"{lrH}x{lrW}")

        self._upload(seqs, cfg.get("device_resident"))

        # index order: the sampler objects a DataLoader would use
        if sampler is not None:
            self.dist_sampler = sampler \
                if isinstance(sampler, DistributedSampler) else None
        elif cfg.get("use_ddp", False) and is_distributed():
            sampler = DistributedSampler(self.dataset, shuffle=cfg["shuffle"])
            self.dist_sampler = sampler
        else:
            sampler = RandomSampler(self.dataset) if cfg["shuffle"] \
                else SequentialSampler(self.dataset)
            self.dist_sampler = None
        self.sampler = sampler
        self.batch_sampler = BatchSampler(sampler, self.batch_size,
                                          bool(cfg["drop_last"]))
        self.last_indices: list[int] = []

        # static device buffers; input jobs first, then GT jobs
        B = self.batch_size
        self._n_inp = B * self.L
        J = self._n_inp + B * self.n_windows
        self._out = torch.zeros(J, 2, kH, kW, device=self.device)
        self._jobs = torch.zeros(J, 4, dtype=torch.int32, device=self.device)
        on_gpu = self.device.type == "cuda"
        ext = get_ext() if on_gpu else None
        self._ext = ext if ext is not None \
            and hasattr(ext, "evs_batch_splat") else None
        if on_gpu and self._ext is None:
            warnings.warn(
                "DeviceSequenceLoader: the native evs_batch_splat kernel is "
                "not built (run `python -m esr_amd.ops.native.build`); using "
                "the torch splat", RuntimeWarning, stacklevel=2)
        # host staging, double-buffered: a block is rewritten only after the
        # copy that read it two batches ago has finished
        self._stage = [{"jobs": torch.zeros(J, 4, dtype=torch.int32,
                                            pin_memory=on_gpu),
                        "done": None} for _ in range(2)]
        self._tick = 0

    # ------------------------------------------------------------------
    def _upload(self, seqs, resident_cfg) -> None:
        """Pack and upload `inp_prefix` and `gt_prefix` of every sequence;
        record where each group starts and the longest window."""
        max_bytes = _DEFAULT_MAX_BYTES
        if isinstance(resident_cfg, dict):
            max_bytes = int(resident_cfg.get("max_bytes", _DEFAULT_MAX_BYTES))
        groups = []                      # (dataset, prefix) in upload order
        for s in seqs:
            d = s.dataset
            prefixes = [d.inp_prefix]
            if d.need_gt_events and d.gt_prefix != d.inp_prefix:
                prefixes.append(d.gt_prefix)
            groups += [(d, p) for p in prefixes]
        total = sum(d.store.num_events(p) for d, p in groups)
        need = 4 * total
        if need > max_bytes:
            raise ValueError(
                f"device_resident: the packed events need {need} bytes, "
                f"more than device_resident.max_bytes = {max_bytes}")
        if total > 2 ** 31 - 1:
            raise ValueError(
                f"device_resident: {total} events exceed the int32 row "
                f"index of the job table")

        packed = np.empty(total, dtype=np.int32)
        base = {}
        off = 0
        for d, p in groups:
            n = d.store.num_events(p)
            st = d.store
            packed[off:off + n] = pack_events(
                st._arr(f"{p}_xs")[:n], st._arr(f"{p}_ys")[:n],
                st._arr(f"{p}_ps")[:n], name=f"{st.path} [{p}]")
            base[(id(d), p)] = off
            off += n
        self._packed = torch.from_numpy(packed).to(self.device)
        self._inp_base = [base[(id(s.dataset), s.dataset.inp_prefix)]
                          for s in seqs]
        self._gt_base = [base[(id(s.dataset), s.dataset.gt_prefix)]
                         if s.dataset.need_gt_events else 0 for s in seqs]
        longest = 0
        for s in seqs:
            d = s.dataset
            spans = list(d.event_indices)
            if d.need_gt_events:
                spans += list(d.gt_event_indices)
            longest = max([longest] + [b - a for a, b in spans])
        self.max_job_len = int(longest)
        self.resident_bytes = need

    # ------------------------------------------------------------------
    def __len__(self):
        return len(self.batch_sampler)

    def set_epoch(self, epoch: int):
        """Advance the per-index augmentation seeds and the sampler's
        shuffle, as `SequenceDataLoader.set_epoch` does."""
        for s in self.dataset.datasets:
            s.set_epoch(epoch)
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    @staticmethod
    def _flip_flags(d, seed: int) -> int:
        """The flips `EventSRDataset._augment_events` applies for `seed`,
        read off its effect on one probe event on a 2x2 grid."""
        if not d.augment_cfg.get("enabled", False):
            return 0
        probe = np.array([[0.0], [0.0], [0.0], [1.0]])
        x, y, _, p = d._augment_events(probe, (2, 2), seed)[:, 0]
        return (FLAG_HFLIP if x != 0 else 0) | (FLAG_VFLIP if y != 0 else 0) \
            | (FLAG_PFLIP if p < 0 else 0)

    def job_table(self, indices) -> np.ndarray:
        """The int32 [J, 4] job table of one batch of dataset indices (host
        work only): rows {begin, end, flags, 0}; unused rows are empty."""
        table = np.zeros((self._jobs.size(0), 4), dtype=np.int32)
        cum = self.dataset.cumulative_sizes
        for b, index in enumerate(indices):
            k = bisect.bisect_right(cum, index)
            local = index - (cum[k - 1] if k else 0)
            s = self.dataset.datasets[k]
            d = s.dataset
            seed, steps = s.window_plan(local)
            flags = self._flip_flags(d, seed)
            for l, (w, paused) in enumerate(steps):
                if paused:
                    continue             # zero input: an empty job
                i0, i1 = d.event_indices[w]
                table[b * self.L + l] = (self._inp_base[k] + i0,
                                         self._inp_base[k] + max(i1, i0),
                                         flags, 0)
            if not d.need_gt_events:
                continue
            for n in range(self.n_windows):
                w, _ = steps[n + self.mid_idx]
                g0, g1 = d.gt_event_indices[w]
                table[self._n_inp + b * self.n_windows + n] = (
                    self._gt_base[k] + g0, self._gt_base[k] + max(g1, g0),
                    flags | FLAG_GT, 0)
        return table

    def _splat(self, zero: bool = True) -> None:
        lrH, lrW = self.inp_sensor_resolution
        if zero:
            self._out.zero_()
        if self._ext is not None:
            self._ext.evs_batch_splat(self._packed, self._jobs, self._out,
                                      lrH, lrW, self.max_job_len)
        else:
            batch_splat_torch(self._packed, self._jobs, self._out, lrH, lrW)

    def load(self, indices) -> dict:
        """Splat the batch made of these dataset indices."""
        indices = [int(i) for i in indices]
        if not 0 < len(indices) <= self.batch_size:
            raise ValueError(f"a batch holds 1..{self.batch_size} indices")
        table = self.job_table(indices)
        stage = self._stage[self._tick % 2]
        if stage["done"] is not None:
            stage["done"].synchronize()
        stage["jobs"].copy_(torch.from_numpy(table))
        self._tick += 1
        self._jobs.copy_(stage["jobs"], non_blocking=True)
        if self.device.type == "cuda":
            stage["done"] = torch.cuda.Event()
            stage["done"].record(torch.cuda.current_stream(self.device))
        self._splat()
        self.last_indices = indices
        B = len(indices)
        kH, kW = self.gt_sensor_resolution
        frames = self._out[:B * self.L].view(B, self.L, 2, kH, kW)
        gt_mids = self._out[self._n_inp:self._n_inp + B * self.n_windows] \
            .view(B, self.n_windows, 2, kH, kW)
        return {"frames": frames, "gt_mids": gt_mids, "seqn": self.seqn}

    def __iter__(self):
        for indices in self.batch_sampler:
            yield self.load(indices)
