"""EVS — the framework's on-disk event store.

The reference keeps each sequence in one HDF5 file with per-scale event
groups and an image group (schema:
ESR:generate_dataset/tools/event_packagers.py:119-224).  h5py is not part of
this environment, and HDF5 chunk decompression in dataloader workers is pure
CPU overhead for data this shape — an EVS sequence is a *directory* of raw
little-endian .npy arrays (memory-mapped on read; the OS page cache does the
work) plus a JSON metadata file:

    seq.evs/
      meta.json                  {"sensor_resolution": [H, W],
                                  "groups": {"ori": N, "down2": N2, ...},
                                  "num_images": M}
      <group>_xs.npy  (uint16)   event x coordinates
      <group>_ys.npy  (uint16)   event y coordinates
      <group>_ts.npy  (float64)  event timestamps (seconds, sorted)
      <group>_ps.npy  (int8)     event polarities in {-1, +1}
      images.npy      (uint8)    [M, H, W] frames (optional)
      image_ts.npy    (float64)  [M] frame timestamps (optional)

`EventStoreWriter.add_group` writes a group in one call;
`EventStoreWriter.open_group` streams one piece by piece (.npy headers written
last into a reserved region), for outputs that do not fit in host memory;
`EventStoreWriter.open_images` does the same for the frames.

Groups follow the reference's naming: 'ori', 'down2', 'down4', 'down8',
'down16' (and 'down8_real' for real-sensor captures).
"""

from __future__ import annotations

import json
import os
from pathlib import Path

import numpy as np

__all__ = ["EventStoreWriter", "EventStore", "GROUP_LEVELS"]

GROUP_LEVELS = {"ori": 1, "down2": 2, "down4": 4, "down8": 8, "down16": 16,
                "down8_real": 8}

_FIELDS = (("xs", np.uint16), ("ys", np.uint16), ("ts", np.float64), ("ps", np.int8))


class EventStoreWriter:
    """Creates an EVS sequence directory."""

    def __init__(self, path, sensor_resolution):
        self.path = Path(path)
        self.path.mkdir(parents=True, exist_ok=True)
        self.meta = {"sensor_resolution": [int(sensor_resolution[0]),
                                           int(sensor_resolution[1])],
                     "groups": {}, "num_images": 0}

    def add_group(self, prefix: str, xs, ys, ts, ps):
        n = len(ts)
        assert len(xs) == len(ys) == len(ps) == n
        for (name, dt), arr in zip(_FIELDS, (xs, ys, ts, ps)):
            np.save(self.path / f"{prefix}_{name}.npy",
                    np.asarray(arr).astype(dt, copy=False))
        self.meta["groups"][prefix] = int(n)

    def open_group(self, prefix: str) -> "GroupAppender":
        """A group written piece by piece (`append`, then `close`), for
        streams that do not fit in host memory.  The files read back exactly
        as `add_group`'s."""
        return GroupAppender(self, prefix)

    def add_images(self, images, timestamps):
        images = np.asarray(images, dtype=np.uint8)
        np.save(self.path / "images.npy", images)
        np.save(self.path / "image_ts.npy",
                np.asarray(timestamps, dtype=np.float64))
        self.meta["num_images"] = int(images.shape[0])

    def open_images(self, shape) -> "ImageAppender":
        """The frames of `add_images` written piece by piece (`append`, then
        `close`): uint8 frames of `shape` = (H, W), so a long video is never
        held at once.  The files read back exactly as `add_images`'s."""
        return ImageAppender(self, shape)

    def close(self):
        with open(self.path / "meta.json", "w") as f:
            json.dump(self.meta, f)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


_NPY_HEADER_BYTES = 128      # magic, version, length and a padded dict


def _npy_header(dtype, n: int, item_shape=()) -> bytes:
    """A version 1.0 .npy header of exactly _NPY_HEADER_BYTES bytes for a
    little-endian C-order array of `n` items of shape `item_shape` (1-D by
    default).  The format lets the dict be padded with spaces before its
    closing newline, so the size does not depend on `n` and the header can
    be written after the data."""
    descr = np.lib.format.dtype_to_descr(np.dtype(dtype))
    shape = "".join(f"{int(d)}, " for d in (n, *item_shape)).rstrip()
    text = (f"{{'descr': {descr!r}, 'fortran_order': False, "
            f"'shape': ({shape}), }}").encode("latin1")
    room = _NPY_HEADER_BYTES - 10
    if len(text) + 1 > room:
        raise ValueError("npy header does not fit its reserved region")
    text = text + b" " * (room - 1 - len(text)) + b"\n"
    return b"\x93NUMPY\x01\x00" + len(text).to_bytes(2, "little") + text


class GroupAppender:
    """Streams one event group to its four .npy files.  Each file starts
    with a reserved header region; `close` writes the headers, now that the
    length is known, and enters the group into the writer's metadata."""

    def __init__(self, writer: "EventStoreWriter", prefix: str):
        self.writer = writer
        self.prefix = prefix
        self.n = 0
        self._files = []
        for name, _ in _FIELDS:
            f = open(writer.path / f"{prefix}_{name}.npy", "wb")
            f.write(b"\x00" * _NPY_HEADER_BYTES)
            self._files.append(f)

    def append(self, xs, ys, ts, ps) -> None:
        n = len(ts)
        assert len(xs) == len(ys) == len(ps) == n
        for f, (_, dt), arr in zip(self._files, _FIELDS, (xs, ys, ts, ps)):
            a = np.ascontiguousarray(np.asarray(arr).astype(dt, copy=False))
            f.write(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes())
        self.n += n

    def close(self) -> None:
        if not self._files:
            return
        for f, (_, dt) in zip(self._files, _FIELDS):
            f.seek(0)
            f.write(_npy_header(np.dtype(dt).newbyteorder("<"), self.n))
            f.close()
        self._files = []
        self.writer.meta["groups"][self.prefix] = int(self.n)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ImageAppender:
    """Streams frames to images.npy and their timestamps to image_ts.npy in
    `GroupAppender`'s manner: reserved header regions, written on `close`."""

    def __init__(self, writer: "EventStoreWriter", shape):
        self.writer = writer
        self.shape = tuple(int(d) for d in shape)
        self.n = 0
        self._img = open(writer.path / "images.npy", "wb")
        self._ts = open(writer.path / "image_ts.npy", "wb")
        for f in (self._img, self._ts):
            f.write(b"\x00" * _NPY_HEADER_BYTES)

    def append(self, images, timestamps) -> None:
        images = np.ascontiguousarray(np.asarray(images, dtype=np.uint8))
        ts = np.ascontiguousarray(np.asarray(timestamps, dtype="<f8"))
        if images.shape[1:] != self.shape or ts.shape != images.shape[:1]:
            raise ValueError(
                f"expected frames [n, {self.shape[0]}, {self.shape[1]}] and "
                f"one timestamp each, got {images.shape} and {ts.shape}")
        self._img.write(images.tobytes())
        self._ts.write(ts.tobytes())
        self.n += images.shape[0]

    def close(self) -> None:
        if self._img is None:
            return
        self._img.seek(0)
        self._img.write(_npy_header(np.uint8, self.n, self.shape))
        self._ts.seek(0)
        self._ts.write(_npy_header(np.dtype("<f8"), self.n))
        self._img.close()
        self._ts.close()
        self._img = self._ts = None
        self.writer.meta["num_images"] = int(self.n)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class EventStore:
    """Read-only, memory-mapped view of an EVS sequence directory."""

    def __init__(self, path):
        self.path = Path(path)
        with open(self.path / "meta.json") as f:
            self.meta = json.load(f)
        self.sensor_resolution = list(self.meta["sensor_resolution"])
        self._mm: dict[str, np.ndarray] = {}

    @property
    def groups(self):
        return dict(self.meta["groups"])

    def _arr(self, name) -> np.ndarray:
        if name not in self._mm:
            self._mm[name] = np.load(self.path / f"{name}.npy", mmap_mode="r")
        return self._mm[name]

    def num_events(self, prefix: str) -> int:
        return int(self.meta["groups"][prefix])

    def ts(self, prefix: str) -> np.ndarray:
        return self._arr(f"{prefix}_ts")

    def events(self, prefix: str, idx0: int, idx1: int) -> np.ndarray:
        """Return a [4, n] float64 array (x, y, t, p) — the layout the
        event-formatting op expects (ESR:dataloader/h5dataset.py:492-498)."""
        sl = slice(idx0, idx1)
        xs = np.asarray(self._arr(f"{prefix}_xs")[sl], dtype=np.float64)
        ys = np.asarray(self._arr(f"{prefix}_ys")[sl], dtype=np.float64)
        ts = np.asarray(self._arr(f"{prefix}_ts")[sl], dtype=np.float64)
        ps = np.asarray(self._arr(f"{prefix}_ps")[sl], dtype=np.float64)
        return np.stack([xs, ys, ts, ps])

    @property
    def num_images(self) -> int:
        return int(self.meta.get("num_images", 0))

    def image(self, i: int) -> np.ndarray:
        return np.asarray(self._arr("images")[i])

    def image_ts(self) -> np.ndarray:
        return np.asarray(self._arr("image_ts"))


def is_event_store(path) -> bool:
    return os.path.isfile(os.path.join(path, "meta.json"))
