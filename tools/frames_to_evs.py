#!/usr/bin/env python3
"""Frames -> multi-scale EVS store: the reference's dataset generation
(ESR:generate_dataset/syn_nfs_rgb.py: simulate five scales from a folder of
frames, package them into one file), with the simulation on the device.

  python tools/frames_to_evs.py --frames clip/ --out clip.evs --fps 240
  python tools/frames_to_evs.py --frames clip.npy --out clip.evs \
      --timestamps ts.txt --cp 0.2 --cn 0.2 --device cpu
  python tools/frames_to_evs.py --data_root nfs/ --out data/nfs --fps 240

A directory is read in sorted order with PIL, one image at a time, and
converted to grey in [0, 1]; a .npy file holds [T, H, W] frames (uint8, or
floats in [0, 1]) and is memory-mapped.  --data_root processes every
sub-directory into OUT/<name>.evs and writes the train/valid datalists.
The thresholds used are printed and written into meta.json.
"""

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

IMAGE_SUFFIXES = {".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff"}


class ImageFolder:
    """A folder of images as a lazy sequence of grey float32 frames."""

    def __init__(self, root, resize=None):
        self.files = sorted(p for p in Path(root).iterdir()
                            if p.suffix.lower() in IMAGE_SUFFIXES)
        if not self.files:
            raise SystemExit(f"no images under {root}")
        self.resize = resize

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from PIL import Image
        with Image.open(self.files[i]) as im:
            im = im.convert("L")
            if self.resize is not None:
                im = im.resize((self.resize[1], self.resize[0]),
                               Image.BICUBIC)
            return np.asarray(im, dtype=np.float32) / 255.0


class ArrayFrames:
    """A [T, H, W] array or memmap as frames in [0, 1]."""

    def __init__(self, arr, resize=None):
        if arr.ndim != 3:
            raise SystemExit(f"expected [T, H, W] frames, got {arr.shape}")
        self.arr = arr
        self.resize = resize

    def __len__(self):
        return self.arr.shape[0]

    def __getitem__(self, i):
        fr = np.asarray(self.arr[i])
        fr = (fr.astype(np.float32) / 255.0 if fr.dtype == np.uint8
              else fr.astype(np.float64))
        if self.resize is not None:
            import torch
            import torch.nn.functional as F
            fr = F.interpolate(torch.from_numpy(fr).float()[None, None],
                               size=tuple(self.resize), mode="bicubic",
                               align_corners=False).clamp(0, 1)[0, 0].numpy()
        return fr


def open_frames(src, resize):
    src = Path(src)
    if src.is_dir():
        return ImageFolder(src, resize)
    return ArrayFrames(np.load(src, mmap_mode="r"), resize)


def convert(args, src, out):
    from esr_amd.data.simulate_device import frames_to_event_store_device
    frames = open_frames(src, args.resize)
    if args.timestamps:
        ts = np.loadtxt(args.timestamps, dtype=np.float64).reshape(-1)
    else:
        ts = np.arange(len(frames), dtype=np.float64) / args.fps
    frames_to_event_store_device(
        out, frames, ts, levels=tuple(args.levels), cp=args.cp, cn=args.cn,
        seed=args.seed, refractory=args.refractory,
        store_images=not args.no_images, device=args.device,
        frame_chunk=args.frame_chunk, max_chunk_events=args.max_chunk_events)
    meta = json.loads((Path(out) / "meta.json").read_text())
    cp, cn = meta["contrast_thresholds"]
    print(f"{out}: {len(frames)} frames, cp = {cp:.6g}, cn = {cn:.6g}, "
          f"events " + ", ".join(f"{g} {n}" for g, n in meta["groups"].items()))
    return str(out)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--frames", help="image directory or [T,H,W] .npy file")
    p.add_argument("--data_root", help="directory of image directories")
    p.add_argument("--out", required=True,
                   help="the store (seq.evs), or with --data_root the "
                        "directory of stores")
    p.add_argument("--fps", type=float)
    p.add_argument("--timestamps", help="text file, one timestamp per frame")
    p.add_argument("--resize", type=int, nargs=2, metavar=("H", "W"))
    p.add_argument("--levels", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    p.add_argument("--cp", type=float)
    p.add_argument("--cn", type=float)
    p.add_argument("--seed", type=int, default=0,
                   help="samples the thresholds when --cp/--cn are not given")
    p.add_argument("--refractory", type=float, default=1e-4)
    p.add_argument("--device", default=None, help="cuda:0 | cpu")
    p.add_argument("--frame_chunk", type=int, default=64)
    p.add_argument("--max_chunk_events", type=int, default=1 << 22)
    p.add_argument("--no_images", action="store_true")
    p.add_argument("--split", type=float, default=0.8,
                   help="train fraction of the --data_root datalists")
    args = p.parse_args(argv)

    if (args.frames is None) == (args.data_root is None):
        p.error("give one of --frames and --data_root")
    if (args.fps is None) == (args.timestamps is None):
        p.error("give one of --fps and --timestamps")
    if (args.cp is None) != (args.cn is None):
        p.error("give --cp and --cn together")
    if args.data_root and args.timestamps:
        p.error("--data_root takes --fps")
    if args.device is None:
        import torch
        args.device = "cuda:0" if torch.cuda.is_available() else "cpu"

    if args.frames:
        convert(args, args.frames, args.out)
        return
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    dirs = sorted(d for d in Path(args.data_root).iterdir() if d.is_dir())
    if not dirs:
        raise SystemExit(f"no sub-directories under {args.data_root}")
    seed = args.seed
    seqs = []
    for i, d in enumerate(dirs):
        args.seed = seed + i          # its own thresholds for each sequence
        seqs.append(convert(args, d, out / f"{d.name}.evs"))
    n_train = max(int(len(seqs) * args.split), 1)
    (out / "train_datalist.txt").write_text("\n".join(seqs[:n_train]) + "\n")
    (out / "valid_datalist.txt").write_text(
        "\n".join(seqs[n_train:] or seqs[-1:]) + "\n")
    print(f"{n_train} train / {len(seqs) - n_train} valid sequences")


if __name__ == "__main__":
    main()
