#!/usr/bin/env python3
"""Microseconds and achieved GB/s of cmdiad_png_unfilter (csrc/png.hip, docs/png.md) beside torch's device-to-device copy of the same
bytes, and the one-wave baseline (waves=1) beside the multi-wave schedule the width selects.

  python tools/bench_png.py [--batch 16] [--size 800] [--launches 30] [--out profiles/png_kernel.json]

batch x (size x size x 3) 8-bit RGB files, their inflated scanlines resident on the device before the clock starts: one case per
forced filter type (None, Sub, Up, Average, Paeth: tests/png_ref.py filters the rows itself) and the mix Pillow's writer chooses for
the same picture.  Every case is checked once against the source picture, then every launch is timed by its own pair of HIP events
after 5 warm-up launches; the figure is the median, with min and max beside it.  The entry point is called directly (the binding's
host-side offset check is not inside the events).  Bytes = what the algorithm has to move: every scanline byte read once, every
pixel byte written once.  There is no pass / fail threshold: the figures go into profiles/png_decode.md.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from bench_tiff import per_launch_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image
    import png_ref as pg
    from cmdiad_amd import _native as nat
    from cmdiad_amd import ops
    from cmdiad_amd.utils import png
    if not torch.cuda.is_available():
        raise SystemExit("bench_png.py measures on the GPU; there is none here")
    B, S = args.batch, args.size
    src = pg.image(S, S, 3, seed=1, smooth=True)
    want = torch.from_numpy(src)
    rec = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "batch": B, "shape": [S, S, 3],
           "launches": args.launches, "cases": {}}
    cases = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "pillow_mix": None}
    fn = nat.lib().cmdiad_png_unfilter
    with tempfile.TemporaryDirectory() as root:
        path = os.path.join(root, "x.png")
        for name, ft in cases.items():
            if ft is None:
                Image.fromarray(src).save(path)
            else:
                pg.write(path, src, filters=ft, level=1)
            raw = png.read_raw(path, "rgb")
            lay, n = raw.layout, raw.data.size
            step = (n + 15) & ~15
            host = np.zeros(B * step, np.uint8)
            for b in range(B):
                host[b * step:b * step + n] = raw.data
            offsets = np.arange(B, dtype=np.int64) * step
            buf, tab = torch.from_numpy(host).cuda(), torch.from_numpy(offsets).cuda()
            moved = B * (n + src.nbytes)
            entry = {"filter_rows": np.bincount(raw.data[::1 + lay.row_bytes], minlength=5).tolist(), "bytes_moved": moved}
            for label, waves in (("waves_by_width", 0), ("one_wave", 1)):
                out = ops.png_unfilter(buf, [lay] * B, offsets, "rgb", offsets_dev=tab, waves=waves)      # (the checked call, once)
                assert all(torch.equal(out[b].cpu(), want) for b in (0, B - 1)), (name, label)
                a = (ops._p(buf), buf.numel(), ops._p(tab), B, lay.width, lay.height, lay.bpp, 0, waves, ops._p(out), ops._stream())
                us = per_launch_us(lambda: nat.check(fn(*a), "cmdiad_png_unfilter"), args.launches, torch)
                entry[label] = {"us": us, "GBps": round(moved / us["median"] / 1e3, 2)}
            rec["cases"][name] = entry
            del buf, tab
        flat = torch.from_numpy(host).cuda()
        dst = torch.empty_like(flat)
        us = per_launch_us(lambda: dst.copy_(flat), args.launches, torch)
        rec["torch_copy"] = {"us": us, "bytes_moved": 2 * flat.numel(), "GBps": round(2 * flat.numel() / us["median"] / 1e3, 1)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
