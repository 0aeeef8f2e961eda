#!/usr/bin/env python3
"""Microseconds and achieved GB/s of cmdiad_tiff_unpack (csrc/tiff.hip, docs/tiff.md) beside torch's device-to-device copy of the
same bytes, the yardstick of a kernel that only moves bytes.

  python tools/bench_tiff.py [--batch 16] [--size 800] [--launches 30] [--out profiles/tiff_kernel.json]

batch x (size x size x 3 float32) files, little-endian, chunky, one strip each, resident on the device before the clock starts:
predictor 1 (a copy through the chunk table; also with 64-row strips, and big-endian in 64 x 64 tiles) and predictor 3 (libtiff's
floating-point predictor undone per row).  Every launch is timed by its own pair of HIP events after 5 warm-up launches; the
figure is the median, with min and max beside it.  The entry point is called directly (the binding's host-side table check is not
inside the events).  Bytes = what the algorithm has to move: every sample read once and written once.  There is no pass / fail
threshold: the figures go into profiles/tiff_decode.md.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def per_launch_us(fn, launches, torch):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs)
    return {"median": round(us[len(us) // 2], 2), "min": round(us[0], 2), "max": round(us[-1], 2), "n": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tiff_ref as tr
    from cmdiad_amd import _native as nat
    from cmdiad_amd import ops
    from cmdiad_amd.utils import tiff
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiff.py measures on the GPU; there is none here")
    B, S = args.batch, args.size
    src = tr.random_bits((S, S, 3), np.float32, seed=1)
    moved = 2 * B * src.nbytes
    rec = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "batch": B, "shape": [S, S, 3],
           "dtype": "float32", "bytes_moved": moved, "launches": args.launches, "cases": {}}
    want = torch.from_numpy(np.ascontiguousarray(src).view(np.int32))
    cases = {"predictor1_one_strip": dict(), "predictor1_strips_of_64_rows": dict(rows_per_strip=64, misalign=2),
             "predictor1_big_endian_tiles_64": dict(big_endian=True, tile=(64, 64), misalign=2),
             "predictor3_one_strip": dict(predictor=3), "predictor3_strips_of_64_rows": dict(predictor=3, rows_per_strip=64, misalign=2)}
    with tempfile.TemporaryDirectory() as root:
        path = os.path.join(root, "x.tiff")
        for name, kw in cases.items():
            tr.write(path, src, **kw)
            raw = tiff.read_raw(path)
            lay, n = raw.layout, raw.data.size
            step = (n + 15) & ~15
            host = np.zeros(B * step, np.uint8)
            table = np.empty((B, lay.n_chunks), np.int64)
            for b in range(B):
                host[b * step:b * step + n] = raw.data
                table[b] = lay.offsets + b * step
            buf, tab = torch.from_numpy(host).cuda(), torch.from_numpy(table).cuda()
            out = ops.tiff_unpack(buf, [lay] * B, table, table_dev=tab)          # (the checked call, once: the result must be the source)
            assert all(torch.equal(out[b].view(torch.int32).cpu(), want) for b in (0, B - 1)), name
            fn = nat.lib().cmdiad_tiff_unpack
            a = (ops._p(buf), buf.numel(), ops._p(tab), B, lay.n_chunks, lay.width, lay.height, lay.channels, lay.chunk_w, lay.chunk_h, int(lay.planar),
                 lay.bytes_per_sample, int(lay.big_endian), lay.predictor, ops._p(out), ops._stream())
            us = per_launch_us(lambda: nat.check(fn(*a), "cmdiad_tiff_unpack"), args.launches, torch)
            rec["cases"][name] = {"us": us, "GBps": round(moved / us["median"] / 1e3, 1), "row_bytes": lay.row_bytes, "chunks": lay.n_chunks}
            del buf, tab
        flat = out.reshape(-1)
        dst = torch.empty_like(flat)
        us = per_launch_us(lambda: dst.copy_(flat), args.launches, torch)
        rec["torch_copy"] = {"us": us, "GBps": round(moved / us["median"] / 1e3, 1)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
