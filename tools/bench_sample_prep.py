#!/usr/bin/env python3
"""Samples per second of sample preparation (docs/sample_prep.md): the device path (cmdiad_amd.dataset.SamplePrep) against the host
'cpu_v1' composition (PIL + torch, one sample at a time, as the reference's dataset.py) on the SAME decoded arrays, and end to end
from files this tool writes itself.

  python tools/bench_sample_prep.py [--batch 32] [--size 800] [--iters 20] [--files 64] [--drains 1] [--tiff-device] [--png-device]
                                    [--out profiles/sample_prep.json]

  arrays      batch x (size x size x 3 uint8 + size x size x 3 float32), already decoded and in host memory.
              device: HIP events around prepare_batch (pinned staging, host-to-device copy, the four kernels, the count's copy back);
              kernels only: HIP events around the kernels on arrays that are already on the device;
              host: wall clock around the PIL + torch composition on this process's torch threads.
  end to end  PNG + cloud files -> prepared samples, through get_data_loader with 1, 4 and 16 reader threads ('hip') and through the
              host datasets in line ('cpu_v1').  Bounded by the host's PNG / tiff decode, not by the kernels.  The clouds are real
              TIFFs: written by `tifffile` when it is installed, else by cmdiad_amd.utils.tiff.  --tiff-device sets
              CMDIAD_TIFF_DEVICE=1 for the 'hip' loaders (the reader threads hand the files' bytes on, cmdiad_tiff_unpack
              unpacks them; docs/tiff.md); --png-device sets CMDIAD_PNG_DEVICE=1 (the reader threads inflate the PNGs,
              cmdiad_png_unfilter undoes their row filters; docs/png.md); --drains N times N drains per reader count and reports
              every one.
There is no pass / fail threshold: the figures go into profiles/sample_prep.md.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def bytes_per_sample(size, rgb_size=224, xyz_size=224):
    """(uploaded, written, what the kernels have to move): the upload is the whole decoded sample; the kernels read the whole image,
    write and re-read the 8-bit intermediate, GATHER 12 + 4 bytes per resized pixel from the cloud, and write the three outputs."""
    up = size * size * 3 + size * size * 12                                      # uint8 image + float32 cloud
    written = 3 * rgb_size * rgb_size * 4 + 3 * xyz_size * xyz_size * 4 + 3 * 224 * 224 * 4      # img, cloud, depth
    kernels = size * size * 3 + 2 * size * rgb_size * 3 + xyz_size * xyz_size * 12 + 224 * 224 * 4 + written
    return up, written, kernels


def events_ms(fn, iters, torch):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-samples", type=int, default=32)
    ap.add_argument("--files", type=int, default=64, help="samples of the end-to-end tree")
    ap.add_argument("--drains", type=int, default=1, help="timed drains of the end-to-end loader per reader count")
    ap.add_argument("--tiff-device", action="store_true", help="CMDIAD_TIFF_DEVICE=1 for the end-to-end 'hip' loaders")
    ap.add_argument("--png-device", action="store_true", help="CMDIAD_PNG_DEVICE=1 for the end-to-end 'hip' loaders")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image
    import sample_prep_ref as spr
    from cmdiad_amd import dataset as ds
    from cmdiad_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_prep.py measures on the GPU; there is none here")
    B, S = args.batch, args.size
    rgbs = [spr.image("random", S, S, seed=i) for i in range(B)]
    pcs = [spr.cloud(S, S, seed=100 + i) for i in range(B)]
    prep = ds.SamplePrep(224, 224, 224, "cuda")
    up, written, kbytes = bytes_per_sample(S)
    rec = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "batch": B, "shape": [S, S], "bytes_up_per_sample": up,
           "bytes_written_per_sample": written, "kernel_bytes_per_sample": kbytes, "host_torch_threads": torch.get_num_threads()}

    # ---- decoded arrays: device path (staging + copy + kernels)
    for _ in range(3):
        out = prep.prepare_batch(rgbs, pcs)
    ms = events_ms(lambda: prep.prepare_batch(rgbs, pcs), args.iters, torch)
    rec["device_ms_per_batch"] = ms
    rec["device_samples_per_s"] = B / ms * 1e3
    rec["device_upload_GBps"] = B * up / ms / 1e6

    # ---- kernels only, inputs resident
    rgb_dev = torch.from_numpy(np.stack(rgbs)).cuda()
    pc_dev = torch.from_numpy(np.stack(pcs)).cuda()
    tab = prep._table("bicubic", S, 224)
    norm = prep._table("norm", 256, 3)
    t224 = (prep._table("torch", S, 224), prep._table("torch", S, 224))

    def kernels():
        ops.resize_bicubic_u8(rgb_dev, 224, 224, tab, tab, norm)
        ops.organized_pc_prep(pc_dev, t224, t224)
    for _ in range(3):
        kernels()
    kms = events_ms(kernels, args.iters, torch)
    rec["kernels_ms_per_batch"] = kms
    rec["kernels_samples_per_s"] = B / kms * 1e3
    rec["kernels_GBps"] = B * kbytes / kms / 1e6      # bytes the algorithm needs over kernel time (a gathered point costs a whole cache line: not counted)

    # ---- the same arrays on the host: the 'cpu_v1' composition, one sample at a time
    n = min(args.host_samples, B)
    t = time.perf_counter()
    for i in range(n):
        img = ds.host_rgb_transform(Image.fromarray(rgbs[i]), 224)
        cloud, depth = ds.host_cloud_transform(pcs[i], 224)
        np.count_nonzero(np.all(cloud.numpy().reshape(3, -1) != 0, axis=0))
    host_s = (time.perf_counter() - t) / n
    rec["host_ms_per_sample"] = host_s * 1e3
    rec["host_samples_per_s"] = 1.0 / host_s
    same = torch.equal(out[0][0][0].cpu(), ds.host_rgb_transform(Image.fromarray(rgbs[0]), 224)) and \
        torch.equal(out[0][0][1].cpu(), ds.host_cloud_transform(pcs[0], 224)[0])
    rec["device_equals_host"] = bool(same)

    # ---- end to end from files
    with tempfile.TemporaryDirectory() as root:
        base = os.path.join(root, "bagel", "train", "good")
        os.makedirs(os.path.join(base, "rgb"))
        os.makedirs(os.path.join(base, "xyz"))
        try:
            import tifffile
        except ImportError:
            from cmdiad_amd.utils import tiff as tifffile
        rec["cloud_files"] = "tiff, written by " + tifffile.__name__
        rec["tiff_device"] = bool(args.tiff_device)
        rec["png_device"] = bool(args.png_device)
        if args.tiff_device:
            os.environ["CMDIAD_TIFF_DEVICE"] = "1"
        if args.png_device:
            os.environ["CMDIAD_PNG_DEVICE"] = "1"
        for i in range(args.files):
            pc, rgb = spr.scan(i, S)
            Image.fromarray(rgb).save(os.path.join(base, "rgb", f"{i:03d}.png"))
            tifffile.imwrite(os.path.join(base, "xyz", f"{i:03d}.tiff"), pc)
        e2e, drains = {}, {}
        for readers in (1, 4, 16):
            a = types.SimpleNamespace(dataset_path=root, img_process_method="hip", num_workers=readers)
            rates = []
            for timed in range(1 + max(1, args.drains)):          # first pass: page cache, tables
                t = time.perf_counter()
                k = sum(1 for _ in ds.get_data_loader("train", "bagel", 224, 224, 224, a))
                torch.cuda.synchronize()
                if timed:
                    rates.append(k / (time.perf_counter() - t))
            e2e[f"hip_readers_{readers}"] = sorted(rates)[len(rates) // 2]
            drains[f"hip_readers_{readers}"] = [round(r, 1) for r in rates]
        os.environ.pop("CMDIAD_TIFF_DEVICE", None)
        os.environ.pop("CMDIAD_PNG_DEVICE", None)
        rec["end_to_end_drains_samples_per_s"] = drains
        host_ds = ds.TrainDataset("bagel", 224, 224, 224, root, "cpu_v1")
        t = time.perf_counter()
        for i in range(min(16, len(host_ds))):
            host_ds[i]
        e2e["cpu_v1_in_line"] = min(16, len(host_ds)) / (time.perf_counter() - t)
        rec["end_to_end_samples_per_s"] = e2e
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
