#!/usr/bin/env python3
"""Scans per second of the Eyecandies depth-to-cloud path (docs/eyecandies.md): the kernel pair cmdiad_eyecandies_cloud ->
cmdiad_organized_pc_prep_f64 on resident inputs (HIP events), the whole chain from files this tool writes itself
(dataset.EyecandiesRawClass: PNG / yaml / pose decoding on reader threads, upload, the kernels), and the vectorised numpy
restatement of the same arithmetic (tests/eyecandies_ref.py) on the host cores.

  python tools/bench_eyecandies_prep.py [--batch 16] [--size 512] [--iters 20] [--files 48] [--out profiles/eyecandies_prep.json]

Per scan the cloud kernel reads 2 bytes and writes 24 (+1 for the removed mask) per pixel; the achieved bytes/s are reported against
that.  There is no pass / fail threshold: the figures go into profiles/eyecandies_prep.md.  Needs a GPU (no fallback)."""
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-scans", type=int, default=4)
    ap.add_argument("--files", type=int, default=48, help="train samples of the end-to-end tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import eyecandies_ref as er
    from cmdiad_amd import dataset as ds
    from cmdiad_amd import ops
    from cmdiad_amd.utils import preprocessing_eyecandies as pe
    if not torch.cuda.is_available():
        raise SystemExit("bench_eyecandies_prep.py measures on the GPU; there is none here")
    B, S = args.batch, args.size
    scans = [er.synthetic_scan(i, S, S) for i in range(B)]
    code = torch.from_numpy(np.stack([s[0] for s in scans])).cuda()
    prm = torch.stack([pe.scan_params(0.5, 3.1, s[1], S, S, s[2]) for s in scans]).cuda()
    prep = ds.SamplePrep(224, 224, 224, "cuda")
    t224 = (prep._table("torch", S, 224), prep._table("torch", S, 224))
    cloud_bytes = S * S * (2 + 24 + 1)
    prep_bytes = 224 * 224 * (24 + 8) + 2 * 3 * 224 * 224 * 4      # gathered doubles (a point costs a whole cache line: not counted) + outputs
    rec = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "batch": B,
           "shape": [S, S], "cloud_kernel_bytes_per_scan": cloud_bytes, "prep_kernel_bytes_per_scan": prep_bytes,
           "host_torch_threads": torch.get_num_threads()}

    def cloud_only():
        return ops.eyecandies_cloud(code, prm)

    def pair():
        cloud, _, _ = ops.eyecandies_cloud(code, prm)
        return ops.organized_pc_prep(cloud, t224, t224)

    for name, fn, nbytes in (("cloud_kernel", cloud_only, cloud_bytes), ("kernel_pair", pair, cloud_bytes + prep_bytes)):
        for _ in range(3):
            fn()
        ms = events_ms(fn, args.iters, torch)      # (includes the allocation of the outputs from torch's caching allocator)
        rec[name + "_ms_per_batch"] = ms
        rec[name + "_scans_per_s"] = B / ms * 1e3
        rec[name + "_GBps"] = B * nbytes / ms / 1e6

    # ---- the same arithmetic on the host: the vectorised numpy restatement + the host cloud transform, one scan at a time
    n = min(args.host_scans, B)
    t = time.perf_counter()
    for i in range(n):
        want = er.restate(scans[i][0], 0.5, 3.1, scans[i][1], scans[i][2])
        ds.host_cloud_transform(want["cloud"], 224)
    host_s = (time.perf_counter() - t) / n
    rec["host_numpy_ms_per_scan"] = host_s * 1e3
    rec["host_numpy_scans_per_s"] = 1.0 / host_s
    got = ops.eyecandies_cloud(code[:1], prm[:1])[0][0].cpu().numpy()
    rec["device_equals_restatement"] = bool(np.array_equal(got.view(np.uint64), er.restate(scans[0][0], 0.5, 3.1, scans[0][1], scans[0][2])["cloud"].view(np.uint64)))

    # ---- end to end from a raw tree: decode + upload + kernels + image / mask preparation
    with tempfile.TemporaryDirectory() as root:
        er.write_raw_tree(root, "CandyCane", n_train=args.files, n_test=1, bad=(), H=S, W=S, rgb_size=S)
        e2e = {}
        for readers in (1, 4, 16):
            a = types.SimpleNamespace(dataset_path=root, img_process_method="hip", num_workers=readers)
            cls = ds.EyecandiesRawClass(root, "CandyCane", a)
            for timed in (False, True):          # first pass: page cache, tables
                t = time.perf_counter()
                k = sum(1 for _ in cls.train())
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
            e2e[f"hip_readers_{readers}"] = k / dt
        rec["end_to_end_samples_per_s"] = e2e
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
