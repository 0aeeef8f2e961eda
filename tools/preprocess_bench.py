#!/usr/bin/env python3
"""Times scan preprocessing on synthetic 800 x 800 scans: the device path (cmdiad_amd/utils/preprocessing.py) and, on the same
scans, the CPU restatement (tests/preprocess_ref.py for the plane, scikit-learn's DBSCAN for the clusters).

  python tools/preprocess_bench.py [--scans 3] [--cpu-scans 1] [--out profiles/preprocess.json]

Device numbers: milliseconds per scan end to end (numpy in, numpy out) and per stage from the kernel times of torch.profiler --
plane (hypotheses + refit + mask), grid build (bounding box, keys, scans, scatter), core test, union, labels (flatten, mark,
label, histogram).  The CPU side runs on as many threads as the host gives scikit-learn (n_jobs=-1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

STAGES = {"plane": ("plane_hypothesis", "plane_refit", "plane_mask"), "grid_build": ("dbscan_bbox", "dbscan_grid", "dbscan_key", "scan_exclusive", "dbscan_scatter"),
          "core_test": ("dbscan_core",), "union": ("dbscan_union",), "labels": ("dbscan_flatten", "dbscan_mark", "dbscan_label", "label_histogram")}


def make_scans(n, size=800):
    """size x size scans over 160 mm (800: 0.2 mm pitch, about 150 k object points) on a noisy background plane, satellites, specks."""
    import preprocess_ref as pr
    return [pr.make_scan(100 + i, H=size, W=size, pitch=0.16 / size) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=3)
    ap.add_argument("--cpu-scans", type=int, default=1)
    ap.add_argument("--cpu-size", type=int, default=400, help="side of the scans of the CPU comparison (scikit-learn's neighbour lists "
                    "of an 800 x 800 scan need more than 10 GB); the device is timed on the same scans next to it")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import preprocess_ref as pr
    from cmdiad_amd.utils import preprocessing as mod
    scans = make_scans(args.scans)
    mod.preprocess_arrays(scans[0]["pc"], scans[0]["rgb"])          # warm-up: library load, allocator
    torch.cuda.synchronize()
    t = time.perf_counter()
    outs = [mod.preprocess_arrays(s["pc"], s["rgb"], s["gt"]) for s in scans]
    torch.cuda.synchronize()
    rec = {"scans": args.scans, "shape": [800, 800], "device": torch.cuda.get_device_name(0),
           "device_ms_per_scan_end_to_end": 1e3 * (time.perf_counter() - t) / args.scans,
           "points_after_plane_removal": [int(np.all(mod.pad_cropped_pc(pr.remove_plane(s["pc"], s["rgb"], s["plane"])[0]) != 0, axis=2).sum()) for s in scans[:1]]}
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for s in scans:
            mod.preprocess_arrays(s["pc"], s["rgb"], s["gt"])
        torch.cuda.synchronize()
    per = {k: 0.0 for k in STAGES}
    kernels = {}
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        for stage, tags in STAGES.items():
            if any(tag in ev.key for tag in tags):
                per[stage] += us / 1e3 / args.scans
                kernels[ev.key.split("::")[-1].split("(")[0]] = round(us / 1e3 / args.scans, 4)
    rec["device_kernel_ms_per_scan"] = {k: round(v, 4) for k, v in per.items()}
    rec["device_kernels_ms_per_scan"] = kernels
    # CPU: the restatement of the plane stage + scikit-learn's DBSCAN, the same glue
    from sklearn.cluster import DBSCAN
    cpu = {"plane": 0.0, "dbscan": 0.0, "total": 0.0}
    same = True
    small = make_scans(args.cpu_scans, args.cpu_size)
    torch.cuda.synchronize()
    t = time.perf_counter()
    small_outs = [mod.preprocess_arrays(s["pc"], s["rgb"]) for s in small]
    rec["cpu_size"] = args.cpu_size
    rec["device_ms_per_scan_end_to_end_at_cpu_size"] = 1e3 * (time.perf_counter() - t) / max(args.cpu_scans, 1)
    for s, o in zip(small, small_outs):
        t0 = time.perf_counter()
        plane = pr.plane_ransac(pr.get_edges(s["pc"]))[0]
        t1 = time.perf_counter()
        pc, rgb = pr.remove_plane(s["pc"], s["rgb"], plane)
        t2 = time.perf_counter()
        pc, rgb = pr.keep_largest(pr.pad_square(pc), pr.pad_square(rgb),
                                  lambda p: DBSCAN(eps=0.006, min_samples=30, n_jobs=-1).fit(p.astype(np.float64)).labels_)
        t3 = time.perf_counter()
        cpu["plane"] += 1e3 * (t1 - t0) / args.cpu_scans
        cpu["dbscan"] += 1e3 * (t3 - t2) / args.cpu_scans
        cpu["total"] += 1e3 * (t3 - t0) / args.cpu_scans
        same = same and np.array_equal(pc, o[0]) and np.array_equal(rgb, o[1])
    rec["cpu_ms_per_scan"] = {k: round(v, 1) for k, v in cpu.items()}
    rec["cpu_threads"] = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    rec["cpu_scans"] = args.cpu_scans
    rec["device_output_equals_cpu_output"] = bool(same) if args.cpu_scans else None
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
