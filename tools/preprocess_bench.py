#!/usr/bin/env python3
"""Times scan preprocessing on synthetic 800 x 800 scans: the device path (cmdiad_amd/utils/preprocessing.py) and, on the same
scans, the CPU restatement (tests/preprocess_ref.py for the plane, scikit-learn's DBSCAN for the clusters).

  python tools/preprocess_bench.py [--scans 3] [--cpu-scans 1] [--out profiles/preprocess.json]
  python tools/preprocess_bench.py --reps 7 [--compare OLD_PREPROCESSING.py] [--loader [--readers N] [--tiff-device]] --cpu-scans 0

--reps N (>= 5 for a figure worth writing down): per-scan wall time of preprocess_on_device (device tensors in, synchronise at the
end) and of preprocess_arrays (numpy in, numpy out), N repetitions over the same scans, reported as min / median / max.  With
--compare FILE the preprocess_arrays of another version of cmdiad_amd/utils/preprocessing.py (for instance `git show
REV:cmdiad_amd/utils/preprocessing.py > FILE`) runs in the same process on the same scans, alternating with this one, and the two
outputs are compared.  --loader writes a synthetic class (20 train, 10 test scans of 800 x 800) and times draining train() and
test() of dataset.MVTec3DRawClass over it against MVTec3DClass('hip') over a copy cleaned by preprocess_dataset: the `load` seconds
of evaluate.ClassRun, i.e. what cleaning in the loader costs.  The scans are real TIFFs (written by `tifffile` when it is installed,
else by cmdiad_amd.utils.tiff); --tiff-device sets CMDIAD_TIFF_DEVICE=1 for both classes (docs/tiff.md), --readers their reader threads.

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
          "core_test": ("dbscan_core",), "union": ("dbscan_union",), "labels": ("dbscan_flatten", "dbscan_mark", "dbscan_label", "label_histogram"),
          "compaction": ("compact_count", "compact_scatter"), "keep_largest": ("cluster_winner", "cluster_keep")}


def make_scans(n, size=800):
    """size x size scans over 160 mm (800: 0.2 mm pitch, about 150 k object points) on a noisy background plane, satellites, specks."""
    import preprocess_ref as pr
    return [pr.make_scan(100 + i, H=size, W=size, pitch=0.16 / size) for i in range(n)]


def _spread(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 3), "median": round(ms[len(ms) // 2], 3), "max": round(ms[-1], 3), "n": len(ms)}


def _load_module(path):
    """Another version of cmdiad_amd/utils/preprocessing.py as a module of the same package (its relative imports resolve here)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("cmdiad_amd.utils._preprocessing_compared", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed_repetitions(mod, scans, reps, other=None):
    """ms per scan, `reps` times over all scans: preprocess_on_device, preprocess_arrays, and (alternating with it) other's."""
    import torch
    dev = [tuple(torch.from_numpy(s[k]).cuda() for k in ("pc", "rgb", "gt")) for s in scans]
    rec = {"on_device": [], "arrays": [], "arrays_compared": []}
    same = True
    for rep in range(reps + 1):                      # the first round is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d in dev:
            mod.preprocess_on_device(*d)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        outs = [mod.preprocess_arrays(s["pc"], s["rgb"], s["gt"]) for s in scans]
        t2 = time.perf_counter()
        if other is not None:
            olds = [other.preprocess_arrays(s["pc"], s["rgb"], s["gt"]) for s in scans]
            t3 = time.perf_counter()
            same = same and all(np.array_equal(a, b) for o, n in zip(olds, outs) for a, b in zip(o, n))
        if rep:
            rec["on_device"].append(1e3 * (t1 - t0) / len(scans))
            rec["arrays"].append(1e3 * (t2 - t1) / len(scans))
            if other is not None:
                rec["arrays_compared"].append(1e3 * (t3 - t2) / len(scans))
    out = {"ms_per_scan_preprocess_on_device": _spread(rec["on_device"]), "ms_per_scan_preprocess_arrays": _spread(rec["arrays"])}
    if other is not None:
        out["ms_per_scan_preprocess_arrays_compared"] = _spread(rec["arrays_compared"])
        out["outputs_equal_compared"] = bool(same)
    return out


def loader_seconds(mod, n_train=20, n_test=10, size=800, reps=3, readers=None, tiff_device=False):
    """Seconds to drain train() + test() (evaluate.ClassRun's `load`): the raw class against MVTec3DClass('hip') over the cleaned copy."""
    import shutil
    import tempfile
    import torch
    from PIL import Image
    import preprocess_ref as pr
    from cmdiad_amd import dataset as ds
    from cmdiad_amd import evaluate as ev
    try:
        import tifffile
    except ImportError:      # the project's own codec writes the same float32 TIFFs (and reads them back: utils/mvtec3d_util.py)
        from cmdiad_amd.utils import tiff as tifffile
    root = tempfile.mkdtemp(prefix="raw_mvtec_")
    try:
        raw, clean = os.path.join(root, "raw"), os.path.join(root, "clean")
        k = 0
        for sub, n, has_gt in (("train/good", n_train, False), ("test/good", n_test // 2, False), ("test/hole", n_test - n_test // 2, True)):
            base = os.path.join(raw, "bagel", sub)
            for d in ("rgb", "xyz", "gt")[:3 if has_gt else 2]:
                os.makedirs(os.path.join(base, d))
            for i in range(n):
                scan = pr.make_scan(200 + k, H=size, W=size, pitch=0.16 / size)
                k += 1
                tifffile.imwrite(os.path.join(base, "xyz", f"{i:03d}.tiff"), scan["pc"])
                Image.fromarray(scan["rgb"]).save(os.path.join(base, "rgb", f"{i:03d}.png"))
                if has_gt:
                    Image.fromarray(scan["gt"], "L").save(os.path.join(base, "gt", f"{i:03d}.png"))
        shutil.copytree(raw, clean)
        t0 = time.perf_counter()
        mod.preprocess_dataset(clean)
        rec = {"train": n_train, "test": n_test, "shape": [size, size], "preprocess_dataset_seconds": round(time.perf_counter() - t0, 3),
               "cloud_files": "tiff, written by " + tifffile.__name__, "tiff_device": bool(tiff_device), "readers": readers, "raw": [], "clean": []}
        if tiff_device:
            os.environ["CMDIAD_TIFF_DEVICE"] = "1"
        more = {} if readers is None else {"num_workers": readers}
        for rep in range(reps + 1):
            for tag, path, kind in (("raw", raw, ds.MVTec3DRawClass), ("clean", clean, ds.MVTec3DClass)):
                cls = kind(path, "bagel", ev.mtfi_args(dataset_path=path, img_process_method="hip", **more))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                items = list(cls.train()) + list(cls.test())
                torch.cuda.synchronize()
                if rep:
                    rec[tag].append(time.perf_counter() - t0)
                assert len(items) == n_train + n_test
        rec["raw_load_seconds"], rec["clean_load_seconds"] = _spread(rec.pop("raw")), _spread(rec.pop("clean"))
        return rec
    finally:
        os.environ.pop("CMDIAD_TIFF_DEVICE", None)
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=3)
    ap.add_argument("--cpu-scans", type=int, default=1)
    ap.add_argument("--cpu-size", type=int, default=400, help="side of the scans of the CPU comparison (scikit-learn's neighbour lists "
                    "of an 800 x 800 scan need more than 10 GB); the device is timed on the same scans next to it")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=0, help="repetitions of the wall-time comparison (0: skip it)")
    ap.add_argument("--compare", default=None, help="another version of cmdiad_amd/utils/preprocessing.py, timed alternately")
    ap.add_argument("--loader", action="store_true", help="time the raw class's loader against the cleaned tree's")
    ap.add_argument("--readers", type=int, default=None, help="reader threads of the --loader classes (default: the classes' own)")
    ap.add_argument("--tiff-device", action="store_true", help="CMDIAD_TIFF_DEVICE=1 for the --loader classes")
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
    if args.reps:
        rec["repetitions"] = timed_repetitions(mod, scans, args.reps, _load_module(args.compare) if args.compare else None)
    if args.loader:
        rec["loader"] = loader_seconds(mod, readers=args.readers, tiff_device=args.tiff_device)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for s in scans:
            mod.preprocess_arrays(s["pc"], s["rgb"], s["gt"])
        torch.cuda.synchronize()
    per = {k: 0.0 for k in STAGES}
    kernels = {}
    all_us, all_n = 0.0, 0
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        all_us, all_n = all_us + us, all_n + (ev.count if us else 0)
        for stage, tags in STAGES.items():
            if any(tag in ev.key for tag in tags):
                per[stage] += us / 1e3 / args.scans
                kernels[ev.key.split("::")[-1].split("(")[0]] = round(us / 1e3 / args.scans, 4)
    rec["device_kernel_ms_per_scan"] = {k: round(v, 4) for k, v in per.items()}
    rec["device_kernels_ms_per_scan"] = kernels
    rec["device_all_events_ms_per_scan"] = round(all_us / 1e3 / args.scans, 4)       # torch's copies, fills and memsets included
    rec["device_events_per_scan"] = round(all_n / args.scans, 1)
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
