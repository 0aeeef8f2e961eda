"""The region-table entry points (csrc/regions.hip, docs/regions.md) at the size of a predictor batch: 32 maps of 224 x 224.

The measurement (cmdiad_region_measure) runs on the table of the same maps and a synthetic organised cloud.  Two inputs: a smooth field (Gaussian-filtered noise thresholded at its 0.97 quantile: a few dozen blobs per image, what score
maps look like) and the stride-2 lattice (12 544 one-pixel components per image: the component tables at capacity).  Every entry
point is timed by HIP events (median of --reps launches after a warm-up) and reported with the bytes its contract moves at least
once and the achieved bytes/s; `find_regions` is the whole call from a device tensor, read-back included (host clock).
Usage: python tools/bench_regions.py [--images 32] [--size 224] [--reps 20] [--regions 16] [--out FILE.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdiad_amd import ops, regions  # noqa: E402


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def inputs(kind, n, size):
    if kind == "smooth":
        maps = ndimage.gaussian_filter(np.random.RandomState(0).rand(n, size, size), sigma=(0, 4, 4))
        return maps, float(np.quantile(maps, 0.97))
    maps = np.zeros((n, size, size))
    maps[:, ::2, ::2] = 1.0 + np.random.RandomState(1).rand(n, (size + 1) // 2, (size + 1) // 2)
    return maps, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, S, K = a.images, a.size, a.regions
    px = n * S * S
    cap = n * ((S + 1) // 2) ** 2
    out, lines = dict(images=n, size=S, max_regions=K, inputs={}), []
    lines.append(f"| input | entry point | ms | MB moved at least once | GB/s |")
    lines.append("|---|---|---:|---:|---:|")
    for kind in ("smooth", "lattice"):
        host, thr_value = inputs(kind, n, S)
        maps = torch.from_numpy(host).to(dev)
        thr = torch.tensor([thr_value], dtype=torch.float64, device=dev)
        mask, _ = ops.threshold_mask(maps, thr)
        labels, n_comp, comp_offset, comp_size, _ = ops.ccl_label(mask)
        comps = int(comp_offset[-1])
        fg = int(mask.sum())
        spec = regions.RegionSpec(thr_value, None, 1, K)
        # the measurement's inputs: the table of these maps and a rough surface as their organised cloud, a tenth of it invalid
        count, ints, _ = ops.region_table(maps, labels, n_comp, comp_offset, comp_size, 1, K)
        rs = np.random.RandomState(2)
        yy, xx = np.mgrid[0:S, 0:S]
        cloud_host = np.stack([0.3 + xx * 0.01 + rs.randn(n, S, S) * 0.002, -0.2 + yy * 0.012 + rs.randn(n, S, S) * 0.002,
                               0.5 + rs.randn(n, S, S) * 0.02], 1).astype(np.float32)
        cloud_host[:, 2][rs.rand(n, S, S) < 0.1] = 0.0
        cloud = torch.from_numpy(cloud_host).to(dev)
        m_out = ops.region_measure(labels, count, ints, cloud)
        kept = torch.arange(K, device=dev)[None, :] < count.clamp(0, K)[:, None]
        box_px = int((((ints[..., 4] - ints[..., 2] + 1) * (ints[..., 5] - ints[..., 3] + 1)) * kept).sum())
        rows = [
            # name, callable, bytes the contract moves at least once
            ("cmdiad_threshold_mask", lambda: ops.threshold_mask(maps, thr), px * (8 + 1)),
            ("cmdiad_ccl_label (7 launches)", lambda: ops.ccl_label(mask), px * (1 + 4 * 2 * 4)),
            # two pixel passes read maps + labels; the tables are set (44 B per slot) and touched per component; the selection
            # reads key + size per component and round, and the kept regions' boxes
            ("cmdiad_region_table (4 launches)",
             lambda: ops.region_table(maps, labels, n_comp, comp_offset, comp_size, 1, K), 2 * px * 12 + cap * 44 + comps * 12),
            # the frames once for bad_count (12 B per point); label + point (16 B) of every box position of the kept regions; the
            # two tables written (16 + 160 B per slot)
            ("cmdiad_region_measure (2 launches)",
             lambda: ops.region_measure(labels, count, ints, cloud, out=m_out), px * 12 + box_px * 16 + n * K * 176),
        ]
        res = dict(threshold=thr_value, components=comps, foreground_pixels=fg, kept_box_pixels=box_px, kernels={})
        print(f"{kind}: {n} x {S} x {S}, {comps} components, {fg} foreground pixels")
        for name, fn, nbytes in rows:
            ms = event_ms(fn, a.reps)
            res["kernels"][name] = dict(ms=round(ms, 4), bytes=int(nbytes), gb_per_s=round(nbytes / ms / 1e6, 1))
            print(f"  {name:46s} {ms:8.3f} ms {nbytes / 1e6:9.1f} MB {nbytes / ms / 1e6:8.1f} GB/s")
            lines.append(f"| {kind} ({comps} components) | `{name}` | {ms:.3f} | {nbytes / 1e6:.1f} | {nbytes / ms / 1e6:.0f} |")

        def whole():
            t0 = time.perf_counter()
            regions.find_regions(maps, spec)
            return time.perf_counter() - t0
        whole()
        res["find_regions_ms"] = round(float(np.median([whole() for _ in range(a.reps)])) * 1e3, 3)
        print(f"  regions.find_regions, device tensor in, host tables out: {res['find_regions_ms']:.3f} ms (host clock, median)")
        lines.append(f"| {kind} | `regions.find_regions` (device maps in, host tables out; host clock) | {res['find_regions_ms']:.3f} | | |")

        def whole_measured():
            t0 = time.perf_counter()
            regions.find_regions(maps, spec, clouds=cloud)
            return time.perf_counter() - t0
        whole_measured()
        res["find_regions_clouds_ms"] = round(float(np.median([whole_measured() for _ in range(a.reps)])) * 1e3, 3)
        print(f"  regions.find_regions(clouds=), device tensors in, host tables out: {res['find_regions_clouds_ms']:.3f} ms (host clock, median)")
        lines.append(f"| {kind} | `regions.find_regions(clouds=)` (device maps and clouds in, host tables out; host clock) | "
                     f"{res['find_regions_clouds_ms']:.3f} | | |")
        out["inputs"][kind] = res
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
