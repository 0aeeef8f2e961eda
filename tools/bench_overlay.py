"""The overlay entry points (csrc/overlay.hip, csrc/png.hip: cmdiad_png_filter; docs/overlay.md) at the size of a predictor batch:
32 maps of 224 x 224 rendered to 224 x 224 and to 800 x 800.

Kernels are timed by HIP events (median of --reps launches after a warm-up) and reported with the bytes their contract moves at least
once (render: the maps read once + the canvas written, + the background where there is one; filter: the image read + the scanlines
written) and the achieved bytes/s.  The host side -- zlib.compress per image at levels 1, 6 and 9 under filter 0 and under the adaptive
filter, and png.write_many of the batch -- is timed on the host clock.  --class_run adds the `overlays` phase of evaluate.ClassRun
beside `predict` on a small synthetic class.
Usage: python tools/bench_overlay.py [--images 32] [--reps 20] [--out FILE.md] [--class_run]"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdiad_amd import ops, overlay  # noqa: E402
from cmdiad_amd.utils import png  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--class_run", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, S = a.images, 224
    rs = np.random.RandomState(0)
    host = ndimage.gaussian_filter(rs.rand(n, S, S), sigma=(0, 4, 4))
    host = (host - host.min()) / (host.max() - host.min())
    thr_value = float(np.quantile(host, 0.97))
    maps = torch.from_numpy(host).to(dev)
    thr = torch.tensor([thr_value], dtype=torch.float64, device=dev)
    count, ints = (torch.full((n,), 16, dtype=torch.int32, device=dev),
                   torch.from_numpy(np.tile(np.array([[1, 9, 16 * j % 200, 13 * j % 200, 16 * j % 200 + 20, 13 * j % 200 + 20, 0, 0] for j in range(16)],
                                                      dtype=np.int32), (n, 1, 1))).to(dev))
    spec = overlay.OverlaySpec(0.0, 1.0)
    ds = overlay.DeviceSpec(spec, n, dev)
    out, lines = dict(images=n, kernels={}, host={}), ["| entry point | case | ms | MB moved at least once | GB/s |", "|---|---|---:|---:|---:|"]

    def row(name, case, fn, nbytes):
        ms = event_ms(fn, a.reps)
        out["kernels"][f"{name} {case}"] = dict(ms=round(ms, 4), bytes=int(nbytes), gb_per_s=round(nbytes / ms / 1e6, 1))
        print(f"  {name:24s} {case:44s} {ms:8.3f} ms {nbytes / 1e6:8.1f} MB {nbytes / ms / 1e6:8.1f} GB/s")
        lines.append(f"| `{name}` | {case} | {ms:.3f} | {nbytes / 1e6:.1f} | {nbytes / ms / 1e6:.0f} |")

    canvases = {}
    for So in (224, 800):
        canvas = torch.empty((n, So, So, 3), dtype=torch.uint8, device=dev)
        nan = torch.zeros((1,), dtype=torch.int32, device=dev)
        # a background with structure at the scale of a photograph's (noise would make every canvas incompressible): coarse noise,
        # enlarged, plus a little pixel noise
        bg = torch.nn.functional.interpolate(torch.randn((n, 3, So // 16, So // 16), device=dev), size=(So, So), mode="bicubic")
        bg = (bg + 0.02 * torch.randn_like(bg)).contiguous()
        base = n * S * S * 8 + n * So * So * 3

        def render(thr=None, tab=(None, None), bg=None):
            return ops.overlay_render(maps, ds.lohi, ds.lut, ds.alpha, size=(So, So), thr=thr, background=bg, count=tab[0], ints=tab[1],
                                      canvas=canvas, nan_count=nan)
        row("cmdiad_overlay_render", f"{n} x 224^2 -> {So}^2 plain", lambda: render(), base)
        row("cmdiad_overlay_render", f"{n} x 224^2 -> {So}^2 contour", lambda: render(thr), base)
        row("cmdiad_overlay_render", f"{n} x 224^2 -> {So}^2 contour + 16 boxes", lambda: render(thr, (count, ints)), base)
        row("cmdiad_overlay_render", f"{n} x 224^2 -> {So}^2 contour + 16 boxes over float32 rgb", lambda: render(thr, (count, ints), bg),
            base + n * So * So * 12)
        canvases[So] = canvas.clone()
        lines_dev = torch.empty((n, So * (1 + So * 3)), dtype=torch.uint8, device=dev)
        for mode in ("none", "adaptive"):
            row("cmdiad_png_filter", f"{n} x {So}^2 x 3 {mode}", lambda: ops.png_filter(canvases[So], mode, out=lines_dev),
                n * So * So * 3 + lines_dev.numel())

    lines += ["", "| canvas | filter | zlib level | bytes per image | zlib.compress ms per image | write_many images/s |", "|---|---|---:|---:|---:|---:|"]
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"{i}.png") for i in range(n)]
        for So in (224, 800):
            for mode in ("none", "adaptive"):
                scan = ops.png_filter(canvases[So], mode).cpu().numpy()
                for level in (1, 6, 9):
                    t0 = time.perf_counter()
                    sizes = [len(zlib.compress(memoryview(r), level)) for r in scan]
                    ms = (time.perf_counter() - t0) * 1e3 / n
                    png.write_many(paths, canvases[So], level=level, mode=mode)
                    t0 = time.perf_counter()
                    png.write_many(paths, canvases[So], level=level, mode=mode)
                    per_s = n / (time.perf_counter() - t0)
                    out["host"][f"{So} {mode} level {level}"] = dict(bytes_per_image=int(np.mean(sizes)), compress_ms=round(ms, 3),
                                                                     write_many_images_per_s=round(per_s, 1))
                    print(f"  {So}^2 {mode:8s} level {level}: {int(np.mean(sizes)):8d} B/image, zlib.compress {ms:7.3f} ms/image, "
                          f"write_many {per_s:7.1f} images/s")
                    lines.append(f"| {So}^2 | {mode} | {level} | {int(np.mean(sizes))} | {ms:.2f} | {per_s:.0f} |")
        if a.class_run:
            from cmdiad_amd import evaluate as ev
            from cmdiad_amd.models.hallucination_network import HallucinationCrossModalityNetwork
            from cmdiad_amd.models.models import PointTransformer, VisionTransformer
            from cmdiad_amd.synth import SyntheticClass, sharpen_pointmae
            os.environ.setdefault("CMDIAD_ALLOW_RANDOM_INIT", "1")    # synthetic weights, as bench.py's class loop
            torch.manual_seed(0)
            weights = ({k: v.detach() for k, v in VisionTransformer().state_dict().items()},
                       sharpen_pointmae({k: v.detach() for k, v in PointTransformer().state_dict().items()}),
                       {k: v.detach() for k, v in HallucinationCrossModalityNetwork(None, 768, 768).state_dict().items()})
            res = ev.run_class(ev.mtfi_args(f_coreset=0.1, random_state=3, calibration_holdout=2, overlay_dir=os.path.join(tmp, "ov")),
                               SyntheticClass("rope", 6, 20, index=8), weights=weights)
            out["class_run"] = {k: res["seconds"].get(k) for k in ("predict", "metrics", "overlays")}
            out["class_run"]["files"] = res["overlays"]["files"]
            print(f"  ClassRun (20 test images): {out['class_run']}")
            lines += ["", f"ClassRun, synthetic class with 20 test images: predict {res['seconds']['predict']} s, overlays "
                      f"{res['seconds']['overlays']} s ({res['overlays']['files']} files)"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
