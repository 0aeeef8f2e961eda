"""The three entry points of csrc/organize.hip (docs/organize.md) at the size of a batch of scans, 32 clouds of 500 000 points onto
448 x 448 with fill = 1, and of one dense scan, 4 M points onto 1024 x 1024: a surface with a smooth relief, sampled uniformly,
with colours and labels, through the orthographic camera that fit_orthographic gives it.

Kernels are timed by HIP events (median of --reps calls after a warm-up) and reported in ms and points/s beside the bytes their
contract moves at least once -- bounds: the points read; splat: the points read, the key map written once and pixel_of_point
written, plus one 8-byte atomic per placed point; resolve: the key map read, index, xyz, rgb and mask written, and the winners'
point, colour and label gathered.
Usage: python tools/bench_organize.py [--reps 20] [--out FILE.md]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd import organize as og  # noqa: E402

from bench_overlay import event_ms  # noqa: E402


def surface(n, per_cloud, dev, seed=0):
    """points [n per_cloud, 3] f32 (x, y uniform over 100 x 100, z a relief about 300; 1 % zeroed), colours, labels"""
    g = torch.Generator(device=dev).manual_seed(seed)
    P = n * per_cloud
    xy = 5.0 + 100.0 * torch.rand((P, 2), generator=g, device=dev)
    z = 300.0 + 4.0 * torch.sin(0.05 * xy[:, 0]) * torch.cos(0.04 * xy[:, 1]) + 0.5 * torch.rand((P,), generator=g, device=dev)
    pts = torch.cat([xy, z[:, None]], dim=1).contiguous()
    pts[torch.rand((P,), generator=g, device=dev) < 0.01] = 0
    colors = torch.randint(0, 256, (P, 3), generator=g, device=dev, dtype=torch.uint8)
    labels = (torch.rand((P,), generator=g, device=dev) < 0.05).to(torch.uint8)
    return pts, colors, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(kernels={})
    lines = ["| entry point | case | ms | M points/s | MB moved at least once | GB/s |", "|---|---|---:|---:|---:|---:|"]
    for n, per_cloud, S, fill in ((32, 500_000, 448, 1), (1, 4_000_000, 1024, 1)):
        pts, colors, labels = surface(n, per_cloud, dev)
        P, lengths = n * per_cloud, [per_cloud] * n
        case = f"{n} x {per_cloud} points -> {S}^2, fill {fill}"
        cams = og.fit_orthographic(pts, lengths, S, S, margin=1)
        kind, cam_rows = og._cams(cams, n, dev, "bench")
        offsets = og._offsets(lengths, dev)
        b_out = ops.cloud_bounds(pts, offsets, cam_rows, per_cloud)
        s_out = ops.organize_splat(pts, offsets, cam_rows, per_cloud, kind, S, S)
        r_out = ops.organize_resolve(pts, offsets, s_out[0], s_out[2], fill, colors, labels)
        stats = s_out[2].cpu().numpy()
        placed, won = P - int(stats[:, :2].sum()), int(stats[:, 2:].sum())
        px = n * S * S
        jobs = (("cmdiad_cloud_bounds", lambda: ops.cloud_bounds(pts, offsets, cam_rows, per_cloud, out=b_out), P * 12),
                ("cmdiad_organize_splat", lambda: ops.organize_splat(pts, offsets, cam_rows, per_cloud, kind, S, S, out=s_out),
                 P * 12 + px * 8 + P * 4 + placed * 8),
                ("cmdiad_organize_resolve", lambda: ops.organize_resolve(pts, offsets, s_out[0], s_out[2], fill, colors, labels, out=r_out),
                 px * (8 + 4 + 12 + 3 + 1) + won * (12 + 3 + 1)))
        for name, fn, nbytes in jobs:
            ms = event_ms(fn, a.reps)
            out["kernels"][f"{name} {case}"] = dict(ms=round(ms, 4), points_per_s=round(P / ms * 1e3), bytes=int(nbytes),
                                                    gb_per_s=round(nbytes / ms / 1e6, 1))
            print(f"  {name:24s} {case:44s} {ms:8.3f} ms {P / ms / 1e3:9.1f} M points/s {nbytes / 1e6:8.1f} MB {nbytes / ms / 1e6:8.1f} GB/s",
                  flush=True)
            lines.append(f"| `{name}` | {case} | {ms:.3f} | {P / ms / 1e3:.0f} | {nbytes / 1e6:.1f} | {nbytes / ms / 1e6:.0f} |")
        out.setdefault("counts", {})[case] = dict(points=P, placed=placed, direct=int(stats[:, 2].sum()), filled=int(stats[:, 3].sum()), pixels=px)
        del pts, colors, labels, b_out, s_out, r_out
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
