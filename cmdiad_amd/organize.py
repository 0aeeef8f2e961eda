"""Unordered point clouds into the pixel grid the rest of the package works on (docs/organize.md): the inverse of
``ops.unorganize``.  A list of points -- with optional colours and per-point defect labels -- is projected through a camera onto an
H x W grid, the nearest point wins each pixel (csrc/organize.hip), and what comes out is what the two datasets deliver: the
organised cloud, the rgb image and the ground-truth mask in the layouts ``SamplePrep.prepare_device_clouds / _images / _masks`` take,
plus the point-to-pixel maps that carry a score map back onto every point.

    cams = fit_orthographic(points, lengths, 448, 448, margin=1)          # or Camera.pinhole(fx, fy, cx, cy), one or one per cloud
    org = organize(points, lengths, cams, 448, 448, fill=1, colors=colors, labels=labels)
    per_point = scores_to_points(score_maps, org)

``python -m cmdiad_amd.organize --src TREE --dst TREE`` writes a tree of PLY scans (dataset.PointCloudClass's layout) as a tree in
MVTec 3D-AD's layout.  Opt-in: nothing on the default path calls this module.
"""
import math
from typing import NamedTuple

import torch

KIND_ORTHOGRAPHIC, KIND_PINHOLE = 0, 1
_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _transform(T):
    """None (identity), or 3 x 4 / 4 x 4 nested sequences (or an array) -> the 12 row-major floats of the 3 x 4 transform"""
    if T is None:
        return _IDENTITY
    rows = [list(map(float, r)) for r in (T.tolist() if hasattr(T, "tolist") else T)]
    if len(rows) not in (3, 4) or any(len(r) != 4 for r in rows):
        raise ValueError(f"Camera: T must be 3 x 4 or 4 x 4, got {len(rows)} rows of {[len(r) for r in rows]}")
    return tuple(v for r in rows[:3] for v in r)


class Camera(NamedTuple):
    """kind (0 orthographic, 1 pinhole), the row-major 3 x 4 transform into the camera frame, and a, b, c, d: x0, y0, sx, sy of an
    orthographic camera (pixel (u, v) = ((c0 - x0) sx, (c1 - y0) sy)), fx, fy, cx, cy of a pinhole one."""
    kind: int
    T: tuple
    params: tuple

    @classmethod
    def orthographic(cls, x0, y0, pitch, pitch_y=None, T=None):
        """Pixel (0, 0)'s centre at camera coordinates (x0, y0), pixels `pitch` apart (`pitch_y` down the rows, default the same)."""
        pitch, pitch_y = float(pitch), float(pitch if pitch_y is None else pitch_y)
        if not (pitch > 0 and pitch_y > 0 and math.isfinite(pitch) and math.isfinite(pitch_y)):
            raise ValueError(f"Camera.orthographic: pitch = {pitch}, pitch_y = {pitch_y} must be positive and finite")
        return cls(KIND_ORTHOGRAPHIC, _transform(T), (float(x0), float(y0), 1.0 / pitch, 1.0 / pitch_y))

    @classmethod
    def pinhole(cls, fx, fy, cx, cy, T=None):
        return cls(KIND_PINHOLE, _transform(T), (float(fx), float(fy), float(cx), float(cy)))

    def row(self):
        """the 16 float64 of this camera's row of `cams`"""
        return list(self.T) + list(self.params)


class Organized(NamedTuple):
    """xyz [n,H,W,3] f32, index [n,H,W] i32 (the winner's index in its cloud, -1: empty), rgb [n,H,W,3] u8, mask [n,H,W] u8 (255:
    defect), pixel_of_point [P] i32 (-2 dropped, -1 outside, else the point's own pixel), keys [n,H,W] i64 (the key map's bits), stats
    [n,4] i32 (dropped, outside, direct, filled) -- all on the device -- and lengths, the clouds' point counts (a tuple of ints)."""
    xyz: torch.Tensor
    index: torch.Tensor
    rgb: torch.Tensor
    mask: torch.Tensor
    pixel_of_point: torch.Tensor
    keys: torch.Tensor
    stats: torch.Tensor
    lengths: tuple


def _point_list(points, lengths, who):
    """a list of [N_i,3] tensors, or one [P,3] tensor with lengths (host ints) -> (points [P,3] f32 on the device, lengths)"""
    if isinstance(points, (list, tuple)):
        if lengths is not None and [int(v) for v in lengths] != [int(p.shape[0]) for p in points]:
            raise ValueError(f"{who}: lengths disagree with the list of clouds")
        lengths = tuple(int(p.shape[0]) for p in points)
        if not points:
            raise ValueError(f"{who}: an empty list of clouds")
        points = torch.cat([p.reshape(-1, 3) for p in points]) if len(points) > 1 else points[0].reshape(-1, 3)
    else:
        if lengths is None:
            raise ValueError(f"{who}: one [P,3] tensor needs lengths")
        if isinstance(lengths, torch.Tensor):
            if lengths.is_cuda:
                raise ValueError(f"{who}: lengths are host ints (a device tensor would have to be read back)")
            lengths = lengths.tolist()
        lengths = tuple(int(v) for v in lengths)
    if min(lengths, default=0) < 0 or sum(lengths) != points.shape[0]:
        raise ValueError(f"{who}: lengths {lengths[:8]}... sum to {sum(lengths)}, points are {tuple(points.shape)}")
    return points.contiguous(), lengths


def _to_device(values, dtype, shape, device):
    """a small host table to the device through pinned memory, without a synchronisation"""
    host = torch.tensor(values, dtype=dtype).reshape(shape).pin_memory()
    return host.to(device, non_blocking=True)


def _offsets(lengths, device):
    off = [0]
    for v in lengths:
        off.append(off[-1] + v)
    return _to_device(off, torch.int64, (len(off),), device)


def _cams(cams, n, device, who):
    """one Camera or one per cloud -> (kind, cams [n,16] f64 on the device)"""
    cams = [cams] * n if isinstance(cams, Camera) else list(cams)
    if len(cams) != n or not all(isinstance(c, Camera) for c in cams):
        raise ValueError(f"{who}: one Camera, or one per cloud ({n}), is expected")
    kinds = {c.kind for c in cams}
    if len(kinds) > 1:
        raise ValueError(f"{who}: the cameras of a batch are of one kind")
    kind = kinds.pop() if kinds else KIND_ORTHOGRAPHIC
    return kind, _to_device([c.row() for c in cams], torch.float64, (n, 16), device)


def orthographic_from_bounds(lo, hi, H, W, margin=0, T=None):
    """The orthographic camera that centres the box lo = (xlo, ylo), hi = (xhi, yhi) of camera coordinates in an H x W grid with
    `margin` free pixels on every side: pitch = max((xhi - xlo) / (W - 1 - 2 m), (yhi - ylo) / (H - 1 - 2 m)), 1 where that is 0;
    x0 = (xlo + xhi) / 2 - pitch (W - 1) / 2 and y0 likewise.  Python floats: float64."""
    (xlo, ylo), (xhi, yhi), m = (float(v) for v in lo), (float(v) for v in hi), int(margin)
    dw, dh = W - 1 - 2 * m, H - 1 - 2 * m
    if m < 0 or not (xlo <= xhi and ylo <= yhi and math.isfinite(xlo + xhi + ylo + yhi)):
        raise ValueError(f"fit_orthographic: an empty or unbounded cloud (x {xlo}..{xhi}, y {ylo}..{yhi}) has no camera")
    if (dw <= 0 and xhi > xlo) or (dh <= 0 and yhi > ylo):
        raise ValueError(f"fit_orthographic: a grid of {H} x {W} has no room for the cloud beside a margin of {m}")
    pitch = max((xhi - xlo) / dw if dw > 0 else 0.0, (yhi - ylo) / dh if dh > 0 else 0.0)
    if pitch == 0.0:
        pitch = 1.0
    return Camera.orthographic((xlo + xhi) / 2 - pitch * (W - 1) / 2, (ylo + yhi) / 2 - pitch * (H - 1) / 2, pitch, T=T)


def fit_orthographic(points, lengths, H, W, margin=0, T=None):
    """Per cloud the orthographic camera that fits its valid points into H x W (`orthographic_from_bounds` on ops.cloud_bounds under
    T) -> a list of Cameras.  Reads the bounds back: one synchronisation.  An empty cloud raises ValueError."""
    from . import ops
    points, lengths = _point_list(points, lengths, "fit_orthographic")
    n = len(lengths)
    _, cams = _cams(Camera(KIND_ORTHOGRAPHIC, _transform(T), (0.0, 0.0, 1.0, 1.0)), n, points.device, "fit_orthographic")
    bounds, count = ops.cloud_bounds(points, _offsets(lengths, points.device), cams, max(lengths, default=0))
    bounds, count = bounds.cpu().tolist(), count.cpu().tolist()
    out = []
    for b in range(n):
        if count[b] == 0:
            raise ValueError(f"fit_orthographic: cloud {b} has no valid point")
        out.append(orthographic_from_bounds(bounds[b][0:2], bounds[b][3:5], H, W, margin, T))
    return out


def organize(points, lengths, cams, H, W, fill=0, colors=None, labels=None):
    """points: a list of [N_i,3] float32 device tensors, or one [P,3] tensor with lengths (host ints); cams: one Camera or one per
    cloud (of one kind); colors [P,3] uint8 and labels [P] uint8 (or lists, as points) are optional -> Organized.  Without colours the
    image is black, without labels the mask is zeros.  Four launches on the current stream; no synchronisation."""
    from . import ops
    points, lengths = _point_list(points, lengths, "organize")
    if isinstance(colors, (list, tuple)):
        colors = torch.cat([c.reshape(-1, 3) for c in colors])
    if isinstance(labels, (list, tuple)):
        labels = torch.cat([v.reshape(-1) for v in labels])
    n, dev = len(lengths), points.device
    kind, cams = _cams(cams, n, dev, "organize")
    offsets = _offsets(lengths, dev)
    keys, pixel_of_point, stats = ops.organize_splat(points, offsets, cams, max(lengths, default=0), kind, H, W)
    index, xyz, rgb, mask = ops.organize_resolve(points, offsets, keys, stats, fill, colors, labels)
    return Organized(xyz, index, rgb, mask, pixel_of_point, keys, stats, lengths)


def scores_to_points(maps, org):
    """maps [n,H,W] (any float dtype, on the device) -> float32 [P]: every placed point reads the map at its OWN pixel -- an occluded
    point too, it lies behind that pixel -- and a dropped or outside point gets NaN.  A gather: torch indexing."""
    n, P = len(org.lengths), int(org.pixel_of_point.shape[0])
    if maps.dim() != 3 or maps.shape[0] != n or tuple(maps.shape[1:]) != tuple(org.index.shape[1:]):
        raise ValueError(f"scores_to_points: maps must be {tuple(org.index.shape)}, got {tuple(maps.shape)}")
    dev = org.pixel_of_point.device
    lengths = _to_device(list(org.lengths), torch.int64, (n,), dev)
    cloud = torch.repeat_interleave(torch.arange(n, device=dev), lengths, output_size=P)
    pix = org.pixel_of_point.to(torch.int64)
    got = maps.reshape(n, -1).to(torch.float32)[cloud, pix.clamp(min=0)]
    return torch.where(pix >= 0, got, torch.full_like(got, float("nan")))


# ------------------------------------------------------------------------------------------------ the command line
def write_mvtec_tree(src, dst, size=448, fill=1, batch=8):
    """Every class directory of the PLY tree `src` (dataset.PointCloudClass's layout) as a class directory of `dst` in MVTec 3D-AD's
    layout: <split>/<kind>/rgb/NNN.png, xyz/NNN.tiff and, under test, gt/NNN.png -- the samples PointCloudClass organises, written with
    utils.png.write_many and utils.tiff.imwrite.  Returns the number of samples written."""
    import os
    import types
    from .dataset import PointCloudClass
    from .utils import png, tiff
    from .utils.batching import in_batches, read_ahead
    args = types.SimpleNamespace(img_process_method="hip", organize_size=int(size), organize_fill=int(fill))
    written = 0
    for name in sorted(os.listdir(src)):
        if not os.path.isdir(os.path.join(src, name, "train")) and not os.path.isdir(os.path.join(src, name, "test")):
            continue
        source = PointCloudClass(src, name, args)
        for split, files, labels in (("train", source.train_files, [0] * source.n_train), ("test", source.test_files, source.test_labels)):
            number, lo = {}, 0
            jobs = [(path, labels[i]) for i, path in enumerate(files)]
            for dec in in_batches(read_ahead(lambda job: source.decode(*job), jobs, source.readers, 2 * source.readers), batch):
                org = source.organize_batch(dec)
                xyz = org.xyz.cpu().numpy()
                rgb_paths, gt_paths = [], []
                for j in range(len(dec)):
                    kind = os.path.basename(os.path.dirname(files[lo + j]))
                    k = number[kind] = number.get(kind, -1) + 1
                    base = os.path.join(dst, name, split, kind)
                    for sub in ("rgb", "xyz") + (("gt",) if split == "test" else ()):
                        os.makedirs(os.path.join(base, sub), exist_ok=True)
                    tiff.imwrite(os.path.join(base, "xyz", f"{k:03d}.tiff"), xyz[j])
                    rgb_paths.append(os.path.join(base, "rgb", f"{k:03d}.png"))
                    gt_paths.append(os.path.join(base, "gt", f"{k:03d}.png"))
                png.write_many(rgb_paths, org.rgb)
                if split == "test":
                    png.write_many(gt_paths, org.mask)
                lo += len(dec)
                written += len(dec)
    return written


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cmdiad_amd.organize", description=write_mvtec_tree.__doc__)
    ap.add_argument("--src", required=True, help="<src>/<class>/train/good/*.ply, <src>/<class>/test/<kind>/*.ply, optional <class>/camera.json")
    ap.add_argument("--dst", required=True, help="the tree to write, in MVTec 3D-AD's layout")
    ap.add_argument("--size", type=int, default=448, help="grid side where a class has no camera.json (default 448)")
    ap.add_argument("--fill", type=int, default=1, choices=(0, 1, 2), help="hole-fill radius where a class has no camera.json (default 1)")
    a = ap.parse_args(argv)
    n = write_mvtec_tree(a.src, a.dst, a.size, a.fill)
    print(f"organize: {n} samples written under {a.dst}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
