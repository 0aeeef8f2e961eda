"""Scored scans as coloured PLY meshes, assembled on the device (docs/mesh.md): the 3-D counterpart of overlay.py.

One file per sample that MeshLab or CloudCompare opens directly: the organised cloud as a triangle mesh, vertex normals, the
overlay's colours, the raw score as a scalar field and the region label.  cmdiad_mesh_count and cmdiad_mesh_write (csrc/mesh.hip)
leave the files' vertex and face records on the device; utils.ply writes them behind a header.

  MeshSpec(lo, hi, colormap, alpha, max_edge, flip_normals)   what to build; MeshSpec.from_calibration(cal, span)
  build(clouds, maps, spec, background, labels) -> Meshes     the device buffers and counts, no synchronisation
  Meshes.to_host()                                            one read of counts, then the used prefixes only
  save(paths, clouds, maps, spec, ...)                        build + ply.write_many; ValueError on a bad point or a NaN score
  python -m cmdiad_amd.mesh --seg_dir DIR --cloud_root DIR --out DIR [--lo LO --hi HI | --cal FILE.cmdcal] [--rgb_root DIR]
                            [--max_edge X] [--flip]
"""
import math
import os
import sys

import numpy as np

from .overlay import CHUNK, COLOR_STOPS, IMAGENET_MEAN, IMAGENET_STD, OverlaySpec


class MeshSpec:
    """lo, hi, colormap, alpha: as OverlaySpec (the colours are the overlay's).  max_edge: None, or the longest edge (in the cloud's
    units, > 0) a triangle may have -- a longer one is a jump between surfaces and is not emitted.  flip_normals: the other winding
    and the opposite normals."""

    def __init__(self, lo, hi, colormap="heat", alpha=None, max_edge=None, flip_normals=False):
        colours = OverlaySpec(lo, hi, colormap=colormap, alpha=alpha)
        self.lo, self.hi, self.lut, self.alpha = colours.lo, colours.hi, colours.lut, colours.alpha
        self.pixel_threshold = None          # (overlay.DeviceSpec reads it: a mesh has no contour)
        if np.any(self.hi < self.lo):
            raise ValueError(f"MeshSpec: hi = {self.hi.tolist()} below lo = {self.lo.tolist()}")
        if max_edge is not None:
            max_edge = float(max_edge)
            if not (max_edge > 0 and math.isfinite(max_edge)):
                raise ValueError(f"MeshSpec: max_edge = {max_edge!r} must be a positive length (None: no edge is cut)")
        self.max_edge = max_edge
        self.flip_normals = bool(flip_normals)

    @property
    def max_edge2(self):
        """what the kernels compare a squared edge with: max_edge * max_edge, one float64 product, or inf"""
        return float("inf") if self.max_edge is None else self.max_edge * self.max_edge

    @classmethod
    def from_calibration(cls, cal, span=2.0, **kw):
        """lo = 0, hi = span x the calibration's pixel threshold, as OverlaySpec.from_calibration"""
        span = float(span)
        if not math.isfinite(span) or span <= 0:
            raise ValueError(f"MeshSpec.from_calibration: span = {span!r} must be positive")
        return cls(0.0, span * cal.pixel_threshold, **kw)


class Meshes:
    """What build() leaves on the device: counts [n,4] i32 (n_vert, n_face, bad, nan), vidx [n,H,W] i32, vertices [n, H W 35] u8 and
    faces [n, 2 (H-1) (W-1) 13] u8, each image's records at the front of its row."""

    def __init__(self, counts, chunks, vidx, vertices, faces):
        self.counts, self.chunks, self.vidx, self.vertices, self.faces = counts, chunks, vidx, vertices, faces

    def to_host(self):
        """(counts as numpy [n,4], list of vertex bytes, list of face bytes): ONE read of counts (the synchronisation), then only
        the used prefix of every row is copied."""
        import torch
        from .utils import ply
        counts = self.counts.cpu().numpy()
        verts, faces = [], []
        for i, (nv, nf) in enumerate(counts[:, :2].tolist()):
            verts.append(torch.empty((nv * ply.VERTEX_BYTES,), dtype=torch.uint8, pin_memory=True).copy_(
                self.vertices[i, :nv * ply.VERTEX_BYTES], non_blocking=True))
            faces.append(torch.empty((nf * ply.FACE_BYTES,), dtype=torch.uint8, pin_memory=True).copy_(
                self.faces[i, :nf * ply.FACE_BYTES], non_blocking=True))
        torch.cuda.current_stream(self.counts.device).synchronize()
        return counts, [v.numpy() for v in verts], [f.numpy() for f in faces]


def build(clouds, maps, spec, background=None, labels=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, layout=None):
    """clouds: the organised clouds of the maps, float32 [n,3,H,W] or [n,H,W,3] (numpy, a tensor or a list); maps: taken as
    regions.find_regions takes them -> Meshes, without a synchronisation.  background: None, uint8 [n,H,W,3] or float32 [n,3,H,W]
    normalised with mean / std; labels: None or int32 [n,H,W] (regions' component labels).  ValueError when the cloud's H, W differ
    from the maps'."""
    import torch
    from . import ops
    from .overlay import DeviceSpec
    from .regions import _device_clouds, _device_maps
    m = _device_maps(maps)
    n, H, W = m.shape
    c = _device_clouds(clouds, m)
    if c.dim() != 4 or c.shape[0] != n or tuple(c.shape[1:]) not in ((3, H, W), (H, W, 3)):
        raise ValueError(f"mesh.build: clouds of shape {tuple(c.shape)} beside maps {tuple(m.shape)}: one xyz per map pixel is needed")
    tables = DeviceSpec(spec, n, m.device)          # (reads lo, hi, lut, alpha of the spec)
    if background is not None:
        background = torch.as_tensor(background).to(m.device).contiguous()
    if labels is not None:
        labels = torch.as_tensor(labels).to(m.device, torch.int32).contiguous()
    chunks, counts = ops.mesh_count(c, m, spec.max_edge2, layout=layout)
    vidx, vertices, faces = ops.mesh_write(c, m, chunks, tables.lohi, tables.lut, tables.alpha, background=background, mean=mean, std=std,
                                           labels=labels, max_edge2=spec.max_edge2, flip=spec.flip_normals, layout=layout)
    return Meshes(counts, chunks, vidx, vertices, faces)


def save(paths, clouds, maps, spec, background=None, labels=None, comments=None, writers=4, **kw):
    """build + utils.ply.write_many: one PLY per map at paths[i].  ValueError (and no file) when a point has a non-finite coordinate
    or a vertex a NaN score.  comments: None or one list of header comment lines per file.  Returns the files' sizes."""
    from .utils import ply
    paths = list(paths)
    meshes = build(clouds, maps, spec, background, labels, **kw)
    if len(paths) != meshes.counts.shape[0]:
        raise ValueError(f"mesh.save: {len(paths)} paths for {meshes.counts.shape[0]} maps")
    counts, verts, faces = meshes.to_host()
    bad, nan = int(counts[:, 2].sum()), int(counts[:, 3].sum())
    if bad or nan:
        raise ValueError(f"mesh.save: {bad} points have a non-finite coordinate, {nan} vertices a NaN score")
    return ply.write_many(paths, counts[:, 0], verts, counts[:, 1], faces, comments=comments, writers=writers)


# ------------------------------------------------------------------------------------------------ the command line
def main(argv=None):
    """Every .pt map under --seg_dir (what --save_seg_results writes) with the .tiff of the same relative path under --cloud_root,
    brought to the map's size as the dataset does -> a PLY at that relative path under --out; with --rgb_root the .png of the same
    relative path colours the surface under the heatmap where it has the map's size."""
    import argparse
    import torch
    from . import regions
    from .dataset import host_cloud_transform
    from .overlay import _seg_files
    from .utils import png, tiff
    ap = argparse.ArgumentParser(prog="python -m cmdiad_amd.mesh")
    ap.add_argument("--seg_dir", required=True)
    ap.add_argument("--cloud_root", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--lo", type=float, default=None)
    ap.add_argument("--hi", type=float, default=None)
    ap.add_argument("--cal", default=None, help="a .cmdcal file: lo = 0, hi = span x its pixel threshold")
    ap.add_argument("--span", type=float, default=2.0)
    ap.add_argument("--rgb_root", default=None)
    ap.add_argument("--max_edge", type=float, default=None)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--colormap", default="heat", choices=sorted(COLOR_STOPS))
    a = ap.parse_args(argv)
    if (a.cal is None) == (a.lo is None or a.hi is None):
        ap.error("give --lo and --hi, or --cal")
    kw = dict(colormap=a.colormap, max_edge=a.max_edge, flip_normals=a.flip)
    spec = MeshSpec.from_calibration(regions.Calibration.load(a.cal), a.span, **kw) if a.cal else MeshSpec(a.lo, a.hi, **kw)
    files = _seg_files(a.seg_dir)
    done = 0
    for at in range(0, len(files), CHUNK):
        groups = {}            # (map shape, has a background) -> [(relative path of the PLY, map, cloud, RawImage | None)]
        for f in files[at:at + CHUNK]:
            m = torch.load(f, map_location="cpu")
            m = m.reshape(m.shape[-2:]).to(torch.float64)
            if m.shape[0] != m.shape[1]:
                raise ValueError(f"{f}: a {tuple(m.shape)} map; the dataset's cloud transform gives square clouds")
            stem = os.path.splitext(os.path.relpath(f, a.seg_dir))[0]
            cloud, _ = host_cloud_transform(tiff.imread(os.path.join(a.cloud_root, stem + ".tiff")), m.shape[0])
            raw, p = None, os.path.join(a.rgb_root, stem + ".png") if a.rgb_root else None
            if p and os.path.exists(p) and png.supported(png.read_layout(p)):
                raw = png.read_raw(p, "rgb")
                raw = raw if raw.shape == (*m.shape, 3) else None
            groups.setdefault((tuple(m.shape), raw is not None), []).append((stem + ".ply", m, cloud, raw))
        for (shape, has_bg), items in groups.items():
            maps = torch.stack([m for _, m, _, _ in items])
            clouds = torch.stack([c.reshape(3, *shape) for _, _, c, _ in items])
            bg = png.decode_on_device([raw for _, _, _, raw in items], "cuda") if has_bg else None
            paths = [os.path.join(a.out, rel) for rel, _, _, _ in items]
            for p in paths:
                os.makedirs(os.path.dirname(p) or ".", exist_ok=True)
            save(paths, clouds, maps, spec, background=bg, layout="planar", comments=[[f"source {rel[:-4]}"] for rel, _, _, _ in items])
            done += len(paths)
    print(f"{done} meshes written under {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
