"""Anomaly overlays: score maps rendered on the device and written as PNGs (docs/overlay.md).

What the reference offers here is ``utils/heatmap.py``, a seaborn script with hard-coded paths over the ``.pt`` maps of
``--save_seg_results``.  This module renders a batch of maps in ONE launch (``cmdiad_overlay_render``, csrc/overlay.hip): the map
resampled to the canvas, normalised between ``lo`` and ``hi``, coloured through a 256-entry table, blended over a background, the
contour of ``score > pixel_threshold`` and the boxes of the region tables (regions.py) drawn on top; ``utils.png.write_many`` then
filters the canvas rows on the device and deflates on host threads.  No Pillow, matplotlib or seaborn.

  OverlaySpec(lo, hi, ...)                what to draw; OverlaySpec.from_calibration(cal, span) puts the threshold mid-scale
  colormap(name), alpha_ramp(k0, k1, a)   the tables, integer interpolation between a few colour stops
  render(maps, spec, background, regions) -> uint8 [n,Ho,Wo,3] on the device, no synchronisation
  save(paths, maps, spec, ...)            render + png.write_many; ValueError when a map holds a NaN
  python -m cmdiad_amd.overlay --seg_dir DIR --out DIR [--lo LO --hi HI | --cal FILE.cmdcal] [--rgb_root DIR]
"""
import math
import os
import sys

import numpy as np

# name -> colour stops (position 0..255, r, g, b); positions ascend from 0 to 255
COLOR_STOPS = {
    "heat": ((0, 0, 0, 64), (64, 0, 96, 255), (128, 0, 224, 96), (192, 255, 224, 0), (255, 255, 0, 0)),
    "grey": ((0, 0, 0, 0), (255, 255, 255, 255)),
}
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CHUNK = 32


def colormap(name):
    """uint8 [256,3]: between two neighbouring stops (p0, c0), (p1, c1) entry p0 + j is (c0 * (d - j) + c1 * j + d // 2) // d with
    d = p1 - p0 -- integers only, no table from outside."""
    if name not in COLOR_STOPS:
        raise ValueError(f"colormap: unknown name {name!r} (known: {sorted(COLOR_STOPS)})")
    stops = COLOR_STOPS[name]
    out = np.zeros((256, 3), dtype=np.uint8)
    for (p0, *c0), (p1, *c1) in zip(stops[:-1], stops[1:]):
        d = p1 - p0
        for j in range(d + 1):
            out[p0 + j] = [(a * (d - j) + b * j + d // 2) // d for a, b in zip(c0, c1)]
    return out


def alpha_ramp(k0=0, k1=128, a_max=200):
    """uint8 [256]: 0 up to index k0, a_max from k1 on, the integer ramp (a_max * (k - k0) + d // 2) // d, d = k1 - k0, between."""
    k0, k1, a_max = int(k0), int(k1), int(a_max)
    if not (0 <= k0 <= k1 <= 255 and 0 <= a_max <= 255):
        raise ValueError(f"alpha_ramp: 0 <= k0 = {k0} <= k1 = {k1} <= 255 and 0 <= a_max = {a_max} <= 255 are required")
    d = k1 - k0
    return np.array([a_max if k >= k1 else 0 if k <= k0 else (a_max * (k - k0) + d // 2) // d for k in range(256)], dtype=np.uint8)


def _rgb(v, what):
    v = tuple(int(c) for c in v)
    if len(v) != 3 or not all(0 <= c <= 255 for c in v):
        raise ValueError(f"OverlaySpec: {what} must be three bytes, got {v!r}")
    return v


class OverlaySpec:
    """lo, hi: the scores that map to the first and the last table entry (one float each, or one per image); finite.
    pixel_threshold: None, or the threshold whose contour is drawn (score > threshold, strict; one float or one per image).
    colormap: a name of COLOR_STOPS or a uint8 [256,3] table.  alpha: a uint8 [256] table (default alpha_ramp()) or one byte for every
    entry; it plays a part only over a background.  line_px (1..8): thickness of the boxes.  size: (Ho, Wo) of the canvas, default the
    map's own size."""

    def __init__(self, lo, hi, pixel_threshold=None, colormap="heat", alpha=None, contour_rgb=(255, 255, 255), box_rgb=(0, 255, 0),
                 line_px=1, size=None):
        self.lo, self.hi = self._values(lo, "lo"), self._values(hi, "hi")
        self.pixel_threshold = None if pixel_threshold is None else self._values(pixel_threshold, "pixel_threshold")
        self.lut = globals()["colormap"](colormap) if isinstance(colormap, str) else np.ascontiguousarray(colormap, dtype=np.uint8)
        if self.lut.shape != (256, 3):
            raise ValueError(f"OverlaySpec: a colour table is uint8 [256,3], got {self.lut.shape}")
        if alpha is None:
            alpha = alpha_ramp()
        self.alpha = np.full(256, int(alpha), dtype=np.uint8) if np.ndim(alpha) == 0 else np.ascontiguousarray(alpha, dtype=np.uint8)
        if self.alpha.shape != (256,):
            raise ValueError(f"OverlaySpec: an alpha table is uint8 [256], got {self.alpha.shape}")
        self.contour_rgb, self.box_rgb = _rgb(contour_rgb, "contour_rgb"), _rgb(box_rgb, "box_rgb")
        if isinstance(line_px, bool) or int(line_px) != line_px or not 1 <= int(line_px) <= 8:
            raise ValueError(f"OverlaySpec: line_px must be an integer in 1..8, got {line_px!r}")
        self.line_px = int(line_px)
        self.size = None if size is None else (int(size[0]), int(size[1]))
        if self.size is not None and not all(1 <= s <= (1 << 14) for s in self.size):
            raise ValueError(f"OverlaySpec: size = {self.size}, sides 1..2^14")

    @staticmethod
    def _values(v, what):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim > 1 or a.size == 0 or not np.isfinite(a).all():
            raise ValueError(f"OverlaySpec: {what} must be one finite float or one per image; got {v!r}")
        return a.reshape(-1).copy()

    @classmethod
    def from_calibration(cls, cal, span=2.0, **kw):
        """lo = 0, hi = span x the calibration's pixel threshold, the contour at that threshold: with span = 2 the threshold sits in
        the middle of the scale.  span is a policy knob, like the quantiles of docs/regions.md; nothing is claimed for 2."""
        span = float(span)
        if not math.isfinite(span) or span <= 0:
            raise ValueError(f"OverlaySpec.from_calibration: span = {span!r} must be positive")
        return cls(0.0, span * cal.pixel_threshold, pixel_threshold=cal.pixel_threshold, **kw)


class DeviceSpec:
    """The tables and values of an OverlaySpec for n images on one device: built once, passed to `render` in place of the spec.
    `thr` and `lohi` are read by the kernel, so rewriting them in place changes the next launch with nothing rebuilt."""

    def __init__(self, spec, n, device):
        import torch
        self.spec, self.n = spec, n
        for name in ("lo", "hi", "pixel_threshold"):
            v = getattr(spec, name)
            if v is not None and v.size not in (1, n):
                raise ValueError(f"overlay: {v.size} values of {name} for {n} maps (one, or one per image)")
        per = n if max(spec.lo.size, spec.hi.size) > 1 else 1
        lohi = np.stack([np.broadcast_to(spec.lo, (per,)), np.broadcast_to(spec.hi, (per,))], axis=1)
        self.lohi = torch.from_numpy(np.ascontiguousarray(lohi)).to(device)
        self.thr = None if spec.pixel_threshold is None else torch.from_numpy(spec.pixel_threshold.copy()).to(device)
        self.lut, self.alpha = torch.from_numpy(spec.lut.copy()).to(device), torch.from_numpy(spec.alpha.copy()).to(device)


def _tables(regions, n, device):
    """regions: None, a regions.Regions (host), or the device tuple of regions.region_tables_device -> (count, ints) on the device"""
    import torch
    if regions is None:
        return None, None
    if isinstance(regions, (tuple, list)):
        count, ints = (regions[1], regions[2]) if len(regions) == 5 else regions
    else:
        count, ints = torch.from_numpy(np.ascontiguousarray(regions.count)), torch.from_numpy(np.ascontiguousarray(regions.ints))
    count, ints = count.to(device), ints.to(device)
    if count.numel() != n or ints.shape[0] != n:
        raise ValueError(f"overlay: region tables of {count.numel()} images for {n} maps")
    return count.contiguous(), ints.contiguous()


def render(maps, spec, background=None, regions=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, canvas=None, nan_count=None,
           return_nan_count=False):
    """maps: numpy, a tensor or a list of [H,W] maps, taken as regions.find_regions takes them; spec: an OverlaySpec or a DeviceSpec
    -> uint8 [n,Ho,Wo,3] on the device, without a synchronisation.  background: None, uint8 [n,Ho,Wo,3], or float32 [n,3,Ho,Wo]
    normalised with mean / std (default: the rgb tensors of the samples); it must have the canvas size.  regions: a regions.Regions or
    the device tuple of regions.region_tables_device.  return_nan_count: also the device counter of NaN scores."""
    import torch
    from . import ops
    from .regions import _device_maps
    m = _device_maps(maps)
    n = m.shape[0]
    dspec = spec if isinstance(spec, DeviceSpec) else DeviceSpec(spec, n, m.device)
    if dspec.n != n or dspec.lut.device != m.device:
        raise ValueError(f"overlay.render: a DeviceSpec for {dspec.n} maps on {dspec.lut.device}, got {n} maps on {m.device}")
    s = dspec.spec
    if background is not None:
        background = torch.as_tensor(background)
        if not background.is_cuda:
            background = background.to(m.device)
        background = background.contiguous()
    count, ints = _tables(regions, n, m.device)
    out, nan = ops.overlay_render(m, dspec.lohi, dspec.lut, dspec.alpha, size=s.size, thr=dspec.thr, background=background, mean=mean,
                                  std=std, count=count, ints=ints, line_px=s.line_px, contour_rgb=s.contour_rgb, box_rgb=s.box_rgb,
                                  canvas=canvas, nan_count=nan_count)
    return (out, nan) if return_nan_count else out


def save(paths, maps, spec, background=None, regions=None, level=6, mode="adaptive", **kw):
    """render + utils.png.write_many: one PNG per map at paths[i].  ValueError (and no file) when a map holds a NaN score, as
    regions.find_regions.  Returns the files' sizes."""
    from .utils import png
    canvas, nan = render(maps, spec, background, regions, return_nan_count=True, **kw)
    bad = int(nan.item())
    if bad:
        raise ValueError(f"overlay.save: {bad} canvas pixels have a NaN score")
    return png.write_many(paths, canvas, level=level, mode=mode)


# ------------------------------------------------------------------------------------------------ the command line
def _seg_files(seg_dir):
    out = []
    for root, _, files in os.walk(seg_dir):
        out += [os.path.join(root, f) for f in files if f.endswith(".pt")]
    return sorted(out)


def main(argv=None):
    """The job of the reference's utils/heatmap.py: every .pt map under --seg_dir (what --save_seg_results writes) -> a PNG at the same
    relative path under --out; with --rgb_root the file of the same relative path (.png) goes behind the heatmap where it has the
    canvas size."""
    import argparse
    import torch
    from . import regions
    from .utils import png
    ap = argparse.ArgumentParser(prog="python -m cmdiad_amd.overlay")
    ap.add_argument("--seg_dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--lo", type=float, default=None)
    ap.add_argument("--hi", type=float, default=None)
    ap.add_argument("--cal", default=None, help="a .cmdcal file: lo = 0, hi = span x its pixel threshold, contour at the threshold")
    ap.add_argument("--span", type=float, default=2.0)
    ap.add_argument("--rgb_root", default=None)
    ap.add_argument("--colormap", default="heat", choices=sorted(COLOR_STOPS))
    a = ap.parse_args(argv)
    if (a.cal is None) == (a.lo is None or a.hi is None):
        ap.error("give --lo and --hi, or --cal")
    spec = OverlaySpec.from_calibration(regions.Calibration.load(a.cal), a.span, colormap=a.colormap) if a.cal else \
        OverlaySpec(a.lo, a.hi, colormap=a.colormap)
    files = _seg_files(a.seg_dir)
    done = 0
    for at in range(0, len(files), CHUNK):
        groups = {}            # (map shape, has a background) -> [(relative path of the PNG, map, RawImage | None)]
        for f in files[at:at + CHUNK]:
            m = torch.load(f, map_location="cpu")
            m = m.reshape(m.shape[-2:]).to(torch.float64)
            rel, raw = os.path.splitext(os.path.relpath(f, a.seg_dir))[0] + ".png", None
            p = os.path.join(a.rgb_root, rel) if a.rgb_root else None
            if p and os.path.exists(p) and png.supported(png.read_layout(p)):
                raw = png.read_raw(p, "rgb")
                raw = raw if raw.shape == (*m.shape, 3) else None
            groups.setdefault((tuple(m.shape), raw is not None), []).append((rel, m, raw))
        for (shape, has_bg), items in groups.items():
            maps = torch.stack([m for _, m, _ in items])
            bg = png.decode_on_device([raw for _, _, raw in items], "cuda") if has_bg else None
            paths = [os.path.join(a.out, rel) for rel, _, _ in items]
            for p in paths:
                os.makedirs(os.path.dirname(p) or ".", exist_ok=True)
            save(paths, maps, spec, background=bg)
            done += len(paths)
    print(f"{done} overlays written under {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
