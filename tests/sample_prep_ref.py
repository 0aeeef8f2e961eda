"""Test infrastructure of the sample-preparation tests (docs/sample_prep.md): a numpy evaluator of Pillow's two 8-bit resampling
passes driven by the HOST tables of cmdiad_amd.dataset (what the device kernels are handed), seeded inputs, and a tiny dataset tree
in the MVTec 3D-AD layout.  Pillow and torch themselves are the yardsticks; nothing here is compared with itself."""
import os

import numpy as np


def one_pass(img, coef, bounds, axis):
    """ImagingResampleHorizontal_8bpc / Vertical_8bpc: accumulator 1 << 21, >> 22, clamp -- along `axis` of img [H,W,C] uint8."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((coef.shape[0],) + src.shape[1:], np.uint8)
    for i in range(coef.shape[0]):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << 21) + np.tensordot(coef[i, :n].astype(np.int64), src[lo:lo + n], 1)
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def two_pass_resize(img, out_h, out_w):
    """Horizontal first into 8 bits, then vertical; a pass whose size does not change is skipped."""
    from cmdiad_amd.dataset import bicubic_tables
    h, w = img.shape[:2]
    if w != out_w:
        img = one_pass(img, *bicubic_tables(w, out_w), 1)
    if h != out_h:
        img = one_pass(img, *bicubic_tables(h, out_h), 0)
    return img


def pil_bicubic(img, out_h, out_w):
    from PIL import Image
    return np.array(Image.fromarray(img).resize((out_w, out_h), Image.BICUBIC))


def pil_nearest(gt, out_h, out_w):
    from PIL import Image
    return np.array(Image.fromarray(gt, "L").resize((out_w, out_h), Image.NEAREST))


def image(kind, h, w, seed=0):
    if kind == "random":
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "checker":      # 0 / 255, period 3: the overshoot of the first pass is clamped before the second
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat(((((y // 3) + (x // 3)) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)
    if kind == "white":        # constant 255: the rounding of the coefficient sum
        return np.full((h, w, 3), 255, np.uint8)
    raise ValueError(kind)


def cloud(h, w, seed=0, zero_frac=0.4):
    """[h,w,3] float32, ~zero_frac of the points zeroed, plus points with exactly ONE zero coordinate (not valid points, not zero points)."""
    rs = np.random.RandomState(seed)
    pc = (rs.rand(h, w, 3).astype(np.float32) + 0.1) * np.array([0.2, 0.2, 0.6], np.float32)
    pc[rs.rand(h, w) < zero_frac] = 0
    one = rs.rand(h, w) < 0.05
    pc[one, rs.randint(0, 3, int(one.sum()))] = 0
    return pc


def scan(seed, size=300):
    """A scan the extractors can work on: the synthetic surface of cmdiad_amd.synth at `size` x `size` (cloud [size,size,3] float32,
    background exact zeros) and a smooth colour image."""
    from cmdiad_amd.synth import synth_cloud
    pc = synth_cloud(seed, 0.45, size=size, texture=0.004)[0].permute(1, 2, 0).contiguous().numpy()
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:size, 0:size]
    rgb = np.stack([127 + 100 * np.sin(x / (7.0 + c) + seed) * np.cos(y / (11.0 - c)) for c in range(3)], 2) + rs.randint(-20, 21, (size, size, 3))
    return pc, np.clip(rgb, 0, 255).astype(np.uint8)


def read_npy_cloud(path):
    """Stand-in for tifffile.imread where `tifffile` is not installed: the *.tiff files of write_tree hold np.save data."""
    return np.load(path)


def write_tree(root, class_name="bagel", size=300, defect="crack"):
    """<root>/<class>/{train/good, test/good, test/<defect>}/{rgb/*.png, xyz/*.tiff[, gt/*.png]}: 3 train samples, 2 good test samples
    and 2 test samples of one defect type with gt.  PNGs through PIL; the clouds through tifffile when it is there, else np.save under
    the same names (-> read_npy_cloud).  Returns {relative stem: (cloud, rgb, gt or None)}."""
    from PIL import Image
    try:
        import tifffile
    except ImportError:
        tifffile = None
    items = {}
    plan = [("train/good", 3, False), ("test/good", 2, False), (f"test/{defect}", 2, True)]
    seed = 40
    for sub, n, has_gt in plan:
        base = os.path.join(root, class_name, sub)
        for d in ("rgb", "xyz") + (("gt",) if has_gt else ()):
            os.makedirs(os.path.join(base, d), exist_ok=True)
        for i in range(n):
            pc, rgb = scan(seed, size)
            seed += 1
            Image.fromarray(rgb).save(os.path.join(base, "rgb", f"{i:03d}.png"))
            path = os.path.join(base, "xyz", f"{i:03d}.tiff")
            if tifffile is not None:
                tifffile.imwrite(path, pc)
            else:
                with open(path, "wb") as fh:
                    np.save(fh, pc)
            gt = None
            if has_gt:
                gt = np.zeros((size, size), np.uint8)
                gt[90 + 10 * i:150, 100:170 + 5 * i] = 255
                gt[150:160, 100:160] = 127 + (np.arange(60) % 2).astype(np.uint8)      # right on the > 0.5 boundary
                Image.fromarray(gt, "L").save(os.path.join(base, "gt", f"{i:03d}.png"))
            items[f"{sub}/{i:03d}"] = (pc, rgb, gt)
    return items


def patch_tiff_reader(monkeypatch):
    """Route read_tiff_organized_pc to np.load when `tifffile` is absent."""
    try:
        import tifffile  # noqa: F401
    except ImportError:
        from cmdiad_amd.utils import mvtec3d_util
        monkeypatch.setattr(mvtec3d_util, "read_tiff_organized_pc", read_npy_cloud)
