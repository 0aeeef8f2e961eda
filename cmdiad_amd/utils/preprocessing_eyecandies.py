"""The reference's utils/preprocessing_eyecandies.py surface (preprocessing_eyecandies.py:13-187) with its per-pixel Python loops and
its numpy stages replaced by the HIP kernel of csrc/eyecandies.hip: numpy in, numpy out, the device in between.  Contract and
operation order: docs/eyecandies.md.

  FOCAL_LENGTH                     preprocessing_eyecandies.py:13
  load_and_convert_depth           preprocessing_eyecandies.py:16-24   device (cmdiad_eyecandies_unproject, depth output)
  depth_to_pointcloud              preprocessing_eyecandies.py:27-59   device (cmdiad_eyecandies_unproject); inv(K4 @ pose) on the host
  remove_point_cloud_background    preprocessing_eyecandies.py:62-89   device (cmdiad_eyecandies_background)
  cloud_arrays                     new: both stages without files, one scan or lists of scans, one launch per shape
                                   (cmdiad_eyecandies_cloud)
  preprocess_dataset, python -m cmdiad_amd.utils.preprocessing_eyecandies --dataset_path ... --target_dir ...
                                   the reference's __main__ loop (:92-187): the same tree, reader and writer threads around one
                                   device stream

The 16-bit PNG is read with Pillow, the yaml with PyYAML; the writer uses `tifffile` when it is installed, else utils/tiff.py.  dataset.EyecandiesRawClass feeds
the extractors from the RAW download without this tree.  The device stages need a GPU: there is no CPU path.
"""
import argparse
import os
from shutil import copyfile

import numpy as np

from . import gpu_device
from .batching import in_batches, read_ahead, scatter_by_shape

# The same camera has been used for all the images
FOCAL_LENGTH = 711.11


def _device(device=None):
    return gpu_device(device, "cmdiad_amd.utils.preprocessing_eyecandies needs a GPU: the depth-to-cloud stages run on the device "
                              "(no CPU path)")


# ------------------------------------------------------------------------------------------------ files
def read_depth_png(depth_img):
    """The 16-bit codes of *_depth.png -> uint16 [H,W]."""
    from PIL import Image
    with Image.open(depth_img) as im:
        if im.mode not in ("I;16", "I;16B", "I;16L", "I"):
            raise ValueError(f"{depth_img}: a 16-bit grey PNG is expected, got mode {im.mode!r}")
        a = np.array(im)
    if a.ndim != 2 or a.min() < 0 or a.max() > 65535:
        raise ValueError(f"{depth_img}: a 16-bit grey PNG is expected")
    return np.ascontiguousarray(a.astype(np.uint16))


def read_info_depth(info_depth):
    """-> (mind, maxd) of *_info_depth.yaml."""
    import yaml
    with open(info_depth) as f:
        data = yaml.safe_load(f)
    return data["normalization"]["min"], data["normalization"]["max"]


def read_scan(depth_img, info_depth, pose_txt):
    """-> (codes uint16 [H,W], mind, maxd, pose float64 [4,4]): what the three files of a sample hold."""
    mind, maxd = read_info_depth(info_depth)
    return read_depth_png(depth_img), mind, maxd, np.loadtxt(pose_txt)


def inv_projection(pose, height, width, focal_length=FOCAL_LENGTH):
    """inv(K4 @ pose), float64 [4,4]: the reference's own two numpy calls (:36-55); the kernel receives the result."""
    intrinsics_4x4 = np.array([
        [focal_length, 0, width / 2, 0],
        [0, focal_length, height / 2, 0],
        [0, 0, 1, 0],
        [0, 0, 0, 1]]
    )
    camera_proj = intrinsics_4x4 @ np.asarray(pose, dtype=np.float64)
    return np.linalg.inv(camera_proj)


def scan_params(mind, maxd, pose, height, width, focal_length=FOCAL_LENGTH):
    """One scan's parameter block (host uint8 [136]; ops.eyecandies_params)."""
    from .. import ops
    return ops.eyecandies_params(mind, maxd, inv_projection(pose, height, width, focal_length))


def _to_device(codes, params, dev):
    import torch
    code = torch.from_numpy(np.ascontiguousarray(np.stack(codes))).to(dev)
    return code, torch.stack(params).to(dev)


def _check_code(code):
    code = np.asarray(code)
    if code.dtype != np.uint16 or code.ndim != 2:
        raise TypeError(f"the depth map must be a uint16 [H,W] array of PNG codes, got {code.dtype} {code.shape}")
    return code


# ------------------------------------------------------------------------------------------------ the reference's functions
def load_and_convert_depth(depth_img, info_depth):
    from .. import ops
    dev = _device()
    mind, maxd = read_info_depth(info_depth)
    code = read_depth_png(depth_img)
    h, w = code.shape
    c, p = _to_device([code], [ops.eyecandies_params(mind, maxd, np.eye(4))], dev)
    return ops.eyecandies_unproject(c, p, want_points=False, want_depth=True)[1][0].cpu().numpy()


def depth_to_pointcloud(depth_img, info_depth, pose_txt, focal_length):
    from .. import ops
    dev = _device()
    code, mind, maxd, pose = read_scan(depth_img, info_depth, pose_txt)
    h, w = code.shape
    c, p = _to_device([code], [scan_params(mind, maxd, pose, h, w, focal_length)], dev)
    return ops.eyecandies_unproject(c, p)[0][0].cpu().numpy()


def remove_point_cloud_background(pc):
    import torch
    from .. import ops
    dev = _device()
    pc = np.ascontiguousarray(pc, dtype=np.float64)
    if pc.ndim != 2 or pc.shape[1] != 3:
        raise ValueError(f"remove_point_cloud_background: pc must be [n,3], got {pc.shape}")
    return ops.eyecandies_background(torch.from_numpy(pc).to(dev))[0].cpu().numpy()


def cloud_on_device(codes, minds, maxds, poses, focal_length=FOCAL_LENGTH, dev=None, want_removed=True):
    """Equal-shaped scans -> (cloud [B,H,W,3] f64, removed [B,H,W] u8 or None) ON THE DEVICE: one upload, one launch on the current
    stream, nothing read back."""
    from .. import ops
    dev = dev if dev is not None else _device()
    codes = [_check_code(c) for c in codes]
    h, w = codes[0].shape
    if any(c.shape != (h, w) for c in codes):
        raise ValueError("cloud_on_device: the scans of one launch must have one shape")
    c, p = _to_device(codes, [scan_params(mi, ma, po, h, w, focal_length) for mi, ma, po in zip(minds, maxds, poses)], dev)
    cloud, removed, _ = ops.eyecandies_cloud(c, p, want_removed=want_removed)
    return cloud, removed


def cloud_arrays(depth_u16, mind, maxd, pose, focal_length=FOCAL_LENGTH, device=None):
    """remove_point_cloud_background(depth_to_pointcloud(...)) without files: (codes uint16 [H,W], mind, maxd, pose [4,4]) ->
    (cloud float64 [H,W,3], removed bool [H,W]).  Lists of scans come back as lists; scans of equal shape share a launch, and every
    scan's result is the one a single call returns."""
    dev = _device(device)
    if not isinstance(depth_u16, (list, tuple)):
        cloud, removed = cloud_on_device([depth_u16], [mind], [maxd], [pose], focal_length, dev)
        return cloud[0].cpu().numpy(), removed[0].cpu().numpy().astype(bool)
    n = len(depth_u16)
    if not (len(mind) == len(maxd) == len(pose) == n):
        raise ValueError("cloud_arrays: the lists of scans differ in length")

    def group(_, idx):
        cloud, removed = cloud_on_device([depth_u16[i] for i in idx], [mind[i] for i in idx], [maxd[i] for i in idx],
                                         [pose[i] for i in idx], focal_length, dev)
        return zip(cloud.cpu().numpy(), removed.cpu().numpy().astype(bool))

    out = scatter_by_shape(depth_u16, range(n), group)
    return [o[0] for o in out], [o[1] for o in out]


# ------------------------------------------------------------------------------------------------ the reference's __main__
def raw_samples(data_dir, digits):
    """Indices of the samples under <class>/{train,test_public}/data, counted by their *_depth.png files; they must be contiguous from
    0 (on a complete download this is the reference's len(listdir) // 17)."""
    suffix = "_depth.png"
    found = sorted(f[:-len(suffix)] for f in os.listdir(data_dir) if f.endswith(suffix))
    want = [str(i).zfill(digits) for i in range(len(found))]
    if found != want:
        missing = sorted(set(want) - set(found))
        raise FileNotFoundError(f"{data_dir}: the samples must be numbered 0..{len(found) - 1} without a gap ({digits} digits); "
                                f"missing {missing[:5]}, unexpected {sorted(set(found) - set(want))[:5]}")
    return len(found)


def sample_files(data_dir, i, digits):
    stem = os.path.join(data_dir, str(i).zfill(digits))
    return {k: f"{stem}_{v}" for k, v in (("depth", "depth.png"), ("info", "info_depth.yaml"), ("pose", "pose.txt"),
                                          ("rgb", "image_4.png"), ("mask", "mask.png"))}


def read_mask(path):
    """*_mask.png as the reference's cv2.imread gives it to np.any and cv2.imwrite: uint8 [H,W,3] (the channel order of a grey mask
    does not matter)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def _tifffile():
    """The module whose imwrite writes the xyz tiffs: `tifffile` when it is installed, else utils/tiff.py."""
    try:
        import tifffile
    except ImportError:
        from . import tiff as tifffile
    return tifffile


def _write(files, target, i, cloud, mask):
    from PIL import Image
    name = str(i).zfill(3)
    _tifffile().imwrite(os.path.join(target, "xyz", name + ".tiff"), cloud)
    copyfile(files["rgb"], os.path.join(target, "rgb", name + ".png"))
    if mask is not None:
        Image.fromarray(mask).save(os.path.join(target, "gt", name + ".png"))


def preprocess_dataset(dataset_path, target_dir, device=None, readers=4, writers=2, batch=8, progress=None):
    """The reference's loop over every category of dataset_path into target_dir ({train,test}/{good,bad}/{rgb,xyz,gt}): reader
    threads decode ahead, this thread drives the device (`batch` scans per launch), writer threads encode behind it.  Returns the
    number of scans."""
    import concurrent.futures as cf
    dev = _device(device)
    _tifffile()
    os.mkdir(target_dir)
    jobs = []
    for category in os.listdir(dataset_path):
        out = os.path.join(target_dir, category)
        for sub, kinds in (("train/good", ("rgb", "xyz")), ("test/good", ("rgb", "xyz", "gt")), ("test/bad", ("rgb", "xyz", "gt"))):
            for kind in kinds:
                os.makedirs(os.path.join(out, sub, kind))
        for split, sub, digits in (("train", "train/data", 3), ("test", "test_public/data", 2)):
            data_dir = os.path.join(dataset_path, category, sub)
            jobs += [(out, split, i, sample_files(data_dir, i, digits)) for i in range(raw_samples(data_dir, digits))]

    def read(job):
        _, split, _, files = job
        return read_scan(files["depth"], files["info"], files["pose"]), (read_mask(files["mask"]) if split == "test" else None)

    done = 0
    with cf.ThreadPoolExecutor(writers) as wr:
        writes = []
        for dec in in_batches(read_ahead(read, jobs, readers, max(2 * readers, 2 * batch)), batch):
            scans = [d[0] for d in dec]
            clouds, _ = cloud_arrays([s[0] for s in scans], [s[1] for s in scans], [s[2] for s in scans], [s[3] for s in scans],
                                     FOCAL_LENGTH, dev.index)
            for (out, split, k, files), (_, mask), cloud in zip(jobs[done:done + len(dec)], dec, clouds):
                sub = "train/good" if split == "train" else ("test/bad" if np.any(mask) else "test/good")
                writes.append(wr.submit(_write, files, os.path.join(out, sub), k, cloud, mask))
            while len(writes) > 4 * writers:
                writes.pop(0).result()
            done += len(dec)
            if progress is not None:
                progress(done, len(jobs))
        for w in writes:
            w.result()
    return len(jobs)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Eyecandies depth maps to the organised-cloud tree of the extractors')
    parser.add_argument('--dataset_path', default='datasets/eyecandies', type=str, help="Original Eyecandies dataset path.")
    parser.add_argument('--target_dir', default='datasets/eyecandies_preprocessed', type=str, help="Processed Eyecandies dataset path")
    parser.add_argument('--device', default=None, type=int, help='GPU index (default: the current device)')
    args = parser.parse_args()
    n = preprocess_dataset(args.dataset_path, args.target_dir, args.device,
                           progress=lambda i, total: print(f"Processed {i} / {total} scans...") if i % 64 == 0 else None)
    print(f'Processed {n} scans of {args.dataset_path} into {args.target_dir}')
