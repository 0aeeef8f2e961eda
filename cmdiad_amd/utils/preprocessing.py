"""The reference's utils/preprocessing.py surface (preprocessing.py:20-143) with its two open3d calls -- segment_plane and
cluster_dbscan -- replaced by the HIP kernels of csrc/preprocess.hip: numpy in, numpy out, the device in between.

  get_edges_of_pc                  preprocessing.py:20-27    host
  get_plane_eq                     preprocessing.py:30-33    device (cmdiad_plane_ransac; contract: docs/preprocessing.md)
  remove_plane                     preprocessing.py:36-57    device (cmdiad_plane_ransac + cmdiad_plane_mask)
  connected_components_cleaning    preprocessing.py:60-92    device (cmdiad_dbscan + cmdiad_label_histogram)
  roundup_next_100, pad_cropped_pc preprocessing.py:95-113   host
  preprocess_pc                    preprocessing.py:116-143  files in place, same path conventions
  preprocess_arrays                new: preprocess_pc without the file I/O, one scan or a list of scans
  preprocess_on_device             new: the same on device tensors -- edge set, plane, mask, padding, compaction, DBSCAN and the final
                                   zeroing without a trip to the host; preprocess_arrays / preprocess_pc are upload + this + download
  python -m cmdiad_amd.utils.preprocessing --dataset_path ...   the reference's __main__ loop; reader and writer threads around
                                   one device stream instead of the --num_process pool

The reference runs its file as a script from inside utils/ (`import mvtec3d_util`); nothing imports it as utils.preprocessing, so
this module is not part of the drop-in table.  The device stages need a GPU: there is no CPU path.
"""
import argparse
import logging
import math
import os
from pathlib import Path

import numpy as np

from . import mvtec3d_util as mvt_util
from . import gpu_device
from .batching import read_ahead

log = logging.getLogger("cmdiad_amd.preprocessing")

RANSAC_THRESHOLD = 0.004      # preprocessing.py:32
RANSAC_ITERATIONS = 1000
DBSCAN_EPS = 0.006            # preprocessing.py:67
DBSCAN_MIN_POINTS = 30
_SEED = 0                     # the surface of the reference has no seed argument; preprocess_arrays takes one


def _device(device=None):
    return gpu_device(device, "cmdiad_amd.utils.preprocessing needs a GPU: plane removal and DBSCAN run on the device (no CPU path)")


def get_edges_of_pc(organized_pc):
    # first and last 10 rows, then first and last 10 columns (the corner blocks appear twice, as in the reference); no zero points
    c = organized_pc.shape[2]
    edges = np.concatenate([organized_pc[0:10, :, :].reshape(-1, c), organized_pc[-10:, :, :].reshape(-1, c),
                            organized_pc[:, 0:10, :].reshape(-1, c), organized_pc[:, -10:, :].reshape(-1, c)], axis=0)
    return edges[np.nonzero(np.all(edges != 0, axis=1))[0], :]


def _plane_on_device(unorganized_pc, ransac_n_pts, seed, dev):
    import torch
    from .. import ops
    pts = np.ascontiguousarray(unorganized_pc, dtype=np.float32).reshape(-1, 3)
    if len(pts) < ransac_n_pts:
        raise ValueError(f"get_plane_eq: {len(pts)} valid edge points, {ransac_n_pts} needed for one RANSAC sample")
    return ops.plane_ransac(torch.from_numpy(pts).to(dev), n=ransac_n_pts, iterations=RANSAC_ITERATIONS,
                            distance_threshold=RANSAC_THRESHOLD, seed=seed)


def get_plane_eq(unorganized_pc, ransac_n_pts=50):
    plane, _ = _plane_on_device(unorganized_pc, ransac_n_pts, _SEED, _device())
    return plane.cpu().numpy()


def _remove_plane(organized_pc, organized_rgb, distance_threshold, seed, dev):
    import torch
    from .. import ops
    if organized_pc.dtype != np.float32:
        raise TypeError(f"remove_plane: the point cloud must be float32 (MVTec 3D-AD tiffs are), got {organized_pc.dtype}")
    plane, _ = _plane_on_device(get_edges_of_pc(organized_pc), 50, seed, dev)
    pc = torch.from_numpy(np.ascontiguousarray(organized_pc)).to(dev)
    rgb = torch.from_numpy(np.ascontiguousarray(organized_rgb)).to(dev)
    ops.plane_mask(pc, rgb, plane, distance_threshold)
    return pc.cpu().numpy().reshape(organized_pc.shape), rgb.cpu().numpy().reshape(organized_rgb.shape)


def remove_plane(organized_pc_clean, organized_rgb, distance_threshold=0.005):
    return _remove_plane(organized_pc_clean, organized_rgb, distance_threshold, _SEED, _device())


def _cluster_labels(points, dev):
    """labels of cluster_dbscan(eps=0.006, min_points=30) -> (labels on the device, histogram on the host: [noise, cluster 0, ...])."""
    import torch
    from .. import ops
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
    labels, ncl = ops.dbscan(pts, DBSCAN_EPS, DBSCAN_MIN_POINTS)
    hist = ops.label_histogram(labels, len(points) + 1)      # at most one cluster per point
    n = int(ncl.item())
    return labels, hist[:n + 1].cpu().numpy()


def _connected_components_cleaning(organized_pc, organized_rgb, image_path, dev):
    unorganized_pc = mvt_util.organized_pc_to_unorganized_pc(organized_pc).copy()
    unorganized_rgb = mvt_util.organized_pc_to_unorganized_pc(organized_rgb).copy()
    nonzero_indices = np.nonzero(np.all(unorganized_pc != 0, axis=1))[0]
    if len(nonzero_indices):      # (the reference fails on a scan without a valid point; here it comes back unchanged)
        labels, hist = _cluster_labels(unorganized_pc[nonzero_indices, :], dev)
        # np.unique(labels, return_counts=True) of the reference, from the histogram: the labels that occur, noise (-1) included
        present = np.nonzero(hist)[0]
        unique_cluster_ids, cluster_size = present - 1, hist[present]
        max_label = int(unique_cluster_ids.max())
        if max_label > 0:
            log.info("Point cloud file %s has %d clusters. Cluster ids: %s. Cluster size %s", image_path, max_label + 1,
                     unique_cluster_ids, cluster_size)
        largest_cluster_id = unique_cluster_ids[np.argmax(cluster_size)]        # ties: the lowest id; noise can win
        outliers = nonzero_indices[(labels != int(largest_cluster_id)).cpu().numpy()]
        unorganized_pc[outliers] = 0
        unorganized_rgb[outliers] = 0
    return unorganized_pc.reshape(organized_pc.shape), unorganized_rgb.reshape(organized_rgb.shape)


def connected_components_cleaning(organized_pc, organized_rgb, image_path):
    return _connected_components_cleaning(organized_pc, organized_rgb, image_path, _device())


def roundup_next_100(x):
    return int(math.ceil(x / 100.0)) * 100


def pad_cropped_pc(cropped_pc, single_channel=False):
    orig_h, orig_w = cropped_pc.shape[0], cropped_pc.shape[1]
    large_side = max(roundup_next_100(orig_h), roundup_next_100(orig_w))
    a = (large_side - orig_h) // 2
    aa = large_side - a - orig_h
    b = (large_side - orig_w) // 2
    bb = large_side - b - orig_w
    if single_channel:
        return np.pad(cropped_pc, pad_width=((a, aa), (b, bb)), mode='constant')
    return np.pad(cropped_pc, pad_width=((a, aa), (b, bb), (0, 0)), mode='constant')


def _pad_on_device(t, side, top, left):
    import torch
    out = torch.zeros((side, side) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    out[top:top + t.shape[0], left:left + t.shape[1]].copy_(t)
    return out


def preprocess_on_device(pc, rgb, gt=None, seed=0):
    """preprocess_pc's steps on device tensors, device tensors back: pc [H,W,3] f32 -> [S,S,3], rgb [H,W,C] u8 -> [S,S,C],
    gt [H,W] u8 or None -> [S,S] or None, S = the larger side rounded up to the next 100; the inputs are not written.  The scan goes
    straight into its padded buffers (masking before or after the padding gives the same arrays: a padded pixel is zero either way);
    the edge set is read from the un-padded window.  Everything runs on the current stream; the host reads two integers: the
    number of valid edge points (fewer than 50: ValueError before any RANSAC launch) and the number of valid points left after
    plane removal (the DBSCAN workspace; none: the cleaning stage changes nothing).  A scan without any valid point comes back
    unchanged, padded.  docs/preprocessing.md."""
    import torch
    from .. import ops
    from .. import _native as nat
    if not (torch.is_tensor(pc) and pc.is_cuda):
        raise nat.NativeError("preprocess_on_device: the scan must be device tensors (preprocess_arrays takes numpy arrays)")
    if pc.dtype != torch.float32:
        raise TypeError(f"preprocess_on_device: the point cloud must be float32 (MVTec 3D-AD tiffs are), got {pc.dtype}")
    if pc.dim() != 3 or pc.shape[2] != 3 or rgb.dim() != 3 or tuple(rgb.shape[:2]) != tuple(pc.shape[:2]) or \
            (gt is not None and tuple(gt.shape) != tuple(pc.shape[:2])):
        raise ValueError(f"preprocess_on_device: pc [H,W,3], rgb [H,W,C], gt [H,W] expected, got {tuple(pc.shape)}, {tuple(rgb.shape)}, "
                         f"{None if gt is None else tuple(gt.shape)}")
    H, W = pc.shape[0], pc.shape[1]
    side = max(roundup_next_100(H), roundup_next_100(W))
    top, left = (side - H) // 2, (side - W) // 2
    with torch.cuda.device(pc.device):
        pc_out, rgb_out = _pad_on_device(pc, side, top, left), _pad_on_device(rgb, side, top, left)
        gt_out = _pad_on_device(gt, side, top, left) if gt is not None else None
        edges, n_edges = ops.scan_edges(pc_out[top:top + H, left:left + W])
        E = int(n_edges.item())
        if E < 50:
            if E == 0 and int(ops.scan_compact(pc_out)[2].item()) == 0:
                return pc_out, rgb_out, gt_out      # a scan without a valid point comes back unchanged, padded
            raise ValueError(f"get_plane_eq: {E} valid edge points, 50 needed for one RANSAC sample")
        plane, _ = ops.plane_ransac(edges[:E], n=50, iterations=RANSAC_ITERATIONS, distance_threshold=RANSAC_THRESHOLD, seed=seed)
        ops.plane_mask(pc_out, rgb_out, plane, 0.005)
        points, index, n_points = ops.scan_compact(pc_out)
        N = int(n_points.item())
        if N:      # (the reference fails on a scan without a valid point; here it comes back unchanged)
            labels, n_clusters = ops.dbscan(points[:N], DBSCAN_EPS, DBSCAN_MIN_POINTS)
            hist = ops.label_histogram(labels, N + 1)      # at most one cluster per point
            ops.keep_largest_cluster(labels, index[:N], hist, n_clusters, pc_out, rgb_out)
    return pc_out, rgb_out, gt_out


def _preprocess_one(organized_pc, organized_rgb, organized_gt, seed, dev):
    import torch
    if organized_pc.dtype != np.float32:
        raise TypeError(f"remove_plane: the point cloud must be float32 (MVTec 3D-AD tiffs are), got {organized_pc.dtype}")
    up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None for a in (organized_pc, organized_rgb, organized_gt)]
    pc, rgb, gt = preprocess_on_device(*up, seed=seed)
    return pc.cpu().numpy(), rgb.cpu().numpy(), (gt.cpu().numpy() if gt is not None else None)


def preprocess_arrays(organized_pc, organized_rgb, organized_gt=None, seed=0, device=None):
    """preprocess_pc without files: (pc [H,W,3] f32, rgb [H,W,C], gt [H,W] or None) -> the cleaned, square-padded (pc, rgb, gt).
    Lists of scans (gt: a list with None entries, or None) are processed as one batch on one stream and come back as lists; every
    scan's result is the one a single call returns."""
    dev = _device(device)
    if isinstance(organized_pc, (list, tuple)):
        gts = organized_gt if organized_gt is not None else [None] * len(organized_pc)
        if not (len(organized_pc) == len(organized_rgb) == len(gts)):
            raise ValueError("preprocess_arrays: the lists of scans differ in length")
        out = [_preprocess_one(p, r, g, seed, dev) for p, r, g in zip(organized_pc, organized_rgb, gts)]
        return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]
    return _preprocess_one(organized_pc, organized_rgb, organized_gt, seed, dev)


def _paths(tiff_path):
    return str(tiff_path).replace("xyz", "rgb").replace("tiff", "png"), str(tiff_path).replace("xyz", "gt").replace("tiff", "png")


def _read(tiff_path):
    from PIL import Image
    organized_pc = mvt_util.read_tiff_organized_pc(tiff_path)
    rgb_path, gt_path = _paths(tiff_path)
    organized_rgb = np.array(Image.open(rgb_path))
    organized_gt = np.array(Image.open(gt_path)) if os.path.isfile(gt_path) else None      # not every pc has gt
    return organized_pc, organized_rgb, organized_gt


def _write(tiff_path, pc, rgb, gt):
    try:
        import tifffile as tiff
    except ImportError:          # (optional: utils/tiff.py writes the same array as an uncompressed float TIFF)
        from . import tiff
    from PIL import Image
    rgb_path, gt_path = _paths(tiff_path)
    tiff.imwrite(tiff_path, pc)
    Image.fromarray(rgb).save(rgb_path)
    if gt is not None:
        Image.fromarray(gt).save(gt_path)


def preprocess_pc(tiff_path, device=None):
    dev = _device(device)
    organized_pc, organized_rgb, organized_gt = _read(tiff_path)
    _write(tiff_path, *_preprocess_one(organized_pc, organized_rgb, organized_gt, _SEED, dev))


def preprocess_dataset(root_path, device=None, readers=4, writers=2, progress=None):
    """Every *.tiff under root_path, in place: reader threads decode ahead, this thread drives the device, writer threads encode
    behind it.  Returns the number of scans."""
    import concurrent.futures as cf
    dev = _device(device)
    paths = sorted(str(p) for p in Path(root_path).rglob('*.tiff'))
    with cf.ThreadPoolExecutor(writers) as wr:
        writes = []
        for i, (pc, rgb, gt) in enumerate(read_ahead(_read, paths, readers, max(2 * readers, 2))):
            writes.append(wr.submit(_write, paths[i], *_preprocess_one(pc, rgb, gt, _SEED, dev)))
            while len(writes) > 2 * writers:
                writes.pop(0).result()
            if progress is not None:
                progress(i + 1, len(paths))
        for w in writes:
            w.result()
    return len(paths)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Preprocess of Dataset')
    parser.add_argument('--dataset_path', '-d', default='datasets/mvtec_3d/', type=str, help='path to dataset')
    parser.add_argument('--device', default=None, type=int, help='GPU index (default: the current device)')
    args = parser.parse_args()
    logging.basicConfig(filename='preprocessing.log', encoding='UTF-8', level=logging.INFO, format='%(asctime)s %(message)s',
                        datefmt='%Y/%m/%d %I:%M:%S %p')
    print(f'Try to find dateset from {args.dataset_path}, current path: {os.getcwd()}')
    n = preprocess_dataset(args.dataset_path, args.device,
                           progress=lambda i, total: print(f"Processed {i} / {total} tiff files...") if i % 50 == 0 else None)
    print(f'Processed {n} files in {args.dataset_path}')
