#!/usr/bin/env python3
"""Generate the preprocessing golden vectors (gpp_preprocess.npz) by IMPORTING THE REFERENCE's utils/preprocessing.py with inert
stubs for open3d and tifffile, as make_golden_dinov2.py does for its module.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_preprocess.py

The stubbed segment_plane / cluster_dbscan return a plane and labels SUPPLIED by this script (the numpy restatement of
tests/preprocess_ref.py on the same points), so what is recorded is the reference's own glue: get_edges_of_pc, pad_cropped_pc,
roundup_next_100, remove_plane, connected_components_cleaning (one scan where a cluster wins, one where noise is the most
frequent label).  Inputs are rebuilt from their seeds by the tests; only the reference's outputs and the supplied plane / labels
are stored."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("CMDIAD_REFERENCE", "/root/reference")

import preprocess_ref as pr  # noqa: E402

SCANS = {"a": dict(seed=41, H=120, W=140, pitch=8e-4), "b": dict(seed=42, H=130, W=120, pitch=8e-4)}
NOISE_SEED = 43
SUPPLIED = {}


def noise_majority_scan():
    """120 x 140: a small dense patch (one cluster) in a field of scattered valid points (noise): noise is the most frequent label."""
    rng = np.random.default_rng(NOISE_SEED)
    pc = np.zeros((120, 140, 3), np.float32)
    ys, xs = np.mgrid[0:120, 0:140]
    patch = (ys >= 40) & (ys < 60) & (xs >= 50) & (xs < 75)
    pc[patch] = np.stack([xs[patch] * 8e-4, ys[patch] * 8e-4, np.full(int(patch.sum()), 0.5)], -1)
    lone = (rng.random(xs.shape) < 0.08) & ~patch
    pc[lone] = rng.uniform(1.0, 3.0, (int(lone.sum()), 3))
    return pc, rng.integers(1, 255, (120, 140, 3), dtype=np.uint8)


def _install_stubs():
    class PointCloud:
        def __init__(self, v):
            self.pts = np.asarray(v)

        def segment_plane(self, distance_threshold, ransac_n, num_iterations):
            assert (distance_threshold, ransac_n, num_iterations) == (0.004, 50, 1000)
            return SUPPLIED["plane"], None

        def cluster_dbscan(self, eps, min_points, print_progress=False):
            assert (eps, min_points) == (0.006, 30)
            return list(SUPPLIED["labels"](self.pts))

    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a))
    sys.modules["open3d"] = o3d
    sys.modules["tifffile"] = types.ModuleType("tifffile")
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda *a, **k: None
    sys.modules.setdefault("tqdm", tq)


def main():
    _install_stubs()
    sys.path.insert(0, os.path.join(REF, "utils"))
    cwd = os.getcwd()
    os.chdir(os.environ.get("TMPDIR", "/tmp"))      # the reference opens preprocessing.log in the working directory at import
    try:
        import preprocessing as ref
    finally:
        os.chdir(cwd)
    out = {}
    for tag, kw in SCANS.items():
        scan = pr.make_scan(**kw)
        pc, rgb, gt = scan["pc"], scan["rgb"], scan["gt"]
        edges = ref.get_edges_of_pc(pc)
        plane = pr.plane_ransac(edges, seed=0)[0]
        SUPPLIED["plane"] = plane
        SUPPLIED["labels"] = pr.dbscan
        out[f"{tag}/edges_shape"] = np.array(edges.shape)
        out[f"{tag}/edges_sum"] = edges.astype(np.float64).sum(0)
        out[f"{tag}/edges_head"] = edges[:64]
        out[f"{tag}/plane"] = plane
        p1, r1 = ref.remove_plane(pc, rgb)
        out[f"{tag}/planeless_zero"] = np.packbits(np.all(p1 == 0, axis=2))
        p2, r2, g2 = ref.pad_cropped_pc(p1), ref.pad_cropped_pc(r1), ref.pad_cropped_pc(gt, single_channel=True)
        out[f"{tag}/padded_shape"] = np.array(p2.shape)
        out[f"{tag}/padded_gt"] = np.packbits(g2 != 0)
        flat = p2.reshape(-1, 3)
        out[f"{tag}/labels"] = pr.dbscan(flat[np.all(flat != 0, axis=1)]).astype(np.int16)
        p3, r3 = ref.connected_components_cleaning(p2, r2, "golden")
        out[f"{tag}/clean_zero"] = np.packbits(np.all(p3 == 0, axis=2))
        out[f"{tag}/clean_pc_sum"] = p3.astype(np.float64).sum((0, 1))
        out[f"{tag}/clean_rgb_sum"] = np.array(r3.astype(np.int64).sum())
    pc, rgb = noise_majority_scan()
    SUPPLIED["labels"] = pr.dbscan
    flat = pc.reshape(-1, 3)
    lab = pr.dbscan(flat[np.all(flat != 0, axis=1)])
    assert (lab == -1).sum() > (lab == 0).sum() > 0
    p3, r3 = ref.connected_components_cleaning(pc, rgb, "golden-noise")
    out["noise/labels"] = lab.astype(np.int16)
    out["noise/clean_zero"] = np.packbits(np.all(p3 == 0, axis=2))
    out["noise/clean_rgb_sum"] = np.array(r3.astype(np.int64).sum())
    out["roundup"] = np.array([[x, ref.roundup_next_100(x)] for x in (1, 99, 100, 101, 250, 799, 800, 801)])
    for h, w in ((120, 140), (250, 180), (300, 300), (1, 401)):
        a = np.arange(h * w * 3, dtype=np.float32).reshape(h, w, 3) + 1
        p = ref.pad_cropped_pc(a)
        out[f"pad/{h}x{w}"] = np.array([p.shape[0], p.shape[1], *np.argwhere(p[:, :, 0] != 0)[0]])
    path = os.path.join(HERE, "gpp_preprocess.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
