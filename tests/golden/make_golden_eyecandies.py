#!/usr/bin/env python3
"""Generate the Eyecandies golden vectors (gec_eyecandies.npz) by IMPORTING THE REFERENCE's utils/preprocessing_eyecandies.py with
inert stubs for cv2, tifffile, imageio and tqdm, as make_golden_preprocess.py does for its module.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eyecandies.py

Three synthetic scans (tests/eyecandies_ref.py: SCANS; at most 40 x 40 pixels, two of them non-square) go through the reference's
depth_to_pointcloud and remove_point_cloud_background.  The stubbed imageio.v3.imread hands the reference the uint16 codes; the yaml
and the pose are real files in a temporary directory.  Stored: the codes, the yaml values, the pose, the focal length and the
reference's outputs (depth, points, final cloud).  Every scan must have each of the three removal rules firing on at least 5 % of
its pixels and at least 20 % of its pixels kept; this script asserts it."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("CMDIAD_REFERENCE", "/root/reference")

import eyecandies_ref as er  # noqa: E402

CODES = {}


def _install_stubs():
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.modules["tifffile"] = types.ModuleType("tifffile")
    iio = types.ModuleType("imageio")
    v3 = types.ModuleType("imageio.v3")
    v3.imread = lambda path: CODES[os.path.basename(path)]
    iio.v3 = v3
    sys.modules["imageio"] = iio
    sys.modules["imageio.v3"] = v3
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules.setdefault("tqdm", tq)


def main():
    _install_stubs()
    sys.path.insert(0, os.path.join(REF, "utils"))
    import preprocessing_eyecandies as ref
    out = {"tags": np.array(sorted(er.SCANS))}
    with tempfile.TemporaryDirectory() as tmp:
        for tag in sorted(er.SCANS):
            code, mind, maxd, pose, focal = er.scan(tag)
            name = f"{tag}_depth.png"
            CODES[name] = code
            info, pose_txt = os.path.join(tmp, f"{tag}_info_depth.yaml"), os.path.join(tmp, f"{tag}_pose.txt")
            with open(info, "w") as fh:
                fh.write(f"normalization:\n  max: {maxd!r}\n  min: {mind!r}\n")
            np.savetxt(pose_txt, pose)
            depth = ref.load_and_convert_depth(os.path.join(tmp, name), info)
            points = ref.depth_to_pointcloud(os.path.join(tmp, name), info, pose_txt, focal)
            cloud = ref.remove_point_cloud_background(points)
            assert depth.dtype == np.float32 and points.dtype == np.float64 and cloud.dtype == np.float64
            plane, far, side = er.rules(points)
            collapsed = er.background(points)[1]
            kept = 1.0 - collapsed.mean()
            print(f"{tag}: {code.shape} plane {plane.mean():.3f} far {far.mean():.3f} side {side.mean():.3f} kept {kept:.3f}")
            assert min(plane.mean(), far.mean(), side.mean()) >= 0.05 and kept >= 0.20, tag
            out[f"{tag}/code"], out[f"{tag}/pose"] = code, np.loadtxt(pose_txt)
            out[f"{tag}/yaml"] = np.array([mind, maxd, focal], dtype=np.float64)
            out[f"{tag}/depth"], out[f"{tag}/points"], out[f"{tag}/cloud"] = depth, points, cloud.reshape(*code.shape, 3)
    path = os.path.join(HERE, "gec_eyecandies.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
