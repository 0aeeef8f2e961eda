"""GPU: dataset.PointCloudClass over a small synthetic tree of PLY scans -- sample for sample and bit for bit what MVTec3DClass
(img_process_method='hip') yields over the tree `python -m cmdiad_amd.organize` writes from the same files, and what organize +
SamplePrep give when they are called by hand.  No network weights are involved."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd import organize as og  # noqa: E402
from cmdiad_amd.dataset import MVTec3DClass, PointCloudClass, SamplePrep  # noqa: E402
from cmdiad_amd.utils import ply  # noqa: E402

PINHOLE = {"kind": "pinhole", "fx": 150.0, "fy": 130.0, "cx": 31.6, "cy": 27.7, "size": [56, 64], "fill": 2,
           "T": [[1, 0, 0, 0.01], [0, 1, 0, -0.02], [0, 0, 1, 0.5]]}


def scan(seed, defect):
    """a bumpy patch of 80 x 80 jittered points in a shuffled order: x, y in -1..1, z about 5; colours; labels where `defect`"""
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:80, 0:80]
    x = (jj + rng.uniform(-0.4, 0.4, jj.shape)) / 40.0 - 0.99
    y = (ii + rng.uniform(-0.4, 0.4, ii.shape)) / 40.0 - 0.98
    z = 5.0 + 0.2 * np.sin(3 * x) * np.cos(2 * y) + (0.15 * np.exp(-((x - 0.3) ** 2 + (y + 0.2) ** 2) / 0.02) if defect else 0.0)
    pts = np.stack([x, y, z], axis=2).reshape(-1, 3).astype(np.float32)
    rgb = np.stack([128 + 100 * np.sin(5 * x), 128 + 100 * np.cos(4 * y), 40 * (z - 4.5)], axis=2).reshape(-1, 3).clip(0, 255).astype(np.uint8)
    label = (3 * (((x - 0.3) ** 2 + (y + 0.2) ** 2) < 0.04)).reshape(-1).astype(np.int32) if defect else None
    order = rng.permutation(len(pts))
    pts[rng.uniform(size=len(pts)) < 0.02] = 0                                          # what a sensor leaves where it saw nothing
    return pts[order], rgb[order], None if label is None else label[order]


def write_ply(path, pts, rgb=None, label=None):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if rgb is not None else []) + \
        ([("label", "<i4")] if label is not None else [])
    names = {"<f4": "float", "u1": "uchar", "<i4": "int"}
    rec = np.zeros(len(pts), np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = pts.T
    if rgb is not None:
        rec["red"], rec["green"], rec["blue"] = rgb.T
    if label is not None:
        rec["label"] = label
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pts)}"] + [f"property {names[t]} {n}" for n, t in fields] + ["end_header"]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def make_tree(root, camera):
    c = os.path.join(root, "bolt")
    write_ply(os.path.join(c, "train", "good", "000.ply"), *scan(1, False)[:2])
    write_ply(os.path.join(c, "train", "good", "001.ply"), scan(2, False)[0])             # no colours: a black image
    write_ply(os.path.join(c, "test", "good", "000.ply"), *scan(3, False)[:2])            # no label: a good scan needs none
    write_ply(os.path.join(c, "test", "dent", "000.ply"), *scan(4, True))
    write_ply(os.path.join(c, "test", "bump", "000.ply"), *scan(5, True))
    if camera is not None:
        with open(os.path.join(c, "camera.json"), "w") as f:
            json.dump(camera, f)
    return c


def same_sample(a, b):
    assert len(a) == len(b) == 3 and a.n_valid == b.n_valid and a.n_valid > 0
    for ta, tb in zip(a, b):
        assert ta.dtype == tb.dtype and ta.shape == tb.shape and torch.equal(ta, tb)


@pytest.mark.parametrize("camera", [None, PINHOLE], ids=["fitted", "camera_json"])
def test_point_cloud_class_equals_the_written_tree(tmp_path, camera):
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    cdir = make_tree(src, camera)
    args = types.SimpleNamespace(img_process_method="hip", organize_size=64, num_workers=2, rgb_size=224, xyz_size=224, gt_size=224)
    assert og.main(["--src", src, "--dst", dst, "--size", "64"]) == 0
    H, W = camera["size"] if camera else (64, 64)
    for sub, n in (("train/good/rgb", 2), ("train/good/xyz", 2), ("test/bump/gt", 1), ("test/dent/xyz", 1), ("test/good/rgb", 1)):
        assert len(os.listdir(os.path.join(dst, "bolt", sub))) == n
    assert not os.path.exists(os.path.join(dst, "bolt", "train", "good", "gt"))
    pc, mv = PointCloudClass(src, "bolt", args), MVTec3DClass(dst, "bolt", args)
    assert (pc.n_train, pc.n_test, pc.size, pc.fill) == (2, 3, (H, W), 2 if camera else 1) and (mv.n_train, mv.n_test) == (2, 3)
    assert pc.test_labels == [1, 1, 0] and [os.path.relpath(p, cdir) for p in pc.test_files] == ["test/bump/000.ply", "test/dent/000.ply",
                                                                                                  "test/good/000.ply"]
    train = list(zip(pc.train(), mv.train()))
    assert len(train) == 2
    for (sa, la), (sb, lb) in train:
        same_sample(sa, sb)
        assert torch.equal(la, lb) and la.tolist() == [0]
    assert float(train[1][0][0][0][0, 0].std()) < 1e-6 < float(train[0][0][0][0][0, 0].std())   # the scan without colours: one colour
    test = list(zip(pc.test(), mv.test()))
    assert len(test) == 3
    for k, ((sa, ma, la, pa), (sb, mb, lb, _)) in enumerate(test):
        same_sample(sa, sb)
        assert torch.equal(ma, mb) and torch.equal(la, lb) and la.tolist() == [pc.test_labels[k]] and pa == [pc.test_files[k]]
        assert bool(ma.any()) == bool(pc.test_labels[k])

    # by hand: read, fit or take the camera, organize, SamplePrep
    prep = SamplePrep(224, 224, 224)
    dec = [PointCloudClass.decode(p, lab) for p, lab in zip(pc.test_files, pc.test_labels)]
    pts = [torch.from_numpy(d[0]).cuda() for d in dec]
    colors = torch.from_numpy(np.concatenate([d[1] for d in dec])).cuda()
    labels = torch.from_numpy(np.concatenate([d[2] if d[2] is not None else np.zeros(len(d[0]), np.uint8) for d in dec])).cuda()
    if camera:
        cams = og.Camera.pinhole(camera["fx"], camera["fy"], camera["cx"], camera["cy"], camera["T"])
    else:
        cams = og.fit_orthographic(pts, None, 64, 64, margin=1)
    org = og.organize(pts, None, cams, H, W, fill=pc.fill, colors=colors, labels=labels)
    stats = org.stats.cpu().numpy()
    assert np.all(stats[:, 0] > 0) and np.all(stats[:, 2] > 0.4 * H * W) and np.all(stats[:, 3] > 0)
    assert np.all(stats[:, 1] == 0) or camera                                              # the fit leaves no valid point outside
    imgs, clouds, masks = prep.prepare_device_images(org.rgb), prep.prepare_device_clouds(org.xyz), prep.prepare_device_masks(org.mask)
    for k, ((sa, ma, _, _), _) in enumerate(test):
        assert torch.equal(sa[0][0], imgs[k]) and torch.equal(sa[1][0], clouds[k][0]) and torch.equal(sa[2][0], clouds[k][1])
        assert sa.n_valid == clouds[k][2].host()
        if pc.test_labels[k]:
            assert torch.equal(ma[0], masks[k].cpu())


def test_point_cloud_class_refusals(tmp_path):
    src = str(tmp_path / "src")
    c = make_tree(src, None)
    write_ply(os.path.join(c, "test", "dent", "001.ply"), *scan(6, False)[:2])             # a defect scan without labels
    args = types.SimpleNamespace(img_process_method="hip", organize_size=64, num_workers=1)
    pc = PointCloudClass(src, "bolt", args)
    with pytest.raises(ValueError, match="needs a per-point integer 'label'"):
        list(pc.test())
    with pytest.raises(ValueError, match="there is no host path"):
        PointCloudClass(src, "bolt", types.SimpleNamespace(img_process_method="cpu_v1"))
    with open(os.path.join(c, "camera.json"), "w") as f:
        json.dump({"kind": "fisheye"}, f)
    with pytest.raises(ValueError, match="orthographic"):
        PointCloudClass(src, "bolt", args)
    with open(os.path.join(c, "test", "dent", "000.ply"), "r+b") as f:
        f.truncate(os.path.getsize(os.path.join(c, "test", "dent", "000.ply")) - 7)
    with pytest.raises(ply.PlyError, match="more than the file"):
        PointCloudClass.decode(os.path.join(c, "test", "dent", "000.ply"), 1)
