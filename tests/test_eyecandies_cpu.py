"""CPU (no GPU): the host side of the Eyecandies path (docs/eyecandies.md) -- the numpy restatement of the documented operation order
against the reference's own outputs (tests/golden/gec_eyecandies.npz), file discovery of EyecandiesRawClass over a raw tree written
here with Pillow, and the C ABI of the new entry points."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eyecandies_ref as er  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmdiad_eyecandies_cloud", "cmdiad_eyecandies_unproject", "cmdiad_eyecandies_background", "cmdiad_organized_pc_prep_f64")

# The largest absolute deviation of the restatement's final cloud from the reference's over the three golden scans, measured when the
# golden file was made: 8.881784197001252e-16 (scan "a", coordinates up to 6.1).  The reference sums its products in BLAS order, the
# restatement in the documented order: that is the only source of difference.  The bound is 8 x the measured maximum.
MEASURED_MAX_DEVIATION = 8.881784197001252e-16
CLOUD_TOLERANCE = 8 * MEASURED_MAX_DEVIATION
MAX_NEAR_THRESHOLD_PIXELS = 2          # per scan: pixels whose margin to a removal threshold is below the tolerance


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "gec_eyecandies.npz"))


def test_golden_scans_are_the_seeded_ones_and_exercise_every_rule(golden):
    tags = list(golden["tags"])
    assert tags == sorted(er.SCANS) and len(tags) == 3
    shapes = []
    for tag in tags:
        code, mind, maxd, pose, focal = er.scan(tag)
        assert np.array_equal(code, golden[f"{tag}/code"]) and np.array_equal(pose, golden[f"{tag}/pose"])
        assert np.array_equal(golden[f"{tag}/yaml"], [mind, maxd, focal])
        assert max(code.shape) <= 40 and code.size >= 513
        shapes.append(code.shape)
        plane, far, side = er.rules(golden[f"{tag}/points"])
        kept = golden[f"{tag}/cloud"][..., 0] != 0
        assert min(plane.mean(), far.mean(), side.mean()) >= 0.05 and kept.mean() >= 0.20, tag
    assert any(h != w for h, w in shapes)


def test_restatement_equals_the_reference(golden):
    worst = 0.0
    for tag in golden["tags"]:
        mind, maxd, focal = golden[f"{tag}/yaml"]
        r = er.restate(golden[f"{tag}/code"], mind, maxd, golden[f"{tag}/pose"], focal)
        assert r["depth"].dtype == np.float32 and np.array_equal(r["depth"], golden[f"{tag}/depth"]), tag      # bit-equal
        ref_cloud = golden[f"{tag}/cloud"]
        dev = float(np.abs(r["cloud"] - ref_cloud).max())
        worst = max(worst, dev)
        print(f"{tag}: largest |restatement - reference| of the cloud {dev!r}")
        assert r["cloud"].dtype == np.float64 and dev <= CLOUD_TOLERANCE, (tag, dev)
        # the reference's removed pixels: the ones that sit on its collapsed point, whose x is an exact zero
        ref_removed = ref_cloud[..., 0] == 0
        collapsed = ref_cloud[ref_removed]
        assert len(collapsed) and np.all(collapsed == collapsed[0]) and np.any(collapsed[0] != 0)      # one point, and not the origin
        # the reference's own margin to a threshold, from ITS points
        margin = er.background(golden[f"{tag}/points"])[2].reshape(ref_removed.shape)
        near = margin < CLOUD_TOLERANCE
        assert int(near.sum()) <= MAX_NEAR_THRESHOLD_PIXELS, (tag, int(near.sum()))
        assert np.array_equal(r["removed"][~near], ref_removed[~near]), tag
    print(f"largest deviation over the scans {worst!r}; bound {CLOUD_TOLERANCE!r}")


def test_depth_restatement_rounds_the_scalars_to_float32():
    code = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    for mind, maxd in ((0.5, 3.1), (0.1, 0.1 + 2.0 / 3.0)):
        want = code.astype(np.float32) / 65535.0 * (maxd - mind) + mind          # the reference's line, as numpy evaluates it
        assert want.dtype == np.float32 and np.array_equal(er.depth(code, mind, maxd), want)
    assert float(np.float32(0.1 + 2.0 / 3.0 - 0.1)) != 0.1 + 2.0 / 3.0 - 0.1      # a range float32 cannot hold


def _args(root, method="hip", **kw):
    return types.SimpleNamespace(dataset_path=str(root), img_process_method=method, num_workers=2, rgb_size=224, xyz_size=224,
                                 gt_size=224, dataset_type="eyecandies", **kw)


def test_raw_tree_discovery_order_and_refusals(tmp_path):
    from cmdiad_amd import dataset as ds
    from cmdiad_amd.utils import preprocessing_eyecandies as pe
    items = er.write_raw_tree(str(tmp_path), "CandyCane", n_train=2, n_test=3, bad=(1,))
    base = tmp_path / "CandyCane"
    assert sorted(os.listdir(base / "train" / "data"))[0] == "000_depth.png"            # 3 digits for train, 2 for test
    assert sorted(os.listdir(base / "test_public" / "data"))[0] == "00_depth.png"
    # the files hold what was written: 16-bit codes, yaml values, pose
    f = pe.sample_files(str(base / "test_public" / "data"), 1, 2)
    code, mind, maxd, pose = pe.read_scan(f["depth"], f["info"], f["pose"])
    it = items[("test", 1)]
    assert code.dtype == np.uint16 and np.array_equal(code, it["code"]) and (mind, maxd) == (it["mind"], it["maxd"])
    assert np.array_equal(pose, it["pose"]) and code.max() > 255
    assert np.array_equal(pe.inv_projection(pose, *code.shape), er.inv_projection(pose, *code.shape))
    assert pe.FOCAL_LENGTH == 711.11

    cls = ds.EyecandiesRawClass(str(tmp_path), "CandyCane", _args(tmp_path))
    assert (cls.name, cls.n_train, cls.n_test) == ("CandyCane", 2, 3)
    assert cls.test_indices == [1, 0, 2] and cls.test_labels == [1, 0, 0]               # bad in index order, then good
    assert [os.path.basename(f["rgb"]) for f in cls._test_files] == ["01_image_4.png", "00_image_4.png", "02_image_4.png"]
    assert [os.path.basename(f["depth"]) for f in cls._train_files] == ["000_depth.png", "001_depth.png"]

    for method in ("cpu_v1", "cpu_v2"):
        with pytest.raises(ValueError, match="no host path"):
            ds.EyecandiesRawClass(str(tmp_path), "CandyCane", _args(tmp_path, method))
    with pytest.raises(ValueError, match="cpu_v1.*cpu_v2.*hip"):
        ds.EyecandiesRawClass(str(tmp_path), "CandyCane", _args(tmp_path, "gpu"))

    # auto-detection: a class with train/data is raw, any other directory is a tree in MVTec 3D-AD's layout (the host methods work there)
    data = ds.dataset_classes(_args(tmp_path))
    assert list(data) == ["CandyCane"] and isinstance(data["CandyCane"], ds.EyecandiesRawClass) and data["CandyCane"].n_test == 3
    pre = tmp_path / "preprocessed"
    for sub in ("train/good/rgb", "train/good/xyz", "test/good/rgb"):
        (pre / "Lollipop" / sub).mkdir(parents=True)
    data = ds.dataset_classes(_args(pre, "cpu_v1"))
    assert list(data) == ["Lollipop"] and isinstance(data["Lollipop"], ds.MVTec3DClass) and data["Lollipop"].n_train == 0
    with pytest.raises(FileNotFoundError):
        ds.dataset_classes(types.SimpleNamespace(**{**vars(_args(tmp_path)), "dataset_type": "mvtec3d"}))

    if not torch.cuda.is_available():      # the samples need a GPU: no host fallback
        with pytest.raises(Exception, match="GPU"):
            next(cls.train())
        with pytest.raises(Exception, match="GPU"):
            pe.cloud_arrays(it["code"], it["mind"], it["maxd"], it["pose"])
        with pytest.raises(Exception, match="GPU"):
            pe.remove_point_cloud_background(np.zeros((600, 3)))
        with pytest.raises(Exception, match="GPU"):
            pe.depth_to_pointcloud(f["depth"], f["info"], f["pose"], pe.FOCAL_LENGTH)

    # a gap in the numbering: the contiguity error
    os.remove(base / "train" / "data" / "000_depth.png")
    with pytest.raises(FileNotFoundError, match="without a gap"):
        ds.EyecandiesRawClass(str(tmp_path), "CandyCane", _args(tmp_path))


def test_parameter_block_layout():
    from cmdiad_amd import ops
    inv_p = np.arange(16, dtype=np.float64).reshape(4, 4) / 7.0
    blk = ops.eyecandies_params(0.1, 0.1 + 2.0 / 3.0, inv_p).numpy()
    assert blk.dtype == np.uint8 and blk.shape == (136,) == (ops.EYECANDIES_PARAM_BYTES,)
    assert np.array_equal(blk[:8].view(np.float32), [np.float32((0.1 + 2.0 / 3.0) - 0.1), np.float32(0.1)])
    assert np.array_equal(blk[8:].view(np.float64), inv_p.reshape(16))
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    assert re.search(r"float range;\s*float mind;\s*double inv_p\[16\];\s*}\s*cmdiad_eyecandies_params;", hdr)


def test_new_entry_points_are_declared_bound_and_reject_bad_arguments():
    from cmdiad_amd import _native as nat
    from cmdiad_amd import ops
    L = nat.lib()
    assert L.cmdiad_abi_version() == 6
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    declared = set(re.findall(r"\b(cmdiad_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(L, name)
        n_args = len(re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(","))
        assert n_args == len(nat.SIGNATURES[name]), name
        args = [None if a is ctypes.c_void_p else 1 for a in nat.SIGNATURES[name]]
        assert getattr(L, name)(*args) == -1 and b"null pointer" in L.cmdiad_last_error(), name
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # bad sizes with valid-looking pointers: rejected before anything is launched
    for B, H, W in ((0, 32, 32), (65536, 32, 32), (1, 0, 600), (1, 32, 1 << 20), (1, 16, 32), (1, 1, 512), (1, 512, 1)):
        assert L.cmdiad_eyecandies_cloud(p, p, B, H, W, p, p, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error(), (B, H, W)
    assert L.cmdiad_eyecandies_cloud(p, p, 1, 32, 32, None, p, p, None) == -1 and b"null pointer" in L.cmdiad_last_error()
    assert L.cmdiad_eyecandies_unproject(p, p, 1, 0, 8, p, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    assert L.cmdiad_eyecandies_unproject(p, p, 1, 8, 8, None, None, None) == -1 and b"null pointer" in L.cmdiad_last_error()
    for n in (512, 0, -1, (1 << 28) + 1):
        assert L.cmdiad_eyecandies_background(p, n, p, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error(), n
    assert L.cmdiad_organized_pc_prep_f64(p, 1, 0, 8, p, p, 4, p, p, 4, p, p, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    assert L.cmdiad_organized_pc_prep_f64(p, 1, 8, 8, p, p, 4, None, None, 4, p, p, p, None) == -1
    assert b"cmdiad_organized_pc_prep_f64" in L.cmdiad_last_error()
    assert L.cmdiad_organized_pc_prep(p, 1, 0, 8, p, p, 4, p, p, 4, p, p, p, None) == -1
    assert b"cmdiad_organized_pc_prep:" in L.cmdiad_last_error()
    # the wrappers: a host tensor is refused with the package's message, a wrong dtype is a TypeError
    tab = (torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(Exception, match="GPU"):
        ops.organized_pc_prep(torch.zeros(1, 8, 8, 3, dtype=torch.float64), tab)
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        ops.organized_pc_prep(torch.zeros(1, 8, 8, 3, dtype=torch.float16), tab)
    prm = torch.stack([ops.eyecandies_params(0.5, 3.1, np.eye(4))])
    code = torch.zeros((1, 32, 32), dtype=torch.uint16)
    with pytest.raises(Exception, match="GPU"):
        ops.eyecandies_cloud(code, prm)
    with pytest.raises(Exception, match="GPU"):
        ops.eyecandies_unproject(code, prm)
    with pytest.raises(Exception, match="GPU"):
        ops.eyecandies_background(torch.zeros(600, 3, dtype=torch.float64))
