"""CPU (no GPU): the host side of sample preparation (docs/sample_prep.md) against Pillow and torch themselves -- the coefficient
and index tables the device kernels are handed, the normalise table, file discovery of the dataset classes, the 'cpu_v1' items
against the PIL + torch composition written inline, and the C ABI of the new entry points."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_prep_ref as spr  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmdiad_resize_bicubic_u8", "cmdiad_organized_pc_prep", "cmdiad_gt_mask_prep")


@pytest.mark.parametrize("h,w,oh,ow", [(800, 800, 224, 224), (512, 512, 224, 224), (100, 130, 224, 224), (37, 801, 224, 518),
                                       (224, 300, 224, 224)])
def test_coefficient_tables_reproduce_pillow_bicubic(h, w, oh, ow):
    img = spr.image("random", h, w, seed=h + w)
    assert np.array_equal(spr.two_pass_resize(img, oh, ow), spr.pil_bicubic(img, oh, ow))


def test_coefficient_tables_on_clamp_and_rounding_images():
    for kind in ("checker", "white"):
        for h, w, oh, ow in ((83, 61, 28, 28), (20, 17, 56, 56), (300, 224, 224, 224)):
            img = spr.image(kind, h, w)
            assert np.array_equal(spr.two_pass_resize(img, oh, ow), spr.pil_bicubic(img, oh, ow)), (kind, h, w)
    from cmdiad_amd.dataset import bicubic_tables
    coef, bounds = bicubic_tables(800, 224)
    assert coef.dtype == np.int32 and bounds.dtype == np.int32 and coef.shape == (224, 17) and bounds.shape == (224, 2)
    assert bounds[:, 0].min() == 0 and (bounds[:, 0] + bounds[:, 1]).max() == 800 and bounds[:, 1].max() <= 17
    assert np.abs(coef.sum(1) - (1 << 22)).max() <= 17          # every row sums to one up to the rounding of its taps


@pytest.mark.parametrize("n_in", [800, 37, 512])
def test_gt_index_table_reproduces_pillow_nearest(n_in):
    from cmdiad_amd.dataset import pillow_nearest_index, torch_nearest_index
    idx = pillow_nearest_index(n_in, 224)
    gt = np.random.RandomState(n_in).randint(0, 256, (n_in, n_in)).astype(np.uint8)
    assert np.array_equal(gt[idx][:, idx], spr.pil_nearest(gt, 224, 224))
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < n_in
    assert not np.array_equal(idx, torch_nearest_index(n_in, 224))          # the two nearest rules differ: each needs its table


def test_cloud_index_rule_is_torch_nearest():
    import torch.nn.functional as F
    from cmdiad_amd.dataset import torch_nearest_index
    for n_in in (800, 50, 70, 224, 300, 513):
        for n_out in (224, 56, 518):
            want = F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None, None], size=(1, n_out), mode="nearest")[0, 0, 0]
            got = torch_nearest_index(n_in, n_out)
            assert got.dtype == np.int32 and np.array_equal(got, want.numpy().astype(np.int32)), (n_in, n_out)


def test_normalize_table_is_the_float32_formula():
    from cmdiad_amd import dataset as ds
    t = ds.normalize_table()
    assert t.shape == (3, 256) and t.dtype == torch.float32
    u8 = torch.arange(256, dtype=torch.uint8)
    for c in range(3):
        want = (u8.to(torch.float32) / 255 - torch.tensor(ds.IMAGENET_MEAN[c], dtype=torch.float32)) / torch.tensor(ds.IMAGENET_STD[c], dtype=torch.float32)
        assert torch.equal(t[c], want)
    # and the mask threshold of the device path: float32 v / 255 > 0.5 exactly for v >= 128
    assert torch.equal(u8.to(torch.float32).div(255) > 0.5, u8 >= 128)


def _args(root, method="cpu_v1"):
    return types.SimpleNamespace(dataset_path=str(root), img_process_method=method, num_workers=0, rgb_size=224, xyz_size=224, gt_size=224)


def test_file_discovery_and_cpu_v1_items(tmp_path, monkeypatch):
    from PIL import Image
    from cmdiad_amd import dataset as ds
    from cmdiad_amd.utils import mvtec3d_util as mu
    items = spr.write_tree(str(tmp_path))
    spr.patch_tiff_reader(monkeypatch)
    (tmp_path / "bagel" / "test" / "good" / "rgb" / "notes.txt").write_text("not a sample")
    train = ds.TrainDataset("bagel", 224, 224, 224, str(tmp_path), "cpu_v1")
    assert len(train) == 3 and train.labels == [0, 0, 0]
    assert [(p.name, q.name) for p, q in train.img_paths] == [(f"{i:03d}.png", f"{i:03d}.tiff") for i in range(3)]
    test = ds.TestDataset("bagel", 224, 224, 224, str(tmp_path), "cpu_v1")
    # sorted defect directories: crack before good; pairs stay pairs; gt only for the defect type
    assert [str(p.parent.parent.name) for p, _ in test.img_paths] == ["crack", "crack", "good", "good"]
    assert all(p.stem == q.stem and p.parent.parent == q.parent.parent for p, q in test.img_paths)
    assert test.labels == [1, 1, 0, 0] and [g if g == 0 else g.name for g in test.gt_paths] == ["000.png", "001.png", 0, 0]
    (tmp_path / "bagel" / "validation" / "good" / "rgb").mkdir(parents=True)
    (tmp_path / "bagel" / "validation" / "good" / "xyz").mkdir(parents=True)
    assert len(ds.TrainValidationDataset("bagel", 224, 224, 224, str(tmp_path), "cpu_v2")) == 3
    for cls in (ds.TrainDataset, ds.TestDataset):
        with pytest.raises(ValueError, match="cpu_v1.*cpu_v2.*hip"):
            cls("bagel", 224, 224, 224, str(tmp_path), "gpu")
    with pytest.raises(ValueError):
        ds.get_data_loader("nope", "bagel", 224, 224, 224, _args(tmp_path))
    # a pair that has lost its gt: the reference's assertion
    os.remove(tmp_path / "bagel" / "test" / "crack" / "gt" / "001.png")
    with pytest.raises(AssertionError, match="ground truth pair"):
        ds.TestDataset("bagel", 224, 224, 224, str(tmp_path), "cpu_v1")
    Image.fromarray(items["test/crack/001"][2], "L").save(tmp_path / "bagel" / "test" / "crack" / "gt" / "001.png")

    # 'cpu_v1' items == the PIL + torch composition, bit for bit (rgb_size 224 and the DINOv2 size; gt at a size of its own)
    mean, std = torch.tensor(ds.IMAGENET_MEAN).view(3, 1, 1), torch.tensor(ds.IMAGENET_STD).view(3, 1, 1)
    for rgb_size, gt_size in ((224, 224), (518, 112)):
        test = ds.TestDataset("bagel", rgb_size, 224, gt_size, str(tmp_path), "cpu_v1")
        for i, key in enumerate(("test/crack/000", "test/crack/001", "test/good/000", "test/good/001")):
            pc, rgb, gt = items[key]
            (img, cloud, depth), mask, label, path = test[i]
            pil = Image.fromarray(rgb).resize((rgb_size, rgb_size), Image.BICUBIC)
            want = (torch.from_numpy(np.array(pil)).permute(2, 0, 1).float().div(255) - mean) / std
            assert img.dtype == torch.float32 and torch.equal(img, want)
            assert torch.equal(cloud, mu.resize_organized_pc(pc)) and cloud.dtype == torch.float32
            assert torch.equal(depth, mu.resize_organized_pc(np.repeat(pc[:, :, 2:3], 3, 2))) and depth.shape == (3, 224, 224)
            if gt is None:
                assert mask.shape == (1, 224, 224) and not mask.any() and label == 0
            else:
                g = torch.from_numpy(np.array(Image.fromarray(gt, "L").resize((gt_size, gt_size), Image.NEAREST)))[None].float().div(255)
                assert torch.equal(mask, torch.where(g > 0.5, 1., .0)) and mask.shape == (1, gt_size, gt_size) and label == 1
                assert 0 < mask.sum() < mask.numel()
            assert path.endswith(key.split("/", 1)[1].replace("/", os.sep + "rgb" + os.sep) + ".png")
    (s, label) = ds.TrainDataset("bagel", 224, 224, 224, str(tmp_path), "cpu_v2")[1]
    assert label == 0 and torch.equal(s[1], mu.resize_organized_pc(items["train/good/001"][0]))

    # the loader and the class source on the host path: the reference's batch-of-one items, in order
    loader = ds.get_data_loader("test", "bagel", 224, 224, 224, _args(tmp_path))
    got = list(loader)
    assert len(got) == 4 and got[0][0][0].shape == (1, 3, 224, 224) and got[0][1].shape == (1, 1, 224, 224)
    assert [int(g[2]) for g in got] == [1, 1, 0, 0] and got[2][3][0].endswith(os.path.join("good", "rgb", "000.png"))
    data = ds.dataset_classes(_args(tmp_path))
    assert list(data) == ["bagel"] and (data["bagel"].name, data["bagel"].n_train, data["bagel"].n_test) == ("bagel", 3, 4)
    assert len(list(data["bagel"].train())) == 3
    with pytest.raises(FileNotFoundError):
        ds.dataset_classes(types.SimpleNamespace(**{**vars(_args(tmp_path)), "dataset_type": "eyecandies"}))
    assert ds.mvtec3d_classes()[0] == "bagel" and len(ds.mvtec3d_classes()) == 10 and len(ds.eyecandies_classes()) == 10
    if not torch.cuda.is_available():      # 'hip' discovers the same files and needs a GPU for the items: no host fallback
        hip = ds.TestDataset("bagel", 224, 224, 224, str(tmp_path), "hip")
        assert hip.img_paths == test.img_paths
        with pytest.raises(Exception, match="GPU"):
            hip[0]


def test_new_entry_points_are_declared_bound_and_reject_bad_arguments():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    assert L.cmdiad_abi_version() == 6
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    declared = set(re.findall(r"\b(cmdiad_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(L, name)
        args = [None if a is ctypes.c_void_p else 1 for a in nat.SIGNATURES[name]]
        assert getattr(L, name)(*args) == -1 and b"null pointer" in L.cmdiad_last_error(), name
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # bad sizes with valid-looking pointers: rejected before anything is launched
    assert L.cmdiad_resize_bicubic_u8(p, 0, 8, 8, 4, 4, p, p, 5, p, p, 5, p, p, p, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    assert L.cmdiad_resize_bicubic_u8(p, 1, 8, 8, 4, 4, p, p, 0, p, p, 5, p, p, p, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    assert L.cmdiad_resize_bicubic_u8(p, 1, 8, 8, 4, 4, p, p, 5, p, p, 5, None, p, p, p, None) == -1      # both sides change: tmp is needed
    assert L.cmdiad_resize_bicubic_u8(p, 1, 8, 8, 4, 4, p, p, 5, p, p, 5, p, None, None, p, None) == -1   # float output without the table
    assert L.cmdiad_resize_bicubic_u8(p, 1, 8, 8, 4, 1 << 20, p, p, 5, p, p, 5, p, p, p, p, None) == -1
    assert L.cmdiad_organized_pc_prep(p, 1, 0, 8, p, p, 4, p, p, 4, p, p, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    assert L.cmdiad_organized_pc_prep(p, 1, 8, 8, p, p, 4, None, None, 4, p, p, p, None) == -1            # depth wanted without its tables
    assert L.cmdiad_gt_mask_prep(p, 1, 8, 8, p, p, -3, p, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    from cmdiad_amd import ops
    with pytest.raises(Exception, match="GPU"):
        ops.gt_mask_prep(torch.zeros(1, 8, 8, dtype=torch.uint8), (torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(Exception, match="GPU"):
        ops.organized_pc_prep(torch.zeros(1, 8, 8, 3), (torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(Exception, match="GPU"):
        ops.resize_bicubic_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4, 4, None, None)
