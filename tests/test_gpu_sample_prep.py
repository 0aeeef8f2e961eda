"""GPU: sample preparation on the device (csrc/sample_prep.hip, cmdiad_amd.dataset.SamplePrep; docs/sample_prep.md) against Pillow
and torch on the host -- every comparison is for EQUAL BYTES: the resize is Pillow's integer arithmetic, the float stage a table
torch built, the cloud and the mask are gathers."""
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_prep_ref as spr  # noqa: E402

from cmdiad_amd import dataset as ds  # noqa: E402
from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd.utils import mvtec3d_util as mu  # noqa: E402

DEV = "cuda"


def _resize(img, oh, ow, want_f32=False):
    h, w = img.shape[:2]
    tab = lambda n_in, n_out: tuple(torch.from_numpy(a).to(DEV) for a in ds.bicubic_tables(n_in, n_out)) if n_in != n_out else None  # noqa: E731
    u8, f32 = ops.resize_bicubic_u8(torch.from_numpy(img)[None].to(DEV), oh, ow, tab(w, ow), tab(h, oh), ds.normalize_table().to(DEV),
                                    want_u8=True, want_f32=want_f32)
    return u8[0].cpu().numpy(), (f32[0].cpu() if want_f32 else None)


@pytest.mark.parametrize("h,w,oh,ow", [(83, 61, 28, 28), (20, 17, 56, 56), (224, 300, 224, 224), (300, 224, 224, 224)])
@pytest.mark.parametrize("kind", ["random", "checker", "white"])
def test_resize_equals_pillow_byte_for_byte(kind, h, w, oh, ow):
    img = spr.image(kind, h, w, seed=h)
    got, _ = _resize(img, oh, ow)
    want = spr.pil_bicubic(img, oh, ow)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


def test_resize_800_equals_pillow_byte_for_byte():
    img = spr.image("random", 800, 800, seed=5)
    got, _ = _resize(img, 224, 224)
    assert np.array_equal(got, spr.pil_bicubic(img, 224, 224))


def test_float_output_is_torch_s_normalize_bit_for_bit():
    # every value 0..255 in every channel, before and after the resize (the ramp is constant along x: an upscale along x keeps it)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 40, 1).repeat(3, 2)
    ramp[:, :, 1] = ramp[::-1, :, 0]
    ramp[:, :, 2] = np.roll(ramp[:, :, 0], 77, 0)
    mean, std = torch.tensor(ds.IMAGENET_MEAN).view(3, 1, 1), torch.tensor(ds.IMAGENET_STD).view(3, 1, 1)
    for oh, ow in ((256, 64), (256, 40), (224, 224)):          # horizontal pass only, no pass at all, both passes
        u8, f32 = _resize(ramp, oh, ow, want_f32=True)
        if oh == 256:
            assert all(len(np.unique(u8[:, :, c])) == 256 for c in range(3))
        assert np.array_equal(u8, spr.pil_bicubic(ramp, oh, ow))
        want = (torch.from_numpy(u8).permute(2, 0, 1).float().div(255) - mean) / std
        assert f32.dtype == torch.float32 and torch.equal(f32, want)


@pytest.mark.parametrize("h,w", [(50, 70), (800, 800)])
def test_cloud_depth_and_count(h, w):
    pc = spr.cloud(h, w, seed=h)
    one_zero = ((pc == 0).sum(2) == 1).sum()
    assert one_zero > 0 and 0.3 < (pc == 0).all(2).mean() < 0.5
    prep = ds.SamplePrep(224, 224, 224, DEV)
    sample, gt = prep.prepare(spr.image("random", h, w), pc)
    assert gt is None and all(t.is_cuda for t in sample)
    want_cloud = mu.resize_organized_pc(pc)
    assert torch.equal(sample[1].cpu(), want_cloud)
    assert torch.equal(sample[2].cpu(), mu.resize_organized_pc(np.repeat(pc[:, :, 2:3], 3, 2)))
    want_n = int(np.count_nonzero(np.all(want_cloud.numpy().reshape(3, -1) != 0, axis=0)))
    assert sample.n_valid == want_n and int(sample.n_valid_dev.cpu()) == want_n and sample.n_valid_dev.dtype == torch.int32
    assert sample.batched().n_valid == want_n and sample.batched()[1].shape == (1, 3, 224, 224)
    # a cloud size of its own (xyz_size != 224): the depth map stays at 224
    s2, _ = ds.SamplePrep(224, 112, 224, DEV).prepare(spr.image("random", h, w), pc)
    assert torch.equal(s2[1].cpu(), mu.resize_organized_pc(pc, 112, 112)) and s2[2].shape == (3, 224, 224)


def test_gt_mask_equals_pil_nearest_and_threshold():
    rs = np.random.RandomState(3)
    for h, w, g in ((800, 800, 224), (37, 61, 224), (512, 300, 112)):
        gt = rs.randint(0, 256, (h, w)).astype(np.uint8)
        gt[: h // 2] = np.where(rs.rand(h // 2, w) < 0.5, 127, 128)          # right on the > 0.5 boundary
        _, mask = ds.SamplePrep(224, 224, g, DEV).prepare(spr.image("white", h, w), spr.cloud(h, w), gt)
        t = torch.from_numpy(spr.pil_nearest(gt, g, g))[None].float().div(255)
        want = torch.where(t > 0.5, 1., .0)
        assert mask.shape == (1, g, g) and mask.dtype == torch.float32 and torch.equal(mask.cpu(), want)
        assert 0.2 < want.mean() < 0.8


def test_batch_invariance():
    """Four samples of three sizes, together and alone: identical bytes (and identical to the host path)."""
    shapes = [(83, 61), (300, 300), (83, 61), (120, 200)]
    rgbs = [spr.image("random", h, w, seed=i) for i, (h, w) in enumerate(shapes)]
    pcs = [spr.cloud(h, w, seed=10 + i) for i, (h, w) in enumerate(shapes)]
    gts = [None, (np.random.RandomState(1).rand(300, 300) < 0.3).astype(np.uint8) * 255, np.full((83, 61), 128, np.uint8), None]
    prep = ds.SamplePrep(224, 224, 224, DEV)
    together = prep.prepare_batch(rgbs, pcs, gts)
    for i in range(4):
        (s, m), (s1, m1) = together[i], prep.prepare(rgbs[i], pcs[i], gts[i])
        assert all(torch.equal(a, b) for a, b in zip(s, s1)) and s.n_valid == s1.n_valid
        assert (m is None and m1 is None) if gts[i] is None else torch.equal(m, m1)
        from PIL import Image
        assert torch.equal(s[0].cpu(), ds.host_rgb_transform(Image.fromarray(rgbs[i]), 224))
        assert torch.equal(s[1].cpu(), ds.host_cloud_transform(pcs[i], 224)[0])


def _args(root, method, **kw):
    a = dict(rgb_backbone_name='vit_base_patch8_224_dino', xyz_backbone_name='Point_MAE', group_size=32, num_group=64,
             rgb_size=224, xyz_size=224, gt_size=224, f_coreset=1.0, coreset_eps=0.9, coreset_dtype='FP16',
             random_state=None, dist_method_s='l2', dist_method_coreset='l2', main_modality='', use_hn=False,
             fusion_module_path='', ocsvm_nu=0.5, ocsvm_maxiter=1000, xyz_s_lambda=1.0, xyz_smap_lambda=1.0,
             rgb_s_lambda=0.1, rgb_smap_lambda=0.1, fusion_s_lambda=1.0, fusion_smap_lambda=1.0,
             save_feature_for_fusion=False, save_seg_results=False, use_depth=False,
             dataset_path=str(root), img_process_method=method, num_workers=0)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_end_to_end_device_samples_equal_host_samples(tmp_path, monkeypatch):
    """DoubleRGBPointFeatures over the same 3 train + 2 test files, once from 'cpu_v1' host tensors and once from 'hip' device samples (both
    through MVTec3DClass): both libraries, image_preds and pixel_preds are identical, and on the device path no sample tensor is moved to
    the host inside _extract_batch."""
    from sklearn import linear_model
    from cmdiad_amd.feature_extractors import multiple_features as mf
    spr.write_tree(str(tmp_path))
    spr.patch_tiff_reader(monkeypatch)
    out = {}
    for method in ("cpu_v1", "hip"):
        args = _args(tmp_path, method)
        data = ds.MVTec3DClass(str(tmp_path), "bagel", args)
        assert (data.n_train, data.n_test) == (3, 4)
        train = list(data.train())
        tests = [t for i, t in enumerate(data.test()) if i in (0, 2)]          # one defect sample (with gt), one good sample
        torch.manual_seed(7)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = mf.DoubleRGBPointFeatures(args)
        sample_ptrs = {t.data_ptr() for item in train + tests for t in item[0]}
        inside, moved = [False], []
        real_extract, real_cpu = mf.DoubleRGBPointFeatures._extract_batch, torch.Tensor.cpu

        def extract(self, *a, **k):
            inside[0] = True
            try:
                return real_extract(self, *a, **k)
            finally:
                inside[0] = False

        def cpu(t, *a, **k):
            if inside[0] and t.data_ptr() in sample_ptrs:
                moved.append(tuple(t.shape))
            return real_cpu(t, *a, **k)

        monkeypatch.setattr(mf.DoubleRGBPointFeatures, "_extract_batch", extract)
        monkeypatch.setattr(torch.Tensor, "cpu", cpu)
        try:
            for sample, label in train:
                assert int(label) == 0
                m.add_sample_to_mem_bank(sample, class_name="bagel")
            m.run_coreset()
            rs = np.random.RandomState(0)
            m.detect_fuser = linear_model.SGDOneClassSVM(random_state=42, nu=0.5, max_iter=1000).fit(rs.rand(64, 2))
            m.seg_fuser = linear_model.SGDOneClassSVM(random_state=42, nu=0.5, max_iter=1000).fit(rs.rand(4096, 2))
            for sample, mask, label, path in tests:
                m.predict(sample, mask, label, path)
            preds = np.concatenate([np.asarray(v).ravel() for v in m.image_preds])
        finally:
            monkeypatch.setattr(mf.DoubleRGBPointFeatures, "_extract_batch", real_extract)
            monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
        if method == "hip":
            assert all(t.is_cuda for item in train + tests for t in item[0]) and not tests[0][1].is_cuda
            assert moved == [] and m.__dict__.get("device_sample_batches", 0) >= 2
        else:
            assert "device_sample_batches" not in m.__dict__
        out[method] = ((m.patch_xyz_lib.cpu(), m.patch_rgb_lib.cpu()), preds, np.asarray(m.pixel_preds), np.asarray(m.pixel_labels),
                       [int(np.asarray(v).ravel()[0]) for v in m.image_labels], [n[0] for n in m.img_name])
    a, b = out["cpu_v1"], out["hip"]
    assert all(x.shape[0] > 0 and x.shape[0] % 3 == 0 and torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a[4] == b[4] == [1, 0] and a[5] == b[5] and a[3].sum() > 0
