"""GPU: Eyecandies depth maps to clouds and samples on the device (csrc/eyecandies.hip, cmdiad_amd.utils.preprocessing_eyecandies,
cmdiad_amd.dataset.EyecandiesRawClass; docs/eyecandies.md) against the numpy restatement of the documented operation order
(tests/eyecandies_ref.py, itself checked against the reference in tests/test_eyecandies_cpu.py) -- every comparison is for EQUAL
BITS: the kernel rounds once per written operation, in the written order."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eyecandies_ref as er  # noqa: E402

from cmdiad_amd import dataset as ds  # noqa: E402
from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd.utils import preprocessing_eyecandies as pe  # noqa: E402

DEV = "cuda"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _device_inputs(scans):
    """[(code, mind, maxd, pose, focal)] of one shape -> (codes [B,H,W] uint16, params [B,136] uint8) on the device."""
    h, w = scans[0][0].shape
    code = torch.from_numpy(np.stack([s[0] for s in scans])).to(DEV)
    prm = torch.stack([ops.eyecandies_params(s[1], s[2], er.inv_projection(s[3], h, w, s[4])) for s in scans]).to(DEV)
    return code, prm


def _host_cloud(pc):
    """host_cloud_transform of a float64 cloud: the cloud comes back as float32 (the reference's .float()), the depth map in the
    cloud's own float64 (dataset.py:108-109 never converts it); the device's depth map is float32, the same rounding of the same z."""
    cloud, depth = ds.host_cloud_transform(pc, 224)
    assert cloud.dtype == torch.float32 and depth.dtype == torch.float64
    return cloud, depth.to(torch.float32)


def _run(scans, **kw):
    cloud, removed, depth = ops.eyecandies_cloud(*_device_inputs(scans), **kw)
    return cloud.cpu().numpy(), (None if removed is None else removed.cpu().numpy()), (None if depth is None else depth.cpu().numpy())


@pytest.mark.parametrize("mind,maxd", [(0.5, 3.1), (0.1, 0.1 + 2.0 / 3.0)])
def test_depth_of_every_code_is_bit_equal(mind, maxd):
    """256 x 256 holding every uint16 code once; the second range is not representable in float32."""
    code = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    assert len(np.unique(code)) == 65536
    pose = er.synthetic_scan(1, 24, 32)[1]
    _, _, depth = _run([(code, mind, maxd, pose, er.FOCAL_LENGTH)], want_depth=True)
    assert _same_bits(depth[0], er.depth(code, mind, maxd))
    only, = ops.eyecandies_unproject(*_device_inputs([(code, mind, maxd, pose, er.FOCAL_LENGTH)]), want_points=False, want_depth=True)[1:]
    assert _same_bits(only[0].cpu().numpy(), depth[0])


@pytest.mark.parametrize("h,w", [(23, 29), (512, 512)])
def test_cloud_and_removed_are_bit_equal_to_the_restatement(h, w):
    code, pose, focal = er.synthetic_scan(h + w, h, w)
    want = er.restate(code, 0.5, 3.1, pose, focal)
    assert 0.2 < want["removed"].mean() < 0.8
    cloud, removed, depth = _run([(code, 0.5, 3.1, pose, focal)], want_depth=True)
    assert removed.dtype == np.uint8 and np.array_equal(removed[0].astype(bool), want["removed"])
    assert _same_bits(depth[0], want["depth"])
    assert _same_bits(cloud[0], want["cloud"]), int((_bits(cloud[0]) != _bits(want["cloud"])).sum())
    # removed points sit on ONE point that is not the origin (its x is an exact +0.0)
    collapsed = cloud[0][want["removed"]]
    assert np.all(_bits(collapsed) == _bits(collapsed[:1])) and collapsed[0, 0] == 0 and not np.signbit(collapsed[0, 0])
    assert collapsed[0, 1] != 0 and collapsed[0, 2] != 0
    # without the optional outputs: the same cloud
    alone, none_r, none_d = _run([(code, 0.5, 3.1, pose, focal)], want_removed=False)
    assert none_r is None and none_d is None and _same_bits(alone, cloud)


def test_stages_alone_and_the_module_surface():
    """unproject + background as two launches == the fused launch; cloud_arrays and remove_point_cloud_background (numpy in, numpy
    out) return the same bits; a zero depth gives NaN coordinates and is kept, as in the reference."""
    code, pose, focal = er.synthetic_scan(9, 23, 29)
    code[3, 4] = 0
    want = er.restate(code, 0.0, 3.1, pose, focal)
    assert np.isnan(want["cloud"][3, 4]).any() and not want["removed"][3, 4]
    c, p = _device_inputs([(code, 0.0, 3.1, pose, focal)])
    fused, removed, _ = ops.eyecandies_cloud(c, p)
    points, _ = ops.eyecandies_unproject(c, p)
    assert _same_bits(points[0].cpu().numpy(), want["points"])
    two, removed2 = ops.eyecandies_background(points[0])
    assert torch.equal(two.view(torch.int64), fused[0].reshape(-1, 3).view(torch.int64)) and torch.equal(removed2, removed[0].reshape(-1))
    assert _same_bits(fused[0].cpu().numpy(), want["cloud"])
    cloud, mask = pe.cloud_arrays(code, 0.0, 3.1, pose, focal)
    assert mask.dtype == np.bool_ and np.array_equal(mask, want["removed"]) and _same_bits(cloud, want["cloud"])
    assert _same_bits(pe.remove_point_cloud_background(want["points"]), want["cloud"].reshape(-1, 3))
    # lists: scans of two shapes, every result the single call's
    code2, pose2, focal2 = er.synthetic_scan(10, 24, 32)
    clouds, masks = pe.cloud_arrays([code, code2, code], [0.0, 0.5, 0.0], [3.1, 3.1, 3.1], [pose, pose2, pose], focal)
    assert _same_bits(clouds[0], cloud) and _same_bits(clouds[2], cloud) and np.array_equal(masks[0], mask)
    assert _same_bits(clouds[1], er.restate(code2, 0.5, 3.1, pose2, focal)["cloud"])


def test_batch_of_three_parameter_blocks_equals_three_single_calls():
    scans = []
    for i in range(3):
        code, pose, focal = er.synthetic_scan(20 + i, 24, 32, mind=0.5 + 0.1 * i, maxd=3.1 + 0.2 * i)
        pose = pose.copy()
        pose[:3, 3] += 0.01 * i
        scans.append((code, 0.5 + 0.1 * i, 3.1 + 0.2 * i, pose, focal))
    singles = [_run([s], want_depth=True) for s in scans]
    assert not np.array_equal(singles[0][0], singles[1][0]) and not np.array_equal(singles[1][0], singles[2][0])
    for stream in (None, torch.cuda.Stream()):
        if stream is None:
            cloud, removed, depth = _run(scans, want_depth=True)
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                cloud, removed, depth = _run(scans, want_depth=True)
            stream.synchronize()
        for i, (c1, r1, d1) in enumerate(singles):
            assert _same_bits(cloud[i], c1[0]) and np.array_equal(removed[i], r1[0]) and _same_bits(depth[i], d1[0])
            assert _same_bits(cloud[i], er.restate(*scans[i])["cloud"])


def test_float64_cloud_prep_equals_the_host_transform():
    """organized_pc_prep on a float64 cloud: values that round to either float32 neighbour, exact zeros, points with ONE zero
    coordinate, a non-square shape -- cloud, depth and count as host_cloud_transform and numpy's all(p != 0) give them."""
    rs = np.random.RandomState(5)
    h, w = 50, 70
    pc = rs.rand(h, w, 3) * np.array([0.2, 0.2, 0.6]) + 0.05
    f32 = pc.astype(np.float32).astype(np.float64)
    assert (f32 > pc).mean() > 0.3 and (f32 < pc).mean() > 0.3              # both rounding directions occur
    up = np.nextafter(np.float32(0.25), np.float32(1)).astype(np.float64)
    pc[rs.rand(h, w) < 0.4] = 0.0
    one = rs.rand(h, w) < 0.05
    pc[one, rs.randint(0, 3, int(one.sum()))] = 0.0
    pc[0, 0] = [(0.25 + up) / 2, 0.25 + (up - 0.25) * 0.49, 0.25 + (up - 0.25) * 0.51]      # a tie (to even), just below, just above
    pc[1, 1] = [1e-60, 0.3, 0.3]                                            # rounds to a float32 zero: not a valid point
    prep = ds.SamplePrep(224, 224, 224, DEV)
    rgb = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    sample, _ = prep.prepare(rgb, pc)
    want_cloud, want_depth = _host_cloud(pc)
    assert sample[1].dtype == torch.float32 and torch.equal(sample[1].cpu(), want_cloud) and torch.equal(sample[2].cpu(), want_depth)
    want_n = int(np.count_nonzero(np.all(want_cloud.numpy().reshape(3, -1) != 0, axis=0)))
    assert sample.n_valid == want_n and 0 < want_n < 224 * 224
    # the float32 entry point and its results do not change; a batch of both dtypes keeps every sample's bytes
    pc32 = pc.astype(np.float32)
    both = prep.prepare_batch([rgb, rgb], [pc32, pc])
    assert torch.equal(both[0][0][1].cpu(), ds.host_cloud_transform(pc32, 224)[0]) and torch.equal(both[1][0][1], sample[1])
    assert torch.equal(both[0][0][1], both[1][0][1]) and both[0][0].n_valid == both[1][0].n_valid == want_n
    with pytest.raises(TypeError, match="float32.*float64"):
        prep.prepare(rgb, pc.astype(np.float16))


def _args(root, **kw):
    from cmdiad_amd import evaluate as ev
    return ev.mtfi_args(dataset_path=str(root), img_process_method="hip", num_workers=2, dataset_type="eyecandies", **kw)


def test_raw_class_samples_equal_the_host_transforms(tmp_path):
    from PIL import Image
    items = er.write_raw_tree(str(tmp_path), "CandyCane", n_train=2, n_test=3, bad=(1,))
    cls = ds.EyecandiesRawClass(str(tmp_path), "CandyCane", _args(tmp_path))
    train, test = list(cls.train()), list(cls.test())
    assert len(train) == 2 and len(test) == 3
    assert [int(t[2]) for t in test] == [1, 0, 0] and [int(t[1]) for t in train] == [0, 0]
    order = [("test", 1), ("test", 0), ("test", 2)]
    assert [t[3] for t in test] == [[items[k]["rgb_path"]] for k in order]
    for got, key in list(zip(train, [("train", 0), ("train", 1)])) + list(zip(test, order)):
        it = items[key]
        sample = got[0]
        want = er.restate(it["code"], it["mind"], it["maxd"], it["pose"])
        assert 0.1 < want["removed"].mean() < 0.9
        want_cloud, want_depth = _host_cloud(want["cloud"])
        assert all(t.is_cuda and t.dtype == torch.float32 and t.shape == (1, 3, 224, 224) for t in sample)
        assert torch.equal(sample[0][0].cpu(), ds.host_rgb_transform(Image.fromarray(it["rgb"]), 224))
        assert torch.equal(sample[1][0].cpu(), want_cloud) and torch.equal(sample[2][0].cpu(), want_depth)
        # valid points: the collapsed point's x is an exact zero, so it is not one; every kept pixel is
        n = int(np.count_nonzero(np.all(want_cloud.numpy().reshape(3, -1) != 0, axis=0)))
        kept = ~want["removed"][ds.torch_nearest_index(40, 224)][:, ds.torch_nearest_index(48, 224)]
        assert sample.n_valid == n == int(kept.sum())
        if key[0] == "test":
            mask = got[1]
            assert not mask.is_cuda and mask.shape == (1, 1, 224, 224)
            if key[1] == 1:
                gt = Image.fromarray(it["mask"]).convert('RGB').convert('L')
                assert torch.equal(mask[0], ds.host_gt_transform(gt, 224)) and 0 < mask.sum() < mask.numel()
            else:
                assert not mask.any()


def test_too_few_pixels_are_rejected_before_launch():
    code = torch.from_numpy(np.zeros((1, 16, 32), np.uint16)).to(DEV)
    prm = torch.stack([ops.eyecandies_params(0.5, 3.1, np.eye(4))]).to(DEV)
    with pytest.raises(Exception, match="bad sizes.*H\\*W >= 513"):
        ops.eyecandies_cloud(code, prm)
    with pytest.raises(Exception, match="bad sizes"):
        ops.eyecandies_background(torch.zeros((512, 3), dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    ops.eyecandies_cloud(torch.from_numpy(np.full((1, 19, 27), 30000, np.uint16)).to(DEV), prm)      # 513 pixels: accepted
    torch.cuda.synchronize()


def test_evaluate_classes_runs_a_raw_class_end_to_end(tmp_path):
    """One class of the raw tree through evaluate.evaluate_classes (drop-in WithHallucination, main modality xyz): the class loop takes
    its samples from EyecandiesRawClass as it takes them from MVTec3DClass."""
    from cmdiad_amd import evaluate as ev
    from oracle import nets
    er.write_raw_tree(str(tmp_path), "CandyCane", n_train=2, n_test=3, bad=(1,))
    a = _args(tmp_path, f_coreset=0.5, random_state=3)
    data = ds.dataset_classes(a)
    assert list(data) == ["CandyCane"] and isinstance(data["CandyCane"], ds.EyecandiesRawClass)
    weights = (nets.synth_state_dict("vit", 31), nets.sharpen_pointmae(nets.synth_state_dict("pointmae", 21)),
               nets.synth_state_dict("halluc", 51))
    res = ev.evaluate_classes(a, data, weights=weights)
    got = res["per_class"]["CandyCane"]
    assert got["n_train"] == 2 and got["n_test"] == 3
    assert got["phases"] == ["memory_bank", "coreset", "late_fusion_bank", "late_fusion_fit", "predict", "metrics"]
    assert all(np.isfinite(got[k]) for k in ("image_rocauc", "pixel_rocauc", "au_pro"))
