"""GPU: MVTec 3D-AD from the raw download -- the scan-cleaning chain that stays on the device (cmdiad_scan_edges, cmdiad_scan_compact,
cmdiad_keep_largest_cluster, utils.preprocessing.preprocess_on_device) and dataset.MVTec3DRawClass.  The yardsticks are numpy, the
numpy / scipy restatement of tests/preprocess_ref.py and tests/golden/gpp_preprocess.npz; preprocess_arrays is not one (it runs on the
code under test).  Everything here is integer or copy work on top of the two float64 contracts of docs/preprocessing.md: every
comparison is for equal bits."""
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as pr  # noqa: E402
import sample_prep_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ kernels
def _planted():
    """23 x 31 with a NaN and a -0.0 coordinate in border pixels: numpy keeps the first, drops the second."""
    pc = np.ascontiguousarray(sr.cloud(23, 31, seed=3, zero_frac=0.2))
    pc[0, 5] = [0.1, np.nan, 0.3]
    pc[22, 30] = [0.1, -0.0, 0.3]
    pc[4, 0] = [np.nan, np.nan, np.nan]
    pc[11, 30] = [-0.0, -0.0, -0.0]
    return pc


EDGE_SCENES = {"23x31": lambda: sr.cloud(23, 31, seed=1), "64x200": lambda: sr.cloud(64, 200, seed=2), "10x10": lambda: sr.cloud(10, 10, seed=3),
               "7x40": lambda: sr.cloud(7, 40, seed=4), "nan_negzero": _planted}


@pytest.mark.parametrize("scene", sorted(EDGE_SCENES))
def test_edges_equal_get_edges_of_pc(scene):
    """ops.scan_edges == preprocessing.get_edges_of_pc: the same points in the same order, the same count -- on a contiguous scan and
    on the same scan read as the window of a larger padded buffer (row pitch)."""
    from cmdiad_amd import ops
    from cmdiad_amd.utils import preprocessing as mod
    pc = np.ascontiguousarray(EDGE_SCENES[scene]())
    want = mod.get_edges_of_pc(pc)
    assert _same(want, pr.get_edges(pc))
    if scene == "nan_negzero":
        assert np.isnan(want).any() and not np.any((want == 0) & np.signbit(want))
    h, w = pc.shape[:2]
    big = torch.full((h + 9, w + 14, 3), 7.0, dtype=torch.float32, device=DEV)      # non-zero surroundings: reading them would show
    big[4:4 + h, 9:9 + w] = _dev(pc)
    for src in (_dev(pc), big[4:4 + h, 9:9 + w]):
        points, count = ops.scan_edges(src)
        n = int(count.item())
        assert points.shape == (2 * min(10, h) * w + 2 * min(10, w) * h, 3)
        assert n == len(want) and _same(points[:n].cpu().numpy(), want)


COMPACT_SCENES = {"1x1_zero": lambda: np.zeros((1, 1, 3), np.float32), "1x1_valid": lambda: np.full((1, 1, 3), 0.5, np.float32),
                  "7x300": lambda: sr.cloud(7, 300, seed=5), "257x129": lambda: sr.cloud(257, 129, seed=6),
                  "64x64_all_valid": lambda: sr.cloud(64, 64, seed=7, zero_frac=0.0) + np.float32(1.0),
                  "64x64_all_zero": lambda: np.zeros((64, 64, 3), np.float32), "nan_negzero": _planted}


@pytest.mark.parametrize("scene", sorted(COMPACT_SCENES))
def test_compaction_equals_numpy_nonzero(scene):
    """ops.scan_compact == np.nonzero(np.all(pc != 0, axis=1)) and the gathered points, in raster order; twice the same."""
    from cmdiad_amd import ops
    pc = np.ascontiguousarray(COMPACT_SCENES[scene]().astype(np.float32))
    flat = pc.reshape(-1, 3)
    want = np.nonzero(np.all(flat != 0, axis=1))[0]
    if scene == "64x64_all_valid":
        assert len(want) == 64 * 64
    for _ in range(2):
        points, index, count = ops.scan_compact(_dev(pc))
        n = int(count.item())
        assert n == len(want)
        assert np.array_equal(index[:n].cpu().numpy(), want.astype(np.int32)) and _same(points[:n].cpu().numpy(), flat[want])


def _numpy_keep(labels, index, pc, rgb):
    ids, sizes = np.unique(labels, return_counts=True)
    winner = int(ids[np.argmax(sizes)])
    out = index[labels != winner]
    pc, rgb = pc.copy(), rgb.copy()
    pc.reshape(-1, 3)[out] = 0
    rgb.reshape(-1, rgb.shape[-1])[out] = 0
    return winner, pc, rgb


def _label_cases():
    rs = np.random.RandomState(9)
    mix = lambda counts: rs.permutation(np.concatenate([np.full(n, lab, np.int32) for lab, n in counts.items()]))  # noqa: E731
    return {"unique_largest": mix({-1: 40, 0: 300, 1: 120, 2: 299}),
            "noise_majority": mix({-1: 500, 0: 200, 1: 100}),
            "noise_tied_with_cluster_0": mix({-1: 250, 0: 250, 1: 100}),
            "clusters_2_and_5_tied": mix({-1: 10, 0: 50, 1: 60, 2: 200, 3: 70, 4: 5, 5: 200}),
            "no_cluster": np.full(700, -1, np.int32),
            "single_point": np.zeros(1, np.int32)}


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("case", sorted(_label_cases()))
def test_keep_largest_cluster_equals_the_numpy_rule(case, channels):
    """ops.keep_largest_cluster on hand-made labels against np.unique + argmax: the first maximum wins, noise included."""
    from cmdiad_amd import ops
    labels = _label_cases()[case]
    N = len(labels)
    rs = np.random.RandomState(N)
    h, w = 40, 50
    index = np.sort(rs.permutation(h * w)[:N]).astype(np.int32)
    pc = (rs.rand(h, w, 3).astype(np.float32) + 0.5)
    rgb = rs.randint(1, 255, (h, w, channels)).astype(np.uint8)
    winner, want_pc, want_rgb = _numpy_keep(labels, index, pc, rgb)
    expect = {"unique_largest": 0, "noise_majority": -1, "noise_tied_with_cluster_0": -1, "clusters_2_and_5_tied": 2, "no_cluster": -1,
              "single_point": 0}[case]
    assert winner == expect
    zeroed = int((labels != winner).sum())
    if case == "noise_majority":
        assert zeroed == 300
    if case in ("no_cluster", "single_point"):
        assert zeroed == 0
    d_lab, d_pc, d_rgb = _dev(labels), _dev(pc), _dev(rgb)
    n_clusters = torch.tensor([int(labels.max()) + 1], dtype=torch.int32, device=DEV)
    hist = ops.label_histogram(d_lab, N + 1)
    got = ops.keep_largest_cluster(d_lab, _dev(index), hist, n_clusters, d_pc, d_rgb)
    assert int(got.item()) == winner
    assert _same(d_pc.cpu().numpy(), want_pc) and _same(d_rgb.cpu().numpy(), want_rgb)
    assert int(np.all(want_pc == 0, axis=2).sum()) == zeroed


# ------------------------------------------------------------------------------------------------------- the chain on the device
def _golden_scans():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_preprocess", os.path.join(os.path.dirname(__file__), "golden", "make_golden_preprocess.py"))
    mgp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mgp)
    return mgp.SCANS


SCENES = {"seed11": dict(seed=11), "seed52": dict(seed=52, H=150, W=260), "seed7": dict(seed=7, H=120, W=120)}


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(scan, restatement with gt) of a scene, computed once for every test that needs it; nothing writes to the arrays."""
    scan = pr.make_scan(**dict(key))
    return scan, pr.preprocess(scan["pc"], scan["rgb"], scan["gt"])


_key = pr.scene_key


def _on_device(scan, with_gt=True, seed=0):
    from cmdiad_amd.utils import preprocessing as mod
    gt = _dev(scan["gt"]) if with_gt else None
    pc, rgb, gt = mod.preprocess_on_device(_dev(scan["pc"]), _dev(scan["rgb"]), gt, seed=seed)
    assert pc.is_cuda and rgb.is_cuda and (gt is None or gt.is_cuda)
    return pc.cpu().numpy(), rgb.cpu().numpy(), (gt.cpu().numpy() if gt is not None else None)


@pytest.mark.parametrize("scene", ["golden_a", "golden_b"] + sorted(SCENES))
def test_preprocess_on_device_equals_the_restatement(scene, golden):
    """preprocess_on_device == preprocess_ref.preprocess bit for bit -- pc, rgb and gt, with and without gt, two calls alike -- on the
    golden's scenes (there also against the reference's own glue: the packed zero masks of gpp_preprocess.npz) and on three more:
    220 x 220 -> 300, 150 x 260 -> 300, 120 x 120 -> 200."""
    kw = _golden_scans()[scene[-1]] if scene.startswith("golden") else SCENES[scene]
    scan, want = _reference(_key(kw))
    got = _on_device(scan)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[2])
    assert got[0].shape[0] == got[0].shape[1] and got[0].shape[0] % 100 == 0 and np.any(got[0] != 0)
    again = _on_device(scan)
    assert all(_same(a, b) for a, b in zip(got, again))
    no_gt = _on_device(scan, with_gt=False)
    assert no_gt[2] is None and _same(no_gt[0], want[0]) and _same(no_gt[1], want[1])
    assert np.all(scan["pc"][scan["valid"]] != 0)
    if scene.startswith("golden"):
        g = golden("gpp_preprocess.npz")
        tag = scene[-1]
        assert np.array_equal(np.packbits(np.all(got[0] == 0, axis=2)), g[f"{tag}/clean_zero"])
        assert np.array_equal(np.packbits(got[2] != 0), g[f"{tag}/padded_gt"])
        assert np.array_equal(got[0].astype(np.float64).sum((0, 1)), g[f"{tag}/clean_pc_sum"])
        assert int(got[1].astype(np.int64).sum()) == int(g[f"{tag}/clean_rgb_sum"])


def test_preprocess_on_device_degenerate_scans():
    """The scan of zeros comes back unchanged, padded (rgb and gt too); so does, from the cleaning stage, a scan whose every valid
    point lies on the plane (all zeros then, as keep_largest of the restatement leaves it).  A scan with 49 valid edge points raises
    ValueError before RANSAC, as the restatement does; with 50 it is accepted."""
    from cmdiad_amd.utils import preprocessing as mod
    zeros, nines, gt = np.zeros((40, 130, 3), np.float32), np.full((40, 130, 3), 9, np.uint8), np.full((40, 130), 255, np.uint8)
    got = mod.preprocess_on_device(_dev(zeros), _dev(nines), _dev(gt))
    for g, w in zip(got, (zeros, nines, gt)):
        assert _same(g.cpu().numpy(), pr.pad_square(w)) and g.shape[:2] == (200, 200)
    ys, xs = np.mgrid[0:60, 0:130]
    flat = np.stack([(xs - 65) * 6e-4, (ys - 30) * 6e-4, 0.5 + 0.05 * (xs - 65) * 6e-4], -1).astype(np.float32)
    rgb = np.full((60, 130, 3), 9, np.uint8)
    want = pr.preprocess(flat, rgb, None)
    assert not want[0].any() and not want[1].any() and want[0].shape == (200, 200, 3)
    pc, rgb_out, gt = mod.preprocess_on_device(_dev(flat), _dev(rgb))
    assert gt is None and _same(pc.cpu().numpy(), want[0]) and _same(rgb_out.cpu().numpy(), want[1])
    few = np.zeros((40, 40, 3), np.float32)      # 49 points in the top strip, outside the column strips: each appears once
    few[0:2, 10:30] = flat[0:2, 10:30]
    few[2, 10:19] = flat[2, 10:19]
    assert len(pr.get_edges(few)) == 49
    with pytest.raises(ValueError):
        pr.preprocess(few, np.zeros((40, 40, 3), np.uint8))
    with pytest.raises(ValueError, match="49 valid edge points"):
        mod.preprocess_on_device(_dev(few), torch.zeros((40, 40, 3), dtype=torch.uint8, device=DEV))
    inner = np.zeros((40, 40, 3), np.float32)      # valid points, none of them on the edge
    inner[15:25, 15:25] = flat[15:25, 15:25]
    with pytest.raises(ValueError, match="0 valid edge points"):
        mod.preprocess_on_device(_dev(inner), torch.zeros((40, 40, 3), dtype=torch.uint8, device=DEV))
    few[2, 19] = flat[2, 19]      # 50: accepted
    assert len(pr.get_edges(few)) == 50
    mod.preprocess_on_device(_dev(few), torch.zeros((40, 40, 3), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    with pytest.raises(TypeError, match="float32"):
        mod.preprocess_on_device(_dev(flat.astype(np.float64)), _dev(rgb))


# ------------------------------------------------------------------------------------------------------------ the raw class
TREE, _fake_tifffile, _write_raw_tree = pr.RAW_TREE, pr.fake_tifffile, pr.write_raw_tree      # (shared with test_gpu_sample_loader.py)


def _args(root, **kw):
    from cmdiad_amd import evaluate as ev
    return ev.mtfi_args(dataset_path=str(root), img_process_method="hip", num_workers=2, **kw)


def _check_protocol(train, test, items, root):
    assert len(train) == 3 and len(test) == 4
    assert [int(t[1]) for t in train] == [0, 0, 0] and [int(t[2]) for t in test] == [0, 0, 1, 1]
    assert [t[3] for t in test] == [[os.path.join(root, "bagel", os.path.dirname(stem), "rgb", os.path.basename(stem) + ".png")]
                                    for stem, _, _ in items[3:]]
    for got in train + test:
        assert all(t.is_cuda and t.dtype == torch.float32 and t.shape == (1, 3, 224, 224) for t in got[0])
    for got in test:
        assert not got[1].is_cuda and got[1].shape == (1, 1, 224, 224) and got[1].dtype == torch.float32


def test_raw_class_equals_the_restatement_and_the_host_transforms(tmp_path, monkeypatch):
    """Every tensor, count, label, path and the order MVTec3DRawClass yields == preprocess_ref.preprocess -> host_rgb_transform /
    host_cloud_transform / host_gt_transform of the files' arrays."""
    from PIL import Image
    from cmdiad_amd import dataset as ds
    root = str(tmp_path)
    items = _write_raw_tree(root, _fake_tifffile(monkeypatch))
    cls = ds.MVTec3DRawClass(root, "bagel", _args(root))
    assert (cls.n_train, cls.n_test) == (3, 4)
    train, test = list(cls.train()), list(cls.test())
    _check_protocol(train, test, items, root)
    for got, (stem, key, has_gt) in zip(train + test, items):
        _, (pc, rgb, gt) = _reference(key)
        sample = got[0]
        want_cloud, want_depth = ds.host_cloud_transform(pc, 224)
        assert torch.equal(sample[0][0].cpu(), ds.host_rgb_transform(Image.fromarray(rgb), 224)), stem
        assert torch.equal(sample[1][0].cpu(), want_cloud) and torch.equal(sample[2][0].cpu(), want_depth), stem
        n = int(np.count_nonzero(np.all(want_cloud.numpy().reshape(3, -1) != 0, axis=0)))
        assert sample.n_valid == n and int(sample.n_valid_dev.item()) == n and n > 128, (stem, n)
        if len(got) == 4:
            if has_gt:
                assert torch.equal(got[1][0], ds.host_gt_transform(Image.fromarray(gt, "L"), 224)) and 0 < got[1].sum() < got[1].numel(), stem
            else:
                assert not got[1].any()


def test_raw_class_equals_mvtec3dclass_over_the_cleaned_tree(tmp_path, monkeypatch):
    """... and == MVTec3DClass(img_process_method='hip') over a copy of the tree that preprocess_dataset has cleaned in place."""
    from cmdiad_amd import dataset as ds
    from cmdiad_amd.utils import preprocessing as mod
    raw, clean = str(tmp_path / "raw"), str(tmp_path / "clean")
    items = _write_raw_tree(raw, _fake_tifffile(monkeypatch))
    shutil.copytree(raw, clean)
    assert mod.preprocess_dataset(clean) == 7
    a = ds.MVTec3DRawClass(raw, "bagel", _args(raw))
    b = ds.MVTec3DClass(clean, "bagel", _args(clean))
    assert (a.n_train, a.n_test) == (b.n_train, b.n_test) == (3, 4)
    ta, tb, sa, sb = list(a.train()), list(b.train()), list(a.test()), list(b.test())
    _check_protocol(ta, sa, items, raw)
    _check_protocol(tb, sb, items, clean)
    for x, y in zip(ta + sa, tb + sb):
        assert all(torch.equal(p, q) for p, q in zip(x[0], y[0])) and x[0].n_valid == y[0].n_valid
        assert torch.equal(x[-1] if len(x) == 2 else x[2], y[-1] if len(y) == 2 else y[2])
        if len(x) == 4:
            assert torch.equal(x[1], y[1]) and [os.path.relpath(x[3][0], raw)] == [os.path.relpath(y[3][0], clean)]
    # the raw tree itself was only read
    assert _same(sys.modules["tifffile"].imread(os.path.join(raw, "bagel", "train", "good", "xyz", "000.tiff")), pr.make_scan(**TREE[0][1][0])["pc"])
    sys.modules["tifffile"].imwrite(os.path.join(raw, "bagel", "train", "good", "xyz", "000.tiff"), np.zeros((120, 120, 3), np.float64))
    with pytest.raises(TypeError, match="float32"):
        list(ds.MVTec3DRawClass(raw, "bagel", _args(raw)).train())


def test_evaluate_classes_with_raw_scans_equals_the_cleaned_tree(tmp_path, monkeypatch):
    """evaluate_classes with raw_scans=True over the raw tree finishes with finite metrics, and its four metrics, counts and library
    rows equal a run with raw_scans=False over the cleaned copy (seeded random weights; two runs over the cleaned copy were first
    confirmed to agree with each other)."""
    from cmdiad_amd import dataset as ds
    from cmdiad_amd import evaluate as ev
    from cmdiad_amd.utils import preprocessing as mod
    from oracle import nets
    raw, clean = str(tmp_path / "raw"), str(tmp_path / "clean")
    _write_raw_tree(raw, _fake_tifffile(monkeypatch))
    shutil.copytree(raw, clean)
    mod.preprocess_dataset(clean)
    weights = (nets.synth_state_dict("vit", 31), nets.sharpen_pointmae(nets.synth_state_dict("pointmae", 21)),
               nets.synth_state_dict("halluc", 51))
    out = {}
    for tag, root, flag, kind in (("raw", raw, True, ds.MVTec3DRawClass), ("clean", clean, False, ds.MVTec3DClass)):
        a = _args(root, f_coreset=0.5, random_state=3, raw_scans=flag)
        data = ds.dataset_classes(a)
        assert list(data) == ["bagel"] and type(data["bagel"]) is kind
        out[tag] = ev.evaluate_classes(a, data, weights=weights)["per_class"]["bagel"]
    got, want = out["raw"], out["clean"]
    assert got["n_train"] == 3 and got["n_test"] == 4
    assert got["phases"] == ["memory_bank", "coreset", "late_fusion_bank", "late_fusion_fit", "predict", "metrics"]
    for k in ev.METRICS:
        print(k, got[k], want[k])
    assert all(np.isfinite(got[k]) for k in ("image_rocauc", "pixel_rocauc", "au_pro"))
    assert (got["n_train"], got["n_test"], got["library_rows"]) == (want["n_train"], want["n_test"], want["library_rows"])
    assert all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in ev.METRICS)
