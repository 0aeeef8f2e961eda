"""CPU (no GPU): the yardstick of the region tables (tests/regions_ref.py) against scipy's own helpers, the nearest-rank quantile
against numpy's, the .cmdcal files, and every argument check of cmdiad_amd/regions.py, the ops wrappers and the two new entry
points that runs before a device is touched."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as rr  # noqa: E402

from cmdiad_amd import fitted, ops, regions  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def smooth_field(n, H, W, seed):
    rs = np.random.RandomState(seed)
    return ndimage.gaussian_filter(rs.rand(n, H, W), sigma=(0, 4, 4))


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("kind", ["random", "smooth", "quantised"])
def test_yardstick_agrees_with_scipy_helpers(kind):
    if kind == "random":
        maps, thr = np.random.RandomState(100).rand(3, 16, 16), 0.75
    else:
        maps = smooth_field(2, 64, 64, 5)
        if kind == "quantised":
            lo, hi = maps.min(), maps.max()
            maps = np.floor((maps - lo) / (hi - lo) * 255.0) / 255.0
        thr = float(np.quantile(maps, 0.9))
    mask, nan = rr.threshold(maps, thr)
    assert nan == 0 and np.array_equal(mask, (maps > thr).astype(np.uint8))
    total = 0
    for i in range(maps.shape[0]):
        labels, comps = rr.components(maps[i], mask[i])
        want_labels, n = ndimage.label(mask[i], np.ones((3, 3)))
        assert np.array_equal(labels, want_labels) and len(comps) == n
        idx = np.arange(1, n + 1)
        boxes = ndimage.find_objects(labels)
        peaks = ndimage.maximum(maps[i], labels, idx)
        pos = ndimage.maximum_position(maps[i], labels, idx)
        sums = ndimage.sum_labels(maps[i], labels, idx)
        areas = ndimage.sum_labels(np.ones_like(maps[i]), labels, idx)
        com = ndimage.center_of_mass(np.ones_like(maps[i]), labels, idx)
        for c, box, pk, (py, px), sm, ar, (cy, cx) in zip(comps, boxes, peaks, pos, sums, areas, com):
            assert (c["y0"], c["y1"] + 1, c["x0"], c["x1"] + 1) == (box[0].start, box[0].stop, box[1].start, box[1].stop)
            W = maps.shape[2]
            assert c["peak"] == pk == maps[i, py, px] == maps[i, c["peak_y"], c["peak_x"]]
            assert c["peak_y"] * W + c["peak_x"] <= py * W + px         # scipy names SOME pixel at the peak, the contract the first
            if kind != "quantised":
                assert (c["peak_y"], c["peak_x"]) == (py, px)
            assert c["area"] == int(ar)
            assert abs(c["score_sum"] - sm) <= c["area"] * 2.0 ** -53 * np.abs(c["values"]).sum()
            assert abs(c["cx"] - cx) <= 1e-12 * max(1.0, cx) and abs(c["cy"] - cy) <= 1e-12 * max(1.0, cy)
        total += n
    assert total >= 5


def test_yardstick_order_filters_and_truncation():
    maps = np.zeros((1, 6, 9))
    maps[0, 0, 0] = 5.0                                   # label 1, area 1
    maps[0, 0, 3:5] = 7.0                                 # label 2, area 2, peak 7 (plateau: the first pixel is x = 3)
    maps[0, 3:5, 0:2] = [[1.0, 7.0], [2.0, 3.0]]          # label 3, area 4, peak 7 at (1, 3): ties label 2 -> behind it
    maps[0, 5, 8] = 9.0                                   # label 4, area 1
    t = rr.region_table(maps, 0.5, min_area=1, max_regions=3)
    assert t["n_comp"][0] == 4 and t["count"][0] == 4 and t["truncated"][0]
    assert [c["label"] for c in t["regions"][0]] == [4, 2, 3]
    assert t["ints"][0, 1].tolist() == [2, 2, 3, 0, 4, 0, 3, 0] and t["ints"][0, 2].tolist() == [3, 4, 0, 3, 1, 4, 1, 3]
    assert t["vals"][0, 2].tolist() == [7.0, 13.0, 0.5, 3.5]
    t = rr.region_table(maps, 0.5, min_area=2, max_regions=3)
    assert t["n_comp"][0] == 4 and t["count"][0] == 2 and not t["truncated"][0]
    assert [c["label"] for c in t["regions"][0]] == [2, 3] and not t["ints"][0, 2].any() and not t["vals"][0, 2].any()
    # threshold rule: equal is background, -0.0 > +0.0 is false, a NaN is background and counted
    m = np.array([[[0.5, -0.0, np.nan, 0.50000001]]])
    mask, nan = rr.threshold(m, 0.5)
    assert mask.tolist() == [[[0, 0, 0, 1]]] and nan == 1
    assert rr.threshold(np.array([[[-0.0, 0.0]]]), 0.0)[0].sum() == 0
    assert rr.threshold(np.array([[[-1.0]], [[-1.0]]]), [-2.0, -0.5])[0].reshape(-1).tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ quantiles
@pytest.mark.parametrize("n,q", [(768, 0.99), (768, 0.999), (768, 1.0), (768, 0.0), (1, 0.999), (1, 1.0), (50176 * 4, 0.999), (7, 0.5)])
def test_nearest_rank_quantile_is_numpys_inverted_cdf(n, q):
    assert abs(q * n - round(q * n)) > 1e-6 or q in (0.0, 1.0)
    v = np.random.RandomState(n % 1000).randn(n)
    want = np.quantile(v, q, method="inverted_cdf")
    assert rr.quantile(v, q) == want
    assert regions.quantile_index(q, n) == rr.quantile_index(q, n)
    assert np.sort(v)[regions.quantile_index(q, n)] == want


def test_quantile_index_refuses_nonsense():
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            regions.quantile_index(q, 10)
    with pytest.raises(ValueError):
        regions.quantile_index(0.5, 0)


# ------------------------------------------------------------------------------------------------ .cmdcal files
def make_fit(path, seed):
    rs = np.random.RandomState(seed)
    fitted.write_file(path, dict(class_name="bagel"), {"patch_xyz_lib": rs.randn(130, 8).astype(np.float32),
                                                       "patch_rgb_lib": rs.randn(7, 8).astype(np.float32),
                                                       "xyz_mean": np.float32(0.5).reshape(())})
    return path


def test_calibration_file_round_trip_and_refusals(tmp_path):
    pt, it = float(np.nextafter(0.1, 1.0)), -float(np.pi) * 1e-7
    cal = regions.Calibration(pt, it, 0.999, 1.0, 3, 3 * 224 * 224, "bagel")
    fit_a, fit_b = make_fit(str(tmp_path / "a.cmdfit"), 1), make_fit(str(tmp_path / "b.cmdfit"), 2)
    before = open(fit_a, "rb").read()
    path = cal.save(str(tmp_path / "bagel.cmdcal"), fit=fit_a)
    assert open(fit_a, "rb").read() == before
    head = regions.read_header(path)
    assert head["format"] == "cmdiad-calibration" and set(head["fit_libraries"]) == {"patch_xyz_lib", "patch_rgb_lib"}
    assert fitted.read_header(fit_a)["format"] == "cmdfit"           # write_file's default is unchanged
    for fit in (None, fit_a, fitted.FittedClass(fit_a)):
        got = regions.Calibration.load(path, fit=fit)
        assert np.float64(got.pixel_threshold).tobytes() == np.float64(pt).tobytes()
        assert np.float64(got.image_threshold).tobytes() == np.float64(it).tobytes()
        assert (got.pixel_quantile, got.image_quantile, got.n_images, got.n_pixels, got.class_name) == (0.999, 1.0, 3, 150528, "bagel")
    with pytest.raises(regions.CalibrationMismatch, match="patch_(rgb|xyz)_lib"):
        regions.Calibration.load(path, fit=fit_b)
    assert issubclass(regions.CalibrationMismatch, ValueError)
    bare = cal.save(str(tmp_path / "bare.cmdcal"))
    assert regions.Calibration.load(bare).pixel_threshold == pt
    with pytest.raises(regions.CalibrationMismatch, match="without a fit"):
        regions.Calibration.load(bare, fit=fit_a)
    with pytest.raises(fitted.FitFileError, match="format"):
        regions.Calibration.load(fit_a)                             # a fit is no calibration
    blob = open(path, "rb").read()
    # truncated: inside the header, and inside the payload
    for cut in (10, 200, len(blob) - 8):
        bad = str(tmp_path / f"cut{cut}.cmdcal")
        open(bad, "wb").write(blob[:cut])
        with pytest.raises(fitted.FitFileError):
            regions.Calibration.load(bad)
    # one flipped byte: in the magic, in the header's text (a digit of a quantile), in a threshold's payload
    off = fitted.array_entry(head, "pixel_threshold")["offset"]
    for at in (3, blob.index(b'"pixel_quantile": 0.999') + len(b'"pixel_quantile": 0.99'), off + 3):
        bad = str(tmp_path / f"flip{at}.cmdcal")
        open(bad, "wb").write(blob[:at] + bytes([blob[at] ^ 0x01]) + blob[at + 1:])
        with pytest.raises(fitted.FitFileError):
            regions.Calibration.load(bad)


def test_info_command_prints_the_header(tmp_path):
    path = regions.Calibration(0.25, 1.5, 0.999, 1.0, 2, 512, "rope").save(str(tmp_path / "rope.cmdcal"))
    res = subprocess.run([sys.executable, "-m", "cmdiad_amd.regions", "info", path], capture_output=True, text=True, cwd=REPO)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout)
    assert out["format"] == "cmdiad-calibration" and out["pixel_threshold"] == 0.25 and out["image_threshold"] == 1.5
    assert out["class_name"] == "rope" and "arrays" not in out


# ------------------------------------------------------------------------------------------------ argument checks
def test_region_spec_and_calibration_checks():
    s = regions.RegionSpec(0.5)
    assert (s.pixel_threshold, s.image_threshold, s.min_area, s.max_regions) == (0.5, None, 1, 16)
    assert regions.RegionSpec([0.1, 0.2], 3, 2, 64).pixel_threshold.tolist() == [0.1, 0.2]
    for kw in (dict(pixel_threshold=float("nan")), dict(pixel_threshold=[]), dict(pixel_threshold=[[1.0]]),
               dict(pixel_threshold=0.5, image_threshold=float("nan")), dict(pixel_threshold=0.5, min_area=0),
               dict(pixel_threshold=float("inf")), dict(pixel_threshold=[0.1, -float("inf")]), dict(pixel_threshold=0.5, image_threshold=float("inf")),
               dict(pixel_threshold=0.5, min_area=1.5), dict(pixel_threshold=0.5, max_regions=0),
               dict(pixel_threshold=0.5, max_regions=65), dict(pixel_threshold=0.5, max_regions=True)):
        with pytest.raises(ValueError):
            regions.RegionSpec(**kw)
    cal = regions.Calibration(0.5, 2.0, 0.999, 1.0, 4, 64)
    spec = regions.as_spec(cal, 3, 8)
    assert (spec.pixel_threshold, spec.image_threshold, spec.min_area, spec.max_regions) == (0.5, 2.0, 3, 8)
    assert regions.as_spec(s) is s
    assert cal.decide([2.0, np.nextafter(2.0, 3.0), -1.0]).tolist() == [False, True, False]      # strict
    with pytest.raises(TypeError):
        regions.as_spec(0.5)
    with pytest.raises(ValueError):
        regions.Calibration(float("nan"), 1.0, 0.9, 1.0, 1, 1)
    with pytest.raises(ValueError):
        regions.Calibration(0.5, float("inf"), 0.9, 1.0, 1, 1)
    r = regions.Regions(np.array([3]), np.array([3]), np.zeros((1, 2, 8), np.int32), np.zeros((1, 2, 4)))
    assert r.truncated.tolist() == [True] and len(r) == 1


def test_pixel_list_truncate_and_result_list_restore():
    from cmdiad_amd.feature_extractors.features import PixelList
    pl = PixelList()
    for k in range(4):
        pl.extend(np.arange(5) + 10 * k)
    first = pl._chunks[0]
    pl.truncate(12)
    assert len(pl) == 12 and len(pl._chunks) == 3 and pl._chunks[0] is first          # whole chunks are kept as they are
    assert np.array_equal(np.array(pl), [0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 20, 21])
    pl.extend([7.0])
    assert len(pl) == 13 and pl[12] == 7
    pl.truncate(10)
    assert len(pl) == 10 and np.array_equal(np.array(pl), [0, 1, 2, 3, 4, 10, 11, 12, 13, 14])
    pl.truncate(50)
    assert len(pl) == 10
    pl.truncate(0)
    assert len(pl) == 0 and np.array(pl).shape == (0,)
    holder = type("M", (), {})()
    holder.pixel_preds, holder.gts = PixelList(), [1, 2, 3]
    holder.pixel_preds.extend(np.arange(6))
    regions._truncate(holder, "pixel_preds", 4)
    regions._truncate(holder, "gts", 1)
    assert np.array_equal(np.array(holder.pixel_preds), [0, 1, 2, 3]) and holder.gts == [1]


def test_ops_wrappers_check_before_any_device_call():
    maps = torch.zeros((2, 4, 4), dtype=torch.float64)
    with pytest.raises(Exception, match="GPU"):
        ops.threshold_mask(maps, torch.zeros(1, dtype=torch.float64))
    i32 = torch.zeros((2, 4, 4), dtype=torch.int32)
    with pytest.raises(Exception, match="GPU"):
        ops.region_table(maps, i32, i32[:, 0, 0], torch.zeros(3, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    for kw in (dict(min_area=0), dict(max_regions=0), dict(max_regions=65)):
        with pytest.raises(ValueError, match="min_area"):
            ops.region_table(maps, i32, i32[:, 0, 0], torch.zeros(3, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), **kw)


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    for name in ("cmdiad_threshold_mask", "cmdiad_region_table", "cmdiad_region_table_workspace_bytes"):
        assert f"{name}(" in hdr and hasattr(L, name) and (name in nat.SIGNATURES or name in nat.SIZE_QUERIES)
    assert L.cmdiad_abi_version() == 6
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # cmdiad_threshold_mask(maps, thr, thr_per_image, n, H, W, mask, nan_count, stream)
    assert L.cmdiad_threshold_mask(None, None, 0, 1, 4, 4, None, None, None) == -1 and b"null pointer" in L.cmdiad_last_error()
    for args in ((p, p, 2, 1, 4, 4, p, None, None), (p, p, 0, -1, 4, 4, p, None, None), (p, p, 0, 1, 0, 4, p, None, None),
                 (p, p, 0, 1, 1 << 13, 1 << 12, p, None, None), (p, p, 0, 65536, 1, 1, p, None, None)):
        assert L.cmdiad_threshold_mask(*args) == -1 and b"cmdiad_threshold_mask: bad sizes" in L.cmdiad_last_error(), args
    assert L.cmdiad_threshold_mask(None, None, 0, 0, 4, 4, None, None, None) == 0            # nothing to do: no launch
    # cmdiad_region_table(maps, labels, n_comp, comp_offset, comp_size, comp_cap, n, H, W, min_area, K, count, ints, vals, ws, bytes, stream)
    ws = L.cmdiad_region_table_workspace_bytes(2, 5, 7)
    assert ws >= 2 * 3 * 4 * 44 and L.cmdiad_region_table_workspace_bytes(0, 5, 7) == 0
    assert L.cmdiad_region_table_workspace_bytes(2, 1 << 13, 1 << 12) == 0 and L.cmdiad_region_table_workspace_bytes(-1, 5, 7) == 0
    ok = [p, p, p, p, p, 24, 2, 5, 7, 1, 16, p, p, p, p, ws, None]
    assert L.cmdiad_region_table(*([None] * 5 + ok[5:11] + [None] * 4 + [ws, None])) == -1 and b"null pointer" in L.cmdiad_last_error()
    for at, value, text in ((9, 0, b"min_area"), (10, 0, b"max_regions"), (10, 65, b"max_regions"), (6, -1, b"bad sizes"),
                            (7, 0, b"bad sizes"), (5, 23, b"24 are possible"), (15, ws - 1, b"workspace of")):
        args = list(ok)
        args[at] = value
        rc = L.cmdiad_region_table(*args)
        assert rc < 0 and text in L.cmdiad_last_error(), (at, value, rc, L.cmdiad_last_error())
    args = list(ok)
    args[6] = 0
    assert L.cmdiad_region_table(*args) == 0                                                    # n = 0: no launch
