"""GPU: the region kernels (csrc/regions.hip) and cmdiad_amd/regions.py against the yardstick tests/regions_ref.py.  Everything is
compared bit for bit except score_sum, which is held to the bound of any summation order and to being reproducible."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as rr  # noqa: E402

from cmdiad_amd import ops, regions  # noqa: E402

DEV = "cuda"


def check(maps, thr, min_area=1, K=64, min_components=0):
    host = maps.cpu().numpy() if torch.is_tensor(maps) else np.asarray(maps, dtype=np.float64)
    want = rr.region_table(host, thr, min_area, K)
    assert want["nan"] == 0 and all(len(c) >= min_components for c in want["all"]), [len(c) for c in want["all"]]
    got = regions.find_regions(maps, regions.RegionSpec(thr, None, min_area, K))
    rr.assert_table_equal(got, want)
    return got, want


def smooth(n, seed):
    return ndimage.gaussian_filter(np.random.RandomState(seed).rand(n, 224, 224), sigma=(0, 4, 4))


@pytest.fixture(scope="module")
def random_maps():
    return np.random.RandomState(100).rand(3, 16, 16), np.random.RandomState(101).rand(2, 17, 23)


# ------------------------------------------------------------------------------------------------ fields
def test_random_maps(random_maps):
    for maps in random_maps:
        check(maps, 0.75, min_components=5)
    check(torch.from_numpy(random_maps[1]).to(DEV), 0.75, min_components=5)             # a device tensor
    check([m.astype(np.float32) for m in random_maps[0]], 0.75, min_components=5)       # a list of float32 maps widens exactly


def test_smooth_field_and_quantised_ties():
    maps = smooth(2, 7)
    check(maps, float(np.quantile(maps, 0.97)), min_components=5)
    lo, hi = maps.min(), maps.max()
    q = np.floor((maps - lo) / (hi - lo) * 255.0) / 255.0
    got, want = check(q, float(np.quantile(q, 0.9)), min_components=2)
    peaks = [c["peak"] for comps in want["all"] for c in comps]
    per_image = [[c["peak"] for c in comps] for comps in want["all"]]
    assert any(len(set(p)) < len(p) for p in per_image), peaks                           # equal peaks: the label decides
    assert any((c["values"] == c["peak"]).sum() > 1 for comps in want["all"] for c in comps)   # a plateau: the first pixel


@pytest.mark.parametrize("equal", [False, True], ids=["distinct", "equal"])
def test_lattice_fills_the_component_table(equal):
    maps = np.zeros((1, 224, 224))
    lattice = np.zeros((224, 224), dtype=bool)
    lattice[::2, ::2] = True
    maps[0][lattice] = 2.0 if equal else 1.0 + np.random.RandomState(3).permutation(12544) / 12544.0
    got, want = check(maps, 0.5, K=16)
    assert got.n_comp[0] == got.count[0] == 12544 and got.truncated[0]
    if equal:
        assert got.ints[0, :, 0].tolist() == list(range(1, 17))


def test_degenerate_images():
    got, _ = check(np.zeros((2, 16, 16)), 0.5)                                            # all background
    assert not got.count.any() and not got.ints.any() and not got.vals.any() and not got.n_comp.any()
    full = 1.0 + np.random.RandomState(5).rand(1, 17, 23)                                 # all foreground, n = 1
    got, _ = check(full, 0.5)
    assert got.count.tolist() == [1] and got.ints[0, 0, 1:6].tolist() == [17 * 23, 0, 0, 22, 16]
    line = np.random.RandomState(6).rand(2, 1, 37)
    check(line, 0.5, min_components=3)                                                    # H = 1
    check(line.reshape(2, 37, 1), 0.5, min_components=3)                                  # W = 1
    check(np.array([[[0.9]]]), 0.5, min_components=1)                                     # one pixel
    check(np.random.RandomState(8).rand(3, 5, 5), 0.6)                                    # odd H W, an odd image offset: scalar loads


def test_threshold_corners():
    m = np.random.RandomState(9).rand(1, 16, 16)
    y, x = np.unravel_index(np.argmin(np.abs(m[0] - 0.75)), (16, 16))                     # a threshold that IS a pixel's score, near 0.75
    thr = float(m[0, y, x])
    got, want = check(m, thr, min_components=5)                                           # the pixel equal to the threshold is background
    mask = ops.threshold_mask(torch.from_numpy(m).to(DEV), torch.tensor([thr], dtype=torch.float64, device=DEV))[0].cpu().numpy()
    assert mask[0, y, x] == 0 and mask.sum() > 0 and np.array_equal(mask, rr.threshold(m, thr)[0])
    z = np.where(np.random.RandomState(10).rand(1, 8, 8) < 0.5, -0.0, 0.0)
    got, _ = check(z, 0.0)                                                                # -0.0 > +0.0 is false
    assert got.n_comp.tolist() == [0]
    z[0, 2, 2] = 5e-324
    assert check(z, 0.0)[0].count.tolist() == [1]
    neg = -1.0 - np.random.RandomState(11).rand(2, 16, 16)
    got, _ = check(neg, -1.25, min_components=5)                                          # negative threshold, negative scores
    assert (got.vals[:, 0, 0] < 0).all()
    signed = np.where(np.random.RandomState(12).rand(1, 16, 16) < 0.5, -0.0, 0.0)         # components of zeros of both signs
    check(signed, -1.0, min_components=1)
    per = np.random.RandomState(13).rand(3, 16, 16)                                       # per-image thresholds
    check(per, np.array([0.6, 0.75, 0.9]), min_components=2)
    bad = per.copy()
    bad[1, 5, 5] = np.nan
    t = torch.from_numpy(bad).to(DEV)
    mask, nan = ops.threshold_mask(t, torch.tensor([0.6], dtype=torch.float64, device=DEV))
    assert int(nan.item()) == 1 and mask[1, 5, 5].item() == 0 and np.array_equal(mask.cpu().numpy(), rr.threshold(bad, 0.6)[0])
    with pytest.raises(ValueError, match="NaN"):
        regions.find_regions(bad, regions.RegionSpec(0.6))


def test_min_area_and_truncation(random_maps):
    maps = np.zeros((1, 9, 16))
    maps[0, 1, 1:4] = 3.0                                                                 # area 3
    maps[0, 4, 1:5] = 2.0                                                                 # area 4
    maps[0, 7, 1:6] = 1.0                                                                 # area 5
    got, _ = check(maps, 0.5, min_area=4)
    assert got.n_comp.tolist() == [3] and got.count.tolist() == [2] and got.ints[0, :2, 1].tolist() == [4, 5]
    got, want = check(random_maps[0], 0.75, K=4, min_components=5)
    assert (got.count > 4).all() and got.truncated.all()
    full = rr.region_table(random_maps[0], 0.75, 1, 64)
    assert np.array_equal(got.ints, full["ints"][:, :4])
    got, _ = check(random_maps[0], 0.75, min_area=2, K=2)                                 # count is reported before the truncation
    assert np.array_equal(got.count, [sum(c["area"] >= 2 for c in comps) for comps in full["all"]])


def test_score_sum_is_reproducible_and_independent_of_the_batch():
    maps = smooth(5, 21)
    thr = float(np.quantile(maps, 0.95))
    spec = regions.RegionSpec(thr, None, 1, 32)
    a, b = regions.find_regions(maps, spec), regions.find_regions(maps, spec)
    assert a.count.min() >= 2 and a.vals.tobytes() == b.vals.tobytes() and a.ints.tobytes() == b.ints.tobytes()
    alone = regions.find_regions(maps[3:4], spec)
    assert alone.vals[0].tobytes() == a.vals[3].tobytes() and alone.ints[0].tobytes() == a.ints[3].tobytes()
    first = regions.find_regions(maps[[3, 0]], spec)
    assert first.vals[0].tobytes() == a.vals[3].tobytes()


# ------------------------------------------------------------------------------------------------ calibration
@pytest.mark.parametrize("shape", [(3, 16, 16), (4, 224, 224)])
def test_calibrate_equals_the_yardstick_quantile(shape):
    rs = np.random.RandomState(shape[1])
    maps, scores = rs.randn(*shape), rs.randn(shape[0])
    for pq, iq in ((0.999, 1.0), (0.99, 0.5), (1.0, 0.0)):
        cal = regions.calibrate(scores, maps, pixel_quantile=pq, image_quantile=iq)
        assert cal.pixel_threshold == rr.quantile(maps, pq) == np.quantile(maps, pq, method="inverted_cdf")
        assert cal.image_threshold == rr.quantile(scores, iq)
        assert (cal.n_images, cal.n_pixels) == (shape[0], maps.size)
    assert not cal.decide(scores).all() and not regions.calibrate(scores, maps).decide(scores).any()   # q = 1: every sample passes
    bad = maps.copy()
    bad[0, 0, 0] = np.inf
    with pytest.raises(ValueError):
        regions.calibrate(scores, bad)
    with pytest.raises(ValueError):
        regions.calibrate(scores[:-1], maps)
