"""GPU: cmdiad_region_measure (csrc/regions.hip) and the clouds= path of cmdiad_amd/regions.py against the yardstick
tests/regions3d_ref.py, on the labels and the region table the device itself produced (those are held to their own yardstick by
tests/test_gpu_regions.py).

The integers, lo, hi, peak_xyz and the pad are compared bit for bit.  The sums are compared with the yardstick's math.fsum of ITS
terms within bounds computed from those terms (regions3d_ref.sum_bounds); nothing in them was tuned on the kernel's output:

  s1, s2  A term is d = p - lo (one float64 subtraction of widened floats) or a product d_a d_b (one more multiplication).  The
          kernel computes the same expressions without contraction, so its terms ARE the yardstick's, and all that differs is
          the order of n_pts additions: any order of summing n values is within (n - 1) u sum|t| (1 + O(n u)) of the exact sum, u =
          2^-53, which  n_pts 2^-53 sum|term|  covers for every n_pts a frame can hold (n <= 2^24, so n u <= 2^-29).  The second part,
          2^-52 sum|term| = two roundings per term, is room for a kernel that contracts d_a d_b + s into one fma (the product is
          then not rounded: 2^-53 |term| per term) and is not needed by the kernel as it stands.
  area    A triangle's term is 0.5 |(b - a) x (c - a)|: six subtractions, six products, three differences, three squares, two
          additions and a root -- at most 16 roundings once an fma drops or adds some, each at most 2^-53 of a quantity bounded by
          |e1| |e2| (the components of the cross product by Lagrange's identity, the root by the norm): 2^-49 sum |e1_t| |e2_t|.
          The n_tri additions are bounded like the sums above: n_tri 2^-53 sum area_t.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions3d_ref as r3  # noqa: E402
import regions_ref as rr  # noqa: E402

from cmdiad_amd import ops, regions  # noqa: E402

DEV = "cuda"
FIELDS_3D = ("n_pts", "n_tri", "peak_valid", "lo", "hi", "peak_xyz", "area_3d", "extent", "centroid_3d", "covariance", "principal_sigma")


def random_cloud(n, H, W, seed, invalid=0.1):
    """[n,3,H,W] float32 (planar): a rough surface in scanner-like units, a tenth of the points invalidated the way the datasets
    do it (one or all coordinates zero, sometimes -0.0)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    c = np.stack([0.3 + x * 0.01 + rs.randn(n, H, W) * 0.002, -0.2 + y * 0.012 + rs.randn(n, H, W) * 0.002,
                  0.5 + rs.randn(n, H, W) * 0.02 + 0 * x], 1).astype(np.float32)
    kill = rs.rand(n, H, W) < invalid
    which = rs.randint(0, 4, (n, H, W))
    for a in range(3):
        c[:, a][kill & ((which == a) | (which == 3))] = 0.0 if a else -0.0
    return c


def device_tables(maps, thr, K, min_area=1):
    """maps [n,H,W] float64 (host) -> the device's own (labels, count, ints)."""
    m = torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float64)).to(DEV)
    mask, nan = ops.threshold_mask(m, torch.full((1,), float(thr), dtype=torch.float64, device=DEV))
    labels, n_comp, comp_offset, comp_size, _ = ops.ccl_label(mask)
    count, ints, _ = ops.region_table(m, labels, n_comp, comp_offset, comp_size, min_area, K)
    assert int(nan.item()) == 0
    return labels, count, ints


def measure(labels, count, ints, cloud, layout="planar"):
    """cloud: planar numpy [n,3,H,W]; measured in `layout` -> (m_ints, m_vals, bad_count) on the host."""
    c = cloud if layout == "planar" else np.ascontiguousarray(cloud.transpose(0, 2, 3, 1))
    got = ops.region_measure(labels, count, ints, torch.from_numpy(c).to(DEV), layout=layout)
    return tuple(t.cpu().numpy() for t in got)


def check(maps, thr, cloud, K=8, min_area=1, want_regions=1):
    labels, count, ints = device_tables(maps, thr, K, min_area)
    want = r3.measure_table(labels.cpu().numpy(), count.cpu().numpy(), ints.cpu().numpy(), cloud, "planar")
    assert sum(len(s) for s in want["slots"]) >= want_regions                 # never an empty comparison
    m_ints, m_vals, bad = measure(labels, count, ints, cloud)
    r3.assert_measures_equal(m_ints, m_vals, want)
    assert int(bad[0]) == want["bad_count"]
    i2, v2, b2 = measure(labels, count, ints, cloud, "interleaved")           # the other layout: the same bits
    assert i2.tobytes() == m_ints.tobytes() and v2.tobytes() == m_vals.tobytes() and b2.tobytes() == bad.tobytes()
    i3, v3, _ = measure(labels, count, ints, cloud)                           # a second run: the same bits
    assert i3.tobytes() == m_ints.tobytes() and v3.tobytes() == m_vals.tobytes()
    return m_ints, m_vals, want, (count.cpu().numpy(), ints.cpu().numpy())


@pytest.fixture(scope="module")
def odd():
    """n = 3, 9 x 11: image 2 repeats image 0 (maps and cloud), image 1 is another one."""
    maps = np.random.RandomState(200).rand(3, 9, 11)
    cloud = random_cloud(3, 9, 11, 201)
    maps[2], cloud[2] = maps[0], cloud[0]
    return maps, cloud


def test_odd_frames_truncated_tables_and_batch_positions(odd):
    maps, cloud = odd
    m_ints, m_vals, want, (count, _) = check(maps, 0.7, cloud, K=3, want_regions=9)
    assert (count > 3).all() and (m_ints[:, :, 0] > 0).all()                   # every table truncated, every slot alive
    assert m_ints[:, :, 1].max() >= 1                                          # some triangles were counted
    assert m_ints[0].tobytes() == m_ints[2].tobytes() and m_vals[0].tobytes() == m_vals[2].tobytes()     # batch positions 0 and 2
    labels, cnt, ints = device_tables(maps[:1], 0.7, 3)                        # and the same image alone (n = 1)
    a_ints, a_vals, _ = measure(labels, cnt, ints, cloud[:1])
    assert a_ints[0].tobytes() == m_ints[0].tobytes() and a_vals[0].tobytes() == m_vals[0].tobytes()


def test_an_image_without_regions_and_untruncated_tables(odd):
    maps, cloud = odd[0].copy(), odd[1]
    maps[1] = 0.0
    m_ints, m_vals, want, (count, _) = check(maps, 0.7, cloud, K=16)
    assert count[1] == 0 and not m_ints[1].any() and not m_vals[1].any()
    assert 0 < count[0] < 16 and not m_ints[0, count[0]:].any() and not m_vals[0, count[0]:].any()


@pytest.mark.parametrize("H,W", [(1, 13), (13, 1), (2, 2)])
def test_degenerate_frames(H, W):
    rs = np.random.RandomState(H * 100 + W)
    maps = rs.rand(2, H, W)
    maps[1] = 1.0                                                              # all foreground: one region, box = image
    cloud = random_cloud(2, H, W, 7 + H, invalid=0.0 if H == W else 0.1)
    m_ints, _, want, _ = check(maps, 0.5, cloud, K=4, want_regions=2)
    if H == W:
        assert m_ints[1, 0].tolist() == [4, 2, 1, 0]                           # one cell, both triangles
    else:
        assert not m_ints[:, :, 1].any()                                       # a line has no cell


def test_a_region_touching_all_four_borders():
    maps = np.zeros((1, 9, 11))
    maps[0, 4, :] = maps[0, :, 5] = 1.0                                        # a cross from border to border
    maps[0, 0, 0] = 2.0                                                        # and a corner pixel, the stronger region
    m_ints, _, want, (_, ints) = check(maps, 0.5, random_cloud(1, 9, 11, 31, invalid=0.0), K=2, want_regions=2)
    assert ints[0, 1, 2:6].tolist() == [0, 0, 10, 8] and m_ints[0, 1, 0] == 19 and m_ints[0, 0].tolist() == [1, 0, 1, 0]


def test_invalid_regions_single_points_and_peaks():
    maps = np.zeros((1, 9, 11))
    maps[0, 0:3, 0:3] = 4.0                                                    # slot 0: every point invalid
    maps[0, 0:3, 5:8] = 3.0                                                    # slot 1: one valid point, not at the peak
    maps[0, 5:8, 0:3] = 2.0                                                    # slot 2: the peak pixel (its first) invalid, the rest valid
    maps[0, 5:8, 5:8] = 1.0                                                    # slot 3: all valid
    cloud = random_cloud(1, 9, 11, 41, invalid=0.0)
    cloud[0, 1, 0:3, 0:3] = 0.0
    cloud[0, :, 0:3, 5:8] = 0.0
    cloud[0, :, 1, 6] = [1.5, -2.5, 3.5]
    cloud[0, 2, 5, 0] = -0.0
    m_ints, m_vals, want, _ = check(maps, 0.5, cloud, K=4, want_regions=4)
    assert m_ints[0].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [8, 6, 0, 0], [9, 8, 1, 0]]      # (5,0) is in one cell only
    assert not m_vals[0, 0].any()
    assert m_vals[0, 1, 0:3].tolist() == m_vals[0, 1, 3:6].tolist() == [1.5, -2.5, 3.5] and not m_vals[0, 1, 6:].any()
    assert not m_vals[0, 2, 6:9].any() and (m_vals[0, 3, 6:9] == cloud[0, :, 5, 5].astype(np.float64)).all()


def test_a_box_longer_than_one_stride():
    maps = np.zeros((1, 48, 50))
    maps[0, 3:43, 5:45] = 1.0 + np.random.RandomState(50).rand(40, 40)         # 1600 box positions: seven rounds of 256
    m_ints, _, _, _ = check(maps, 0.5, random_cloud(1, 48, 50, 51), K=2)
    assert 1200 < m_ints[0, 0, 0] < 1600 and m_ints[0, 0, 1] > 1500


def test_a_full_frame_region():
    maps = 1.0 + np.random.RandomState(60).rand(1, 224, 224)
    m_ints, _, _, _ = check(maps, 0.5, random_cloud(1, 224, 224, 61), K=1)
    assert 40000 < m_ints[0, 0, 0] < 224 * 224 and m_ints[0, 0, 1] > 50000


def test_nonfinite_points_are_invalid_and_counted_over_the_whole_frames(odd):
    maps, cloud = odd[0], odd[1].copy()
    cloud[0, 0, 0, 0], cloud[1, 2, 4, 4], cloud[2, 1, 8, 10] = np.nan, np.inf, -np.inf
    cloud[1, :, 5, 5] = np.nan                                                 # one point, three bad coordinates: counted once
    _, _, want, _ = check(maps, 0.7, cloud, K=3)
    assert want["bad_count"] == 4
    _, _, want, _ = check(maps, 2.0, cloud, K=3, want_regions=0)                # no region at all: the count does not depend on thr
    assert want["bad_count"] == 4
    with pytest.raises(ValueError, match="non-finite"):
        regions.find_regions(maps, regions.RegionSpec(0.7), clouds=cloud)


def test_find_regions_with_clouds(odd):
    maps, cloud = odd
    spec = regions.RegionSpec(0.7, None, 2, 5)
    plain = regions.find_regions(maps, spec)
    got = regions.find_regions(maps, spec, clouds=cloud)
    assert plain.measures is None and got.measures is not None
    for f in ("n_comp", "count", "ints", "vals", "truncated"):                 # the tables themselves are today's
        assert getattr(got, f).tobytes() == getattr(plain, f).tobytes(), f
    rr.assert_table_equal(plain, rr.region_table(maps, 0.7, 2, 5))
    labels, count, ints = device_tables(maps, 0.7, 5, 2)
    want = r3.measure_table(labels.cpu().numpy(), count.cpu().numpy(), ints.cpu().numpy(), cloud, "planar")
    r3.assert_measures_equal(got.measures.m_ints, got.measures.m_vals, want)
    # every input form gives the same bits: interleaved numpy, a device tensor, a list of single clouds
    nhwc = np.ascontiguousarray(cloud.transpose(0, 2, 3, 1))
    for other in (nhwc, torch.from_numpy(cloud).to(DEV), [c for c in cloud], [c for c in nhwc]):
        again = regions.find_regions(maps, spec, clouds=other)
        assert again.measures.m_ints.tobytes() == got.measures.m_ints.tobytes()
        assert again.measures.m_vals.tobytes() == got.measures.m_vals.tobytes()
    listed, bare = got.to_list(), plain.to_list()
    assert sum(len(r) for r in listed) >= 3
    for i, regs in enumerate(listed):
        for k, d in enumerate(regs):
            assert {f: d[f] for f in bare[i][k]} == bare[i][k] and not set(FIELDS_3D) & set(bare[i][k])
            ref = regions.measure_fields(want["m_ints"][i, k], want["m_vals"][i, k])       # the shared function on the yardstick's table
            assert set(ref) == set(FIELDS_3D) and all(f in d for f in FIELDS_3D)
            for f in ("n_pts", "n_tri", "peak_valid", "lo", "hi", "peak_xyz", "extent"):
                assert d[f] == ref[f], (i, k, f)
            ext = max(max(d["extent"]), 1e-30)
            assert np.allclose(d["centroid_3d"], ref["centroid_3d"], rtol=0, atol=1e-12 * ext)
            assert np.allclose(d["covariance"], ref["covariance"], rtol=0, atol=1e-12 * ext * ext)
            assert np.allclose(d["principal_sigma"], ref["principal_sigma"], rtol=0, atol=1e-6 * ext)
            assert d["principal_sigma"] == sorted(d["principal_sigma"]) and min(d["principal_sigma"]) >= 0.0
            assert all(lo - 1e-12 * ext <= c <= hi + 1e-12 * ext for lo, c, hi in zip(d["lo"], d["centroid_3d"], d["hi"]))
    # refusals: another frame size, float64 clouds, a shape that reads both ways
    with pytest.raises(ValueError):
        regions.find_regions(maps, spec, clouds=random_cloud(3, 9, 12, 1))
    with pytest.raises(ValueError):
        regions.find_regions(maps, spec, clouds=cloud[:2])
    with pytest.raises(TypeError, match="float32"):
        regions.find_regions(maps, spec, clouds=cloud.astype(np.float64))
    three = np.random.RandomState(9).rand(2, 3, 5)
    with pytest.raises(ValueError, match="layout="):
        regions.find_regions(three, regions.RegionSpec(0.5), clouds=random_cloud(2, 3, 5, 2))
    a = regions.find_regions(three, regions.RegionSpec(0.5), clouds=random_cloud(2, 3, 5, 2), layout="planar")
    b = regions.find_regions(three, regions.RegionSpec(0.5), clouds=np.ascontiguousarray(random_cloud(2, 3, 5, 2).transpose(0, 2, 3, 1)))
    assert a.measures.m_vals.tobytes() == b.measures.m_vals.tobytes() and a.measures.m_ints[:, :, 0].sum() > 0
    empty = regions.find_regions(np.zeros((0, 9, 11)), spec, clouds=np.zeros((0, 3, 9, 11), np.float32))
    assert empty.measures.m_ints.shape == (0, 5, 4) and empty.measures.m_vals.shape == (0, 5, 20)


def test_out_buffers_and_an_untrusted_table(odd):
    """The table is an input the kernel must not trust: a count above K or below 0, a box outside the image, a label that no pixel
    carries.  The yardstick clamps the same way; nothing is read outside the frame."""
    maps, cloud = odd
    labels, count, ints = device_tables(maps, 0.7, 4)
    count, ints = count.clone(), ints.clone()
    count[0], count[1] = 1000, -7
    ints[0, 0, 2:6] = torch.tensor([-50, -50, 5000, 5000], dtype=torch.int32)
    ints[0, 1, 2:6] = torch.tensor([8, 8, 2, 2], dtype=torch.int32)            # an inverted box: empty
    ints[0, 2, 0] = 0                                                          # the background's label
    ints[0, 3, 0] = -3
    ints[2, 0, 6:8] = torch.tensor([-1, 400], dtype=torch.int32)               # a peak outside the image: peak_valid 0
    out = (torch.full((3, 4, 4), 77, dtype=torch.int32, device=DEV), torch.full((3, 4, 20), 7.0, dtype=torch.float64, device=DEV),
           torch.full((1,), 5, dtype=torch.int32, device=DEV))
    got = ops.region_measure(labels, count, ints, torch.from_numpy(cloud).to(DEV), out=out)
    assert all(g is o for g, o in zip(got, out))                               # written in place, every entry, no stale value
    want = r3.measure_table(labels.cpu().numpy(), count.cpu().numpy(), ints.cpu().numpy(), cloud, "planar")
    r3.assert_measures_equal(got[0].cpu().numpy(), got[1].cpu().numpy(), want)
    m = got[0].cpu().numpy()
    assert m[0, 0, 0] > 0 and not m[0, 1:].any() and not m[1].any() and m[2, 0, 2] == 0 and int(got[2].item()) == 0
