"""CPU (no GPU): the yardstick of the measurement tables (tests/regions3d_ref.py) against facts it did not compute -- areas and
triangle counts of flat and tilted grids, the covariance of a regular grid in closed form, the triangles of a cell with an invalid
corner -- and every argument check of cmdiad_region_measure and its wrappers that runs before a device is touched."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions3d_ref as r3  # noqa: E402
import regions_ref as rr  # noqa: E402

from cmdiad_amd import ops, regions  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_cloud(H, W, dx, dy, origin=(1.0, 2.0, 3.0), theta=0.0):
    """[H,W,3] float64: a grid over the footprint x = column dx, y = row dy, flat at height origin[2] or, with theta, tilted about
    the x axis: the height rises by tan(theta) per unit of y."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([origin[0] + x * dx, origin[1] + y * dy, origin[2] + y * dy * math.tan(theta)], -1)


def one_region(H, W, y0, x0, m, k):
    """A frame whose only region is the m x k (rows x columns) rectangle at (y0, x0) -> (labels [1,H,W], count [1], ints [1,1,8])."""
    maps = np.zeros((1, H, W))
    maps[0, y0:y0 + m, x0:x0 + k] = 1.0
    t = rr.region_table(maps, 0.5, max_regions=1)
    labels, _ = rr.components(maps[0], (maps[0] > 0.5).astype(np.uint8))
    assert t["count"][0] == 1 and t["ints"][0, 0, 1] == m * k
    return labels[None].astype(np.int32), t["count"], t["ints"]


@pytest.mark.parametrize("theta", [0.0, 0.5, 1.0])
def test_area_and_triangles_of_a_flat_and_a_tilted_grid(theta):
    """An m x k rectangle of a grid with spacings dx, dy has (m - 1)(k - 1) cells of area dx dy, two triangles each.  The same
    footprint on a plane tilted by theta about the x axis: every area scales by 1 / cos(theta)."""
    H, W, m, k, dx, dy = 9, 11, 5, 7, 0.25, 0.5                 # binary fractions: the flat areas are exact
    labels, count, ints = one_region(H, W, 2, 3, m, k)
    cloud = grid_cloud(H, W, dx, dy, theta=theta).astype(np.float32)
    t = r3.measure_table(labels, count, ints, cloud[None], "interleaved")
    s = t["slots"][0][0]
    assert s["m_ints"].tolist() == [m * k, 2 * (m - 1) * (k - 1), 1, 0]
    flat = (m - 1) * (k - 1) * dx * dy
    if theta == 0.0:
        assert s["m_vals"][18] == flat
    else:       # float32 heights: 2^-24 relative each, far inside 1e-6
        assert abs(s["m_vals"][18] - flat / math.cos(theta)) <= 1e-6 * flat
    assert (s["m_vals"][6:9] == cloud[2, 3].astype(np.float64)).all()      # the peak of a plateau: its first pixel


def test_covariance_of_a_regular_grid_against_its_closed_form():
    """m x k points with spacings dy, dx: var_x = dx^2 (k^2 - 1) / 12, var_y = dy^2 (m^2 - 1) / 12, no covariance between the axes, no
    extent in z; the centroid is the middle of the box.  Derived with the shared regions.measure_fields."""
    H, W, m, k, dx, dy = 12, 10, 6, 4, 0.5, 0.25
    labels, count, ints = one_region(H, W, 1, 2, m, k)
    cloud = grid_cloud(H, W, dx, dy).astype(np.float32)
    t = r3.measure_table(labels, count, ints, cloud.transpose(2, 0, 1)[None], "planar")
    f = regions.measure_fields(t["m_ints"][0, 0], t["m_vals"][0, 0])
    assert f["n_pts"] == m * k and f["lo"] == [1.0 + 2 * dx, 2.0 + 1 * dy, 3.0] and f["extent"] == [(k - 1) * dx, (m - 1) * dy, 0.0]
    assert np.allclose(f["centroid_3d"], [1.0 + 2 * dx + (k - 1) * dx / 2, 2.0 + dy + (m - 1) * dy / 2, 3.0], rtol=0, atol=1e-15)
    want = np.diag([dx * dx * (k * k - 1) / 12, dy * dy * (m * m - 1) / 12, 0.0])
    assert np.allclose(f["covariance"], want, rtol=0, atol=1e-14)
    assert np.allclose(f["principal_sigma"], np.sqrt(np.sort(np.diag(want))), rtol=0, atol=1e-7)
    assert f["area_3d"] == (m - 1) * (k - 1) * dx * dy


@pytest.mark.parametrize("corner,n_tri,area", [((0, 0), 0, 0.0), ((0, 1), 1, 0.5), ((1, 1), 0, 0.0), ((1, 0), 1, 0.5), (None, 2, 1.0)])
def test_a_cell_with_one_invalid_corner(corner, n_tri, area):
    """One 2 x 2 cell of unit spacing.  Both triangles hold the diagonal (0,0) - (1,1): without either of its ends nothing is
    counted; without (0,1) only the second triangle is left, without (1,0) only the first."""
    labels, count, ints = one_region(2, 2, 0, 0, 2, 2)
    cloud = grid_cloud(2, 2, 1.0, 1.0).astype(np.float32)
    for bad in (0.0, -0.0, np.nan, np.inf):
        c = cloud.copy()
        if corner is not None:
            c[corner[0], corner[1], 1] = bad
        t = r3.measure_table(labels, count, ints, c[None], "interleaved")
        s = t["slots"][0][0]
        assert s["m_ints"].tolist() == [3 if corner else 4, n_tri, int(corner != (0, 0)), 0]
        assert s["m_vals"][18] == area
        assert t["bad_count"] == int(corner is not None and not np.isfinite(bad))
        assert (s["m_vals"][6:9] == 0).all() == (corner == (0, 0))


def test_yardstick_empty_cases_and_clamping():
    labels, count, ints = one_region(4, 5, 1, 1, 2, 3)
    cloud = grid_cloud(4, 5, 1.0, 1.0).astype(np.float32)
    dead = cloud.copy()
    dead[1:3, 1:4, 0] = 0.0                                        # every point of the region invalid: the whole slot is zero
    t = r3.measure_table(labels, count, ints, dead[None], "interleaved")
    assert not t["m_ints"].any() and not t["m_vals"].any()
    one = dead.copy()
    one[2, 2, 0] = 7.0                                             # one valid point: lo == hi, no triangle
    s = r3.measure_table(labels, count, ints, one[None], "interleaved")["slots"][0][0]
    assert s["m_ints"].tolist() == [1, 0, 0, 0] and (s["m_vals"][0:3] == s["m_vals"][3:6]).all() and not s["m_vals"][9:].any()
    wild = ints.copy()
    wild[0, 0, 2:6] = [-5, -5, 99, 99]                             # a box outside the image is clamped to it
    a = r3.measure_table(labels, count, wild, cloud[None], "interleaved")
    b = r3.measure_table(labels, count, ints, cloud[None], "interleaved")
    assert np.array_equal(a["m_vals"], b["m_vals"]) and np.array_equal(a["m_ints"], b["m_ints"])
    none = ints.copy()
    none[0, 0, 0] = 0                                              # label 0 is the background: it matches no pixel
    assert not r3.measure_table(labels, count, none, cloud[None], "interleaved")["m_ints"].any()
    assert not r3.measure_table(labels, np.array([-3]), ints, cloud[None], "interleaved")["m_ints"].any()


# ------------------------------------------------------------------------------------------------ argument checks
def test_measure_fields_of_an_empty_slot_and_regions_without_measures():
    f = regions.measure_fields(np.zeros(4, np.int32), np.zeros(20))
    assert f["n_pts"] == 0 and f["centroid_3d"] == [0.0, 0.0, 0.0] and f["principal_sigma"] == [0.0, 0.0, 0.0] and f["area_3d"] == 0.0
    r = regions.Regions(np.array([1]), np.array([1]), np.ones((1, 2, 8), np.int32), np.ones((1, 2, 4)))
    assert r.measures is None and "n_pts" not in r.to_list()[0][0]
    r = regions.Regions(np.array([1]), np.array([1]), np.ones((1, 2, 8), np.int32), np.ones((1, 2, 4)),
                        regions.Measures(np.zeros((1, 2, 4), np.int32), np.zeros((1, 2, 20))))
    d = r.to_list()[0][0]
    for name in ("n_pts", "n_tri", "peak_valid", "lo", "hi", "peak_xyz", "area_3d", "extent", "centroid_3d", "covariance", "principal_sigma"):
        assert name in d, name


def test_cloud_layout_is_worked_out_from_the_shape():
    z = torch.zeros
    assert ops.cloud_layout(z(2, 3, 9, 11), 9, 11) == "planar" and ops.cloud_layout(z(2, 9, 11, 3), 9, 11) == "interleaved"
    assert ops.cloud_layout(z(2, 3, 3, 5), 3, 5, "planar") == "planar" and ops.cloud_layout(z(2, 3, 3, 3), 3, 3, "interleaved") == "interleaved"
    for shape, hw in (((2, 3, 3, 5), (3, 5)), ((2, 3, 5, 3), (5, 3)), ((2, 3, 3, 3), (3, 3))):
        with pytest.raises(ValueError, match="layout="):
            ops.cloud_layout(z(*shape), *hw)
    for shape, hw, layout in (((2, 3, 9, 11), (9, 12), None), ((2, 9, 11, 3), (9, 11), "planar"), ((2, 3, 9), (3, 9), None),
                              ((2, 3, 9, 11), (9, 11), "nhwc")):
        with pytest.raises(ValueError):
            ops.cloud_layout(z(*shape), *hw, layout)


def test_wrappers_check_before_any_device_call():
    i32 = torch.zeros((2, 4, 5), dtype=torch.int32)
    with pytest.raises(Exception, match="GPU"):
        ops.region_measure(i32, i32[:, 0, 0], torch.zeros((2, 16, 8), dtype=torch.int32), torch.zeros((2, 3, 4, 5)))
    from cmdiad_amd.predictor import BatchPredictor
    with pytest.raises(ValueError, match="measure=True"):
        BatchPredictor(None, None, None, None, None, None, measure=True)
    with pytest.raises(ValueError, match="gt_size"):
        BatchPredictor(None, None, None, None, None, None, regions=regions.RegionSpec(0.5), measure=True, size=224, gt_size=112)


def test_region_measure_refuses_bad_arguments_without_a_device():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    assert "cmdiad_region_measure(" in hdr and hasattr(L, "cmdiad_region_measure") and "cmdiad_region_measure" in nat.SIGNATURES
    assert L.cmdiad_abi_version() == 6
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # cmdiad_region_measure(labels, count, ints, cloud, pix_stride, ch_stride, n, H, W, K, m_ints, m_vals, bad_count, stream)
    ok = [p, p, p, p, 1, 35, 2, 5, 7, 16, p, p, None, None]
    for at in (0, 1, 2, 3, 10, 11):
        args = list(ok)
        args[at] = None
        assert L.cmdiad_region_measure(*args) == -1 and b"null pointer" in L.cmdiad_last_error(), at
    for pix, ch in ((1, 1), (3, 35), (1, 34), (2, 1), (0, 0), (-1, 35), (3, 0), (35, 1)):
        args = list(ok)
        args[4], args[5] = pix, ch
        assert L.cmdiad_region_measure(*args) == -1 and b"bad strides" in L.cmdiad_last_error(), (pix, ch)
    for at, value in ((9, 0), (9, 65), (6, -1), (6, 65536), (7, 0), (8, 0)):
        args = list(ok)
        args[at] = value
        assert L.cmdiad_region_measure(*args) == -1 and b"cmdiad_region_measure: bad sizes" in L.cmdiad_last_error(), (at, value)
    # oversize frames: H * W above 2^24, n * H * W above 2^30 (with the strides those sizes would need)
    assert L.cmdiad_region_measure(p, p, p, p, 1, (1 << 13) * (1 << 12), 1, 1 << 13, 1 << 12, 16, p, p, None, None) == -1
    assert b"bad sizes" in L.cmdiad_last_error()
    assert L.cmdiad_region_measure(p, p, p, p, 3, 1, 65, 1 << 12, 1 << 12, 16, p, p, None, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    # n = 0: nothing to do, no launch, with either layout's strides
    assert L.cmdiad_region_measure(None, None, None, None, 1, 35, 0, 5, 7, 16, None, None, None, None) == 0
    assert L.cmdiad_region_measure(None, None, None, None, 3, 1, 0, 5, 7, 16, None, None, None, None) == 0
