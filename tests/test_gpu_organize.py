"""GPU: csrc/organize.hip (cmdiad_cloud_bounds, cmdiad_organize_splat, cmdiad_organize_resolve) and cmdiad_amd.organize byte for byte
against the yardstick tests/organize_ref.py: the key map, pixel_of_point, index, xyz, rgb, mask and stats.  Every output is a window
of a larger buffer filled with 0x5A, so a write outside it -- or to an element the contract leaves alone -- shows.  The shapes are
the smallest at which the kernels can go wrong: a workgroup is 256 points or pixels (2048 points for the bounds)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import organize_ref as R  # noqa: E402

from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd import organize as og  # noqa: E402

DEV = "cuda"
GUARD = 256
CANARY_I32 = int(np.frombuffer(b"\x5a" * 4, np.int32)[0])
F32 = np.float32


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """a device tensor of `shape` in the middle of a buffer of 0x5A bytes"""

    def __init__(self, shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        self.nbytes = nbytes
        self.t = self.raw[GUARD:GUARD + nbytes].view(dtype).reshape(shape)

    def numpy(self):
        raw = self.raw.cpu().numpy()
        assert np.all(raw[:GUARD] == 0x5A) and np.all(raw[GUARD + self.nbytes:] == 0x5A), "a write outside the buffer"
        return self.t.cpu().numpy()


def device_organize(points, offsets, cams, kind, H, W, fill=0, colors=None, labels=None, max_len=None, want_rgb=True, want_mask=True):
    """the yardstick's dict from the two entry points, every output guarded; an output that was not asked for is None"""
    points = np.asarray(points, F32).reshape(-1, 3)
    P, n = len(points), len(offsets) - 1
    if max_len is None:
        max_len = max([hi - lo for lo, hi in R.ranges(offsets, P)], default=0)
    dp, do, dc = dev(points), dev(np.asarray(offsets, np.int64)), dev(np.asarray(cams, np.float64).reshape(n, 16))
    keys, pop, stats = Guarded((n, H, W), torch.int64), Guarded((P,), torch.int32), Guarded((n, 4), torch.int32)
    ops.organize_splat(dp, do, dc, max_len, kind, H, W, out=(keys.t, pop.t, stats.t))
    index, xyz = Guarded((n, H, W), torch.int32), Guarded((n, H, W, 3), torch.float32)
    rgb = Guarded((n, H, W, 3), torch.uint8) if want_rgb else None
    mask = Guarded((n, H, W), torch.uint8) if want_mask else None
    ops.organize_resolve(dp, do, keys.t, stats.t, fill, dev(colors), dev(labels), out=(index.t, xyz.t, rgb and rgb.t, mask and mask.t))
    return dict(keys=keys.numpy().view(np.uint64), pixel_of_point=pop.numpy(), index=index.numpy(), xyz=xyz.numpy(),
                rgb=rgb.numpy() if rgb else None, mask=mask.numpy() if mask else None, stats=stats.numpy())


def reference(points, offsets, cams, kind, H, W, fill=0, colors=None, labels=None, max_len=None):
    points = np.asarray(points, F32).reshape(-1, 3)
    keys, pop, s01 = R.splat(points, offsets, cams, kind, H, W, max_len, pixel_of_point=np.full(len(points), CANARY_I32, np.int32))
    index, xyz, rgb, mask, s23 = R.resolve(points, offsets, keys, fill, colors, labels)
    return dict(keys=keys, pixel_of_point=pop, index=index, xyz=xyz, rgb=rgb, mask=mask, stats=np.concatenate([s01, s23], axis=1))


def check(points, offsets, cams, kind, H, W, **kw):
    """device == yardstick, byte for byte; returns the device's dict"""
    got = device_organize(points, offsets, cams, kind, H, W, **kw)
    ref = reference(points, offsets, cams, kind, H, W, **{k: v for k, v in kw.items() if not k.startswith("want_")})
    for name, want in ref.items():
        if got[name] is None:
            continue
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, name
        if got[name].tobytes() != want.tobytes():
            bad = np.nonzero((got[name].reshape(-1) != want.reshape(-1)) if name != "xyz" else
                             (got[name].view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1)))[0]
            raise AssertionError(f"{name}: {len(bad)} elements differ, first at {bad[:5]}: {got[name].reshape(-1)[bad[:5]]} for "
                                 f"{want.reshape(-1)[bad[:5]]}")
    return got


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def scene(N, H, W, kind, rng, identity=False):
    """(points [N,3] f32, camera row): a slab of points whose projection overhangs the grid on every side, some of them invalid, seen
    through a camera with a rotation and a shift (or the identity)"""
    u, v = rng.uniform(-1.5, W + 0.5, N), rng.uniform(-1.5, H + 0.5, N)
    d = rng.uniform(2.0, 3.0, N)
    d[rng.uniform(size=N) < 0.2] = 2.5                                   # equal depths: the lowest index wins
    if kind == 0:
        params = [-3.0, 4.0, 1 / 0.25, 1 / 0.5]
        cam_pts = np.stack([-3.0 + u * 0.25, 4.0 + v * 0.5, d], axis=1)
    else:
        params = [50.0, 40.0, W / 2 - 0.25, H / 2 + 0.125]
        cam_pts = np.stack([(u - params[2]) / 50.0 * d, (v - params[3]) / 40.0 * d, d], axis=1)
    if identity:
        T = np.eye(3, 4)
        pts = cam_pts
    else:
        Rm, t = rotation(rng), rng.uniform(-5, 5, 3)
        T = np.concatenate([Rm, t[:, None]], axis=1)
        pts = (cam_pts - t) @ Rm                                          # c = R p + t  <=>  p = R^T (c - t)
    pts = pts.astype(F32)
    bad = rng.uniform(size=N)
    pts[bad < 0.03] = 0
    pts[(bad >= 0.03) & (bad < 0.04), 1] = -0.0
    pts[(bad >= 0.04) & (bad < 0.05), 2] = np.nan
    pts[(bad >= 0.05) & (bad < 0.06), 0] = np.inf
    return pts, R.camera_row(params, T)


def attributes(P, rng):
    return rng.integers(0, 256, (P, 3)).astype(np.uint8), (rng.integers(0, 4, P) * (rng.uniform(size=P) < 0.3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ shapes
LENGTHS = (1025, 64, 0, 65, 1, 20011, 63)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (33, 65), (64, 64)])
def test_grids_and_cloud_sizes(H, W, kind):
    rng = np.random.default_rng(H * 1000 + W * 10 + kind)
    clouds, cams = zip(*(scene(N, H, W, kind, rng, identity=(k == 0)) for k, N in enumerate(LENGTHS)))
    points = np.concatenate(clouds)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)])
    colors, labels = attributes(len(points), rng)
    for extra in (0, 1000):                                                             # max_len equal to and above the longest cloud
        got = check(points, offsets, cams, kind, H, W, fill=1, colors=colors, labels=labels, max_len=max(LENGTHS) + extra)
    assert got["stats"][2].tolist() == [0, 0, 0, 0] and np.all(got["index"][2] == -1)   # the empty cloud in the middle
    assert np.all(got["stats"][[0, 5], :3] > 0) or (H, W) == (1, 1)
    for k, N in enumerate(LENGTHS):                                                     # and every cloud on its own
        check(clouds[k], [0, N], [cams[k]], kind, H, W, fill=0)
    check(np.zeros((0, 3), F32), [0, 0], [cams[0]], kind, H, W, fill=2)                 # no point at all


def test_two_runs_are_byte_equal():
    rng = np.random.default_rng(77)
    pts, cam = scene(20011, 7, 5, 0, rng)                                               # ~400 points contend for every pixel
    a = device_organize(pts, [0, len(pts)], [cam], 0, 7, 5, fill=1)
    b = device_organize(pts, [0, len(pts)], [cam], 0, 7, 5, fill=1)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


# ------------------------------------------------------------------------------------------------ several points in one pixel
def test_nearest_wins_and_ties_go_to_the_lowest_index():
    cam = R.camera_row([0, 0, 1, 1])
    one = F32(1.0)
    pts = np.array([[2, 1, 5], [2.2, 1.1, one], [1.9, 0.8, 3], [2.1, 1.3, one], [2, 1, np.nextafter(one, F32(2))]], F32)
    got = check(pts, [0, 5], [cam], 0, 4, 4)
    assert got["index"][0, 1, 2] == 1 and np.all(got["pixel_of_point"] == 6)            # the occluded points know their pixel too
    # equal in float32, different in float64: the lowest index wins, not the nearest double
    T = np.eye(3, 4)
    T[2, 0] = 2.0 ** -40
    pts = np.array([[1, 1, 1], [3, 1, 1], [-8, 1, 1]], F32)
    got = check(pts, [0, 3], [R.camera_row([0, 0, 0.01, 1], T)], 0, 4, 4)
    assert got["index"][0, 1, 0] == 0
    # negative and mixed-sign depths under the orthographic camera: -3 < -0.5 < 0 < 2
    T = np.eye(3, 4)
    T[2, 3] = -4.0
    pts = np.array([[1, 1, 6], [1, 1, 4], [1, 1, 1], [1, 1, 3.5], [2, 2, 4.5], [2, 2, 3.75]], F32)
    got = check(pts, [0, 6], [R.camera_row([0, 0, 1, 1], T)], 0, 4, 4)
    assert got["index"][0, 1, 1] == 2 and got["index"][0, 2, 2] == 5
    # -0.0 against +0.0, from the arithmetic and from the rounding to float32: one depth, the lowest index wins
    T = np.eye(3, 4)
    T[2] = [-0.0, -0.0, -0.0, -0.0]
    pts = np.array([[-2, 1, 1], [2, 1, 1], [2, 150, 1], [-2, 150, 1]], F32)               # c2 = +0.0, -0.0 | -0.0, +0.0
    c2 = R.camera_coords(pts, R.camera_row([0, 0, 0.01, 0.01], T))[2]
    assert np.signbit(c2).tolist() == [False, True, True, False] and np.all(c2 == 0)
    got = check(pts, [0, 4], [R.camera_row([0, 0, 0.01, 0.01], T)], 0, 4, 4)
    assert got["index"][0, 0, 0] == 0 and got["index"][0, 2, 0] == 2
    T[2] = [0, 0, 1e-300, 0]
    pts = np.array([[1, 1, 1], [1, 1, -1], [2, 2, -1], [2, 2, 1]], F32)                  # (float)(+-1e-300) = +-0.0
    got = check(pts, [0, 4], [R.camera_row([0, 0, 1, 1], T)], 0, 4, 4)
    assert got["index"][0, 1, 1] == 0 and got["index"][0, 2, 2] == 2


# ------------------------------------------------------------------------------------------------ boundaries
def test_pixel_boundaries_and_non_finite_values():
    W, H = 6, 4
    below = lambda x: np.nextafter(F32(x), F32(-np.inf))
    above = lambda x: np.nextafter(F32(x), F32(np.inf))
    cam = R.camera_row([0, 0, 1, 1])
    for axis, limit in ((0, W), (1, H)):
        vals = [0.5, 1.5, 2.5, -0.5, below(-0.5), above(-0.5), limit - 0.5, below(limit - 0.5), above(limit - 0.5), -1, limit,
                limit - 1, 1e30, -1e30, np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0]
        pts = np.ones((len(vals), 3), F32)
        pts[:, axis] = vals
        pts[:, 2] = 1 + np.arange(len(vals))
        got = check(pts, [0, len(pts)], [cam], 0, H, W)
        pop = got["pixel_of_point"]
        col = lambda p: p % W if axis == 0 else p // W
        assert [col(pop[0]), col(pop[1]), col(pop[2])] == [1, 2, 3]                        # u + 0.5 an integer: floor keeps it
        assert col(pop[3]) == 0 and pop[4] == -1 and col(pop[5]) == 0                      # the 0 edge, one ulp either side
        assert pop[6] == -1 and col(pop[7]) == limit - 1 and pop[8] == -1                  # the far edge
        assert pop[9] == -1 and pop[10] == -1 and col(pop[11]) == limit - 1                # uf = -1, uf = W
        assert pop[12] == -1 and pop[13] == -1 and pop[14:19].tolist() == [-2] * 5 and col(pop[19]) == 3
    # u = 1e300 and beyond, a NaN u (inf - inf), a depth that overflows float32
    pts = np.array([[1, 1, 1], [3e38, 1, 1], [1, 1, 2], [1, 1, 3], [2, 1, 1]], F32)
    got = check(pts[:2], [0, 2], [R.camera_row([0, 0, 1e300, 1])], 0, H, W)
    assert got["pixel_of_point"].tolist() == [-1, -1]
    T = np.eye(3, 4)
    T[0] = [np.inf, -np.inf, 0, 0]
    assert check(pts[:1], [0, 1], [R.camera_row([0, 0, 1, 1], T)], 0, H, W)["pixel_of_point"].tolist() == [-1]
    T = np.eye(3, 4)
    T[2, 2] = 2e38
    got = check(pts, [0, 5], [R.camera_row([0, 0, 1, 1], T)], 0, H, W)                      # depths 2e38, (u = 3e38), 4e38, 6e38, 2e38
    assert got["pixel_of_point"].tolist() == [W + 1, -1, -1, -1, W + 2] and got["stats"][0].tolist() == [0, 3, 2, 0]


def test_pinhole_depths():
    H, W = 4, 6
    cam = R.camera_row([2, 2, 2.5, 1.5])
    pts = np.array([[1, 1, 2], [1, 1, -2], [1, 1, 1e-30], [1, 1, -1e-30], [-1, -1, 4], [1e-38, -1e-38, 1e-38]], F32)   # (the last: subnormals)
    got = check(pts, [0, len(pts)], [cam], 1, H, W)
    assert got["pixel_of_point"].tolist() == [3 * W + 4, -1, -1, -1, 1 * W + 2, 0 * W + 5]
    # c2 = 0 of either sign and a tiny c2 from the transform; c0 = 0 over a tiny c2 is a finite pixel at depth (float)1e-300 = 0
    for t2, want in (([0, 0, 0, 0], -1), ([-0.0, -0.0, -0.0, -0.0], -1), ([0, 0, 1e-300, 0], -1), ([0, 0, -1e-300, 0], -1)):
        T = np.eye(3, 4)
        T[2] = t2
        assert check(pts[:1], [0, 1], [R.camera_row([2, 2, 2.5, 1.5], T)], 1, H, W)["pixel_of_point"].tolist() == [want]
    T = np.zeros((3, 4))
    T[2, 2] = 1e-300
    got = check(pts[:1], [0, 1], [R.camera_row([2, 2, 2.4, 1.4], T)], 1, H, W)
    assert got["pixel_of_point"].tolist() == [1 * W + 2] and got["keys"][0, 1, 2] == np.uint64(0x80000000) << np.uint64(32)


# ------------------------------------------------------------------------------------------------ fill, attributes, offsets
def holey_grid(rng):
    H, W = 12, 9
    ii, jj = np.mgrid[0:H, 0:W]
    whole = np.stack([1.0 + jj, 1.0 + ii, rng.uniform(1, 2, (H, W))], axis=2).astype(F32)
    pc = whole.copy()
    pc[rng.uniform(size=(H, W)) < 0.4] = 0             # holes whose windows hold several direct hits
    pc[0:6, 0:6] = 0                                   # a hole whose inner windows hold only holes
    pc[7:10, 3:6] = whole[7:10, 3:6]
    pc[8, 4] = 0                                       # an isolated hole, direct hits all round
    pc[0, W - 1] = pc[H - 1, 0] = pc[H - 1, W - 1] = 0  # the corners: clipped windows
    flat = pc.reshape(-1, 3)
    return flat[R.valid(flat)], H, W


@pytest.mark.parametrize("fill", [0, 1, 2])
def test_fill(fill):
    rng = np.random.default_rng(3)
    pts, H, W = holey_grid(rng)
    pts = pts[rng.permutation(len(pts))]
    colors, labels = attributes(len(pts), rng)
    got = check(pts, [0, len(pts)], [R.camera_row([1, 1, 1, 1])], 0, H, W, fill=fill, colors=colors, labels=labels)
    direct = got["keys"][0] != R.EMPTY
    assert not direct[8, 4] and got["stats"][0, 2] == direct.sum() == len(pts)
    assert (got["index"][0, 8, 4] >= 0) == (fill > 0) and got["index"][0, 0, 0] == -1 and got["index"][0, 2, 2] == -1
    assert got["stats"][0, 3] == ((got["index"][0] >= 0) & ~direct).sum() and (got["stats"][0, 3] > 0) == (fill > 0)


@pytest.mark.parametrize("with_colors,with_labels", [(True, True), (True, False), (False, True), (False, False)])
def test_attributes_present_and_absent(with_colors, with_labels):
    rng = np.random.default_rng(11)
    pts, cam = scene(3000, 33, 65, 1, rng)
    colors, labels = attributes(len(pts), rng)
    kw = dict(colors=colors if with_colors else None, labels=labels if with_labels else None)
    got = check(pts, [0, len(pts)], [cam], 1, 33, 65, fill=1, **kw)
    assert got["rgb"].any() == with_colors and got["mask"].any() == with_labels and set(np.unique(got["mask"])) <= {0, 255}
    check(pts, [0, len(pts)], [cam], 1, 33, 65, fill=1, want_rgb=False, want_mask=with_labels, **kw)
    check(pts, [0, len(pts)], [cam], 1, 33, 65, fill=1, want_rgb=with_colors, want_mask=False, **kw)


def test_offsets_are_not_trusted():
    rng = np.random.default_rng(13)
    pts, cam = scene(300, 7, 5, 0, rng)
    offsets = [-5, 100, 50, 400, 10, 2 ** 40]           # -> [0,100) [100,100) [50,300) [300,300) [10,300); overlaps see one camera
    assert R.ranges(offsets, 300) == [(0, 100), (100, 100), (50, 300), (300, 300), (10, 300)]
    got = check(pts, offsets, [cam] * 5, 0, 7, 5, fill=1, max_len=300)
    assert got["stats"][1].tolist() == [0, 0, 0, 0] and got["stats"][3].tolist() == [0, 0, 0, 0]
    offsets = [200, 250, -(2 ** 62), 2 ** 62]             # points 0..199 belong to no cloud... until the last one takes them all
    check(pts, offsets[:2], [cam], 0, 7, 5)
    got = device_organize(pts, offsets[:2], [cam], 0, 7, 5)
    assert np.all(got["pixel_of_point"][:200] == CANARY_I32) and np.all(got["pixel_of_point"][250:] == CANARY_I32)
    check(pts, offsets, [cam] * 3, 0, 7, 5, max_len=300)
    check(pts, [0, 300], [cam], 0, 7, 5, max_len=100)                                    # only the first max_len points are looked at
    # the key map is not trusted either: an index outside the cloud is an empty pixel
    keys = np.full((1, 7, 5), R.EMPTY, np.uint64)
    keys[0, 0, 0], keys[0, 0, 1], keys[0, 0, 2], keys[0, 3, 3] = 299, 300, 0xFFFFFFFF, (1 << 32) | 7
    stats = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    index, xyz, _, _ = ops.organize_resolve(dev(pts), dev(np.array([0, 300])), dev(keys.view(np.int64)), stats, fill=0)
    want = R.resolve(pts, [0, 300], keys, 0)
    assert np.array_equal(index.cpu().numpy(), want[0]) and xyz.cpu().numpy().tobytes() == want[1].tobytes()
    assert index[0, 0, :3].tolist() == [299, -1, -1] and index[0, 3, 3].item() == 7 and stats.cpu().numpy()[0].tolist() == [0, 0, 2, 0]


# ------------------------------------------------------------------------------------------------ the Python layer
def jittered_grid(H, W, x0, y0, pitch, rng):
    ii, jj = np.mgrid[0:H, 0:W]
    pc = np.stack([x0 + (jj + rng.uniform(-0.3, 0.3, (H, W))) * pitch, y0 + (ii + rng.uniform(-0.3, 0.3, (H, W))) * pitch,
                   rng.uniform(1, 2, (H, W))], axis=2).astype(F32)
    pc[rng.uniform(size=(H, W)) < 0.15] = 0
    return pc


def test_round_trip_through_unorganize():
    rng = np.random.default_rng(21)
    H, W, x0, y0, pitch = 33, 65, 0.7, -3.1, 0.013
    pcs = np.stack([jittered_grid(H, W, x0, y0, pitch, rng) for _ in range(3)])
    xyz, _, pix2pt, n_valid = ops.unorganize(dev(pcs.transpose(0, 3, 1, 2)))
    lengths = n_valid.cpu().tolist()
    org = og.organize([xyz[b, :lengths[b]] for b in range(3)], None, og.Camera.orthographic(x0, y0, pitch), H, W)
    assert org.xyz.cpu().numpy().tobytes() == pcs.tobytes() and org.lengths == tuple(lengths)
    assert np.array_equal(org.index.cpu().numpy().reshape(3, -1), pix2pt.cpu().numpy())
    assert org.stats.cpu().numpy().tolist() == [[0, 0, v, 0] for v in lengths] and not org.rgb.any() and not org.mask.any()


def test_round_trip_through_a_pinhole_camera():
    rng = np.random.default_rng(22)
    H, W, fx, fy, cx, cy = 64, 64, 80.0, 75.0, 31.37, 30.81
    ii, jj = np.mgrid[0:H, 0:W]
    z = rng.uniform(1, 3, (H, W))
    pts = np.stack([(jj - cx) / fx * z, (ii - cy) / fy * z, z], axis=2).reshape(-1, 3).astype(F32)
    perm = rng.permutation(H * W)
    org = og.organize(dev(pts[perm]), [H * W], [og.Camera.pinhole(fx, fy, cx, cy)], H, W)
    assert np.array_equal(perm[org.index.cpu().numpy().reshape(-1)], np.arange(H * W))
    assert org.xyz.cpu().numpy().tobytes() == pts.tobytes() and np.array_equal(org.pixel_of_point.cpu().numpy()[np.argsort(perm)], np.arange(H * W))


def test_organize_and_scores_to_points_against_the_yardstick():
    rng = np.random.default_rng(23)
    H, W, lengths = 33, 65, (700, 0, 1500)
    clouds, rows = zip(*(scene(N, H, W, 0, rng) for N in lengths))
    cams = [og.Camera(0, tuple(r[:12]), tuple(r[12:])) for r in rows]
    points = np.concatenate(clouds)
    colors, labels = attributes(len(points), rng)
    org = og.organize(dev(points), list(lengths), cams, H, W, fill=2, colors=dev(colors), labels=dev(labels))
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    ref = R.organize(points, offsets, rows, 0, H, W, 2, colors, labels)
    for name in ("xyz", "index", "rgb", "mask", "pixel_of_point", "stats"):
        assert getattr(org, name).cpu().numpy().tobytes() == ref[name].tobytes(), name
    assert org.keys.cpu().numpy().view(np.uint64).tobytes() == ref["keys"].tobytes()
    by_list = og.organize([dev(c) for c in clouds], None, cams, H, W, fill=2, colors=[dev(colors[offsets[b]:offsets[b + 1]]) for b in range(3)],
                          labels=dev(labels))
    assert all(torch.equal(a, b) for a, b in zip(org[:7], by_list[:7]))
    for dtype in (np.float32, np.float64):
        maps = rng.normal(size=(3, H, W)).astype(dtype)
        got = og.scores_to_points(dev(maps), org).cpu().numpy()
        want = R.scores_to_points(maps, ref["pixel_of_point"], offsets)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        assert np.array_equal(np.isnan(got), ref["pixel_of_point"] < 0) and np.isnan(got).any() and not np.isnan(got).all()
    with pytest.raises(ValueError, match="one kind"):
        og.organize(dev(points), list(lengths), [cams[0], og.Camera.pinhole(1, 1, 0, 0), cams[2]], H, W)


def test_cloud_bounds():
    rng = np.random.default_rng(24)
    lengths = (5000, 0, 300, 2049, 2)
    clouds, rows = zip(*(scene(N, 33, 65, 0, rng) for N in lengths))
    clouds = list(clouds)
    clouds[2][:] = rng.choice([0.0, np.nan, np.inf], size=clouds[2].shape[0])[:, None]   # every point dropped
    clouds[4][:] = [[1, 1, 1], [-1, 1, 1]]
    rows = list(rows)
    rows[4] = R.camera_row([0, 0, 1, 1], [[-0.0, -0.0, -0.0, -0.0], [0, 1, 0, -1], [0, 0, 1, 0]])  # c0 = -0.0 and +0.0, c1 = 0: all +0.0
    points = np.concatenate(clouds)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    want_b, want_n = R.bounds(points, offsets, rows)
    for max_len in (max(lengths), max(lengths) + 5000):
        bounds, count = Guarded((5, 6), torch.float64), Guarded((5,), torch.int32)
        ops.cloud_bounds(dev(points), dev(offsets), dev(np.stack(rows)), max_len, out=(bounds.t, count.t))
        assert bounds.numpy().tobytes() == want_b.tobytes() and count.numpy().tobytes() == want_n.tobytes()
    assert want_n.tolist()[1:3] == [0, 0] and want_b[1].tolist() == [np.inf] * 3 + [-np.inf] * 3 and want_b[2].tolist() == want_b[1].tolist()
    assert want_b[4, [0, 3, 1, 4]].tobytes() == np.zeros(4).tobytes()
    # clamped offsets and a short max_len
    bad = np.array([-3, 4000, 100, 2 ** 50])
    want_b, want_n = R.bounds(points, bad, rows[:3], max_len=1000)
    bounds, count = ops.cloud_bounds(dev(points), dev(bad), dev(np.stack(rows[:3])), 1000)
    assert bounds.cpu().numpy().tobytes() == want_b.tobytes() and count.cpu().numpy().tobytes() == want_n.tobytes()
    # fit_orthographic is that formula on these bounds
    good = [0, 3]
    cams = og.fit_orthographic([dev(clouds[b]) for b in good], None, 33, 65, margin=1, T=np.asarray(rows[0][:12]).reshape(3, 4))
    wb, _ = R.bounds(np.concatenate([clouds[b] for b in good]), [0, lengths[0], lengths[0] + lengths[3]], [rows[0]] * 2)
    for cam, b in zip(cams, wb):
        assert cam == og.orthographic_from_bounds(b[0:2], b[3:5], 33, 65, 1, T=np.asarray(rows[0][:12]).reshape(3, 4))
    with pytest.raises(ValueError, match="no valid point"):
        og.fit_orthographic([dev(clouds[0]), dev(clouds[2])], None, 33, 65)
