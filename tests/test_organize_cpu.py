"""CPU (no GPU): the three entry points of csrc/organize.hip in the header, the binding and the library, and their argument
validation, which happens before any launch; utils.ply.read_points on hand-built files and its refusals; fit_orthographic's
formula; and the properties of the yardstick itself (tests/organize_ref.py), against which tests/test_gpu_organize.py compares the
device byte for byte."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import organize_ref as R  # noqa: E402

from cmdiad_amd import organize as og  # noqa: E402
from cmdiad_amd.utils import ply  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmdiad_cloud_bounds", "cmdiad_organize_splat", "cmdiad_organize_resolve")
_C2CT = {"int": ctypes.c_int, "double": ctypes.c_double, "cmdiad_stream_t": ctypes.c_void_p}


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_bound_and_exported():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    assert L.cmdiad_abi_version() == 6
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    for name in NAMES:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", hdr)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(ctypes.c_void_p if "*" in arg else _C2CT[arg.rsplit(" ", 1)[0]])
        assert name in nat.SIGNATURES and nat.SIGNATURES[name] == want, (name, want)
        assert hasattr(L, name) and getattr(L, name).argtypes == nat.SIGNATURES[name]
    assert not any("organize" in q or "bounds" in q for q in nat.SIZE_QUERIES)        # caller-owned outputs only, no workspace query
    mk = open(os.path.join(REPO, "cmdiad_amd", "csrc", "Makefile")).read()
    assert "organize.o" in re.search(r"^EXACT\s*:=(.*)$", mk, re.M).group(1)           # one rounding per operation


def test_arguments_are_checked_before_any_launch():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused on the host

    def refused(name, args, match):
        rc = getattr(L, name)(*args)
        assert rc == -1 and re.search(match, L.cmdiad_last_error().decode()), (name, rc, L.cmdiad_last_error())

    # cmdiad_cloud_bounds(points, offsets, cams, n, P, max_len, bounds, count, stream)
    refused("cmdiad_cloud_bounds", (None, None, None, 1, 1, 1, None, None, None), "null pointer")
    refused("cmdiad_cloud_bounds", (None, one, one, 1, 1, 1, one, one, None), "null pointer")          # points with P, max_len > 0
    refused("cmdiad_cloud_bounds", (one, one, one, -1, 1, 1, one, one, None), "bad sizes")
    refused("cmdiad_cloud_bounds", (one, one, one, 65536, 1, 1, one, one, None), "bad sizes")
    refused("cmdiad_cloud_bounds", (one, one, one, 1, -1, 1, one, one, None), "bad sizes")
    refused("cmdiad_cloud_bounds", (one, one, one, 1, 1, -1, one, one, None), "bad sizes")
    assert L.cmdiad_cloud_bounds(None, None, None, 0, 0, 0, None, None, None) == 0                    # n = 0: nothing to do
    # cmdiad_organize_splat(points, offsets, cams, n, P, max_len, kind, H, W, keys, pixel_of_point, stats, stream)
    refused("cmdiad_organize_splat", (None, None, None, 1, 1, 1, 0, 4, 4, None, None, None, None), "null pointer")
    refused("cmdiad_organize_splat", (one, one, one, 1, 1, 1, 0, 4, 4, one, None, one, None), "null pointer")
    refused("cmdiad_organize_splat", (one, one, one, 1, 1, 1, 2, 4, 4, one, one, one, None), "kind")
    refused("cmdiad_organize_splat", (one, one, one, 1, 1, 1, -1, 4, 4, one, one, one, None), "kind")
    refused("cmdiad_organize_splat", (one, one, one, 1, 1, 1, 0, 0, 4, one, one, one, None), "bad grid")
    refused("cmdiad_organize_splat", (one, one, one, 1, 1, 1, 0, 4, -4, one, one, one, None), "bad grid")
    refused("cmdiad_organize_splat", (one, one, one, 1, 1, 1, 0, 4097, 4096, one, one, one, None), "bad grid")       # H W > 2^24
    refused("cmdiad_organize_splat", (one, one, one, 65, 1, 1, 0, 4096, 4096, one, one, one, None), "bad grid")      # n H W > 2^30
    refused("cmdiad_organize_splat", (one, one, one, 70000, 1, 1, 0, 4, 4, one, one, one, None), "bad sizes")
    assert L.cmdiad_organize_splat(None, None, None, 0, 0, 0, 0, 4, 4, None, None, None, None) == 0
    # cmdiad_organize_resolve(points, offsets, colors, labels, keys, n, P, H, W, fill, index, xyz, rgb, mask, stats, stream)
    refused("cmdiad_organize_resolve", (None,) * 5 + (1, 1, 4, 4, 0) + (None,) * 6, "null pointer")
    refused("cmdiad_organize_resolve", (one, one, None, None, one, 1, 1, 4, 4, 0, one, None, None, None, one, None), "null pointer")
    refused("cmdiad_organize_resolve", (one, one, None, None, one, 1, 1, 4, 4, 3, one, one, None, None, one, None), "fill")
    refused("cmdiad_organize_resolve", (one, one, None, None, one, 1, 1, 4, 4, -1, one, one, None, None, one, None), "fill")
    refused("cmdiad_organize_resolve", (one, one, None, None, one, 1, 1, 0, 4, 0, one, one, None, None, one, None), "bad grid")
    refused("cmdiad_organize_resolve", (one, one, None, None, one, 1, -2, 4, 4, 0, one, one, None, None, one, None), "bad sizes")
    assert L.cmdiad_organize_resolve(*((None,) * 5 + (0, 0, 4, 4, 0) + (None,) * 6)) == 0


def test_ops_check_their_tensors_without_a_gpu():
    import torch
    from cmdiad_amd import _native as nat
    from cmdiad_amd import ops
    pts, off, cams = torch.zeros(4, 3), torch.tensor([0, 4]), torch.zeros(1, 16, dtype=torch.float64)
    for call in (lambda: ops.cloud_bounds(pts, off, cams, 4), lambda: ops.organize_splat(pts, off, cams, 4, 0, 4, 4),
                 lambda: ops.organize_resolve(pts, off, torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int32))):
        with pytest.raises(nat.NativeError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="one \\[P,3\\] tensor needs lengths"):
        og.organize(pts, None, og.Camera.pinhole(1, 1, 0, 0), 4, 4)
    with pytest.raises(ValueError, match="sum to"):
        og.organize(pts, [3], og.Camera.pinhole(1, 1, 0, 0), 4, 4)


# ------------------------------------------------------------------------------------------------ read_points
def _ply(tmp_path, header_lines, payload, name="a.ply"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(("\n".join(["ply"] + header_lines + ["end_header"]) + "\n").encode("ascii"))
        f.write(payload)
    return path


def test_read_points_ascii_and_binary(tmp_path):
    head = ["format ascii 1.0", "comment made by hand", "element vertex 3", "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue", "property int label", "property float32 quality",
            "element face 1", "property list uchar int vertex_indices"]
    body = b"1 2 3 10 20 30 0 0.5\n-1.5 2.25 1e3 255 0 7 4 1.5\n0 0 0 1 2 3 0 2\n3 0 1 2\n"
    v = ply.read_points(_ply(tmp_path, head, body))
    assert v["x"].dtype == np.float32 and v["x"].tolist() == [1.0, -1.5, 0.0] and v["z"].tolist() == [3.0, 1000.0, 0.0]
    assert v["red"].dtype == np.uint8 and v["red"].tolist() == [10, 255, 1] and v["blue"].tolist() == [30, 7, 3]
    assert v["label"].dtype == np.int32 and v["label"].tolist() == [0, 4, 0] and v["quality"].tolist() == [0.5, 1.5, 2.0]
    # binary, double coordinates (rounded to float32), the int8..float64 aliases, an extra property in front, a face element behind
    head = ["format binary_little_endian 1.0", "element vertex 2", "property uint16 id", "property float64 x", "property double y",
            "property float64 z", "property uint8 red", "property uint8 green", "property uint8 blue", "property int8 label",
            "element face 1", "property list uchar int vertex_indices"]
    rec = struct.Struct("<HdddBBBb")
    third = 1.0 / 3.0
    body = rec.pack(7, third, 2.0, -1e-300, 1, 2, 3, -1) + rec.pack(9, 1e40, 5.0, 6.0, 4, 5, 6, 0) + b"\x03" + struct.pack("<iii", 0, 1, 0)
    with np.errstate(over="ignore"):
        v = ply.read_points(_ply(tmp_path, head, body))
    assert v["x"].dtype == np.float32 and v["x"][0] == np.float32(third) and np.isinf(v["x"][1]) and v["z"][0] == 0 and np.signbit(v["z"][0])
    assert v["id"].tolist() == [7, 9] and v["label"].dtype == np.int8 and v["label"].tolist() == [-1, 0] and v["green"].tolist() == [2, 5]
    # no vertex at all
    v = ply.read_points(_ply(tmp_path, ["format ascii 1.0", "element vertex 0", "property float x", "property float y", "property float z"], b""))
    assert v["x"].shape == (0,) and v["x"].dtype == np.float32


def test_read_points_reads_the_package_s_own_meshes(tmp_path):
    verts = np.zeros(5, ply.VERTEX)
    verts["x"], verts["y"], verts["z"] = np.arange(5) + 1.0, np.arange(5) * 2.0 + 1.0, 3.0
    verts["red"], verts["score"], verts["region"] = [1, 2, 3, 4, 5], 0.25, [0, 1, 1, 0, 2]
    faces = np.zeros(2, ply.FACE)
    faces["n"], faces["vertex_indices"] = 3, [[0, 1, 2], [2, 3, 4]]
    path = str(tmp_path / "m.ply")
    ply.write(path, 5, verts, 2, faces, ["class rope"])
    v = ply.read_points(path)
    assert v["x"].tobytes() == verts["x"].tobytes() and v["y"].tobytes() == verts["y"].tobytes() and v["z"].tobytes() == verts["z"].tobytes()
    assert v["red"].tolist() == [1, 2, 3, 4, 5] and v["region"].tolist() == [0, 1, 1, 0, 2] and v["score"].tolist() == [0.25] * 5
    assert len(ply.read(path)[0]) == 5                                                # the mesh reader is as it was


def test_read_points_refusals(tmp_path):
    xyz = ["property float x", "property float y", "property float z"]
    pay = struct.pack("<fff", 1, 2, 3)

    def refused(header_lines, payload, match):
        with pytest.raises(ply.PlyError, match=match):
            ply.read_points(_ply(tmp_path, header_lines, payload))
    refused(["format binary_little_endian 1.0", "element vertex 1"] + xyz + ["property list uchar int n"], pay, "list property inside the vertex")
    refused(["format binary_little_endian 1.0", "element face 1", "property list uchar int vertex_indices", "element vertex 1"] + xyz,
            b"\x00" + pay, "list property in element 'face' in front")
    refused(["format binary_big_endian 1.0", "element vertex 1"] + xyz, pay, "big-endian")
    refused(["format binary_little_endian 1.0", "element vertex 2"] + xyz, pay, "more than the file")                 # truncated
    refused(["format binary_little_endian 1.0", "element vertex 1"] + xyz, pay[:-1], "more than the file")
    refused(["format binary_little_endian 1.0", "element vertex 999999999999"] + xyz, pay, "more than the file")       # no allocation first
    refused(["format ascii 1.0", "element vertex 999999999"] + xyz, b"1 2 3\n", "do not fit")
    refused(["format ascii 1.0", "element vertex 2"] + xyz, b"10.5 20.5 30.5\n", "ended inside")
    refused(["format ascii 1.0", "element vertex 1"] + xyz, b"1.25 2.25\n", "ended inside")
    refused(["format ascii 1.0", "element vertex 1"] + xyz, b"1 2 x\n", "not a number")
    refused(["format binary_little_endian 1.0", "element vertex 1", "property float x", "property float y"], pay, "needs float or double x, y and z")
    refused(["format binary_little_endian 1.0", "element vertex 1", "property int x", "property float y", "property float z"], pay, "needs float")
    refused(["format binary_little_endian 1.0", "element vertex 1"] + xyz + ["property float label"], pay + pay[:4], "label must be an integer")
    refused(["format binary_little_endian 1.0", "element vertex 1"] + xyz + ["property quad w"], pay, "bad header line")
    refused(["format binary_little_endian 1.0", "element vertex -1"] + xyz, pay, "bad header line")
    refused(["format binary_little_endian 1.0"] + xyz, pay, "in front of the vertices|no vertex element")
    refused(["element vertex 1"] + xyz, pay, "no format line")
    with open(str(tmp_path / "b.ply"), "wb") as f:
        f.write(b"plx\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ply.PlyError, match="not a PLY file"):
        ply.read_points(str(tmp_path / "b.ply"))


# ------------------------------------------------------------------------------------------------ the orthographic fit
@pytest.mark.parametrize("H,W,margin", [(64, 64, 0), (64, 64, 1), (33, 65, 0), (7, 5, 1), (2, 2, 0)])
def test_fit_orthographic_places_every_valid_point_inside(H, W, margin):
    rng = np.random.default_rng(H * 100 + W + margin)
    for scale, shift in ((1.0, 0.0), (1e-3, 5.0), (250.0, -1e4), (1.0, 1e6)):
        pts = (rng.uniform(-1, 1, (500, 3)) * scale * [1.0, 0.37, 1.0] + shift).astype(np.float32)
        pts[::50] = 0                                                                  # dropped points do not count
        cam0 = R.camera_row([0, 0, 1, 1])
        (lohi,), (cnt,) = R.bounds(pts, [0, len(pts)], [cam0])
        assert cnt == R.valid(pts).sum()
        cam = og.orthographic_from_bounds(lohi[0:2], lohi[3:5], H, W, margin)
        pitch = max((lohi[3] - lohi[0]) / (W - 1 - 2 * margin), (lohi[4] - lohi[1]) / (H - 1 - 2 * margin))
        assert cam.kind == 0 and cam.params[2] == cam.params[3] == 1.0 / pitch
        assert cam.params[0] == (lohi[0] + lohi[3]) / 2 - pitch * (W - 1) / 2 and cam.params[1] == (lohi[1] + lohi[4]) / 2 - pitch * (H - 1) / 2
        pix, _ = R.project(pts, np.array(cam.row()), 0, H, W)
        assert np.all(pix[R.valid(pts)] >= 0) and np.all(pix[~R.valid(pts)] == -2)
        ys, xs = pix[pix >= 0] // W, pix[pix >= 0] % W
        assert xs.min() >= margin and xs.max() <= W - 1 - margin and ys.min() >= margin and ys.max() <= H - 1 - margin
    # one point, or points on one spot: pitch 1, the point at the centre
    cam = og.orthographic_from_bounds((2.0, 3.0), (2.0, 3.0), 5, 7)
    assert cam.params == (2.0 - 3.0, 3.0 - 2.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="empty or unbounded"):
        og.orthographic_from_bounds((np.inf, np.inf), (-np.inf, -np.inf), 5, 7)
    with pytest.raises(ValueError, match="no room"):
        og.orthographic_from_bounds((0.0, 0.0), (1.0, 1.0), 3, 3, margin=1)


def test_camera_rows():
    c = og.Camera.orthographic(1, 2, 0.5, 0.25, T=[[0, 1, 0, 5], [1, 0, 0, 6], [0, 0, -1, 7], [0, 0, 0, 1]])
    assert c.row() == [0, 1, 0, 5, 1, 0, 0, 6, 0, 0, -1, 7, 1, 2, 2, 4]
    assert og.Camera.pinhole(10, 11, 3, 4).row() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 10, 11, 3, 4]
    with pytest.raises(ValueError):
        og.Camera.orthographic(0, 0, 0)
    with pytest.raises(ValueError):
        og.Camera.pinhole(1, 1, 0, 0, T=[[1, 0, 0]])


# ------------------------------------------------------------------------------------------------ the yardstick's own properties
def grid_cloud(H, W, x0, y0, pitch, rng, holes=0.1, jitter=0.3):
    """organised [H,W,3]: x = x0 + j pitch, y = y0 + i pitch with jitter within +-`jitter` pitch, z in 1..2; `holes` of it zeroed"""
    ii, jj = np.mgrid[0:H, 0:W]
    pc = np.stack([x0 + (jj + rng.uniform(-jitter, jitter, (H, W))) * pitch, y0 + (ii + rng.uniform(-jitter, jitter, (H, W))) * pitch,
                   rng.uniform(1, 2, (H, W))], axis=2).astype(np.float32)
    pc[rng.uniform(size=(H, W)) < holes] = 0
    return pc


def unorganize(pc):
    """(points [N,3], pix2pt [H W]) of an organised cloud, as cmdiad_unorganize: the valid pixels in raster order"""
    flat = pc.reshape(-1, 3)
    ok = R.valid(flat)
    pix2pt = np.where(ok, np.cumsum(ok) - 1, -1).astype(np.int32)
    return flat[ok], pix2pt


def test_grid_cloud_comes_back():
    rng = np.random.default_rng(5)
    for H, W, x0, y0, pitch in ((33, 65, 0.7, -3.1, 0.013), (64, 64, -20.0, 11.0, 1.7)):
        pc = grid_cloud(H, W, x0, y0, pitch, rng)
        pts, pix2pt = unorganize(pc)
        cam = np.array(og.Camera.orthographic(x0, y0, pitch).row())
        out = R.organize(pts, [0, len(pts)], [cam], 0, H, W)
        assert np.array_equal(out["index"][0].reshape(-1), pix2pt) and out["xyz"][0].tobytes() == pc.tobytes()
        assert out["stats"].tolist() == [[0, 0, len(pts), 0]] and np.array_equal(out["pixel_of_point"], np.nonzero(pix2pt >= 0)[0])


def test_tie_rule_and_occlusion():
    cam = R.camera_row([0, 0, 1, 1])
    near = np.float32(1.0)
    pts = np.array([[2, 1, 5], [2.2, 1.1, near], [1.9, 0.8, 3], [2.1, 1.3, near], [2, 1, np.nextafter(near, np.float32(2))]], np.float32)
    out = R.organize(pts, [0, 5], [cam], 0, 4, 4)
    assert np.all(out["pixel_of_point"] == 1 * 4 + 2) and out["index"][0, 1, 2] == 1            # the nearest; of two equal, the first
    assert (out["index"] >= 0).sum() == 1 and out["stats"].tolist() == [[0, 0, 1, 0]]
    # equal after rounding to float32 only: a T that adds 2^-40 to the second point's depth
    T = np.eye(3, 4)
    T[2, 0] = 2.0 ** -40
    pts = np.array([[1, 1, 1], [3, 1, 1], [-8, 1, 1]], np.float32)
    cam = R.camera_row([0, 0, 0.01, 1], T)                                                     # u = x / 100: all three in column 0
    c2 = R.camera_coords(pts, cam)[2]
    assert c2[2] < c2[0] < c2[1] and len(set(c2.astype(np.float32))) == 1
    assert R.organize(pts, [0, 3], [cam], 0, 4, 4)["index"][0, 1, 0] == 0
    # -0.0 and +0.0 are one depth, negative depths are nearer than positive ones
    T = np.eye(3, 4)
    T[2, 2], T[2, 3] = 1.0, -1.0
    pts = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 0.5], [1, 1, 2]], np.float32)
    pts_flip = pts.copy()
    out = R.organize(pts_flip, [0, 4], [R.camera_row([0, 0, 1, 1], T)], 0, 4, 4)
    assert out["index"][0, 1, 1] == 2                                                          # depth -0.5 wins over 0 and 1


def test_fill_never_overrides_and_does_not_cascade():
    rng = np.random.default_rng(9)
    H, W = 12, 9
    pc = grid_cloud(H, W, 1.0, 1.0, 1.0, rng, holes=0.5, jitter=0.0)
    pc[0:6, 0:6] = 0                                                                            # a hole wider than any window
    pts, pix2pt = unorganize(pc)
    cam = R.camera_row([1, 1, 1, 1])
    base = R.organize(pts, [0, len(pts)], [cam], 0, H, W)
    assert np.array_equal(base["index"][0].reshape(-1), pix2pt)
    for fill in (1, 2):
        out = R.organize(pts, [0, len(pts)], [cam], 0, H, W, fill=fill)
        direct = base["index"][0] >= 0
        assert np.array_equal(out["index"][0][direct], base["index"][0][direct]) and out["keys"].tobytes() == base["keys"].tobytes()
        assert out["stats"][0, 2] == direct.sum() and out["stats"][0, 3] == ((out["index"][0] >= 0) & ~direct).sum()
        for y, x in zip(*np.nonzero(~direct)):
            win = base["keys"][0][max(y - fill, 0):y + fill + 1, max(x - fill, 0):x + fill + 1]
            if np.all(win == R.EMPTY):
                assert out["index"][0, y, x] == -1                                              # only holes around: stays a hole
            else:
                assert out["index"][0, y, x] == int(win.min() & np.uint64(0xFFFFFFFF))
        assert out["index"][0, 0, 0] == -1 and out["index"][0, 2, 2] == -1
    assert out["stats"][0, 3] > 0


def test_offsets_are_clamped():
    assert R.ranges([0, 5, 3, 99, -4], 10) == [(0, 5), (5, 5), (3, 10), (10, 10)]
    assert R.ranges([-7, -2, 4], 10) == [(0, 0), (0, 4)]
