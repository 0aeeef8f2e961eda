"""CPU (no GPU): the PLY container (utils/ply.py) through its round trip and its refusals, the yardstick of the mesh contract
(tests/mesh_ref.py) on a plane, MeshSpec's checks, and the argument validation of cmdiad_mesh_count / cmdiad_mesh_write, which
happens before any launch."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402

from cmdiad_amd import mesh  # noqa: E402
from cmdiad_amd.utils import ply  # noqa: E402

GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
OPAQUE = np.full(256, 255, np.uint8)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plane(H, W, z=2.0):
    """a fully valid plane z = const over a unit grid that starts at (1, 1): no coordinate is zero"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([xx + 1.0, yy + 1.0, np.full((H, W), z)], axis=2).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the container
def test_record_sizes_and_header():
    assert ply.VERTEX_BYTES == R.VERTEX_BYTES == 35 and ply.FACE_BYTES == R.FACE_BYTES == 13
    lines = ply.header(7, 4, ["class rope", "index 3"]).decode("ascii").split("\n")
    assert lines[:5] == ["ply", "format binary_little_endian 1.0", "comment cmdiad_amd mesh 1", "comment class rope", "comment index 3"]
    assert lines[5] == "element vertex 7" and lines[-4:] == ["element face 4", "property list uchar int vertex_indices", "end_header", ""]
    props = [ln for ln in lines if ln.startswith("property ") and "list" not in ln]
    assert props == ["property float x", "property float y", "property float z", "property float nx", "property float ny",
                     "property float nz", "property uchar red", "property uchar green", "property uchar blue", "property float score",
                     "property int region"]
    assert b"\r" not in ply.header(0, 0)
    for bad in ("two\nlines", "tab\there", "café", "cr\r"):
        with pytest.raises(ply.PlyError, match="printable ASCII"):
            ply.header(1, 1, [bad])
    with pytest.raises(ply.PlyError):
        ply.header(-1, 0)


def test_write_read_round_trip(tmp_path):
    cloud = plane(4, 5)
    score = np.linspace(0.0, 1.0, 20).reshape(4, 5)
    labels = np.arange(20, dtype=np.int32).reshape(4, 5) % 3
    vb, fb, counts, vidx = R.mesh(cloud, score, 0.0, 1.0, GREY, OPAQUE, labels=labels)
    path = str(tmp_path / "a.ply")
    size = ply.write(path, counts[0], vb, counts[1], fb, ["hello"])
    assert size == os.path.getsize(path) == len(ply.header(20, 24, ["hello"])) + 20 * 35 + 24 * 13
    assert os.listdir(tmp_path) == ["a.ply"]                                      # the temporary name is gone
    verts, faces, comments = ply.read(path)
    assert comments == ["hello"] and verts.tobytes() == vb and faces.tobytes() == fb
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], axis=1), cloud.reshape(-1, 3))
    assert np.array_equal(verts["score"], score.reshape(-1).astype(np.float32)) and np.array_equal(verts["region"], labels.reshape(-1))
    assert np.array_equal(verts["red"], [R.index_of(s, 0.0, 1.0)[0] for s in score.reshape(-1)])
    assert np.all(faces["n"] == 3) and faces["vertex_indices"].shape == (24, 3)
    # structured arrays and numpy bytes are taken as well as bytes
    ply.write(path, 20, verts, 24, np.frombuffer(fb, np.uint8), [])
    assert ply.read(path)[0].tobytes() == vb
    # no vertex and no face
    empty = str(tmp_path / "empty.ply")
    ply.write(empty, 0, b"", 0, b"")
    verts, faces, comments = ply.read(empty)
    assert len(verts) == 0 and len(faces) == 0 and comments == [] and verts.dtype == ply.VERTEX and faces.dtype == ply.FACE
    # vertices without faces
    ply.write(empty, 20, vb, 0, b"")
    assert len(ply.read(empty)[0]) == 20 and len(ply.read(empty)[1]) == 0
    sizes = ply.write_many([str(tmp_path / f"m{i}.ply") for i in range(3)], [20, 0, 20], [np.frombuffer(vb, np.uint8)] * 3, [24, 0, 0],
                           [np.frombuffer(fb, np.uint8)] * 3, comments=[["a"], [], ["b", "c"]], writers=2)
    assert sizes == [os.path.getsize(str(tmp_path / f"m{i}.ply")) for i in range(3)]
    assert ply.read(str(tmp_path / "m2.ply"))[2] == ["b", "c"] and len(ply.read(str(tmp_path / "m1.ply"))[0]) == 0
    with pytest.raises(ply.PlyError, match="paths"):
        ply.write_many([path], [1, 2], [vb], [0], [fb])


def test_damaged_files_are_refused(tmp_path):
    vb, fb, counts, _ = R.mesh(plane(3, 3), np.zeros((3, 3)), 0.0, 1.0, GREY, OPAQUE)
    path = str(tmp_path / "a.ply")
    ply.write(path, 9, vb, 8, fb, ["c"])
    good = open(path, "rb").read()

    def refused(blob, match):
        with open(path, "wb") as f:
            f.write(blob)
        with pytest.raises(ply.PlyError, match=match):
            ply.read(path)
    refused(good[:-1], "the file has")                                                       # truncated by one byte
    refused(good[:len(good) // 2], "the file has")
    refused(good + b"\0", "the file has")
    refused(good[:40], "not a PLY file")                                                      # cut inside the header
    refused(b"plx" + good[3:], "not a PLY file")
    refused(good.replace(b"binary_little_endian", b"binary_big_endian", 1), "does not start with")
    refused(good.replace(b"comment cmdiad_amd mesh 1\n", b"", 1), "does not start with")
    refused(good.replace(b"element vertex 9", b"element vertex 8", 1), "the file has")         # wrong counts
    refused(good.replace(b"element face 8", b"element face 9", 1), "the file has")
    refused(good.replace(b"element vertex 9", b"element vertex -9", 1), "bad header line")
    refused(good.replace(b"element vertex 9", b"element vertex 99999999999999999999", 1), "bad header line")
    refused(good.replace(b"property float nx\n", b"", 1), "element and property lines")
    refused(good.replace(b"property float score", b"property double score", 1), "bad header line")
    at = len(ply.header(9, 8, ["c"])) + 9 * 35
    refused(good[:at] + b"\x04" + good[at + 1:], "not a triangle")                             # a quad
    refused(good[:at + 1] + (9).to_bytes(4, "little") + good[at + 5:], "not a triangle")       # an index past the vertices
    with pytest.raises(ply.PlyError, match="bytes of vertex records"):
        ply.write(path, 9, vb[:-1], 8, fb)
    with pytest.raises(ply.PlyError, match="bytes of face records"):
        ply.write(path, 9, vb, 7, fb)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_plane_gives_every_triangle_and_unit_normals():
    H, W = 5, 7
    cloud = plane(H, W)
    vb, fb, counts, vidx = R.mesh(cloud, np.zeros((H, W)), 0.0, 1.0, GREY, OPAQUE)
    assert counts.tolist() == [H * W, 2 * (H - 1) * (W - 1), 0, 0] and np.array_equal(vidx, np.arange(H * W).reshape(H, W))
    v, f = np.frombuffer(vb, ply.VERTEX), np.frombuffer(fb, ply.FACE)
    # x grows with the column and y with the row: (b - a) x (c - a) of T0 and T1 points along +z
    assert np.all(v["nx"] == 0) and np.all(v["ny"] == 0) and np.all(v["nz"] == 1)
    assert f["vertex_indices"][0].tolist() == [0, 1, W + 1] and f["vertex_indices"][1].tolist() == [0, W + 1, W]       # cell (0,0): T0, T1
    assert f["vertex_indices"][2].tolist() == [1, 2, W + 2]                                                            # then cell (0,1)
    vb2, fb2, counts2, _ = R.mesh(cloud, np.zeros((H, W)), 0.0, 1.0, GREY, OPAQUE, flip=True)
    v2, f2 = np.frombuffer(vb2, ply.VERTEX), np.frombuffer(fb2, ply.FACE)
    assert np.array_equal(counts2, counts) and np.all(v2["nz"] == -1) and np.all(v2["nx"] == 0) and np.all(v2["ny"] == 0)
    assert np.array_equal(f2["vertex_indices"], f["vertex_indices"][:, [0, 2, 1]])                                      # a, c, b
    for name in ("x", "y", "z", "red", "score", "region"):
        assert np.array_equal(v2[name], v[name])
    # a plane seen from the other side (x decreasing with the column) has normals along -z without the flip
    v3 = np.frombuffer(R.mesh(cloud[:, ::-1], np.zeros((H, W)), 0.0, 1.0, GREY, OPAQUE)[0], ply.VERTEX)
    assert np.all(v3["nz"] == -1)


def test_validity_cut_and_counts_of_the_yardstick():
    cloud = plane(4, 4)
    cloud[0, 0] = 0.0                      # the reference's invalid point
    cloud[1, 1, 2] = -0.0                  # -0.0 is zero
    cloud[2, 2, 0] = 0.0                   # one zero coordinate is enough
    cloud[3, 3, 1] = np.inf                # not finite: invalid and counted
    cloud[3, 0, 2] = np.nan
    score = np.zeros((4, 4))
    score[0, 1], score[3, 3] = np.nan, np.nan        # the second NaN sits on an invalid point: not counted
    vb, fb, counts, vidx = R.mesh(cloud, score, 0.0, 1.0, GREY, OPAQUE)
    assert counts.tolist() == [11, len(fb) // 13, 2, 1]
    assert vidx[0, 0] == vidx[1, 1] == vidx[2, 2] == vidx[3, 3] == vidx[3, 0] == -1 and vidx[0, 1] == 0 and vidx.max() == 10
    v = np.frombuffer(vb, ply.VERTEX)
    assert np.isnan(v["score"][0]) and v["red"][0] == 0                                     # t = 0
    kept = R.kept_triangles(cloud)
    assert sum(kept.values()) == counts[1] and not kept[(0, 0, 0)] and kept[(0, 2, 0)] and kept[(0, 2, 1)]
    # an isolated vertex has the zero normal: (1, 0) touches cells whose other corners (0,0), (1,1) are invalid
    lonely = np.zeros((2, 2, 3), np.float32)
    lonely[0, 0] = (1, 1, 1)
    v = np.frombuffer(R.mesh(lonely, np.zeros((2, 2)), 0.0, 1.0, GREY, OPAQUE)[0], ply.VERTEX)
    assert len(v) == 1 and (v["nx"][0], v["ny"][0], v["nz"][0]) == (0, 0, 0)
    # max_edge2: a step of 3 along z between columns 1 and 2 cuts the triangles that cross it, and only those
    step = plane(3, 4)
    step[:, 2:, 2] += 3.0
    kept = R.kept_triangles(step, max_edge2=2.5)                                            # unit edges 1, diagonals 2
    assert all(kept[(y, x, t)] == (x != 1) for y in range(2) for x in range(3) for t in range(2))
    assert all(R.kept_triangles(step).values())


def test_mesh_spec_checks():
    s = mesh.MeshSpec(0.0, 2.0)
    assert s.max_edge is None and s.max_edge2 == math.inf and s.flip_normals is False and s.lut.shape == (256, 3) and s.alpha.shape == (256,)
    assert mesh.MeshSpec(0.0, 2.0, max_edge=1.5, flip_normals=True).max_edge2 == 2.25
    assert mesh.MeshSpec(1.0, 1.0).hi.tolist() == [1.0]                                     # a step at lo, as the overlay's
    for lo, hi in ((math.nan, 1.0), (0.0, math.nan), (0.0, math.inf), (2.0, 1.0), ([0.0, 3.0], [1.0, 2.0])):
        with pytest.raises(ValueError):
            mesh.MeshSpec(lo, hi)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_edge"):
            mesh.MeshSpec(0.0, 1.0, max_edge=bad)

    class Cal:
        pixel_threshold = 0.75
    s = mesh.MeshSpec.from_calibration(Cal(), 2.0, max_edge=0.5)
    assert s.lo.tolist() == [0.0] and s.hi.tolist() == [1.5] and s.max_edge == 0.5
    with pytest.raises(ValueError, match="span"):
        mesh.MeshSpec.from_calibration(Cal(), 0.0)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_reject_bad_arguments_before_any_launch():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    assert L.cmdiad_abi_version() == 6
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    for name in ("cmdiad_mesh_count", "cmdiad_mesh_write"):
        assert f"int {name}(" in hdr and name in nat.SIGNATURES and hasattr(L, name)
        assert getattr(L, name).argtypes == nat.SIGNATURES[name]
    assert not [q for q in nat.SIZE_QUERIES if "mesh" in q]                                  # neither has a workspace
    one = ctypes.c_void_p(16)             # a non-null pointer that a rejected call never follows
    inf = math.inf

    def count(n=1, H=4, W=5, pix=None, ch=None, max2=inf, ptr=one, **over):
        pix, ch = (1, H * W) if pix is None else (pix, ch)
        a = dict(cloud=ptr, maps=ptr, chunks=ptr, counts=ptr)
        a.update(over)
        return L.cmdiad_mesh_count(a["cloud"], pix, ch, a["maps"], n, H, W, max2, a["chunks"], a["counts"], None)

    def write(n=1, H=4, W=5, pix=None, ch=None, max2=inf, ptr=one, lohi_per=0, kind=0, flip=0, **over):
        pix, ch = (1, H * W) if pix is None else (pix, ch)
        a = dict(cloud=ptr, maps=ptr, lohi=ptr, lut=ptr, alpha=ptr, bg=None, labels=None, chunks=ptr, vidx=ptr, vertices=ptr, faces=ptr)
        a.update(over)
        return L.cmdiad_mesh_write(a["cloud"], pix, ch, a["maps"], n, H, W, a["lohi"], lohi_per, a["lut"], a["alpha"], a["bg"], kind,
                                   0.0, 0.0, 0.0, 1.0, 1.0, 1.0, a["labels"], max2, flip, a["chunks"], a["vidx"], a["vertices"],
                                   a["faces"], None)
    for fn, name in ((count, b"cmdiad_mesh_count"), (write, b"cmdiad_mesh_write")):
        for kw in (dict(H=0), dict(W=0), dict(H=(1 << 14) + 1), dict(W=(1 << 14) + 1), dict(n=-1), dict(n=65536),
                   dict(n=5, H=1 << 11, W=1 << 11), dict(n=2, H=1 << 12, W=(1 << 11) + 1)):
            assert fn(**kw) == -1 and name + b": bad sizes" in L.cmdiad_last_error(), (kw, L.cmdiad_last_error())
        for pix, ch in ((1, 19), (3, 2), (2, 1), (0, 0), (20, 1)):
            assert fn(pix=pix, ch=ch) == -1 and name + b": bad strides" in L.cmdiad_last_error(), (pix, ch)
        for max2 in (0.0, -1.0, math.nan, -inf):
            assert fn(max2=max2) == -1 and name + b": max_edge2" in L.cmdiad_last_error(), max2
        assert fn(ptr=None) == -1 and b"null pointer" in L.cmdiad_last_error()
        assert fn(n=0, ptr=None) == 0                                                        # nothing to do: no launch
        assert fn(n=0, pix=3, ch=1, ptr=None) == 0
        assert fn(n=0, H=0, ptr=None) == -1                                                  # the sizes are checked first
    for at in ("cloud", "maps", "chunks", "counts"):
        assert count(**{at: None}) == -1 and b"cmdiad_mesh_count: null pointer" in L.cmdiad_last_error(), at
    for at in ("cloud", "maps", "lohi", "lut", "alpha", "chunks", "vidx", "vertices", "faces"):
        assert write(**{at: None}) == -1 and b"cmdiad_mesh_write: null pointer" in L.cmdiad_last_error(), at
    for kw, text in ((dict(kind=3), b"background kind 3"), (dict(kind=-1), b"background kind -1"), (dict(kind=1), b"null pointer"),
                     (dict(kind=2), b"null pointer"), (dict(flip=2), b"flip=2"), (dict(flip=-1), b"flip=-1"), (dict(lohi_per=2), b"lohi_per_image=2")):
        assert write(**kw) == -1 and text in L.cmdiad_last_error(), (kw, L.cmdiad_last_error())


def test_wrappers_refuse_before_a_device_is_touched():
    import torch
    from cmdiad_amd import ops
    with pytest.raises(Exception, match="GPU"):
        ops.mesh_count(torch.zeros(1, 3, 4, 5), torch.zeros(1, 4, 5, dtype=torch.float64))
    assert callable(ops.mesh_write) and ops.MESH_VERTEX_BYTES == ply.VERTEX_BYTES and ops.MESH_FACE_BYTES == ply.FACE_BYTES
