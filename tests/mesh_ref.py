"""The yardstick of the mesh contract (docs/mesh.md), written from the contract's text with per-pixel loops -- not from the
kernels: nothing here imports cmdiad_amd.  Every floating-point step is ONE float64 operation per statement: Python floats are IEEE
float64 scalars, every coordinate is widened from its float32 first, and math.sqrt is correctly rounded.

mesh(cloud [H,W,3] f32, score [H,W] f64, lo, hi, lut, alpha, ...) -> (vertex bytes, face bytes, counts [4], vidx [H,W]) of ONE image;
batch(...) runs it per image.  The colour steps are overlay_ref's (index_of, bg_byte): the contract names them.
"""
import math
import struct

import numpy as np

from overlay_ref import bg_byte, index_of

VERTEX_BYTES, FACE_BYTES = 35, 13


def finite(p):
    return all(math.isfinite(float(v)) for v in p)


def valid(p):
    """all three coordinates non-zero (-0.0 is zero) and finite"""
    return finite(p) and all(float(v) != 0.0 for v in p)


def edge_d2(p, q):
    dx = float(p[0]) - float(q[0])
    dy = float(p[1]) - float(q[1])
    dz = float(p[2]) - float(q[2])
    xx = dx * dx
    yy = dy * dy
    zz = dz * dz
    s = xx + yy
    return s + zz


def cross(a, b, c):
    """(b - a) x (c - a): per component two products and one difference"""
    ux, uy, uz = float(b[0]) - float(a[0]), float(b[1]) - float(a[1]), float(b[2]) - float(a[2])
    vx, vy, vz = float(c[0]) - float(a[0]), float(c[1]) - float(a[1]), float(c[2]) - float(a[2])
    p0, p1 = uy * vz, uz * vy
    p2, p3 = uz * vx, ux * vz
    p4, p5 = ux * vy, uy * vx
    return p0 - p1, p2 - p3, p4 - p5


def cell_triangles(y, x):
    """T0, T1 of cell (y, x) as pixel triples"""
    return ((y, x), (y, x + 1), (y + 1, x + 1)), ((y, x), (y + 1, x + 1), (y + 1, x))


def mesh(cloud, score, lo, hi, lut, alpha, bg=None, bg_kind=0, mean=(0, 0, 0), std=(1, 1, 1), labels=None, max_edge2=math.inf, flip=False):
    cloud = np.asarray(cloud, dtype=np.float32)
    score = np.asarray(score, dtype=np.float64)
    H, W = score.shape
    assert cloud.shape == (H, W, 3)
    max_edge2 = float(max_edge2)
    ok = np.array([[valid(cloud[y, x]) for x in range(W)] for y in range(H)], dtype=bool).reshape(H, W)
    bad = sum(not finite(cloud[y, x]) for y in range(H) for x in range(W))
    vidx = np.full((H, W), -1, dtype=np.int32)
    vidx[ok] = np.arange(int(ok.sum()), dtype=np.int32)          # raster order

    def emitted(tri):
        if not all(0 <= y < H and 0 <= x < W and ok[y, x] for y, x in tri):
            return False
        a, b, c = (cloud[y, x] for y, x in tri)
        return edge_d2(a, b) <= max_edge2 and edge_d2(b, c) <= max_edge2 and edge_d2(c, a) <= max_edge2

    faces, kept = bytearray(), {}
    for y in range(H - 1):
        for x in range(W - 1):
            for t, tri in enumerate(cell_triangles(y, x)):
                kept[(y, x, t)] = emitted(tri)
                if kept[(y, x, t)]:
                    a, b, c = (int(vidx[p]) for p in tri)
                    faces += struct.pack("<Biii", 3, a, c, b) if flip else struct.pack("<Biii", 3, a, b, c)

    verts, nan = bytearray(), 0
    for y in range(H):
        for x in range(W):
            if not ok[y, x]:
                continue
            nx = ny = nz = 0.0
            for cy, cx, t in ((y - 1, x - 1, 0), (y - 1, x - 1, 1), (y - 1, x, 1), (y, x - 1, 0), (y, x, 0), (y, x, 1)):
                if kept.get((cy, cx, t), False):
                    a, b, c = (cloud[p] for p in cell_triangles(cy, cx)[t])
                    n0, n1, n2 = cross(a, b, c)
                    nx = nx + n0
                    ny = ny + n1
                    nz = nz + n2
            xx = nx * nx
            yy = ny * ny
            zz = nz * nz
            s2 = xx + yy
            s2 = s2 + zz
            length = math.sqrt(s2)
            normal = [np.float32(0.0)] * 3
            if length > 0 and math.isfinite(length):
                normal = [np.float32(nx / length), np.float32(ny / length), np.float32(nz / length)]
            if flip:
                normal = [-v for v in normal]
            s = score[y, x]
            k, is_nan = index_of(s, lo, hi)
            nan += is_nan
            c = [int(v) for v in lut[k]]
            if bg_kind:
                a = int(alpha[k])
                g = [int(v) for v in bg[y, x]] if bg_kind == 1 else [bg_byte(bg[ch, y, x], mean[ch], std[ch]) for ch in range(3)]
                c = [(c[ch] * a + g[ch] * (255 - a) + 127) // 255 for ch in range(3)]
            with np.errstate(over="ignore"):
                s32 = np.float32(s)
            verts += cloud[y, x].tobytes() + np.array(normal, dtype="<f4").tobytes() + bytes(c) + np.array([s32], dtype="<f4").tobytes()
            verts += struct.pack("<i", int(labels[y, x]) if labels is not None else 0)
    counts = np.array([int(ok.sum()), len(faces) // FACE_BYTES, bad, nan], dtype=np.int32)
    return bytes(verts), bytes(faces), counts, vidx


def batch(clouds, maps, lo, hi, lut, alpha, bg=None, bg_kind=0, labels=None, **kw):
    """clouds [n,H,W,3]; lo, hi: scalars or one per image -> lists of vertex bytes and face bytes, counts [n,4], vidx [n,H,W]"""
    n = len(maps)
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64).reshape(-1), (n,)), np.broadcast_to(np.asarray(hi, np.float64).reshape(-1), (n,))
    out = [mesh(clouds[i], maps[i], lo[i], hi[i], lut, alpha, bg=None if bg is None else bg[i], bg_kind=bg_kind,
                labels=None if labels is None else labels[i], **kw) for i in range(n)]
    return [o[0] for o in out], [o[1] for o in out], np.stack([o[2] for o in out]), np.stack([o[3] for o in out])


def kept_triangles(cloud, max_edge2=math.inf):
    """{(y, x, t): emitted} of one image, for tests that reason about which triangles a case keeps"""
    cloud = np.asarray(cloud, dtype=np.float32)
    H, W = cloud.shape[:2]
    out = {}
    for y in range(H - 1):
        for x in range(W - 1):
            for t, tri in enumerate(cell_triangles(y, x)):
                pts = [cloud[p] for p in tri]
                out[(y, x, t)] = all(valid(p) for p in pts) and all(edge_d2(pts[i], pts[(i + 1) % 3]) <= max_edge2 for i in range(3))
    return out
