"""The yardstick of docs/organize.md in numpy float64: element-wise arithmetic in the written order (numpy never contracts a
multiply and an add), a `np.minimum.at` key map, and a plain loop over the holes for the fill.  Used byte for byte by
tests/test_organize_cpu.py and tests/test_gpu_organize.py; it shares no code with cmdiad_amd."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def f2ord(f32):
    u = np.asarray(f32, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ranges(offsets, P):
    """[(lo_b, hi_b)]: both ends clamped, whatever the table holds"""
    out = []
    for b in range(len(offsets) - 1):
        lo = min(max(int(offsets[b]), 0), P)
        hi = min(max(int(offsets[b + 1]), lo), P)
        out.append((lo, hi))
    return out


def valid(pts):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return np.all(np.isfinite(pts), axis=1) & np.all(pts != 0, axis=1)


def camera_coords(pts, cam):
    """c_0, c_1, c_2 of float32 points [N,3] under the 16 doubles of a camera"""
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    t = np.asarray(cam, np.float64)
    with np.errstate(all="ignore"):
        return [((t[4 * k] * x + t[4 * k + 1] * y) + t[4 * k + 2] * z) + t[4 * k + 3] for k in range(3)]


def project(pts, cam, kind, H, W):
    """-> (pixel_of_point int32 [N] (-2 dropped, -1 outside, vf W + uf), d32 float32 [N])"""
    t = np.asarray(cam, np.float64)
    a, b, c, d = t[12:16]
    c0, c1, c2 = camera_coords(pts, cam)
    with np.errstate(all="ignore"):
        if kind == 0:
            u, v = (c0 - a) * c, (c1 - b) * d
            ok = np.ones(len(c0), bool)
        else:
            u, v = a * (c0 / c2) + c, b * (c1 / c2) + d
            ok = c2 > 0
        uf, vf = np.floor(u + 0.5), np.floor(v + 0.5)
        d32 = c2.astype(np.float32)
        d32 = np.where(d32 == 0, np.float32(0), d32).astype(np.float32)
        inside = ok & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H) & (np.abs(d32) < np.inf)
    pix = np.full(len(c0), -1, np.int64)
    pix[inside] = vf[inside].astype(np.int64) * W + uf[inside].astype(np.int64)
    pix[~valid(pts)] = -2
    return pix.astype(np.int32), d32


def splat(points, offsets, cams, kind, H, W, max_len=None, pixel_of_point=None):
    """-> (keys uint64 [n,H,W], pixel_of_point int32 [P], stats int32 [n,2] = dropped, outside).  pixel_of_point: the buffer to write
    into (only the points looked at are written), default a fresh one of -3."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    P, n = len(points), len(offsets) - 1
    keys = np.full((n, H * W), EMPTY, np.uint64)
    pop = np.full(P, -3, np.int32) if pixel_of_point is None else pixel_of_point
    stats = np.zeros((n, 2), np.int32)
    for b, (lo, hi) in enumerate(ranges(offsets, P)):
        if max_len is not None:
            hi = min(hi, lo + int(max_len))
        pix, d32 = project(points[lo:hi], cams[b], kind, H, W)
        pop[lo:hi] = pix
        stats[b] = [(pix == -2).sum(), (pix == -1).sum()]
        placed = np.nonzero(pix >= 0)[0]
        key = (f2ord(d32[placed]).astype(np.uint64) << np.uint64(32)) | placed.astype(np.uint64)
        np.minimum.at(keys[b], pix[placed], key)
    return keys.reshape(n, H, W), pop, stats


def resolve(points, offsets, keys, fill=0, colors=None, labels=None):
    """-> (index int32 [n,H,W], xyz float32 [n,H,W,3], rgb uint8 [n,H,W,3], mask uint8 [n,H,W], stats int32 [n,2] = direct, filled)"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    P = len(points)
    n, H, W = keys.shape
    index = np.full((n, H, W), -1, np.int32)
    xyz = np.zeros((n, H, W, 3), np.float32)
    rgb = np.zeros((n, H, W, 3), np.uint8)
    mask = np.zeros((n, H, W), np.uint8)
    stats = np.zeros((n, 2), np.int32)
    for b, (lo, hi) in enumerate(ranges(offsets, P)):
        win = keys[b].copy()
        if fill:
            for y, x in zip(*np.nonzero(keys[b] == EMPTY)):
                win[y, x] = keys[b][max(y - fill, 0):y + fill + 1, max(x - fill, 0):x + fill + 1].min()
        idx = (win & np.uint64(0xFFFFFFFF)).astype(np.int64)
        won = (win != EMPTY) & (lo + idx < hi)
        direct = keys[b] != EMPTY
        stats[b] = [(won & direct).sum(), (won & ~direct).sum()]
        src = lo + idx[won]
        index[b][won] = idx[won]
        xyz[b][won] = points[src]
        if colors is not None:
            rgb[b][won] = np.asarray(colors, np.uint8).reshape(-1, 3)[src]
        if labels is not None:
            mask[b][won] = np.where(np.asarray(labels, np.uint8).reshape(-1)[src] != 0, 255, 0)
    return index, xyz, rgb, mask, stats


def organize(points, offsets, cams, kind, H, W, fill=0, colors=None, labels=None, max_len=None):
    """-> dict of everything the device returns; stats int32 [n,4]"""
    keys, pop, s01 = splat(points, offsets, cams, kind, H, W, max_len)
    index, xyz, rgb, mask, s23 = resolve(points, offsets, keys, fill, colors, labels)
    return dict(keys=keys, pixel_of_point=pop, index=index, xyz=xyz, rgb=rgb, mask=mask, stats=np.concatenate([s01, s23], axis=1))


def bounds(points, offsets, cams, max_len=None):
    """-> (float64 [n,6] = min of c_0..c_2, then max, over the valid points; int32 [n]).  A NaN enters neither; zeros are +0.0."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    P, n = len(points), len(offsets) - 1
    out, cnt = np.empty((n, 6), np.float64), np.zeros(n, np.int32)
    for b, (lo, hi) in enumerate(ranges(offsets, P)):
        if max_len is not None:
            hi = min(hi, lo + int(max_len))
        p = points[lo:hi][valid(points[lo:hi])]
        cnt[b] = len(p)
        for k, c in enumerate(camera_coords(p, cams[b])):
            c = np.where(c == 0, 0.0, c)
            out[b, k] = np.fmin.reduce(c, initial=np.inf)
            out[b, 3 + k] = np.fmax.reduce(c, initial=-np.inf)
    return out, cnt


def scores_to_points(maps, pixel_of_point, offsets):
    """float32 [P]: the map at each placed point's own pixel, NaN elsewhere"""
    maps = np.asarray(maps)
    n = maps.shape[0]
    flat = maps.reshape(n, -1).astype(np.float32)
    out = np.full(len(pixel_of_point), np.nan, np.float32)
    for b, (lo, hi) in enumerate(ranges(offsets, len(pixel_of_point))):
        pix = pixel_of_point[lo:hi]
        ok = pix >= 0
        out[lo:hi][ok] = flat[b][pix[ok]]
    return out


def camera_row(kind_params, T=None):
    """16 doubles: T (3 x 4, default identity) and a, b, c, d"""
    T = np.eye(3, 4) if T is None else np.asarray(T, np.float64)[:3]
    return np.concatenate([T.reshape(-1), np.asarray(kind_params, np.float64)])
