"""The yardstick of the measurement tables (docs/regions.md, "Contract of a measurement table"): numpy only -- per-label loops over
the box, every sum by math.fsum over terms computed one float64 operation at a time, and the per-term arrays kept, so that a
test can compute its bounds from them.  Not a test file; tests/test_regions3d_cpu.py validates it against closed forms, the GPU
tests hold cmdiad_region_measure to it."""
import math

import numpy as np

S2_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # xx, xy, xz, yy, yz, zz


def interleaved(cloud, layout):
    """One image's cloud as [H,W,3] float32, from 'planar' [3,H,W] or 'interleaved' [H,W,3]."""
    c = np.asarray(cloud)
    assert c.dtype == np.float32, c.dtype
    return np.ascontiguousarray(c.transpose(1, 2, 0)) if layout == "planar" else c


def valid(points):
    """[...,3] float32 -> bool: all three coordinates non-zero (-0.0 is zero) and finite."""
    return ((points != 0) & np.isfinite(points)).all(-1)


def bad_points(clouds_hw3):
    """Points of whole frames [n,H,W,3] with a non-finite coordinate."""
    return int((~np.isfinite(clouds_hw3)).any(-1).sum())


def triangle(a, b, c):
    """float64 [m,3] each -> (0.5 |(b - a) x (c - a)| [m], |b - a| |c - a| [m]), every step one rounded float64 operation in the
    contract's order (cross = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), squares summed left to right)."""
    u, v = b - a, c - a
    cx, cy, cz = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz), np.sqrt((u * u).sum(1)) * np.sqrt((v * v).sum(1))


def measure_slot(labels, row, cloud):
    """labels [H,W] int32, row = the slot's eight integers, cloud [H,W,3] float32 -> dict(m_ints [4] int32, m_vals [20] float64,
    s1_terms [n_pts,3], s2_terms [n_pts,6], area_terms [n_tri], edge_terms [n_tri] = |e1| |e2| of every counted triangle)."""
    H, W = labels.shape
    L, x0, y0, x1, y1, px, py = int(row[0]), int(row[2]), int(row[3]), int(row[4]), int(row[5]), int(row[6]), int(row[7])
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    mi, mv = np.zeros(4, np.int32), np.zeros(20, np.float64)
    empty = dict(m_ints=mi, m_vals=mv, s1_terms=np.zeros((0, 3)), s2_terms=np.zeros((0, 6)), area_terms=np.zeros(0), edge_terms=np.zeros(0))
    if L < 1 or x1 < x0 or y1 < y0:
        return empty
    ok = (labels == L) & valid(cloud)                 # vertices: anywhere in the image
    inbox = np.zeros_like(ok)
    inbox[y0:y1 + 1, x0:x1 + 1] = True
    ys, xs = np.nonzero(ok & inbox)                   # raster order
    if ys.size == 0:
        return empty
    p = cloud[ys, xs].astype(np.float64)              # widened: exact
    lo, hi = p.min(0), p.max(0)
    d = p - lo
    s1_terms = d
    s2_terms = np.stack([d[:, a] * d[:, b] for a, b in S2_PAIRS], 1)
    c64 = cloud.astype(np.float64)
    cell = (ys + 1 < H) & (xs + 1 < W)                # top-left pixels of a grid cell
    cy, cx = ys[cell], xs[cell]
    area_terms, edge_terms = [], []
    for (ya, xa), (yb, xb) in (((cy, cx + 1), (cy + 1, cx + 1)), ((cy + 1, cx + 1), (cy + 1, cx))):
        keep = ok[ya, xa] & ok[yb, xb]
        t, e = triangle(c64[cy[keep], cx[keep]], c64[ya[keep], xa[keep]], c64[yb[keep], xb[keep]])
        area_terms += t.tolist()
        edge_terms += e.tolist()
    peak_ok = 0 <= px < W and 0 <= py < H and bool(valid(cloud[py, px]))
    mi[:] = [ys.size, len(area_terms), int(peak_ok), 0]
    mv[0:3], mv[3:6] = lo, hi
    if peak_ok:
        mv[6:9] = cloud[py, px].astype(np.float64)
    mv[9:12] = [math.fsum(s1_terms[:, a].tolist()) for a in range(3)]
    mv[12:18] = [math.fsum(s2_terms[:, a].tolist()) for a in range(6)]
    mv[18] = math.fsum(area_terms)
    return dict(m_ints=mi, m_vals=mv, s1_terms=s1_terms, s2_terms=s2_terms, area_terms=np.asarray(area_terms, dtype=np.float64),
                edge_terms=np.asarray(edge_terms, dtype=np.float64))


def measure_table(labels, count, ints, clouds, layout="planar"):
    """labels [n,H,W] int32, count [n], ints [n,K,8] as the labelling and the region table leave them, clouds [n,3,H,W] ('planar')
    or [n,H,W,3] ('interleaved') float32 -> dict(m_ints [n,K,4], m_vals [n,K,20], bad_count, slots: per image the measure_slot
    dicts of slots 0 .. min(count, K) - 1)."""
    labels, count, ints = np.asarray(labels), np.asarray(count), np.asarray(ints)
    n, K = ints.shape[0], ints.shape[1]
    hw3 = [interleaved(c, layout) for c in clouds]
    res = dict(m_ints=np.zeros((n, K, 4), np.int32), m_vals=np.zeros((n, K, 20), np.float64),
               bad_count=bad_points(np.stack(hw3)) if n else 0, slots=[])
    for i in range(n):
        slots = [measure_slot(labels[i], ints[i, j], hw3[i]) for j in range(min(max(int(count[i]), 0), K))]
        for j, s in enumerate(slots):
            res["m_ints"][i, j], res["m_vals"][i, j] = s["m_ints"], s["m_vals"]
        res["slots"].append(slots)
    return res


def sum_bounds(slot):
    """The derived bounds of one slot's sums against their fsum (tests/test_gpu_regions3d.py has the derivation):
    -> (bound of s1 [3], bound of s2 [6], bound of the area)."""
    n_pts, n_tri = int(slot["m_ints"][0]), int(slot["m_ints"][1])
    a1 = np.array([math.fsum(np.abs(slot["s1_terms"][:, a]).tolist()) for a in range(3)])
    a2 = np.array([math.fsum(np.abs(slot["s2_terms"][:, a]).tolist()) for a in range(6)])
    b_area = n_tri * 2.0 ** -53 * math.fsum(slot["area_terms"].tolist()) + 2.0 ** -49 * math.fsum(slot["edge_terms"].tolist())
    return n_pts * 2.0 ** -53 * a1 + 2.0 ** -52 * a1, n_pts * 2.0 ** -53 * a2 + 2.0 ** -52 * a2, b_area


def assert_measures_equal(got_ints, got_vals, want):
    """got: m_ints [n,K,4], m_vals [n,K,20] of the kernel; want: measure_table's dict.  The integers, lo, hi, peak_xyz and the pad
    bit for bit, the sums within sum_bounds of the yardstick's fsum."""
    got_ints, got_vals = np.asarray(got_ints), np.asarray(got_vals)
    assert got_ints.dtype == np.int32 and got_vals.dtype == np.float64
    assert got_ints.shape == want["m_ints"].shape and got_vals.shape == want["m_vals"].shape
    assert np.array_equal(got_ints, want["m_ints"]), np.argwhere(got_ints != want["m_ints"])[:5]
    exact = list(range(9)) + [19]
    same = got_vals[..., exact].view(np.uint64) == want["m_vals"][..., exact].view(np.uint64)
    assert same.all(), np.argwhere(~same)[:5]
    for i, slots in enumerate(want["slots"]):
        for j, s in enumerate(slots):
            b1, b2, ba = sum_bounds(s)
            err = np.abs(got_vals[i, j, 9:19] - s["m_vals"][9:19])
            print(f"image {i} slot {j}: n_pts {s['m_ints'][0]} n_tri {s['m_ints'][1]} |err| s1 {err[0:3]} (<= {b1}) s2 {err[3:9]} (<= {b2}) "
                  f"area {err[9]} (<= {ba})")
            assert (err[0:3] <= b1).all() and (err[3:9] <= b2).all() and err[9] <= ba, (i, j, err, b1, b2, ba)
        assert not got_vals[i, len(slots):].any() and not got_ints[i, len(slots):].any()
