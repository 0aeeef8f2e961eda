"""Helper of the preprocessing tests (not a test): the numpy float64 restatement of the two device stages' contract
(docs/preprocessing.md), the reference's glue restated on top of it, and the synthetic scan generator.

  plane:   the same counter-based hash and draw rule as cmdiad_plane_ransac, numpy.linalg.eigh (or svd) for the fit
  dbscan:  cKDTree + connected_components: core = at least min_points neighbours counting itself, clusters = components of the core
           graph numbered by their lowest core index, a border point takes the lowest cluster number among its core neighbours
           (what sklearn.cluster.DBSCAN returns: tests/test_preprocess_cpu.py compares the two on every scene)
"""
import os
import sys
import types

import numpy as np

M32 = 0xFFFFFFFF
MAX_DRAWS = 65536


# ------------------------------------------------------------------------------------------------------------------- plane
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample_indices(seed, h, E, n=50):
    """The n distinct point indices of hypothesis h: draw c is mix32(mix32(seed + 0x9E3779B9 (h + 1)) + c) mod E, a repeated index
    is skipped.  None when MAX_DRAWS draws do not give n distinct ones (such a hypothesis does not compete)."""
    base = mix32((seed & M32) + 0x9E3779B9 * (h + 1))
    out, seen = [], set()
    for c in range(MAX_DRAWS):
        i = mix32(base + c) % E
        if i not in seen:
            seen.add(i)
            out.append(i)
            if len(out) == n:
                return np.array(out, dtype=np.int64)
    return None


def _orient(nrm, cen):
    nrm = nrm / np.sqrt((nrm * nrm).sum())
    if nrm[2] < 0:
        nrm = -nrm
    return np.array([nrm[0], nrm[1], nrm[2], -((nrm[0] * cen[0] + nrm[1] * cen[1]) + nrm[2] * cen[2])])


def fit_plane(P):
    """Least-squares plane of float64 points [m,3]: eigenvector of the smallest eigenvalue of the centred scatter matrix."""
    cen = P.mean(0)
    X = P - cen
    w, V = np.linalg.eigh(X.T @ X)
    return _orient(V[:, 0], cen)


def fit_plane_svd(P):
    """The same plane through the SVD of the centred points (another order of the same float64 arithmetic: the yardstick for the
    coefficient tolerance of the GPU test)."""
    cen = P.mean(0)
    _, _, Vt = np.linalg.svd(P - cen, full_matrices=False)
    return _orient(Vt[-1], cen)


def plane_distance(plane, P):
    a, b, c, d = (float(v) for v in plane)
    P = np.asarray(P)
    x, y, z = P[..., 0].astype(np.float64), P[..., 1].astype(np.float64), P[..., 2].astype(np.float64)
    return np.abs(((a * x + b * y) + c * z) + d)


def plane_ransac(points, n=50, iterations=1000, threshold=0.004, seed=0, fit=fit_plane):
    """-> (plane [4] f64 refitted over the winner's inliers, inliers, winning h, counts [iterations])."""
    pts = np.asarray(points, dtype=np.float32)
    E = len(pts)
    if E < n:
        raise ValueError(f"{E} points, {n} needed for one sample")
    P = pts.astype(np.float64)
    counts = np.zeros(iterations, dtype=np.int64)
    planes = np.zeros((iterations, 4))
    for h in range(iterations):
        idx = sample_indices(seed, h, E, n)
        if idx is None:
            counts[h] = -1
            continue
        planes[h] = fit(P[idx])
        counts[h] = int((plane_distance(planes[h], pts) < threshold).sum())
    h = int(np.argmax(counts))          # first maximum = lowest h
    inl = plane_distance(planes[h], pts) < threshold
    plane = fit(P[inl]) if inl.sum() >= 3 else planes[h]
    return plane, int(counts[h]), h, counts


# ------------------------------------------------------------------------------------------------------------------ DBSCAN
def dbscan(points, eps=0.006, min_points=30, details=False):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    P = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = len(P)
    if n == 0:
        return (np.zeros(0, np.int32), {}) if details else np.zeros(0, np.int32)
    pairs = cKDTree(P).query_pairs(eps, output_type="ndarray")
    deg = np.bincount(pairs.ravel(), minlength=n) + 1
    core = deg >= min_points
    cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]]
    _, comp = connected_components(coo_matrix((np.ones(len(cc)), (cc[:, 0], cc[:, 1])), shape=(n, n)), directed=False)
    first = np.full(comp.max() + 1, n)
    np.minimum.at(first, comp[core], np.nonzero(core)[0])
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    lab = np.full(n, -1, dtype=np.int64)
    lab[core] = rank[comp[core]]
    big = 1 << 30
    best = np.full(n, big)
    worst = np.full(n, -1)
    for a, b in ((0, 1), (1, 0)):
        m = core[pairs[:, a]] & ~core[pairs[:, b]]
        np.minimum.at(best, pairs[m, b], lab[pairs[m, a]])
        np.maximum.at(worst, pairs[m, b], lab[pairs[m, a]])
    border = (~core) & (best < big)
    lab[border] = best[border]
    lab = lab.astype(np.int32)
    if details:
        return lab, dict(core=core, border=border, two_cluster_border=int((border & (worst > best)).sum()), degree=deg)
    return lab


def boundary_pairs(points, eps, rel=1e-12):
    """Number of pairs whose squared distance lies within rel * eps^2 of eps^2 (the label comparison is only defined without)."""
    from scipy.spatial import cKDTree
    P = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    if len(P) < 2:
        return 0
    t = cKDTree(P)
    return int(t.count_neighbors(t, eps * (1 + rel)) - t.count_neighbors(t, eps * (1 - rel)))


# -------------------------------------------------------------------------------------------------- the reference's glue
def get_edges(pc):
    e = np.concatenate([pc[0:10].reshape(-1, pc.shape[2]), pc[-10:].reshape(-1, pc.shape[2]), pc[:, 0:10].reshape(-1, pc.shape[2]),
                        pc[:, -10:].reshape(-1, pc.shape[2])], axis=0)
    return e[np.all(e != 0, axis=1)]


def pad_square(a):
    h, w = a.shape[:2]
    side = max(-(-h // 100) * 100, -(-w // 100) * 100)
    t, l = (side - h) // 2, (side - w) // 2
    width = ((t, side - t - h), (l, side - l - w)) + ((0, 0),) * (a.ndim - 2)
    return np.pad(a, width, mode="constant")


def remove_plane(pc, rgb, plane, threshold=0.005):
    near = plane_distance(plane, pc) < threshold
    pc, rgb = pc.copy(), rgb.copy()
    pc[near] = 0
    rgb[near] = 0
    return pc, rgb


def keep_largest(pc, rgb, labels_of=dbscan):
    flat = pc.reshape(-1, 3)
    nz = np.nonzero(np.all(flat != 0, axis=1))[0]
    pc, rgb = pc.copy(), rgb.copy()
    if len(nz) == 0:
        return pc, rgb
    labels = labels_of(flat[nz])
    ids, sizes = np.unique(labels, return_counts=True)
    out = nz[labels != ids[np.argmax(sizes)]]
    pc.reshape(-1, 3)[out] = 0
    rgb.reshape(-1, rgb.shape[2])[out] = 0
    return pc, rgb


def preprocess(pc, rgb, gt=None, seed=0, labels_of=dbscan):
    plane = plane_ransac(get_edges(pc), seed=seed)[0]
    pc, rgb = remove_plane(pc, rgb, plane)
    pc, rgb = keep_largest(pad_square(pc), pad_square(rgb), labels_of)
    return pc, rgb, (pad_square(gt) if gt is not None else None)


# -------------------------------------------------------------------------------------------------------------- generator
PLANE_TILT = (0.05, -0.03, 0.5)     # z = 0.5 + 0.05 x - 0.03 y


def planted_plane():
    tx, ty, z0 = PLANE_TILT
    nrm = np.array([-tx, -ty, 1.0])
    s = np.sqrt((nrm * nrm).sum())
    return np.array([nrm[0] / s, nrm[1] / s, nrm[2] / s, -z0 / s])


def make_scan(seed, H=220, W=220, pitch=6e-4, eps=0.006, specks=0.003, holes=0.01):
    """A synthetic organized scan [H,W,3] f32 + rgb [H,W,3] u8 + gt [H,W] u8 and what was planted.  A tilted background plane with
    bounded noise (sigma 2.5 mm, |offset| <= 4.5 mm along the normal: RANSAC hypotheses differ in their inlier counts; raised
    points: |offset| <= 0.8 mm), an object (a pedestal 12 mm above the plane with a bump on it), satellites
    of fixture residue (one next to the object's rim, a one-pixel bridge leading to it), isolated specks, two patches 1.5 eps apart
    with a few lifted points in the gap (border points adjacent to both clusters), and invalid pixels (exact zeros).  The outer 10
    rows and columns are background."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    x = (xs - W / 2) * pitch + rng.normal(0, 0.03 * pitch, xs.shape)
    y = (ys - H / 2) * pitch + rng.normal(0, 0.03 * pitch, xs.shape)
    tx, ty, z0 = PLANE_TILT
    pl = planted_plane()
    offset = np.clip(rng.normal(0, 2.5e-3, xs.shape), -4.5e-3, 4.5e-3)
    fine = np.clip(rng.normal(0, 2e-4, xs.shape), -8e-4, 8e-4)
    height = np.zeros(xs.shape)
    cy, cx, R = H * 0.55, W * 0.5, 0.28 * min(H, W)
    r2 = (xs - cx) ** 2 + (ys - cy) ** 2
    obj = r2 < R * R
    height[obj] = 0.012 + 0.02 * np.exp(-r2[obj] / (2 * (0.5 * R) ** 2))
    raised = obj.copy()
    g = max(2, int(round(eps / pitch)))                     # eps in pixels
    sats = [(int(cy), int(cx + R + g * 0.9 + 6), 6), (int(H * 0.15), int(W * 0.8), 7), (int(H * 0.9) - 12, int(W * 0.15), 5)]
    for sy, sx, sr in sats:
        m = ((xs - sx) ** 2 + (ys - sy) ** 2 < sr * sr) & (xs >= 12) & (xs < W - 12) & (ys >= 12) & (ys < H - 12)
        height[m] = 0.010
        raised |= m
    bridge = (ys == int(cy)) & (xs >= int(cx + R) - 1) & (xs <= sats[0][1] - sats[0][2] + 1)
    height[bridge] = 0.011
    raised |= bridge
    # twin patches, 1.5 eps apart, lifted sparse points in the middle of the gap
    gap = int(round(1.5 * eps / pitch))
    py, px, ph, pw = 14, 14, max(12, 2 * g), max(12, 2 * g)
    twin = np.zeros(xs.shape, bool)
    twin[py:py + ph, px:px + pw] = True
    twin[py:py + ph, px + pw + gap:px + 2 * pw + gap] = True
    height[twin] = 0.010
    mid = np.zeros(xs.shape, bool)
    mid[py + 2:py + ph - 2:4, px + pw + gap // 2] = True
    height[mid] = 0.010 + 0.5 * eps
    raised |= twin | mid
    sp = (rng.random(xs.shape) < specks) & ~raised & (xs >= 12) & (xs < W - 12) & (ys >= 12) & (ys < H - 12)
    height[sp] = rng.uniform(0.010, 0.030, int(sp.sum()))
    raised |= sp
    z = z0 + tx * x + ty * y + (np.where(raised, fine, offset) + height) / pl[2]
    pc = np.stack([x, y, z], -1).astype(np.float32)
    hole = rng.random(xs.shape) < holes
    pc[hole] = 0
    pc[np.any(pc == 0, axis=2)] = 0
    rgb = rng.integers(1, 255, (H, W, 3), dtype=np.uint8)
    gt = (obj & (rng.random(xs.shape) < 0.02)).astype(np.uint8) * 255
    valid = np.all(pc != 0, axis=2)
    return dict(pc=pc, rgb=rgb, gt=gt, plane=pl, offset=plane_distance(pl, pc) * valid, raised=raised & valid,
                background=~raised & valid, obj=obj & valid, valid=valid)


def raised_points(scan):
    return np.ascontiguousarray(scan["pc"][scan["raised"]])


def _blob(rng, n, center, size, pitch):
    side = int(np.ceil(np.sqrt(n)))
    ys, xs = np.mgrid[0:side, 0:side]
    p = np.stack([xs.ravel() * pitch, ys.ravel() * pitch, np.zeros(side * side)], -1)[:n]
    return (p + rng.normal(0, 0.03 * pitch, p.shape) + np.asarray(center)).astype(np.float32)


def dbscan_scenes(eps=0.006):
    """name -> points [N,3] f32 (the committed seeds)."""
    out = {}
    out["scan_a"] = raised_points(make_scan(11, eps=eps))
    out["scan_b"] = raised_points(make_scan(12, H=260, W=240, pitch=5e-4, eps=eps))
    rng = np.random.default_rng(21)
    noise = rng.uniform(-0.4, 0.4, (9000, 3)).astype(np.float32)
    out["noise_majority"] = np.concatenate([noise[:4000], _blob(rng, 3000, (0.0, 0.0, 1.0), 0, 5e-4), noise[4000:]])
    out["single"] = _blob(np.random.default_rng(22), 12000, (0.1, -0.2, 0.6), 0, 6e-4)
    out["few"] = _blob(np.random.default_rng(23), 20, (0, 0, 0.5), 0, 6e-4)
    out["empty"] = np.zeros((0, 3), np.float32)
    rng = np.random.default_rng(24)
    b = _blob(rng, 10000, (0.0, 0.0, 0.5), 0, 6e-4)
    pile = np.repeat(np.array([[0.3, 0.3, 0.5]], np.float32), 40, axis=0)        # 40 identical points: a cluster of its own
    lone = np.repeat(np.array([[-0.3, 0.3, 0.5]], np.float32), 7, axis=0)        # 7 identical points: noise
    out["duplicates"] = np.concatenate([pile[:20], b, b[rng.integers(0, len(b), 300)], lone, pile[20:]])
    return out


def full_size_scene(seed=31, H=800, W=800, pitch=2e-4, eps=0.006):
    """800 x 800 points at 0.2 mm pitch whose DBSCAN partition is known by construction: discs (every point has far more than
    min_points neighbours, so all are core) more than eps apart from each other, and lone points on a lattice coarser than eps
    (noise).  -> (points [N,3] f32 in row-major pixel order, planted component per point with -1 for the lone points)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    comp = np.full(xs.shape, -2)
    discs = [(400, 400, 300), (50, 60, 30), (60, 730, 35), (745, 70, 28), (750, 740, 32)]
    for k, (dy, dx, r) in enumerate(discs):
        comp[(xs - dx) ** 2 + (ys - dy) ** 2 < r * r] = k
    margin = int(np.ceil(2 * eps / pitch))
    near = np.zeros(xs.shape, bool)
    for dy, dx, r in discs:
        near |= (xs - dx) ** 2 + (ys - dy) ** 2 < (r + margin) ** 2
    lone = (ys % (2 * margin) == 3) & (xs % (2 * margin) == 5) & ~near
    comp[lone] = -1
    keep = comp > -2
    x = (xs - W / 2) * pitch + rng.normal(0, 0.03 * pitch, xs.shape)
    y = (ys - H / 2) * pitch + rng.normal(0, 0.03 * pitch, xs.shape)
    z = 0.5 + 0.01 * np.cos(xs / 90.0) + rng.normal(0, 0.03 * pitch, xs.shape)
    pts = np.stack([x, y, z], -1).astype(np.float32)[keep]
    planted = comp[keep]
    # number the components by their lowest point index, as the contract does
    ids = [k for k in np.unique(planted) if k >= 0]
    firsts = sorted((int(np.nonzero(planted == k)[0][0]), k) for k in ids)
    remap = {k: i for i, (_, k) in enumerate(firsts)}
    want = np.array([remap.get(int(k), -1) for k in range(-1, len(discs))])[planted + 1]
    return pts, want.astype(np.int32)


# ------------------------------------------------------------------------------------------------ a raw MVTec 3D-AD class directory
def scene_key(kw):
    return tuple(sorted(kw.items()))


RAW_TREE = [("train/good", [dict(seed=7, H=120, W=120), dict(seed=61, H=120, W=120), dict(seed=52, H=150, W=260)], False),
            ("test/good", [dict(seed=62, H=120, W=120), dict(seed=63, H=120, W=120)], False),
            ("test/hole", [dict(seed=64, H=120, W=120), dict(seed=65, H=130, W=110)], True)]


def fake_tifffile(monkeypatch):
    """`tifffile` stand-in that reads and writes np.save content under the .tiff name (float32 arrays either way: lossless)."""
    fake = types.ModuleType("tifffile")

    def imread(path):
        with open(path, "rb") as fh:
            return np.load(fh)

    def imwrite(path, a):
        with open(path, "wb") as fh:
            np.save(fh, a)
    fake.imread, fake.imwrite = imread, imwrite
    monkeypatch.setitem(sys.modules, "tifffile", fake)
    return fake


def write_raw_tree(root, fake):
    """<root>/bagel/{train/good x 3, test/good x 2, test/hole x 2 with gt} from make_scan, one scan 150 x 260 -> [(stem, scene key)]."""
    from PIL import Image
    items = []
    for sub, scenes, has_gt in RAW_TREE:
        base = os.path.join(root, "bagel", sub)
        for d in ("rgb", "xyz") + (("gt",) if has_gt else ()):
            os.makedirs(os.path.join(base, d))
        for i, kw in enumerate(scenes):
            scan = make_scan(**kw)
            fake.imwrite(os.path.join(base, "xyz", f"{i:03d}.tiff"), scan["pc"])
            Image.fromarray(scan["rgb"]).save(os.path.join(base, "rgb", f"{i:03d}.png"))
            if has_gt:
                Image.fromarray(scan["gt"], "L").save(os.path.join(base, "gt", f"{i:03d}.png"))
            items.append((f"{sub}/{i:03d}", scene_key(kw), has_gt))
    return items
