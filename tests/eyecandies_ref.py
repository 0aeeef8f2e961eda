"""Test infrastructure of the Eyecandies tests (docs/eyecandies.md): an element-wise numpy restatement of the reference's
utils/preprocessing_eyecandies.py in the DOCUMENTED operation order -- float32 for the depth stage, float64 after it, every written
operation rounded once, no matrix product and no BLAS call -- the seeded synthetic scans of the golden file, and a tiny raw tree in
the layout of the Eyecandies download.  The reference itself (tests/golden/gec_eyecandies.npz) is the yardstick of the restatement;
the restatement is the yardstick of the kernels."""
import os

import numpy as np

FOCAL_LENGTH = 711.11


def inv_projection(pose, height, width, focal_length=FOCAL_LENGTH):
    """inv(K4 @ pose) by the reference's own two numpy calls (depth_to_pointcloud, :36-55)."""
    k4 = np.array([[focal_length, 0, width / 2, 0], [0, focal_length, height / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return np.linalg.inv(k4 @ np.asarray(pose, dtype=np.float64))


def depth(code, mind, maxd):
    """load_and_convert_depth: three float32 operations; the Python scalars are rounded to float32 where they meet the array."""
    d = code.astype(np.float32)
    d = d / np.float32(65535.0)
    d = d * np.float32(float(maxd) - float(mind))
    return d + np.float32(float(mind))


def unproject(d, inv_p):
    """d [H,W] float32 -> points [H*W,3] float64: h[k] = ((m[k][0] u + m[k][1] v) + m[k][2]) + m[k][3] r, point = float64(d) h."""
    h_, w_ = d.shape
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (np.float32(1) / d).astype(np.float64).reshape(-1)
        v, u = np.divmod(np.arange(h_ * w_), w_)
        u, v, dd, m = u.astype(np.float64), v.astype(np.float64), d.astype(np.float64).reshape(-1), np.asarray(inv_p, np.float64)
        cols = [dd * (((m[k, 0] * u + m[k, 1] * v) + m[k, 2]) + m[k, 3] * r) for k in range(3)]
    return np.stack(cols, 1)


def background(pts):
    """remove_point_cloud_background on [n,3] float64 -> (cloud [n,3], removed [n] bool, margin [n]): margin = the smallest distance
    of a point's rotated coordinates to one of the four thresholds."""
    n = len(pts)
    a, e = pts[256], pts[n - 256]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dz, dy = a[1] - e[1], a[2] - e[2]
        norm = np.sqrt(dz * dz + dy * dy)
        c, s = dy / norm, dz / norm
        ns = -s
        t1, t2 = pts[:, 1] - e[1], pts[:, 2] - e[2]
        p0, p1, p2 = pts[:, 0].copy(), c * t1 + ns * t2, s * t1 + c * t2
        removed = (p1 > -0.02) | (p2 > 1.8) | (p0 > 1.0) | (p0 < -1.0)
        margin = np.minimum(np.minimum(np.abs(p1 + 0.02), np.abs(p2 - 1.8)), np.minimum(np.abs(p0 - 1.0), np.abs(p0 + 1.0)))
        p0 = np.where(removed, -0.0, p0)
        p1 = np.where(removed, -e[1], p1)
        p2 = np.where(removed, -e[2], p2)
        q0, q1, q2 = p0 + 0.0, (c * p1 + s * p2) + e[1], (ns * p1 + c * p2) + e[2]
        cloud = np.stack([q0 * 0.1, q2 * -0.1, q1 * 0.1], 1)
    return cloud, removed, margin


def rules(pts):
    """The three removal rules of a cloud one by one -> (plane [n], far [n], side [n]) bool."""
    n = len(pts)
    a, e = pts[256], pts[n - 256]
    dz, dy = a[1] - e[1], a[2] - e[2]
    norm = np.sqrt(dz * dz + dy * dy)
    c, s = dy / norm, dz / norm
    t1, t2 = pts[:, 1] - e[1], pts[:, 2] - e[2]
    return c * t1 - s * t2 > -0.02, s * t1 + c * t2 > 1.8, np.abs(pts[:, 0]) > 1.0


def restate(code, mind, maxd, pose, focal_length=FOCAL_LENGTH):
    """code [H,W] uint16 -> dict(depth [H,W] f32, points [H*W,3] f64, cloud [H,W,3] f64, removed [H,W] bool, margin [H,W] f64)."""
    h_, w_ = code.shape
    d = depth(code, mind, maxd)
    pts = unproject(d, inv_projection(pose, h_, w_, focal_length))
    cloud, removed, margin = background(pts)
    return dict(depth=d, points=pts, cloud=cloud.reshape(h_, w_, 3), removed=removed.reshape(h_, w_), margin=margin.reshape(h_, w_))


# ------------------------------------------------------------------------------------------------ synthetic scans
def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def make_scan(seed, H, W, focal, wall, slope, bump, mind, maxd, tilt=(0.05, -0.03), shift=(0.02, -0.01, 0.03)):
    """A tilted wall `wall` metres from the camera (depth grows by `slope` per row) with a nearer block in the middle of the image
    (`bump` metres in front) and seeded roughness: (code [H,W] uint16, pose [4,4] float64).  The wall is the background the plane rule
    removes, the top rows lie beyond the 1.8 limit, the outer columns beyond |x| = 1, the block is kept."""
    rs = np.random.RandomState(seed)
    v, u = np.mgrid[0:H, 0:W]
    d = wall + slope * (v - H / 2) + rs.uniform(-0.004, 0.004, (H, W))
    block = (v > 0.3 * H) & (u > 0.18 * W) & (u < 0.82 * W)
    d = d - np.where(block, bump + 0.1 * bump * np.sin(u / 3.0) * np.cos(v / 4.0), 0.0)
    code = np.clip(np.rint((d - mind) / (maxd - mind) * 65535.0), 0, 65535).astype(np.uint16)
    pose = np.eye(4)
    pose[:3, :3] = _rot(*tilt)
    pose[:3, 3] = shift
    return code, pose


# three scans: every rule fires on > 5 % of the pixels, > 20 % are kept (asserted by make_golden_eyecandies.py and the tests)
SCANS = {
    "a": dict(seed=71, H=40, W=40, focal=FOCAL_LENGTH, wall=60.0, slope=0.05, bump=6.0, mind=40.0, maxd=70.0, tilt=(0.01, -0.004)),
    "b": dict(seed=72, H=32, W=40, focal=22.0, wall=2.0, slope=0.004, bump=0.3, mind=0.5, maxd=3.1),
    "c": dict(seed=73, H=36, W=24, focal=22.0, wall=2.4, slope=-0.003, bump=0.5, mind=1.0, maxd=3.2),
}


def scan(tag):
    """-> (code, mind, maxd, pose, focal_length) of one of the three golden scans."""
    kw = SCANS[tag]
    code, pose = make_scan(**kw)
    return code, kw["mind"], kw["maxd"], pose, kw["focal"]


def synthetic_scan(seed, H, W, mind=0.5, maxd=3.1):
    """The scene of scan "b" at any size, with the focal length that gives this size the same field of view ->
    (code [H,W] uint16, pose, focal_length)."""
    focal = 22.0 * max(H, W) / 40.0
    code, pose = make_scan(seed, H, W, focal, 2.0, 0.128 / H, 0.3, mind, maxd)
    return code, pose, focal


# ------------------------------------------------------------------------------------------------ a raw tree
def write_raw_tree(root, class_name="CandyCane", n_train=2, n_test=3, bad=(1,), H=40, W=48, rgb_size=64, seed=300):
    """<root>/<class>/{train/data/{i:03d}_*, test_public/data/{i:02d}_*}: depth.png (16 bit), info_depth.yaml, pose.txt, image_4.png and,
    for the test samples, mask.png (non-zero for the indices in `bad`).  Returns {('train'|'test', i): dict(code, mind, maxd, pose, rgb,
    mask or None, rgb_path)}."""
    from PIL import Image
    items = {}
    for split, sub, n, fmt in (("train", "train/data", n_train, "{:03d}"), ("test", "test_public/data", n_test, "{:02d}")):
        base = os.path.join(root, class_name, sub)
        os.makedirs(base, exist_ok=True)
        for i in range(n):
            mind, maxd = 40.0 + 0.01 * i, 70.0 + 0.02 * i
            # the scene of scan "a": far enough from the camera for the true focal length to reach |x| > 1 at this size
            code, pose = make_scan(seed, H, W, FOCAL_LENGTH, 60.0, 0.05, 6.0, mind, maxd, tilt=(0.01, -0.004), shift=(0.02 * (i + 1), -0.01, 0.03))
            rs = np.random.RandomState(seed)
            seed += 1
            rgb = rs.randint(0, 256, (rgb_size, rgb_size, 3)).astype(np.uint8)
            stem = os.path.join(base, fmt.format(i))
            Image.fromarray(code).save(stem + "_depth.png")
            with open(stem + "_info_depth.yaml", "w") as fh:
                fh.write(f"image: {fmt.format(i)}_depth.png\nnormalization:\n  max: {maxd!r}\n  min: {mind!r}\n")
            np.savetxt(stem + "_pose.txt", pose)
            Image.fromarray(rgb).save(stem + "_image_4.png")
            mask = None
            if split == "test":
                mask = np.zeros((rgb_size, rgb_size, 3), np.uint8)
                if i in bad:
                    mask[10:30 + i, 20:50] = 255
                    mask[30 + i:34 + i, 20:50] = 127 + (np.arange(30) % 2).astype(np.uint8)[None, :, None]      # on the > 0.5 boundary
                Image.fromarray(mask).save(stem + "_mask.png")
            items[(split, i)] = dict(code=code, mind=mind, maxd=maxd, pose=pose, rgb=rgb, mask=mask, rgb_path=stem + "_image_4.png")
    return items
