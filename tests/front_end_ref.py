"""Numpy restatements and hand-built inputs for the kernels at the two ends of an inference step: unorganize_kernel
(csrc/interp_pool.hip), ball_query_kernel and gather_points_kernel (csrc/ballquery.hip), ocsvm_score_maps_kernel and
blur8_maps_kernel (csrc/post.hip).  Shared by tests/test_gpu_front_end_edges.py and pinned by tests/test_front_end_ref_cpu.py.
No GPU, no cmdiad_amd import.

Nothing here needs a tolerance.  unorganize and the gathers move bits.  The ball-query scenes sit on a lattice of multiples of 2^-6
with |coordinate| <= 4, so every difference, square and sum of three squares is exact in fp32 and `<` against radius^2 = 25 * 2^-12
is decided by integers.  The score maps follow the kernel's formula operation by operation (csrc/post.hip is built without
contraction).  The blur is integer arithmetic between two correctly rounded float steps."""
import collections
import fractions

import numpy as np

SENT32 = 0x4B3C5A69                   # the sentinel of tests/gemm_ref.py: finite as a float, no index, no count, in no reference here
SENT64 = 0x4B3C5A694B3C5A69
CHUNK = 1024                          # pixels per step of unorganize_kernel
AHEAD = 7                             # chunks it fetches ahead (one look-ahead group = 7 168 pixels)


# ================================================================================================ unorganize
def unorganize(pc, n_max):
    """pc [3, H, W] f32 -> (xyz [n, 3] f32, nz [n] i32, pix2pt [HW] i32, n): the pixels whose three coordinates are all != 0, in
    raster order, the first n_max of them; pix2pt = position of a kept pixel, -1 for every other one (cut off by n_max included)."""
    pc = np.asarray(pc)
    assert pc.dtype == np.float32 and pc.ndim == 3 and pc.shape[0] == 3
    p = pc.reshape(3, -1).T
    keep = np.nonzero(np.all(p != 0, axis=1))[0][:n_max]
    n = len(keep)
    pix2pt = np.full(p.shape[0], -1, np.int32)
    pix2pt[keep] = np.arange(n, dtype=np.int32)
    return np.ascontiguousarray(p[keep]), keep.astype(np.int32), pix2pt, n


FRAMES = [(1, 1), (30, 30), (32, 32), (25, 41), (64, 112), (67, 107), (64, 128), (96, 96), (100, 37), (224, 224)]


def frame_batch(H, W):
    """[3, 3, H, W] f32: a random frame with about 60 % valid pixels in irregular runs (a background pixel is zero in one, two or
    all three coordinates), an all-background frame, an all-valid frame.  No value is a zero by accident: |v| in [0.25, 4)."""
    HW = H * W
    rs = np.random.RandomState(1000 * H + W)
    val = (rs.uniform(0.25, 4.0, (3, 3, HW)) * rs.choice([-1.0, 1.0], (3, 3, HW))).astype(np.float32)
    valid = np.zeros(HW, bool)
    i, on = 0, True
    while i < HW:                                            # runs of 1 .. 40 valid and 1 .. 26 background pixels, alternating
        run = int(rs.randint(1, 41)) if on else int(rs.randint(1, 27))
        valid[i:i + run] = on
        i, on = i + run, not on
    zero = rs.randint(1, 8, HW)                              # bit c set: coordinate c of a background pixel is zero
    for c in range(3):
        val[0, c, ~valid & ((zero >> c) & 1 == 1)] = 0.0
    val[1] = 0.0
    return val.reshape(3, 3, H, W)


def chunk_cuts(pc):
    """Nmax values that cut the kept pixels of pc [3, H, W] exactly at a 1 024-pixel chunk boundary (the last kept pixel of a chunk
    is the last one stored) and five pixels into the following chunk's kept ones; empty for a frame of one chunk."""
    keep = unorganize(pc, pc[0].size)[1]
    cuts = []
    for c in range(1, (pc[0].size + CHUNK - 1) // CHUNK):
        at = int(np.count_nonzero(keep < c * CHUNK))
        inside = int(np.count_nonzero(keep < c * CHUNK + CHUNK))
        if 0 < at < len(keep) and at + 5 < inside:
            cuts.append((at, at + 5))
    return cuts


EDGE_H, EDGE_W = 32, 40               # 1 280 pixels: one full chunk and a partial one, planted pixels in both
# name -> (pixel, coordinate, value bits, kept by the reference's all(pc != 0))
EDGE_PLANTED = collections.OrderedDict([
    ("x_zero", (3, 0, 0x00000000, False)),
    ("y_zero", (517, 1, 0x00000000, False)),
    ("z_zero", (1023, 2, 0x00000000, False)),
    ("neg_zero", (1024, 1, 0x80000000, False)),
    ("nan", (700, 2, 0x7FC00000, True)),
    ("inf", (1100, 0, 0x7F800000, True)),
    ("denormal", (64, 1, 0x00000001, True)),                 # the smallest fp32 denormal: not zero
])


def edge_frame():
    """[3, 32, 40] f32, every pixel valid except the planted ones of EDGE_PLANTED (each changes ONE coordinate of one pixel)."""
    rs = np.random.RandomState(77)
    pc = (rs.uniform(0.25, 4.0, (3, EDGE_H * EDGE_W)) * rs.choice([-1.0, 1.0], (3, EDGE_H * EDGE_W))).astype(np.float32)
    bits = pc.view(np.uint32)
    for pixel, coord, pattern, _ in EDGE_PLANTED.values():
        bits[coord, pixel] = pattern
    return pc.reshape(3, EDGE_H, EDGE_W)


# ================================================================================================ ball query
STEP = 2.0 ** -6                      # the lattice
RADIUS = 5 * STEP                     # radius^2 = 25 lattice units: (3, 4, 0) and (5, 0, 0) lie ON the sphere, (4, 0, 0) one step inside
R2_UNITS = 25
NSAMPLES = [1, 8, 64, 65, 130]
# query offsets in lattice units: all inside the cube {-1, 0, 1}^3, so a garbage row (below) is within the radius of every query
QUERIES = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (-1, -1, 1), (1, -1, -1)]
# points around the sphere of query 0, in lattice units: squared distances 0, 16, 16, 16, 16, 16, 25, 25, 22, 24, 25, 24, 36, 9
SHELL = [(0, 0, 0), (4, 0, 0), (-4, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 4), (3, 4, 0), (5, 0, 0), (3, 3, 2), (4, 2, 2), (4, 3, 0),
         (2, 2, 4), (6, 0, 0), (-2, 2, 1)]

Scene = collections.namedtuple("Scene", "name xyz query n_valid")   # xyz [B, N, 3] f32, query [B, M, 3] f32, n_valid [B] i32


def _far(k):
    """a point far outside every query's radius, another one for every row k"""
    return (128 + k % 32, 128 + k // 32, -128)


def _garbage(k):
    """what the rows behind n_valid hold: a point within the radius of EVERY query (squared distance <= 9 units)"""
    return (k % 3 - 1, (k // 3) % 3 - 1, 0)


def _cloud(N, n_valid, hits):
    """[N, 3] lattice units: rows < n_valid are far points except where `hits` (row -> point) says otherwise; rows behind are garbage"""
    pts = np.array([_far(k) if k < n_valid else _garbage(k) for k in range(N)], np.int64).reshape(N, 3)
    for k, p in hits.items():
        assert 0 <= k < n_valid, (k, n_valid)
        pts[k] = p
    return pts


def _shell(rows, skip=0):
    """row -> a SHELL point, cycling; every `skip`-th row (skip > 0) stays far"""
    return {k: SHELL[k % len(SHELL)] for k in rows if not (skip and k % skip == 0)}


def _core(rows):
    """row -> a point that every query hits (a garbage-like point, but in the valid part)"""
    return {k: _garbage(k) for k in rows}


def _scene(name, M, clouds):
    N = clouds[0][0]
    assert all(c[0] == N for c in clouds)
    units = np.stack([_cloud(*c) for c in clouds])
    q = np.array(QUERIES[:M], np.int64)
    query = np.broadcast_to(q, (len(clouds), M, 3))
    return Scene(name, (units * STEP).astype(np.float32), np.ascontiguousarray((query * STEP).astype(np.float32)),
                 np.array([c[1] for c in clouds], np.int32))


def scenes():
    """Every N of 1, 63, 64, 65, 128, 129, 300, every M of 1, 3, 4, 5, 9 (M = 1, 3, 5, 9 leave the last block of four queries
    ragged), B <= 3, n_valid < N on at least one cloud of every scene.  (N, n_valid, {row: point})."""
    return [
        _scene("n1", 1, [(1, 1, {0: (4, 0, 0)}), (1, 0, {})]),                         # one point, one step inside; an EMPTY cloud
        _scene("n63", 3, [(63, 63, _shell(range(63))), (63, 40, _shell(range(40), skip=4)), (63, 10, {})]),   # cloud 2: no hit at all
        _scene("n64", 4, [(64, 64, _core(range(64))), (64, 63, {62: (0, 0, 0)})]),      # 64 hits in the only step; one hit, last valid row
        _scene("n65", 5, [(65, 65, {64: (1, 0, 0)}), (65, 64, {62: (0, 0, 0), 63: (4, 0, 0)})]),   # the first hit IS row 64
        _scene("n128", 9, [(128, 128, _shell(range(60, 71))), (128, 100, _shell(range(100))), (128, 127, {126: (0, 1, 0)})]),
        _scene("n129", 5, [(129, 129, _core(range(64, 129))), (129, 128, {127: (0, 0, 0)})]),   # 64 hits in step 1, one in step 2
        _scene("n300", 9, [(300, 300, _shell(range(300), skip=5)),
                           (300, 257, _core([63, 64, 127, 128, 191, 192, 255, 256])),
                           (300, 200, _core(range(192, 200)))]),
    ]


def ball_query(radius, nsample, xyz, query):
    """xyz [n, 3], query [M, 3] f32 -> idx [M, nsample] i32.  fp32 with one rounding per operation:
    ((dx*dx + dy*dy) + dz*dz) < float32(radius) * float32(radius); the first nsample hits in index order, the first hit pre-fills
    every slot, no hit leaves zeros."""
    xyz, query = np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(query, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    d = query[:, None, :] - xyz[None, :, :]
    sq = d * d
    d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    assert d2.dtype == np.float32 and r2.dtype == np.float32
    return _select(d2 < r2, nsample)


def _select(hit, nsample):
    out = np.zeros((hit.shape[0], nsample), np.int32)
    for j in range(hit.shape[0]):
        h = np.nonzero(hit[j])[0]
        if len(h):
            out[j, :] = h[0]
            out[j, :min(len(h), nsample)] = h[:nsample]
    return out


def scene_units(scene):
    """(cloud [B, N, 3], query [B, M, 3]) of a scene as int64 lattice units; asserts that the floats ARE on the lattice"""
    pts, q = scene.xyz.astype(np.float64) / STEP, scene.query.astype(np.float64) / STEP
    assert (pts == np.round(pts)).all() and (q == np.round(q)).all() and np.abs(pts).max() <= 4 / STEP
    return pts.astype(np.int64), q.astype(np.int64)


def hits_units(scene, b, valid_only=True, inclusive=False):
    """hit matrix [M, n] of cloud b decided in integers: d2 < 25 (inclusive: <= 25, the rule of a kernel written with <=)"""
    pts, q = scene_units(scene)
    n = int(scene.n_valid[b]) if valid_only else pts.shape[1]
    d2 = ((q[b][:, None, :] - pts[b][None, :n, :]) ** 2).sum(-1)
    return (d2 <= R2_UNITS) if inclusive else (d2 < R2_UNITS), d2


def ball_query_units(scene, b, nsample, **kw):
    return _select(hits_units(scene, b, **kw)[0], nsample)


def scene_conditions(scene, nsample):
    """names of the situations that (scene, nsample) holds for at least one query"""
    found = set()
    for b in range(len(scene.n_valid)):
        hit, d2 = hits_units(scene, b)
        n, N = hit.shape[1], scene.xyz.shape[1]
        if (d2 == R2_UNITS).any():
            found.add("on_radius")
        pts, q = scene_units(scene)
        disp = np.sort(np.abs(q[b][:, None, :] - pts[b][None, :n, :]), axis=-1)
        if (disp == (0, 0, 4)).all(-1).any():                 # (5, 0, 0) from the query is on the sphere: this point is one step inside
            assert hit[(disp == (0, 0, 4)).all(-1)].all()
            found.add("one_step_inside")
        if n < N:
            found.add("ragged")
        for j in range(hit.shape[0]):
            h = np.nonzero(hit[j])[0]
            if len(h) == 0:
                found.add("no_hit")
                if n < N:
                    found.add("no_hit_before_garbage")
                continue
            if h[0] >= 64:
                found.add("first_hit_late")
            if len(h) < nsample:
                found.add("prefill_survives")
                if nsample > 64:
                    found.add("prefill_survives_past_slot_64")
            placed = h[:nsample]
            if any(k % 64 == 63 and k + 1 in placed for k in placed):
                found.add("straddle")
            cnt = 0
            for s in range(0, n, 64):
                if cnt >= nsample:
                    break
                here = int(np.count_nonzero((h >= s) & (h < s + 64)))
                if here > nsample - cnt:
                    found.add("clip")
                    if cnt > 0:
                        found.add("clip_after_earlier_hits")
                cnt += here
    return found


# ================================================================================================ gather
GATHER_CASES = [(J, C, ms) for C in (1, 5) for J, ms in ((1, (1, 1)), (255, (3, 85)), (256, (4, 64)), (257, (1, 257)))]   # ms: J = M * ns
GATHER_B, GATHER_N = 2, 129


def gather_case(J, C):
    """(feat [B, C, N] f32, idx [B, J] i32): indices over the whole range, 0 and N - 1 among them in every row (J = 1: N - 1 in
    image 0, 0 in image 1)"""
    rs = np.random.RandomState(31 * J + C)
    feat = rs.standard_normal((GATHER_B, C, GATHER_N)).astype(np.float32)
    idx = rs.randint(0, GATHER_N, (GATHER_B, J)).astype(np.int32)
    if J == 1:
        idx[0, 0], idx[1, 0] = GATHER_N - 1, 0
    else:
        idx[:, 0], idx[:, -1] = GATHER_N - 1, 0
    return feat, idx


def gather(feat, idx):
    """out[b, c, ...] = feat[b, c, idx[b, ...]]"""
    return np.stack([feat[b][:, idx[b]] for b in range(feat.shape[0])])


# ================================================================================================ one-class SVM score maps
def ocsvm_scores(maps, lam, coef, offset):
    """maps [B, K, HW] f32 -> [B, HW] f64, the kernel's formula: s = 0; for k in order s = s + float64(float32(lam_k) * maps[:, k]) *
    coef_k; result (s - offset) + offset.  One rounding per operation."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3
    coef, offset = np.asarray(coef, np.float64).reshape(-1), np.float64(np.asarray(offset).reshape(-1)[0])
    s = np.zeros((maps.shape[0], maps.shape[2]), np.float64)
    for k in range(maps.shape[1]):
        v = np.float32(lam[k]) * maps[:, k]
        assert v.dtype == np.float32
        s = s + v.astype(np.float64) * coef[k]
    return (s - offset) + offset


def ocsvm_scores_fma(maps, lam, coef, offset):
    """what a kernel gives that contracts s + v * coef_k into one fused multiply-add (exact product, ONE rounding); in rationals"""
    maps = np.asarray(maps)
    out = np.empty((maps.shape[0], maps.shape[2]), np.float64)
    for b in range(maps.shape[0]):
        for i in range(maps.shape[2]):
            s = 0.0
            for k in range(maps.shape[1]):
                v = float(np.float32(lam[k]) * maps[b, k, i])
                s = float(fractions.Fraction(s) + fractions.Fraction(v) * fractions.Fraction(float(coef[k])))
            out[b, i] = (s - float(offset)) + float(offset)
    return out


OCSVM_LAM = (1.0, 0.1, 3.7, 0.013)
OCSVM_COEF = (0.83, -12.57, 3.1e-3, -417.3)          # none a short binary fraction: every product float64(v) * coef_k needs rounding
OCSVM_CASES = [(B, K, HW) for K in (1, 2, 3, 4) for HW in (1, 255, 256, 257, 900) for B in (1, 3)]


def ocsvm_case(B, K, HW):
    """(maps, lam, coef, (offset, small offset)): coefficients of mixed sign and magnitude; the offset about 1e3 times the typical
    sum and of either sign, so that (s - offset) + offset rounds away ten bits of s -- and with them, almost always, the last-bit
    difference a fused multiply-add makes; the small offset (about 1e-3 times the sum) keeps every bit of s in play."""
    rs = np.random.RandomState(97 * K + HW + B)
    maps = (rs.uniform(0.0, 1.0, (B, K, HW)) * np.array([2.0, 20.0, 0.5, 1.0])[:K].reshape(1, K, 1)).astype(np.float32)
    lam, coef = OCSVM_LAM[:K], np.array(OCSVM_COEF[:K], np.float64)
    typical = float(np.abs(ocsvm_scores(maps, lam, coef, 0.0)).mean()) * 1.0371
    sign = -1.0 if (K + HW) % 2 else 1.0
    return maps, lam, coef, (sign * 1.0e3 * typical, -sign * 1.0e-3 * typical)


# ================================================================================================ 8-bit blur
def blur_box_radius(radius):
    """the integer box radius r that cmdiad_blur8_maps derives from the Gaussian radius: Pillow's _gaussian_blur_radius with float
    variables and double intermediates, three passes"""
    f32, f64 = np.float32, np.float64
    radius = f32(radius)
    sigma2 = f32(f32(radius * radius) / f32(3))
    L = f32(np.sqrt(f64(12.0) * f64(sigma2) + 1.0))
    l = f32(np.floor((f64(L) - 1.0) / 2.0))                                                    # noqa: E741
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    return int(f32(l + a))


BLUR_RADII = (4.0, 1.5)


def blur_shapes(radius):
    """(2r+2) x (2r+2): the shortest side the entry accepts (the box filter's middle loop is empty); a long side of 300 and a side of
    260 against 256 threads (a thread filters two lines) in both orientations"""
    s = 2 * blur_box_radius(radius) + 2
    return [(s, s), (s, 300), (300, s + 1), (260, 40), (40, 260)]


def blur_maps(H, W):
    """name -> map [H, W] f32: random, constant positive, one hot pixel in each corner, all zero"""
    rs = np.random.RandomState(H * 1000 + W)
    rnd = (rs.uniform(0.0, 1.0, (H, W)) ** 2 * 3.7).astype(np.float32)
    rnd[: H // 2] *= np.float32(0.01)
    corners = np.full((H, W), 0.125, np.float32)
    corners[0, 0], corners[0, -1], corners[-1, 0], corners[-1, -1] = 7.5, 6.25, 5.0, 3.75
    return collections.OrderedDict([("random", rnd), ("constant", np.full((H, W), 2.71875, np.float32)), ("corners", corners),
                                    ("zero", np.zeros((H, W), np.float32))])
