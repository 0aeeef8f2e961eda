"""GPU: the kernels at the two ends of an inference step, off the 224 x 224 production frame and bit for bit -- unorganize_kernel
(csrc/interp_pool.hip), ball_query_kernel and gather_points_kernel (csrc/ballquery.hip) with the compat layer on top of them,
ocsvm_score_maps_kernel and blur8_maps_kernel (csrc/post.hip).  References and inputs: tests/front_end_ref.py;
tests/test_front_end_ref_cpu.py shows without a GPU that the references equal independent yardsticks, that the inputs contain the
situations the tests below are named after, and that the wrong kernels named in the docstrings below would give other bits.

No tolerance anywhere: every kernel here is built without contraction or only moves values.  Outputs that a test allocates itself
are the leading part of a buffer of sentinel bit patterns; what a launch has no business writing must keep them."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_end_ref as fr  # noqa: E402

from cmdiad_amd import _native as nat  # noqa: E402
from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd._native import NativeError  # noqa: E402
from oracle import kernels as ok  # noqa: E402

DEV = "cuda"
GUARD = 64                               # sentinel elements (rows of xyz) behind every output
SCENES = fr.scenes()
p = ops._p


def _sent(n):
    return torch.full((n,), fr.SENT32, dtype=torch.int32, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ================================================================================================ unorganize
def _unorganize(pcs, n_max, nz=True, pix2pt=True, n_valid=True):
    """one cmdiad_unorganize launch on pcs [B, 3, H, W] into sentinel buffers; the WHOLE buffers as int32 bit patterns, on the host
    (None for an output passed as a null pointer)"""
    B, HW = pcs.shape[0], pcs.shape[2] * pcs.shape[3]
    d = _dev(pcs)
    bufs = {"xyz": _sent((B * n_max + GUARD) * 3), "nz": _sent(B * n_max + GUARD) if nz else None,
            "pix2pt": _sent(B * HW + GUARD) if pix2pt else None, "n_valid": _sent(B + GUARD) if n_valid else None}
    ops._call("cmdiad_unorganize", p(d), B, HW, n_max, p(bufs["xyz"]), p(bufs["nz"]), p(bufs["pix2pt"]), p(bufs["n_valid"]), ops._stream())
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in bufs.items()}


def _check_unorganize(out, pcs, n_max, what):
    B, HW = pcs.shape[0], pcs.shape[2] * pcs.shape[3]
    xyz = out["xyz"].reshape(-1, 3)
    for b in range(B):
        rx, rnz, rp, n = fr.unorganize(pcs[b], n_max)
        w = f"{what} image {b} (n = {n}, Nmax = {n_max})"
        lo = b * n_max
        np.testing.assert_array_equal(xyz[lo:lo + n], _bits(rx), err_msg=w + ": xyz")
        assert (xyz[lo + n:lo + n_max] == fr.SENT32).all(), w + ": xyz rows n .. Nmax - 1 were written"
        if out["nz"] is not None:
            np.testing.assert_array_equal(out["nz"][lo:lo + n], rnz, err_msg=w + ": nz")
            assert (out["nz"][lo + n:lo + n_max] == fr.SENT32).all(), w + ": nz rows n .. Nmax - 1 were written"
        if out["pix2pt"] is not None:
            np.testing.assert_array_equal(out["pix2pt"][b * HW:(b + 1) * HW], rp, err_msg=w + ": pix2pt")
        if out["n_valid"] is not None:
            assert out["n_valid"][b] == n, w + f": n_valid = {out['n_valid'][b]}"
    assert (xyz[B * n_max:] == fr.SENT32).all(), what + ": the guard behind xyz was written"
    for k, used in (("nz", B * n_max), ("pix2pt", B * HW), ("n_valid", B)):
        assert out[k] is None or (out[k][used:] == fr.SENT32).all(), f"{what}: the guard behind {k} was written"


def _same_buffers(a, b, what):
    for k in a:
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _n_max_values(pcs):
    HW = pcs.shape[2] * pcs.shape[3]
    n = fr.unorganize(pcs[0], HW)[3]
    cuts = fr.chunk_cuts(pcs[0])
    vals = [HW, n, n - 1, 1] + [v for c in (cuts[:1] + cuts[-1:]) for v in c] + ([fr.CHUNK, 3 * fr.CHUNK + 77] if HW > 4 * fr.CHUNK else [])
    return sorted({v for v in vals if 0 < v <= HW}, reverse=True)


@pytest.mark.parametrize("H,W", fr.FRAMES)
def test_unorganize_frames_bit_for_bit(H, W):
    """A batch of three images (about 60 % valid in irregular runs, all background, all valid) and each image alone, for Nmax = HW,
    exactly n, n - 1, 1 and cuts on and inside a chunk boundary: rows 0 .. n - 1 of xyz and nz, all of pix2pt and n_valid equal
    the numpy rule; rows n .. Nmax - 1 and the guards keep their sentinel; alone = batched; a second launch gives the same bits.
    A kernel that drops the partial last chunk loses the kept pixels there (1 x 1, 30 x 30, 25 x 41, 67 x 107, 100 x 37); one that
    restarts its running count at a look-ahead group stores the pixels past 7 168 over rows 0 .. (67 x 107, 64 x 128, 96 x 96,
    224 x 224): xyz, nz, pix2pt and n_valid all differ."""
    pcs = fr.frame_batch(H, W)
    for n_max in _n_max_values(pcs):
        what = f"{H} x {W}, Nmax = {n_max}"
        out = _unorganize(pcs, n_max)
        _check_unorganize(out, pcs, n_max, what + ", batch")
        for b in range(3):
            alone = _unorganize(pcs[b:b + 1], n_max)
            _check_unorganize(alone, pcs[b:b + 1], n_max, what + f", image {b} alone")
            np.testing.assert_array_equal(alone["xyz"][:n_max * 3], out["xyz"][b * n_max * 3:(b + 1) * n_max * 3], err_msg=what)
            np.testing.assert_array_equal(alone["nz"][:n_max], out["nz"][b * n_max:(b + 1) * n_max], err_msg=what)
            np.testing.assert_array_equal(alone["pix2pt"][:H * W], out["pix2pt"][b * H * W:(b + 1) * H * W], err_msg=what)
            assert alone["n_valid"][0] == out["n_valid"][b]
    _same_buffers(_unorganize(pcs, H * W), _unorganize(pcs, H * W), f"{H} x {W}: two launches")


def test_unorganize_value_edges():
    """The keep rule is the reference's all(pc != 0): a pixel with ONE coordinate +0.0 or -0.0 is dropped; NaN, +inf and the
    smallest fp32 denormal in one coordinate are kept, with their bits.  (A kernel that flushes denormals drops the last one.)"""
    pc = fr.edge_frame()[None]
    HW = fr.EDGE_H * fr.EDGE_W
    n = HW - 4
    for n_max in (HW, n, n - 1):
        out = _unorganize(pc, n_max)
        _check_unorganize(out, pc, n_max, f"value edges, Nmax = {n_max}")
    out = _unorganize(pc, HW)
    assert out["n_valid"][0] == n
    for name, (pixel, coord, pattern, keep) in fr.EDGE_PLANTED.items():
        pos = out["pix2pt"][pixel]
        assert (pos >= 0) == keep, f"{name}: pix2pt = {pos}"
        if keep:
            assert out["nz"][pos] == pixel and int(out["xyz"].reshape(-1, 3)[pos, coord]) & 0xFFFFFFFF == pattern, name


def test_unorganize_null_outputs():
    """nz, pix2pt and n_valid each null in turn, and all three: what remains is what the full launch gives, sentinels included"""
    pcs = fr.frame_batch(67, 107)
    n_max = fr.unorganize(pcs[0], 67 * 107)[3] - 1             # image 0 and image 2 are truncated, image 1 is empty
    full = _unorganize(pcs, n_max)
    _check_unorganize(full, pcs, n_max, "all outputs")
    for drop in (("nz",), ("pix2pt",), ("n_valid",), ("nz", "pix2pt", "n_valid")):
        out = _unorganize(pcs, n_max, **{k: False for k in drop})
        assert all(out[k] is None for k in drop)
        _same_buffers({k: v for k, v in out.items() if k not in drop}, {k: v for k, v in full.items() if k not in drop}, f"without {drop}")
        _check_unorganize(out, pcs, n_max, f"without {drop}")


# ================================================================================================ ball query
def _ball_query(scene, nsample, with_n_valid=True):
    """one cmdiad_ball_query launch into a sentinel buffer -> (idx [B, M, nsample], guard), on the host"""
    B, N, M = scene.xyz.shape[0], scene.xyz.shape[1], scene.query.shape[1]
    xyz, q, nv = _dev(scene.xyz), _dev(scene.query), _dev(scene.n_valid)
    out = _sent(B * M * nsample + GUARD)
    ops._call("cmdiad_ball_query", p(xyz), p(nv) if with_n_valid else None, p(q), B, N, M, float(fr.RADIUS), nsample, p(out), ops._stream())
    out = out.cpu().numpy()
    return out[:B * M * nsample].reshape(B, M, nsample), out[B * M * nsample:]


@pytest.mark.parametrize("scene", SCENES, ids=[s.name for s in SCENES])
def test_ball_query_scenes_bit_for_bit(scene):
    """Lattice scenes (every squared distance exact) with ragged n_valid and in-range garbage behind it, nsample 1, 8, 64, 65, 130:
    the kernel equals the numpy restatement and the C oracle on the cloud sliced to its valid length, twice.
    `<=` for `<` admits the points planted ON the sphere; a kernel that ignores n_valid admits the garbage rows, every one of them
    inside every query's radius; a pre-fill of only the first 64 slots leaves slots 64 .. of nsample 65 and 130 unwritten where
    fewer than 65 points hit (n65: the only hit is row 64); a missing slot clip writes past a query's slots, into the next
    query's or the guard."""
    B, N = scene.xyz.shape[:2]
    for ns in fr.NSAMPLES:
        got, guard = _ball_query(scene, ns)
        what = f"{scene.name}, nsample = {ns}"
        assert (guard == fr.SENT32).all(), what + ": the guard behind idx was written"
        for b, n in enumerate(scene.n_valid):
            want = fr.ball_query(fr.RADIUS, ns, scene.xyz[b, :n], scene.query[b])
            np.testing.assert_array_equal(got[b], want, err_msg=f"{what}, cloud {b} (n_valid = {n} of {N})")
            if n > 0:
                oracle = ok.ball_query(fr.RADIUS, ns, scene.xyz[b:b + 1, :n], scene.query[b:b + 1])[0]
                np.testing.assert_array_equal(got[b], oracle, err_msg=f"{what}, cloud {b}: C oracle")
        again = ops.ball_query(fr.RADIUS, ns, _dev(scene.xyz), _dev(scene.query), n_valid=_dev(scene.n_valid))
        assert again.dtype == torch.int32 and again.shape == got.shape
        np.testing.assert_array_equal(again.cpu().numpy(), got, err_msg=what + ": second launch")
        whole, guard = _ball_query(scene, ns, with_n_valid=False)          # no n_valid: the garbage rows ARE points
        assert (guard == fr.SENT32).all()
        np.testing.assert_array_equal(whole, ok.ball_query(fr.RADIUS, ns, scene.xyz, scene.query), err_msg=what + ": no n_valid")
        for b in range(B):
            np.testing.assert_array_equal(whole[b], fr.ball_query(fr.RADIUS, ns, scene.xyz[b], scene.query[b]), err_msg=what)


def test_ball_query_empty_batch_or_no_query_launches_nothing():
    s = SCENES[1]
    xyz, q, nv, out = _dev(s.xyz), _dev(s.query), _dev(s.n_valid), _sent(256)
    for B, M in ((0, 3), (3, 0), (0, 0)):
        ops._call("cmdiad_ball_query", p(xyz), p(nv), p(q), B, s.xyz.shape[1], M, float(fr.RADIUS), 8, p(out), ops._stream())
        assert (out.cpu().numpy() == fr.SENT32).all(), (B, M)


@pytest.mark.parametrize("J,C,ms", fr.GATHER_CASES)
def test_gather_points_bit_for_bit(J, C, ms):
    """cmdiad_gather_points at J = 1, 255, 256, 257 (one element, one short of a block, a block, one over) and C = 1, 5 against
    numpy fancy indexing, indices 0 and N - 1 included, the output behind a guard; then the grouping form idx [B, M, ns]"""
    feat, idx = fr.gather_case(J, C)
    B, N = fr.GATHER_B, fr.GATHER_N
    dfeat, didx, out = _dev(feat), _dev(idx), _sent(B * C * J + GUARD)
    ops._call("cmdiad_gather_points", p(dfeat), p(didx), B, C, N, J, p(out), ops._stream())
    out = out.cpu().numpy()
    np.testing.assert_array_equal(out[:B * C * J].reshape(B, C, J), _bits(fr.gather(feat, idx)))
    assert (out[B * C * J:] == fr.SENT32).all(), "the guard behind the output was written"
    grouped = ops.gather_points(dfeat, didx.view(B, *ms))
    assert grouped.shape == (B, C, *ms) and grouped.dtype == torch.float32
    np.testing.assert_array_equal(_bits(grouped.cpu().numpy()), _bits(fr.gather(feat, idx.reshape(B, *ms))))
    ops._call("cmdiad_gather_points", p(dfeat), p(didx), 0, C, N, J, p(dfeat), ops._stream())      # B = 0, J = 0: no launch
    ops._call("cmdiad_gather_points", p(dfeat), p(didx), B, C, N, 0, p(dfeat), ops._stream())
    np.testing.assert_array_equal(_bits(dfeat.cpu().numpy()), _bits(feat))


# ------------------------------------------------------------------------------------------------ compat layer
def test_knn_untransposed_mode_is_the_transpose():
    """knn_cuda.KNN(k, transpose_mode=False) on [B, 3, N] / [B, 3, M] returns [B, k, M]: the transposes of the transposed mode's"""
    from cmdiad_amd.compat import knn_cuda
    rs = np.random.RandomState(5)
    ref, query = _dev(rs.standard_normal((2, 200, 3)).astype(np.float32)), _dev(rs.standard_normal((2, 7, 3)).astype(np.float32))
    dist_t, idx_t = knn_cuda.KNN(k=5, transpose_mode=True)(ref, query)
    dist, idx = knn_cuda.KNN(k=5, transpose_mode=False)(ref.transpose(1, 2).contiguous(), query.transpose(1, 2).contiguous())
    assert dist_t.shape == (2, 7, 5) and dist.shape == (2, 5, 7) and idx.shape == (2, 5, 7) and idx.dtype == torch.int64
    assert torch.equal(idx, idx_t.transpose(1, 2)) and torch.equal(dist, dist_t.transpose(1, 2))
    np.testing.assert_array_equal(idx_t.cpu().numpy(), ok.knn_group(ref.cpu().numpy(), query.cpu().numpy(), 5)[0])
    assert knn_cuda.KNN(k=5)(ref.transpose(1, 2), query.transpose(1, 2))[1].equal(idx)             # the default mode; strided inputs


@pytest.mark.parametrize("use_xyz", [True, False])
def test_query_and_group_with_features(use_xyz):
    """QueryAndGroup(r, ns) with features [B, 5, N]: ball query restated in numpy, then plain indexing; use_xyz=False returns the
    grouped features alone.  (The compat entry passes no n_valid: the whole lattice cloud of scene n128 counts.)"""
    from cmdiad_amd.compat import pointnet2_utils as p2
    s, ns = SCENES[4], 8
    B, N, M = s.xyz.shape[0], s.xyz.shape[1], s.query.shape[1]
    feat = np.random.RandomState(11).standard_normal((B, 5, N)).astype(np.float32)
    got = p2.QueryAndGroup(fr.RADIUS, ns, use_xyz=use_xyz)(_dev(s.xyz), _dev(s.query), _dev(feat))
    idx = np.stack([fr.ball_query(fr.RADIUS, ns, s.xyz[b], s.query[b]) for b in range(B)])             # [B, M, ns]
    assert len({tuple(r) for r in idx.reshape(-1, ns)}) > 4                                           # not one answer for every query
    gxyz = np.stack([(s.xyz[b][idx[b]] - s.query[b][:, None, :]).transpose(2, 0, 1) for b in range(B)])   # [B, 3, M, ns]
    want = np.concatenate([gxyz, fr.gather(feat, idx)], 1) if use_xyz else fr.gather(feat, idx)
    assert got.shape == (B, 8 if use_xyz else 5, M, ns)
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    no_feat = p2.QueryAndGroup(fr.RADIUS, ns)(_dev(s.xyz), _dev(s.query))
    np.testing.assert_array_equal(_bits(no_feat.cpu().numpy()), _bits(gxyz))


def test_group_all():
    """GroupAll: xyz [B, N, 3] -> [B, 3, 1, N], features [B, C, N] -> [B, C, 1, N], concatenated when use_xyz"""
    from cmdiad_amd.compat import pointnet2_utils as p2
    rs = np.random.RandomState(13)
    xyz, feat = rs.standard_normal((2, 33, 3)).astype(np.float32), rs.standard_normal((2, 5, 33)).astype(np.float32)
    gx = xyz.transpose(0, 2, 1).reshape(2, 3, 1, 33)
    gf = feat.reshape(2, 5, 1, 33)
    for use_xyz, f, want in ((True, None, gx), (False, None, gx), (True, feat, np.concatenate([gx, gf], 1)), (False, feat, gf)):
        got = p2.GroupAll(use_xyz=use_xyz)(_dev(xyz), None, _dev(f) if f is not None else None)
        assert got.shape == want.shape, (use_xyz, f is None)
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))


# ================================================================================================ one-class SVM score maps
def _score(maps, lam, coef, offset, B=None):
    """one cmdiad_ocsvm_score_maps launch into a sentinel buffer -> (scores [B, HW] f64, guard as int64), on the host"""
    nB, K, HW = maps.shape
    B = nB if B is None else B
    d = _dev(maps)
    out = torch.full((nB * HW + GUARD,), fr.SENT64, dtype=torch.int64, device=DEV)
    lam32, cf = np.ascontiguousarray(lam, np.float32), np.ascontiguousarray(coef, np.float64)
    ops._call("cmdiad_ocsvm_score_maps", p(d), B, K, HW, lam32.ctypes.data, cf.ctypes.data, float(offset), p(out), ops._stream())
    out = out.cpu().numpy()
    return out[:nB * HW].view(np.float64).reshape(nB, HW), out[nB * HW:], out


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_ocsvm_score_maps_bit_for_bit(K):
    """K = 1 .. 4 maps, HW = 1, 255, 256, 257, 900, B = 1, 3, coefficients of mixed sign and magnitude; with an offset about 1e3
    times the sum and with one about 1e-3 times it: float64 equality with the formula of the kernel's comment.  A kernel that fuses
    s + v * coef_k into one multiply-add rounds once where the formula rounds twice: behind the small offset more than a tenth of
    the elements of every K >= 2 case differ in the last bit (behind the large one ten bits of s are rounded away and few do)."""
    for B, k, HW in fr.OCSVM_CASES:
        if k != K:
            continue
        maps, lam, coef, offsets = fr.ocsvm_case(B, K, HW)
        for offset in offsets:
            got, guard, _ = _score(maps, lam, coef, offset)
            what = f"B = {B}, K = {K}, HW = {HW}, offset = {offset!r}"
            assert (guard == fr.SENT64).all(), what + ": the guard behind the output was written"
            np.testing.assert_array_equal(got, fr.ocsvm_scores(maps, lam, coef, offset), err_msg=what)
        via_ops = ops.ocsvm_score_maps(_dev(maps), lam, coef, offsets[0])
        assert via_ops.dtype == torch.float64 and via_ops.shape == (B, HW)
        np.testing.assert_array_equal(via_ops.cpu().numpy(), fr.ocsvm_scores(maps, lam, coef, offsets[0]))


def test_ocsvm_score_maps_arguments():
    """B = 0 returns without a launch; K = 5 (and K = 0) is an argument error, and nothing is written"""
    maps, lam, coef, offsets = fr.ocsvm_case(3, 4, 257)
    _, _, whole = _score(maps, lam, coef, offsets[0], B=0)
    assert (whole == fr.SENT64).all()
    five = _dev(np.concatenate([maps, maps[:, :1]], 1))
    lam5, coef5 = np.array(fr.OCSVM_LAM + (0.5,), np.float32), np.array(fr.OCSVM_COEF + (1.5,), np.float64)
    with pytest.raises(NativeError, match="K=5"):
        ops.ocsvm_score_maps(five, lam5, coef5, offsets[0])
    out = torch.full((3 * 257 + GUARD,), fr.SENT64, dtype=torch.int64, device=DEV)
    for K in (5, 0):
        with pytest.raises(NativeError, match=f"K={K}"):
            ops._call("cmdiad_ocsvm_score_maps", p(five), 3, K, 257, lam5.ctypes.data, coef5.ctypes.data, float(offsets[0]), p(out), ops._stream())
    assert (out.cpu().numpy() == fr.SENT64).all()


# ================================================================================================ 8-bit blur
def _blur(maps, radius):
    """one cmdiad_blur8_maps launch on maps [n, H, W] into a sentinel buffer -> (out [n, H, W] f32, guard bits), on the host"""
    n, H, W = maps.shape
    d, out = _dev(maps), _sent(n * H * W + GUARD)
    ops._call("cmdiad_blur8_maps", p(d), n, H, W, float(radius), p(out), ops._stream())
    out = out.cpu().numpy()
    return out[:n * H * W].view(np.float32).reshape(n, H, W), out[n * H * W:], out


def _blur_yardstick(m, radius):
    """the yardstick of test_blur8_maps_bit_exact: torch quantisation as the reference's KNNGaussianBlur does it, Pillow's blur from
    the C oracle"""
    t = torch.from_numpy(m)
    mx = t.max()
    u8 = (t / mx).mul(255).byte().numpy()
    return (torch.from_numpy(ok.pil_gaussian_blur_u8(u8, radius)).float().div(255) * mx).numpy()


BLUR_CASES = [(radius, H, W) for radius in fr.BLUR_RADII for H, W in fr.blur_shapes(radius)]


@pytest.mark.parametrize("radius,H,W", BLUR_CASES)
def test_blur8_maps_edge_shapes(radius, H, W):
    """Radius 4.0 (r = 3) and 1.5 (r = 1): a side of exactly 2r + 2 (the middle loop of the box filter is empty) in one or both
    directions, a side of 300 or 260 against the 256 threads (a thread filters two lines), a random map, a constant positive map
    (out = in exactly), a hot pixel in each corner, an all-zero map (0 / 0 quantises to some byte, times a maximum of 0: zeros, no
    NaN).  A blur that skips a thread's second line leaves lines 256 .. of the 300- and 260-sided maps unfiltered or unwritten:
    the random and the corner maps differ from the yardstick there."""
    r = fr.blur_box_radius(radius)
    assert min(H, W) >= 2 * r + 2
    maps = fr.blur_maps(H, W)
    out, guard, _ = _blur(np.stack(list(maps.values())), radius)
    assert (guard == fr.SENT32).all(), "the guard behind the output was written"
    assert not (_bits(out) == fr.SENT32).any(), "elements of the output were never written"
    got = dict(zip(maps, out))
    for name in ("random", "corners", "constant"):
        np.testing.assert_array_equal(_bits(got[name]), _bits(_blur_yardstick(maps[name], radius)), err_msg=f"{name} {H} x {W} r = {r}")
    np.testing.assert_array_equal(_bits(got["constant"]), _bits(maps["constant"]))
    assert not np.isnan(got["zero"]).any() and (got["zero"] == 0).all()
    alone, _, _ = _blur(maps["corners"][None], radius)                          # a map alone = the map in the batch
    np.testing.assert_array_equal(_bits(alone[0]), _bits(got["corners"]))


@pytest.mark.parametrize("radius", fr.BLUR_RADII)
def test_blur8_maps_refuses_a_side_below_the_window(radius):
    """a side of 2r + 1 is refused by the oracle and by the entry point, which launches nothing"""
    s = 2 * fr.blur_box_radius(radius) + 1
    for H, W in ((s, 64), (64, s), (s, s)):
        with pytest.raises(ValueError):
            ok.pil_gaussian_blur_u8(np.zeros((H, W), np.uint8), radius)
        d, out = _dev(np.ones((1, H, W), np.float32)), _sent(H * W + GUARD)
        with pytest.raises(NativeError, match="shorter than the box window"):
            ops._call("cmdiad_blur8_maps", p(d), 1, H, W, float(radius), p(out), ops._stream())
        assert (out.cpu().numpy() == fr.SENT32).all()


def test_blur8_maps_refuses_what_does_not_fit_the_lds():
    """cmdiad_blur8_lds_bytes (two copies of the padded byte image in the larger of its orientations) decides: every shape the entry
    point accepts needs less than every shape it refuses; a refusal launches nothing, an accepted shape equals the yardstick.  A
    thin strip needs little whatever its length; 1024 x 1024 needs 2 MiB, more than any LDS."""
    need = nat.lib().cmdiad_blur8_lds_bytes
    shapes = [(40, 40), (8, 4000), (280, 280), (284, 284), (285, 285), (288, 288), (320, 320), (8, 20000), (1024, 1024)]
    assert need(8, 300) == 2 * 300 * 12 and need(300, 9) == 2 * 300 * 16 and need(224, 224) == 2 * 224 * 228
    accepted, refused = [], []
    for H, W in shapes:
        m = fr.blur_maps(H, W)["random"]
        d, out = _dev(m[None]), _sent(H * W + GUARD)
        try:
            ops._call("cmdiad_blur8_maps", p(d), 1, H, W, 4.0, p(out), ops._stream())
        except NativeError as e:
            assert "LDS" in str(e), e
            assert (out.cpu().numpy() == fr.SENT32).all(), f"{H} x {W} was refused, but something was written"
            refused.append(int(need(H, W)))
            continue
        out = out.cpu().numpy()
        assert (out[H * W:] == fr.SENT32).all()
        np.testing.assert_array_equal(out[:H * W].reshape(H, W), _bits(_blur_yardstick(m, 4.0)), err_msg=f"{H} x {W}")
        accepted.append(int(need(H, W)))
    assert accepted and refused and max(accepted) < min(refused), (accepted, refused)
    assert int(need(1024, 1024)) in refused and int(need(40, 40)) in accepted and int(need(8, 4000)) in accepted
