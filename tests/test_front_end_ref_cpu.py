"""CPU: the references and inputs of tests/front_end_ref.py, on which tests/test_gpu_front_end_edges.py compares bits.

A bit comparison against a restatement says something about a kernel only if (1) the restatement equals an independent yardstick
(the oracle's unorganize_no_zeros, the C oracle's ball query, scikit-learn's score_samples), (2) the inputs really contain the
situations a test is named after, and (3) the subtly wrong kernels the GPU file is meant to catch would give another answer on
these very inputs.  Each is asserted here, without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_end_ref as fr  # noqa: E402

from oracle import kernels as ok  # noqa: E402
from oracle import scoring  # noqa: E402

SCENES = fr.scenes()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ unorganize
def _against_oracle(pc):
    xyz, nz, pix2pt, n = fr.unorganize(pc, pc[0].size)
    ref_pc, ref_nz = scoring.unorganize_no_zeros(torch.from_numpy(pc)[None])
    np.testing.assert_array_equal(_bits(xyz), _bits(ref_pc[0].T.numpy()))
    np.testing.assert_array_equal(nz, ref_nz)
    assert n == len(ref_nz) and (pix2pt[ref_nz] == np.arange(n)).all() and np.count_nonzero(pix2pt >= 0) == n
    return nz


def test_unorganize_equals_the_oracle_on_the_value_edge_frame():
    pc = fr.edge_frame()
    kept = set(_against_oracle(pc).tolist())
    assert sorted(fr.EDGE_PLANTED) == sorted(["x_zero", "y_zero", "z_zero", "neg_zero", "nan", "inf", "denormal"])
    pixels = [p for p, _, _, _ in fr.EDGE_PLANTED.values()]
    assert len(set(pixels)) == len(pixels) and min(pixels) < fr.CHUNK <= max(pixels) < pc[0].size   # in both chunks
    flat = pc.reshape(3, -1)
    for name, (pixel, coord, pattern, keep) in fr.EDGE_PLANTED.items():
        assert int(flat.view(np.uint32)[coord, pixel]) == pattern, name
        others = np.delete(flat[:, pixel], coord)
        assert np.isfinite(others).all() and (np.abs(others) >= 0.25).all(), name        # ONE coordinate decides
        assert (pixel in kept) == keep, name
    assert [k for k, v in fr.EDGE_PLANTED.items() if not v[3]] == ["x_zero", "y_zero", "z_zero", "neg_zero"]
    assert {v[1] for k, v in fr.EDGE_PLANTED.items() if k.endswith("_zero") and k != "neg_zero"} == {0, 1, 2}
    d = flat[fr.EDGE_PLANTED["denormal"][1], fr.EDGE_PLANTED["denormal"][0]]
    assert d == np.float32(2.0 ** -149) and d != 0 and d < np.finfo(np.float32).tiny
    assert np.isnan(flat[2, fr.EDGE_PLANTED["nan"][0]]) and np.isposinf(flat[0, fr.EDGE_PLANTED["inf"][0]])
    assert np.signbit(flat[1, fr.EDGE_PLANTED["neg_zero"][0]]) and flat[1, fr.EDGE_PLANTED["neg_zero"][0]] == 0
    assert len(kept) == pc[0].size - 4


def test_frames_are_what_the_gpu_test_says_they_are():
    assert fr.FRAMES == [(1, 1), (30, 30), (32, 32), (25, 41), (64, 112), (67, 107), (64, 128), (96, 96), (100, 37), (224, 224)]
    sizes = [h * w for h, w in fr.FRAMES]
    group = fr.CHUNK * fr.AHEAD
    assert min(sizes) == 1 and any(1 < s < fr.CHUNK for s in sizes) and fr.CHUNK in sizes and fr.CHUNK + 1 in sizes
    assert group in sizes and group + 1 in sizes and 8 * fr.CHUNK in sizes and 9 * fr.CHUNK in sizes
    assert any(s % fr.CHUNK and s > fr.CHUNK and s < group for s in sizes)
    for H, W in fr.FRAMES:
        b = fr.frame_batch(H, W)
        assert b.shape == (3, 3, H, W) and b.dtype == np.float32
        nz = _against_oracle(b[0])
        assert len(_against_oracle(b[1])) == 0 and len(_against_oracle(b[2])) == H * W
        nonzero = b[b != 0]
        assert (np.abs(nonzero) >= 0.25).all() and np.isfinite(nonzero).all()
        if H * W >= 900:
            assert 0.5 < len(nz) / (H * W) < 0.7, (H, W, len(nz))
            bg = np.all(b[0].reshape(3, -1) != 0, axis=0) == 0
            zeros_per_bg = (b[0].reshape(3, -1)[:, bg] == 0).sum(0)
            assert set(zeros_per_bg.tolist()) == {1, 2, 3}                # background is not only "all three zero"
            runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], (~bg).astype(np.int8), [0]]))))
            assert len(set(runs.tolist())) > 10                           # irregular runs


def test_unorganize_truncation_rule():
    """pix2pt of a pixel cut off by n_max is -1, and the chunk cuts fall where they claim"""
    pc = fr.frame_batch(67, 107)[0]
    xyz, nz, pix2pt, n = fr.unorganize(pc, pc[0].size)
    cuts = fr.chunk_cuts(pc)
    assert len(cuts) == 6                                                   # chunks 1 .. 6; the last chunk holds ONE pixel
    for at, inside in cuts:
        x2, nz2, p2, n2 = fr.unorganize(pc, at)
        assert n2 == at and (nz2 == nz[:at]).all() and (_bits(x2) == _bits(xyz[:at])).all()
        assert nz[at - 1] // fr.CHUNK < nz[at] // fr.CHUNK                  # the cut is ON a chunk boundary
        assert (p2[nz[at:]] == -1).all() and (p2[nz[:at]] == np.arange(at)).all() and np.count_nonzero(p2 >= 0) == at
        assert nz[inside - 1] // fr.CHUNK == nz[inside] // fr.CHUNK         # this one falls INSIDE a chunk
    assert fr.unorganize(pc, 1)[3] == 1 and fr.unorganize(fr.frame_batch(30, 30)[1], 5)[3] == 0


def test_wrong_unorganize_kernels_would_differ():
    """a kernel that drops the partial last chunk, or restarts its running count at a look-ahead group, gives another answer on
    the frames that have a partial chunk / more than one group"""
    group = fr.CHUNK * fr.AHEAD
    for H, W in fr.FRAMES:
        HW = H * W
        for img in fr.frame_batch(H, W)[[0, 2]]:
            nz = fr.unorganize(img, HW)[1]
            if HW % fr.CHUNK:
                assert (nz >= HW // fr.CHUNK * fr.CHUNK).any(), (H, W)      # kept pixels live in the partial chunk
            if HW > group:
                assert (nz < group).any() and (nz >= group).any(), (H, W)   # a count restarted at the group would collide with row 0
    assert sum(1 for h, w in fr.FRAMES if h * w % fr.CHUNK) >= 5 and sum(1 for h, w in fr.FRAMES if h * w > group) >= 4


# ------------------------------------------------------------------------------------------------ ball query
@pytest.mark.parametrize("scene", SCENES, ids=[s.name for s in SCENES])
def test_ball_query_restatement_equals_the_c_oracle_and_integers(scene):
    for ns in fr.NSAMPLES:
        for b, n in enumerate(scene.n_valid):
            got = fr.ball_query(fr.RADIUS, ns, scene.xyz[b, :n], scene.query[b])
            np.testing.assert_array_equal(got, fr.ball_query_units(scene, b, ns), err_msg=f"{scene.name} b={b} ns={ns}")
            if n > 0:
                want = ok.ball_query(fr.RADIUS, ns, scene.xyz[b:b + 1, :n], scene.query[b:b + 1])[0]
            else:
                want = np.zeros_like(got)                                     # an empty cloud has no hit
            np.testing.assert_array_equal(got, want, err_msg=f"{scene.name} b={b} ns={ns}")


def test_scene_table_holds_what_the_issue_lists():
    assert [s.xyz.shape[1] for s in SCENES] == [1, 63, 64, 65, 128, 129, 300]
    assert {s.query.shape[1] for s in SCENES} == {1, 3, 4, 5, 9} and fr.NSAMPLES == [1, 8, 64, 65, 130]
    assert max(len(s.n_valid) for s in SCENES) == 3 and np.float32(fr.RADIUS) == fr.RADIUS
    assert float(np.float32(fr.RADIUS) * np.float32(fr.RADIUS)) == fr.R2_UNITS * fr.STEP ** 2
    for s in SCENES:
        assert s.xyz.dtype == np.float32 and s.query.dtype == np.float32 and s.n_valid.dtype == np.int32
        assert (s.n_valid < s.xyz.shape[1]).any() and (s.n_valid <= s.xyz.shape[1]).all() and (s.n_valid >= 0).all()
        fr.scene_units(s)                                                     # on the lattice, |coordinate| <= 4
        for b, n in enumerate(s.n_valid):                                     # rows behind n_valid: inside EVERY query's radius
            hit_all, _ = fr.hits_units(s, b, valid_only=False)
            assert hit_all[:, n:].all(), (s.name, b)


def test_scenes_contain_their_situations():
    need = {"clip", "clip_after_earlier_hits", "straddle", "first_hit_late", "prefill_survives", "prefill_survives_past_slot_64",
            "no_hit", "no_hit_before_garbage", "on_radius", "one_step_inside", "ragged"}
    found = {}
    for s in SCENES:
        for ns in fr.NSAMPLES:
            for c in fr.scene_conditions(s, ns):
                found.setdefault(c, []).append((s.name, ns))
    assert need <= set(found), need - set(found)
    assert {ns for _, ns in found["clip_after_earlier_hits"]} >= {64, 65, 130}      # the clip inside a later step, wide slots too
    assert {ns for _, ns in found["prefill_survives_past_slot_64"]} == {65, 130}


def test_wrong_ball_query_kernels_would_differ():
    """`<=` for `<`, n_valid ignored, and a pre-fill of only the first 64 slots each change the result of at least one scene"""
    le = ragged = 0
    for s in SCENES:
        for b, n in enumerate(s.n_valid):
            for ns in fr.NSAMPLES:
                ref = fr.ball_query_units(s, b, ns)
                le += not np.array_equal(ref, fr.ball_query_units(s, b, ns, inclusive=True))
                if n < s.xyz.shape[1]:
                    tells = not np.array_equal(ref, fr.ball_query_units(s, b, ns, valid_only=False))
                    # every ragged cloud tells where slots are left to fill (N = 1: the garbage row is row 0, which "no hit" reports too)
                    assert tells or ns < 130 or s.xyz.shape[1] == 1, (s.name, b, ns)
                    ragged += tells
    assert le >= 10 and ragged >= 30, (le, ragged)
    short = 0                                                                 # slots 64.. that hold the pre-fill of a NON-ZERO first hit
    for s in SCENES:
        for b in range(len(s.n_valid)):
            for ns in (65, 130):
                ref = fr.ball_query_units(s, b, ns)
                hit, _ = fr.hits_units(s, b)
                for j in range(ref.shape[0]):
                    nh = int(hit[j].sum())
                    short += 0 < nh <= 64 and ref[j, 0] != 0 and (ref[j, 64:] == ref[j, 0]).all()
    assert short >= 4


# ------------------------------------------------------------------------------------------------ gather
def test_gather_cases():
    assert {J for J, _, _ in fr.GATHER_CASES} == {1, 255, 256, 257} and {C for _, C, _ in fr.GATHER_CASES} == {1, 5}
    for J, C, (M, ns) in fr.GATHER_CASES:
        feat, idx = fr.gather_case(J, C)
        assert M * ns == J and idx.shape == (fr.GATHER_B, J) and idx.min() == 0 and idx.max() == fr.GATHER_N - 1
        out = fr.gather(feat, idx.reshape(fr.GATHER_B, M, ns))
        assert out.shape == (fr.GATHER_B, C, M, ns)
        want = torch.gather(torch.from_numpy(feat), 2, torch.from_numpy(idx).long()[:, None, :].expand(-1, C, -1)).numpy()
        np.testing.assert_array_equal(out.reshape(fr.GATHER_B, C, J), want)
        assert not (_bits(out) == fr.SENT32).any()


# ------------------------------------------------------------------------------------------------ one-class SVM score maps
def test_ocsvm_scores_agree_with_sklearn_on_the_existing_tests_inputs():
    """the inputs and the tolerance of tests/test_gpu_kernels.py test_ocsvm_score_maps_vs_sklearn"""
    from sklearn import linear_model
    g = torch.Generator().manual_seed(3)
    maps = torch.rand(3, 2, 224 * 224, generator=g) * torch.tensor([2.0, 20.0]).view(1, 2, 1)
    lam = (1.0, 0.1)
    X = torch.stack([lam[0] * maps[:, 0], lam[1] * maps[:, 1]], -1).reshape(-1, 2)
    svm = linear_model.SGDOneClassSVM(random_state=42, nu=0.5, max_iter=1000).fit(X[::7])
    want = svm.score_samples(X).reshape(3, -1)
    got = fr.ocsvm_scores(maps.numpy(), lam, svm.coef_, svm.offset_)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_ocsvm_cases_tell_a_fused_multiply_add():
    assert {K for _, K, _ in fr.OCSVM_CASES} == {1, 2, 3, 4} and {HW for _, _, HW in fr.OCSVM_CASES} == {1, 255, 256, 257, 900}
    assert {B for B, _, _ in fr.OCSVM_CASES} == {1, 3} and len(fr.OCSVM_CASES) == 40
    assert len({np.sign(c) for c in fr.OCSVM_COEF}) == 2 and max(map(abs, fr.OCSVM_COEF)) / min(map(abs, fr.OCSVM_COEF)) > 1e4
    signs = set()
    for B, K, HW in fr.OCSVM_CASES:
        maps, lam, coef, (offset, small) = fr.ocsvm_case(B, K, HW)
        s = fr.ocsvm_scores(maps, lam, coef, 0.0)
        assert 300 < abs(offset) / np.abs(s).mean() < 3000 and 3e-4 < abs(small) / np.abs(s).mean() < 3e-3
        assert np.isfinite(fr.ocsvm_scores(maps, lam, coef, offset)).all()
        signs.add(np.sign(offset))
    assert signs == {-1.0, 1.0}
    # K >= 2: the product float64(v) * coef_k has 77 significant bits, so rounding it before the add shows in s.  Behind the large
    # offset ten bits of s are rounded away again and the difference rarely survives; behind the small one it does.
    for B, K, HW in fr.OCSVM_CASES:
        if K >= 2 and HW >= 255 and B == 1:
            maps, lam, coef, (offset, small) = fr.ocsvm_case(B, K, HW)
            differ = fr.ocsvm_scores(maps, lam, coef, small) != fr.ocsvm_scores_fma(maps, lam, coef, small)
            assert differ.mean() > 0.1, (K, HW, differ.mean())
    maps, lam, coef, (offset, small) = fr.ocsvm_case(1, 1, 257)                # K = 1: s = 0 + v * c, nothing to fuse
    np.testing.assert_array_equal(fr.ocsvm_scores(maps, lam, coef, small), fr.ocsvm_scores_fma(maps, lam, coef, small))


# ------------------------------------------------------------------------------------------------ 8-bit blur
def test_blur_shapes_and_maps():
    assert fr.blur_box_radius(4.0) == 3 and fr.blur_box_radius(1.5) == 1
    for radius in fr.BLUR_RADII:
        r = fr.blur_box_radius(radius)
        s = 2 * r + 2
        assert fr.blur_shapes(radius) == [(s, s), (s, 300), (300, s + 1), (260, 40), (40, 260)]
        ok.pil_gaussian_blur_u8(np.zeros((s, s), np.uint8), radius)          # the shortest side the oracle restates ...
        for shape in ((s - 1, 64), (64, s - 1)):                              # ... and one shorter: refused
            with pytest.raises(ValueError):
                ok.pil_gaussian_blur_u8(np.zeros(shape, np.uint8), radius)
        for H, W in fr.blur_shapes(radius):
            m = fr.blur_maps(H, W)
            assert list(m) == ["random", "constant", "corners", "zero"] and all(v.shape == (H, W) and v.dtype == np.float32 for v in m.values())
            assert len(np.unique(m["constant"])) == 1 and m["constant"][0, 0] > 0 and not m["zero"].any()
            c = m["corners"]
            hot = sorted([c[0, 0], c[0, -1], c[-1, 0], c[-1, -1]])
            assert hot[0] > 0.125 and len(set(hot)) == 4 and np.count_nonzero(c != 0.125) == 4
            # the yardstick on the constant map: 255 everywhere in, 255 everywhere out
            assert (ok.pil_gaussian_blur_u8(np.full((H, W), 255, np.uint8), radius) == 255).all()
    # a blur that skips a thread's second line (lines 256 ..) shows on the 260-sided maps: the yardstick changes those lines
    m = torch.from_numpy(fr.blur_maps(260, 40)["random"])
    u8 = (m / m.max()).mul(255).byte().numpy()
    assert (ok.pil_gaussian_blur_u8(u8, 4.0)[256:] != u8[256:]).any()
