"""CPU: the numpy restatement of the FP16 greedy coreset selection (tests/coreset_ref.py) against the two statements of it that
already exist -- the torch restatement inside tests/test_gpu_engine.py::test_greedy_coreset_matches_fp16_restatement at its own
shape (3000 x 62), and the picks the REFERENCE's own function made (tests/golden/g9_coreset.npz) -- before
tests/test_gpu_coreset.py holds the HIP kernels to it.  No GPU, no cmdiad_amd import."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreset_ref as cr  # noqa: E402


def _torch_restatement(z, n_select):
    """The loop of test_greedy_coreset_matches_fp16_restatement (torch's CPU norm: fp32 sums in torch's own order)."""
    zh = z.half()
    min_d = torch.linalg.norm(z - z[0:1], dim=1).half()
    ref, last = [0], zh[0:1]
    for _ in range(n_select - 1):
        d = torch.linalg.norm((zh - last).float(), dim=1).half()
        min_d = torch.minimum(d, min_d)
        i = int(torch.nonzero(min_d == min_d.max())[0])
        ref.append(i)
        last = zh[i:i + 1]
    return np.asarray(ref)


def test_restatement_equals_the_torch_restatement_at_its_shape():
    z = torch.randn(3000, 62, generator=torch.Generator().manual_seed(7))
    np.testing.assert_array_equal(cr.greedy_fp16(z, 200), _torch_restatement(z, 200))


def test_restatement_equals_the_reference_golden(golden):
    from sklearn import random_projection
    g = golden("g9_coreset.npz")
    z = torch.randn(int(g["rows"]), int(g["dim"]), generator=torch.Generator().manual_seed(int(g["z_seed"])))
    tr = random_projection.SparseRandomProjection(eps=float(g["eps"]), random_state=int(g["random_state"]))
    zp = tr.fit_transform(z.numpy()).astype(np.float32)
    np.testing.assert_array_equal(cr.greedy_fp16(zp, int(g["n"])), g["idx"])


def test_round_distance_is_sequential_fp32_over_pairs():
    """Three rows by hand: the pair sums enter the accumulator one after the other (a large first pair swallows later small
    ones that a pairwise or float64 sum would keep), and the difference is rounded to half before it is squared."""
    zh = np.zeros((3, 6), np.float16)
    zh[1] = [2048, 0, 1, 0, 1, 0]                      # acc: 2^22, then + 1 twice -- exact in fp32
    zh[2, 0], zh[2, 1] = 1.0, np.float16(2.0 ** -11)   # 1 - 0 = 1; the other difference is a half already
    d = cr.round_distances(zh, 0)
    assert d[0] == 0
    assert d[1] == np.float16(np.sqrt(np.float32(2048.0 ** 2 + 2)))
    assert d[2] == np.float16(np.sqrt(np.float32(1.0 + 2.0 ** -22)))
    # difference rounded to half: 2049 is not a half (spacing 2 above 2048) although 2048 and -1 are
    zh2 = np.array([[-1.0, 0.0], [2048.0, 0.0]], np.float16)
    assert cr.round_distances(zh2, 0)[1] == np.float16(2048.0)


def test_first_argmax_duplicates_and_exhaustion():
    """Equal running minima go to the lowest row, and once every minimum is 0 (all distinct rows taken) the pick is row 0 again."""
    z = np.array([[0, 0], [3, 0], [3, 0], [0, 3], [0, 0]], np.float32)
    picks = cr.greedy_fp16(z, 5)
    assert picks.tolist() == [0, 1, 3, 0, 0]


def test_odd_dimension_is_zero_padded():
    g = np.random.default_rng(3)
    z = g.standard_normal((50, 7)).astype(np.float32)
    zp = np.concatenate([z, np.zeros((50, 1), np.float32)], 1)
    np.testing.assert_array_equal(cr.greedy_fp16(z, 20), cr.greedy_fp16(zp, 20))


def test_midpoint_margin_and_snapping():
    # 1 + 2^-11 is the midpoint between the halves 1 and 1 + 2^-10
    m = cr.midpoint_margin(np.array([1.0 + 2.0 ** -11, 1.0, 0.0, 1.0 + 2.0 ** -11 + 1e-4]))
    assert m[0] == 0 and abs(m[1] - 2.0 ** -11) < 1e-6 and np.isinf(m[2]) and abs(m[3] - 1e-4) < 1e-6
    g = np.random.default_rng(5)
    z = g.standard_normal((2000, 62)).astype(np.float32)
    z[100:110] = z[99]
    z[500] = z[0]
    assert cr.midpoint_margin(cr.initial_distances64(z)).min() < 1e-5          # random rows: some row sits next to a midpoint
    zs = cr.snap_initial_distances(z)
    d = cr.initial_distances64(zs)
    assert cr.midpoint_margin(d).min() > 2e-4                                  # half an fp16 spacing is >= 2^-12 relative
    assert np.array_equal(zs[0], z[0]) and np.array_equal(zs[500], z[0]) and all(np.array_equal(zs[i], zs[99]) for i in range(100, 110))
    # the rescaling is a relative change below half an fp16 spacing per row
    assert np.abs(d / cr.initial_distances64(z)[None][0].clip(1e-30) - 1)[d > 0].max() < 2.0 ** -11 + 1e-6
