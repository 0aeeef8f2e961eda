"""CPU: the float64 restatement of the point-cloud -> patch-grid chain (tests/patch_ref.py) against torch's own fp32 operators in the
reference's composition (oracle.scoring.get_xyz_patch) and against the C oracle (oracle.kernels.interp3nn / xyz_patch), at one small
case -- the proof of the yardstick that tests/test_gpu_patch_path.py holds the HIP kernels to.  No GPU.

Both comparands are fp32, so they agree with float64 to fp32 round-off only: 1e-5 relative to the absolute sum A that
patch_ref returns (A >= |value|; a sum of ~150 fp32 terms is within ~150 * 2^-24 = 9e-6 of A in the worst case)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_ref as pr  # noqa: E402
from oracle import kernels as ok  # noqa: E402
from oracle import scoring  # noqa: E402

SIZE, S, D = 40, 24, 8


def _case():
    pcs, cen, feat = pr.synth_batch(1, SIZE, S, D, seed=3)
    pc, nz = scoring.unorganize_no_zeros(pcs[0:1])
    xyz = np.ascontiguousarray(pc[0].T.numpy())
    out32, idx3, w3 = ok.interp3nn(xyz, cen[0].numpy(), feat[0].numpy())
    pix2pt = np.full(SIZE * SIZE, -1, np.int64)
    pix2pt[nz] = np.arange(len(nz))
    assert 0 < len(nz) < SIZE * SIZE
    return feat[0].numpy(), idx3, w3, pix2pt, nz, out32


def test_gather_against_the_oracle():
    feat, idx3, w3, _, _, out32 = _case()
    val, ab = pr.interp_gather(feat, idx3, w3)
    assert np.all(np.abs(val.numpy() - out32) <= 1e-5 * ab.numpy())
    assert np.all(ab.numpy() >= np.abs(val.numpy()))


def test_patch_against_torch_fp32_and_the_oracle():
    feat, idx3, w3, pix2pt, nz, out32 = _case()
    for P in (10, 7, 38, 48):                      # bins of 3-4 and 5-6 rows, P = size - 2 (bins of one), P > size - 2 (overlapping)
        ref, A, n_e = pr.xyz_patch(feat, idx3, w3, pix2pt, SIZE, P)
        assert ref.shape == (P * P, D) and A.shape == ref.shape and n_e.shape == (P * P,)
        t32 = scoring.get_xyz_patch(torch.from_numpy(out32.T.copy())[None], nz, SIZE, P).numpy()
        assert np.all(np.abs(ref - t32) <= 1e-5 * A + 1e-30)
        c32 = ok.xyz_patch(out32, nz, SIZE, P)
        assert np.all(np.abs(ref - c32) <= 1e-5 * A + 1e-30)
        refn, An, _ = pr.xyz_patch(feat, idx3, w3, pix2pt, SIZE, P, mean=0.25, inv_std=1 / 1.7)
        np.testing.assert_allclose(refn, (ref - 0.25) / 1.7, rtol=1e-14, atol=1e-15)
        assert np.array_equal(An, A)


def test_absolute_sum_and_footprint_by_hand():
    """size 5, P 1: the 3 x 3 pooled map is averaged whole, so pixel (Y, X) has coefficient cy * cx / 81 with cy, cx = 1, 2, 3, 2, 1."""
    size, P = 5, 1
    feat = np.array([[2.0], [-3.0]], np.float32)
    idx3 = np.array([[0, 1, 0]], np.int32)
    w3 = np.array([[0.5, 0.25, 0.25]], np.float32)
    pix2pt = np.full(25, -1)
    pix2pt[1 * 5 + 2] = 0                                  # Y = 1 (cy = 2), X = 2 (cx = 3)
    ref, A, n_e = pr.xyz_patch(feat, idx3, w3, pix2pt, size, P)
    assert n_e.tolist() == [75]
    np.testing.assert_allclose(ref, [[6 / 81 * (0.5 * 2 - 0.25 * 3 + 0.25 * 2)]], rtol=1e-15)
    np.testing.assert_allclose(A, [[6 / 81 * (0.5 * 2 + 0.25 * 3 + 0.25 * 2)]], rtol=1e-15)
    y0, y1, x0, x1 = pr.footprint_windows(224, 56)
    assert (y0[0], y1[0], x0[57], x1[57]) == (0, 6, 3, 10) and pr.footprint_entries(224, 56).max() == 3 * 7 * 7
    assert pr.footprint_entries(96, 12).max() == 363 and pr.footprint_entries(224, 14).max() == 3 * 19 * 19


def test_synth_batch_is_ragged_with_a_nearly_empty_and_a_full_cloud():
    pcs, cen, feat = pr.synth_batch(11, 10, 8, 4, seed=1)
    n = [(pcs[b] != 0).all(0).sum().item() for b in range(11)]
    assert n[1] == 5 and n[2] == 100 and len(set(n)) >= 9 and min(n) >= 1
    assert cen.shape == (11, 8, 3) and feat.shape == (11, 8, 4)
