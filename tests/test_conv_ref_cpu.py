"""CPU: the float64 numpy references of tests/conv_ref.py against torch's float64 operators (F.conv2d, F.interpolate,
F.layer_norm) -- an independent implementation each, so the yardstick that tests/test_gpu_conv_edges.py and
tests/test_gpu_layernorm.py hold the HIP kernels to is itself pinned.  Also the preconditions of the GPU tests' exact cases, on
the very operands those tests run.  No GPU, no cmdiad_amd import."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402


def _torch_conv(x, w, N, ks, stride, bias, act, residual):
    C = x.shape[-1]
    wt = torch.from_numpy(w).reshape(N, ks, ks, C).permute(0, 3, 1, 2)
    y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), wt, torch.from_numpy(bias) if bias is not None else None,
                 stride=stride, padding=1 if ks == 3 else 0).permute(0, 2, 3, 1)
    if act == cr.ACT_RELU:
        y = y.relu()
    if residual is not None:
        y = y + torch.from_numpy(residual)
    if act == cr.ACT_RELU_POST:
        y = y.relu()
    return y.numpy()


@pytest.mark.parametrize("B,H,W,C,N,ks,stride,act,res", [
    (2, 9, 7, 8, 5, 3, 2, cr.ACT_NONE, False),          # stride 2, odd H and W
    (1, 1, 6, 4, 3, 3, 1, cr.ACT_RELU, True),           # H = 1
    (2, 5, 2, 4, 6, 3, 2, cr.ACT_RELU_POST, True),      # W = 2 at stride 2
    (1, 2, 2, 3, 2, 3, 2, cr.ACT_RELU, False),          # smaller than the window
    (2, 6, 8, 8, 4, 3, 1, cr.ACT_RELU_POST, False),     # stride 1, even sides
    (3, 4, 5, 16, 7, 1, 1, cr.ACT_RELU, True),          # 1 x 1
])
def test_conv2d_nhwc_equals_torch_float64(B, H, W, C, N, ks, stride, act, res):
    g = np.random.default_rng(H * 100 + W)
    x = g.standard_normal((B, H, W, C))
    w = g.standard_normal((N, ks * ks * C))
    bias = g.standard_normal(N)
    Ho, Wo = cr.conv_out_size(H, ks, stride), cr.conv_out_size(W, ks, stride)
    residual = g.standard_normal((B, Ho, Wo, N)) if res else None
    got, mag = cr.conv2d_nhwc(x, w, N, ks, stride, bias, act, residual)
    want = _torch_conv(x, w, N, ks, stride, bias, act, residual)
    assert got.shape == want.shape == (B, Ho, Wo, N)
    assert np.abs(got - want).max() <= 1e-12        # float64 sums of <= 145 terms of size ~1: round-off is ~1e-15
    # sum_abs is the same convolution of the absolute values
    want_mag = _torch_conv(np.abs(x), np.abs(w), N, ks, stride, np.abs(bias), cr.ACT_NONE, np.abs(residual) if res else None)
    assert np.abs(mag - want_mag).max() <= 1e-12
    assert (np.abs(got) <= mag + 1e-12).all()


@pytest.mark.parametrize("geom", cr.EXACT_GEOMS)
def test_exact_cases_meet_their_preconditions(geom):
    """What makes the GPU's exact cases exact: bf16 holds every operand, every partial sum in any order is an integer below 2^24
    (sum_abs bounds them all), and the float64 reference equals torch's."""
    B, H, W, C, N, ks, stride = geom
    x, w, bias, residual = cr.exact_case(geom)
    for a in (x, w, bias, residual):
        assert np.array_equal(a, np.round(a))
        assert torch.equal(torch.from_numpy(a).to(torch.bfloat16).double(), torch.from_numpy(a))
    assert np.abs(x).max() == 4 and np.abs(w).max() == 2
    for act in (cr.ACT_NONE, cr.ACT_RELU, cr.ACT_RELU_POST):
        got, mag = cr.conv2d_nhwc(x, w, N, ks, stride, bias, act, residual)
        assert mag.max() < 2 ** 24
        assert np.array_equal(got, np.round(got))
        assert np.array_equal(got, _torch_conv(x, w, N, ks, stride, bias, act, residual))
    # the cases are not degenerate: the ReLU forms clip something wherever there is more than a handful of outputs
    if got.size > 100:
        plain, _ = cr.conv2d_nhwc(x, w, N, ks, stride, bias, cr.ACT_NONE, residual)
        assert (plain < 0).any() and (plain > 0).any()


@pytest.mark.parametrize("stride", [1, 2])
def test_onehot_weights_touch_every_tap_and_shift_the_input(stride):
    x = cr.onehot_input()
    assert torch.equal(torch.from_numpy(x).to(torch.bfloat16).double(), torch.from_numpy(x))
    touched = np.zeros(9, dtype=bool)
    chunks = set()
    for tap in range(9):
        w = cr.onehot_weights(tap)
        assert w.sum() == cr.ONEHOT_N and (w.sum(axis=(1, 2)) == 1).all()
        touched |= w.any(axis=(0, 2))
        assert not w[:, np.arange(9) != tap].any()
        got, _ = cr.conv2d_nhwc(x, w.reshape(cr.ONEHOT_N, -1), cr.ONEHOT_N, 3, stride)
        want = cr.shifted_input(x, tap, stride)[..., cr.ONEHOT_CHANNELS]
        assert np.array_equal(got, want)
        if tap != 4:    # an off-centre tap does fall outside this image somewhere, and the shift is visible
            assert not np.array_equal(got, cr.shifted_input(x, 4, stride)[..., cr.ONEHOT_CHANNELS])
    assert touched.all()
    for c in cr.ONEHOT_CHANNELS:
        chunks.add((c // 64, c % 64))
    for k in range(cr.ONEHOT_C // 64):      # both ends of every 64-channel chunk
        assert (k, 0) in chunks and (k, 63) in chunks


@pytest.mark.parametrize("h,w,H,W", cr.BICUBIC_GEOMS)
@pytest.mark.parametrize("fma", [False, True])
def test_bicubic_equals_torch_float64(h, w, H, W, fma):
    g = np.random.default_rng(h * 10 + w)
    x = g.standard_normal((2, h, w, 3))
    got, wsum = cr.bicubic(x, H, W, fma=fma)
    want = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(H, W), mode="bicubic", align_corners=False)
    want = want.permute(0, 2, 3, 1).numpy()
    # torch computes the coordinate in the tensor's dtype (float64), conv_ref in fp32.  The fp32 coordinate is off by the rounding
    # of the scale (<= in * 2^-24 after the product), of the product and of the difference (<= in * 2^-24 each):
    # <= 1.5 * in * 2^-23.  The interpolant is continuous in the coordinate (also across a change of floor) with, per axis,
    # |d/dsrc| <= sum |w'| * sum |w| * max|x| <= 4.2 * 1.375 * max|x|  (|w0'|, |w3'| <= 0.75, |w1'|, |w2'| <= 1.35; sum |w| <= 1.375,
    # reached at t = 0.5: test_cubic_weights_partition_unity); two axes: <= 11.55 * 1.5 < 18 times max|x| * in * 2^-23.
    tol = 18 * np.abs(x).max() * max(h, w) * 2.0 ** -23
    assert np.abs(got - want).max() <= tol
    assert (np.abs(got) <= wsum).all()
    if (h, w) == (H, W):        # identity: t = 0, weights (0, 1, 0, 0) exactly
        assert np.array_equal(got, x)


def test_cubic_weights_partition_unity():
    t = np.linspace(0.0, 1.0, 257)
    w = cr.cubic_weights(t)
    assert np.abs(w.sum(0) - 1.0).max() <= 1e-15
    assert np.array_equal(cr.cubic_weights(0.0), [0.0, 1.0, 0.0, 0.0])
    assert np.abs(w).sum(0).max() <= 1.375 + 1e-15


@pytest.mark.parametrize("h", cr.BILINEAR_IN)
@pytest.mark.parametrize("fma", [False, True])
def test_bilinear_equals_torch_float64(h, fma):
    g = np.random.default_rng(h)
    x = g.standard_normal((3, h, h))
    for H in cr.bilinear_out_sizes(h):
        got = cr.bilinear(x, H, fma=fma)
        want = F.interpolate(torch.from_numpy(x)[:, None], size=(H, H), mode="bilinear", align_corners=False)[:, 0].numpy()
        # coordinate: fp32 here, float64 in torch, <= 1.5 * h * 2^-23 apart (as for bicubic).  The bilinear interpolant is continuous
        # and piecewise linear with slope <= |p1 - p0| <= 2 max|x| per axis: <= 2 * 2 * 1.5 = 6 times max|x| * h * 2^-23.
        tol = 6 * np.abs(x).max() * h * 2.0 ** -23
        assert np.abs(got - want).max() <= tol, (h, H)
        if H == h:
            assert np.array_equal(got, x)


def test_source_coords_forms_differ_only_for_inexact_scales():
    for out_n, in_n in [(224, 56), (8, 2), (4, 9), (5, 5), (16, 4)]:       # exact quotients: the product is exact, nothing to fuse
        assert np.array_equal(cr.source_coords(out_n, in_n, False), cr.source_coords(out_n, in_n, True))
    a, b = cr.source_coords(224, 37, False), cr.source_coords(224, 37, True)
    assert a.dtype == b.dtype == np.float32
    assert np.abs(a.astype(np.float64) - b).max() <= 37 * 2.0 ** -23 and not np.array_equal(a, b)


@pytest.mark.parametrize("M,C", [(1, 128), (7, 640), (33, 1024)])
def test_layernorm_equals_torch_float64(M, C):
    g = np.random.default_rng(C)
    x = g.standard_normal((M, C)) * 3 + 1
    gamma, beta = g.standard_normal(C), g.standard_normal(C)
    y, mean, rstd = cr.layernorm(x, gamma, beta, 1e-5)
    want = F.layer_norm(torch.from_numpy(x), (C,), torch.from_numpy(gamma), torch.from_numpy(beta), 1e-5).numpy()
    assert np.abs(y - want).max() <= 1e-12
    assert np.abs(mean - x.mean(1)).max() <= 1e-14 and np.abs(rstd - 1 / np.sqrt(x.var(1) + 1e-5)).max() <= 1e-13
