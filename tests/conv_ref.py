"""Float64 references, in numpy only, of the kernels behind the distillation heads and the ViT / score-map plumbing:
cmdiad_conv2d_nhwc_bf16, cmdiad_upsample_bicubic, cmdiad_bilinear_up, cmdiad_layernorm.  Written from the definitions (no torch
operator is called), so tests/test_conv_ref_cpu.py can pin them to torch's float64 operators as an independent implementation, and
tests/test_gpu_conv_edges.py / tests/test_gpu_layernorm.py hold the HIP kernels to them.

Besides the value every reference returns the magnitude sum its error bound is stated in (sum |terms|), and this module owns the
operand generators of the EXACT convolution cases (small integers, one-hot weights), so the CPU test checks the preconditions of
exactly the data the GPU test runs."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_RELU_POST = 0, 2, 3      # cmdiad_amd.ops.ACT_* (the GPU test asserts they are the same numbers)


# ------------------------------------------------------------------------------------------------ convolution
def conv_out_size(n, ksize, stride):
    pad = 1 if ksize == 3 else 0
    return (n + 2 * pad - ksize) // stride + 1


def conv2d_nhwc(x, w_packed, N, ksize=3, stride=1, bias=None, act=ACT_NONE, residual=None):
    """x [B,H,W,C], w_packed [N, ksize*ksize*C] (or [N, tap, C]), tap-major, tap = ky * ksize + kx; padding 1 for 3 x 3, 0 for 1 x 1.
    out[b,yo,xo,n] = sum_{ky,kx,c} x[b, yo*s + ky - p, xo*s + kx - p, c] * w[n, ky*k + kx, c]  (pixels outside the image are zero),
    then + bias, ReLU (ACT_RELU), + residual, ReLU (ACT_RELU_POST).
    -> (out [B,Ho,Wo,N] float64, sum_abs [B,Ho,Wo,N] = sum |x||w| + |bias| + |residual|)."""
    x = np.asarray(x, dtype=np.float64)
    B, H, W, C = x.shape
    taps = ksize * ksize
    w = np.asarray(w_packed, dtype=np.float64).reshape(N, taps, C)
    pad = 1 if ksize == 3 else 0
    Ho, Wo = conv_out_size(H, ksize, stride), conv_out_size(W, ksize, stride)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
    xp[:, pad:pad + H, pad:pad + W] = x
    out = np.zeros((B, Ho, Wo, N))
    mag = np.zeros((B, Ho, Wo, N))
    for ky in range(ksize):
        for kx in range(ksize):
            win = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]     # [B,Ho,Wo,C]
            wt = w[:, ky * ksize + kx]                                                                  # [N,C]
            out += win @ wt.T
            mag += np.abs(win) @ np.abs(wt).T
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        out = out + b
        mag = mag + np.abs(b)
    if act == ACT_RELU:
        out = np.maximum(out, 0.0)
    if residual is not None:
        r = np.asarray(residual, dtype=np.float64)
        out = out + r
        mag = mag + np.abs(r)
    if act == ACT_RELU_POST:
        out = np.maximum(out, 0.0)
    return out, mag


def shifted_input(x, tap, stride):
    """What a 3 x 3 / padding 1 convolution whose only non-zero weight sits on `tap` reads: out[b,yo,xo,c] =
    x[b, yo*s + ky - 1, xo*s + kx - 1, c], zero outside the image.  Plain indexing, independent of conv2d_nhwc."""
    x = np.asarray(x)
    B, H, W, C = x.shape
    ky, kx = divmod(tap, 3)
    Ho, Wo = conv_out_size(H, 3, stride), conv_out_size(W, 3, stride)
    out = np.zeros((B, Ho, Wo, C), dtype=x.dtype)
    for yo in range(Ho):
        y = yo * stride + ky - 1
        if not 0 <= y < H:
            continue
        for xo in range(Wo):
            xx = xo * stride + kx - 1
            if 0 <= xx < W:
                out[:, yo, xo] = x[:, y, xx]
    return out


# (B, H, W, C, N, ksize, stride): the geometries of the exact cases
EXACT_GEOMS = [
    (2, 31, 23, 64, 68, 3, 2),      # stride 2, odd H and W: the bottom / right padding is read
    (1, 1, 1, 64, 4, 3, 1),         # image smaller than the window
    (1, 2, 1, 128, 8, 3, 2),        # image smaller than the window, stride 2
    (3, 1, 7, 64, 12, 3, 2),        # H = 1 at stride 2
    (1, 2, 2, 64, 4, 3, 2),         # H = W = 2 at stride 2
    (5, 7, 5, 192, 132, 3, 1),      # 175 rows: the second 128-row tile starts mid-image, ragged last tile, two N tiles
    (2, 9, 9, 320, 260, 3, 1),      # kt_per_tap = 5, three N tiles
    (2, 5, 3, 64, 4, 1, 1),         # 1 x 1 at C = 64
    (1, 12, 12, 64, 96, 3, 2),      # stride 2 at C = 64
]


def exact_case(geom, seed=0):
    """Integer operands of an exact case: x in [-4, 4], w in [-2, 2], bias and residual in [-64, 64] (all exact in bf16; every
    partial sum of the convolution is an integer of magnitude <= 8 * 9 * 320 + 128 < 2^24, so exact in fp32 in any order).
    -> x [B,H,W,C], w [N, taps*C], bias [N], residual [B,Ho,Wo,N], float64 arrays holding integers."""
    B, H, W, C, N, ks, stride = geom
    g = np.random.default_rng(1000 + seed + 7 * H + 13 * W + C + N)
    Ho, Wo = conv_out_size(H, ks, stride), conv_out_size(W, ks, stride)
    x = g.integers(-4, 5, (B, H, W, C)).astype(np.float64)
    w = g.integers(-2, 3, (N, ks * ks * C)).astype(np.float64)
    bias = g.integers(-64, 65, (N,)).astype(np.float64)
    residual = g.integers(-64, 65, (B, Ho, Wo, N)).astype(np.float64)
    return x, w, bias, residual


ONEHOT_C, ONEHOT_N = 192, 8
# one input channel per output: both ends of every 64-channel chunk (K-step), and two inner ones
ONEHOT_CHANNELS = [0, 63, 64, 127, 128, 191, 1, 100]


def onehot_weights(tap):
    """w [N, 9, C] with w[n, tap, ONEHOT_CHANNELS[n]] = 1 and zero elsewhere."""
    w = np.zeros((ONEHOT_N, 9, ONEHOT_C))
    for n, c in enumerate(ONEHOT_CHANNELS):
        w[n, tap, c] = 1.0
    return w


def onehot_input(B=2, H=7, W=5, seed=3):
    """Integers in [-127, 127] (exact in bf16), an image with odd sides."""
    return np.random.default_rng(seed).integers(-127, 128, (B, H, W, ONEHOT_C)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ resizes
def source_coords(out_n, in_n, fma=False):
    """src = (dst + 0.5) * in/out - 0.5 for dst = 0..out_n-1 in fp32, as ATen and the kernels compute it: the scale is the fp32
    quotient, dst + 0.5 is exact.  fma=False rounds the product and the difference separately (ATen's CPU kernels); fma=True rounds
    once (what a compiler that contracts a * b - c into one fused multiply-add produces).  The two differ only when in/out is not
    exact in fp32."""
    scale = np.float32(in_n) / np.float32(out_n)
    d = np.arange(out_n, dtype=np.float32) + np.float32(0.5)
    if fma:     # the product of two fp32 numbers and its difference with 0.5 are exact in float64: one rounding
        return (scale.astype(np.float64) * d.astype(np.float64) - 0.5).astype(np.float32)
    return scale * d - np.float32(0.5)


CUBIC_A = -0.75
# (h, w, H, W): downscale, h or w of 1 or 2 (the clamped taps collapse), identity, exact 4x -- shared by the CPU and GPU tests
BICUBIC_GEOMS = [(9, 7, 4, 3), (1, 5, 4, 20), (5, 1, 7, 3), (2, 2, 8, 8), (6, 5, 6, 5), (3, 4, 12, 16)]
BILINEAR_IN = [1, 2, 7, 37, 56]


def bilinear_out_sizes(h):
    """224 (production), 5, the identity, half the size."""
    return sorted({224, 5, h, max(1, h // 2)})


def cubic_weights(t):
    """Keys' cubic convolution weights of the four taps floor-1 .. floor+2 at fraction t (float64), A = -0.75."""
    A = CUBIC_A
    t = np.asarray(t, dtype=np.float64)
    x0, x2, x3 = t + 1.0, 1.0 - t, 2.0 - t
    return np.stack([((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A,
                     ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0,
                     ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0,
                     ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A])


def _cubic_axis(out_n, in_n, fma):
    src = source_coords(out_n, in_n, fma)
    fl = np.floor(src)
    t = src.astype(np.float64) - fl.astype(np.float64)              # exact (also in fp32)
    idx = np.clip(fl.astype(np.int64)[None] + np.arange(-1, 3)[:, None], 0, in_n - 1)      # [4, out_n], clamped to the image
    return cubic_weights(t), idx


def bicubic(x_nhwc, H, W, fma=False):
    """torch.nn.functional.interpolate(mode='bicubic', align_corners=False) of x [B,h,w,C] to [B,H,W,C]: coordinates in fp32
    (source_coords), weights and blend in float64.
    -> (out, wsum) with wsum = sum over the 16 taps of (|wy| + |wx| + |wy||wx|) |value|: the magnitude the fp32 error bound of the
    kernels is stated in (an ABSOLUTE error of the weights -- the outer ones come out of cancelling terms of size 3..6 -- and a
    relative one of the blend)."""
    x = np.asarray(x_nhwc, dtype=np.float64)
    B, h, w, C = x.shape
    wy, iy = _cubic_axis(H, h, fma)
    wx, ix = _cubic_axis(W, w, fma)
    out = np.zeros((B, H, W, C))
    wsum = np.zeros((B, H, W, C))
    for a in range(4):
        rows = x[:, iy[a]]                                          # [B,H,w,C]
        for e in range(4):
            v = rows[:, :, ix[e]]                                   # [B,H,W,C]
            wa, we = wy[a][None, :, None, None], wx[e][None, None, :, None]
            out += wa * we * v
            wsum += (np.abs(wa) + np.abs(we) + np.abs(wa * we)) * np.abs(v)
    return out, wsum


def bilinear(x, H, fma=False):
    """ATen's upsample_bilinear2d, align_corners=False, of square maps x [B,h,h] to [B,H,H]: src = max(scale * (dst + 0.5) - 0.5, 0)
    in fp32, i0 = int(src), i1 = i0 + (i0 < h - 1), l = src - i0; the blend in float64."""
    x = np.asarray(x, dtype=np.float64)
    B, h, _ = x.shape
    src = np.maximum(source_coords(H, h, fma), np.float32(0.0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < h - 1)
    l1 = src.astype(np.float64) - i0
    l0 = 1.0 - l1
    rows = l0[None, :, None] * x[:, i0] + l1[None, :, None] * x[:, i1]                   # [B,H,h]
    return l0[None, None, :] * rows[:, :, i0] + l1[None, None, :] * rows[:, :, i1]        # [B,H,H]


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm(x, gamma, beta, eps):
    """-> (y, mean, rstd) in float64: y = (x - mean) * rstd * gamma + beta, biased variance, rstd = 1 / sqrt(var + eps)."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None] * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
    return y, mean, rstd
