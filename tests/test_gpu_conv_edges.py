"""GPU: cmdiad_conv2d_nhwc_bf16, cmdiad_upsample_bicubic, cmdiad_bilinear_up and the small operators of misc.hip OFF the production
shapes, against the float64 numpy references of tests/conv_ref.py (pinned to torch's float64 operators by
tests/test_conv_ref_cpu.py, which also checks the preconditions of the exact cases on the operands used here).

Convolution: integer operands make every partial sum exact in fp32 whatever the K order, so the borders (stride 2 on odd sides,
images smaller than the window, tiles that start mid-image), the tap decode (kt_per_tap = 1, 3, 5) and the epilogue forms are held
BIT FOR BIT; one-hot weights turn the kernel into a shift of the input, tap by tap.  Resizes: downscale, identity, sizes 1 and 2,
padded channel pitches, both bicubic kernels.  Every tolerance below is zero or derived next to its assertion."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402

from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd._native import NativeError  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24                       # fp32 unit round-off
SENT32 = 0x4B3C5A69                  # sentinel bit patterns (finite, unlike anything the kernels produce here)
SENT16 = 0x5A69
ACTS = [cr.ACT_NONE, cr.ACT_RELU, cr.ACT_RELU_POST]
OUTS = ["f32", "bf16", "both"]


def test_act_codes_match():
    assert (cr.ACT_NONE, cr.ACT_RELU, cr.ACT_RELU_POST) == (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_RELU_POST)


def _sent32(shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device=DEV).view(torch.float32)


def _sent16(shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _is_sent(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32) == SENT32
    return t.contiguous().view(torch.int16) == SENT16


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _rne_bf16(a64):
    """float64 array -> nearest-even bf16 (through fp32; exact for the integers of the exact cases), as a float64 tensor."""
    return torch.from_numpy(np.ascontiguousarray(a64)).float().to(torch.bfloat16).double()


def _conv(x, w, geom, bias, act, residual, outs, pitch=(0, 0, 0), res_pad=0.0):
    """Run the kernel on float64 numpy operands (cast to the kernel's types: x, w bf16; bias, residual f32).  pitch = extra columns
    of (out_f32, out_bf16, residual); buffers are sentinel-filled and returned whole, on the host."""
    B, H, W, C, N, ks, stride = geom
    Ho, Wo = cr.conv_out_size(H, ks, stride), cr.conv_out_size(W, ks, stride)
    o32 = _sent32((B, Ho, Wo, N + pitch[0])) if outs in ("f32", "both") else None
    o16 = _sent16((B, Ho, Wo, N + pitch[1])) if outs in ("bf16", "both") else None
    r = None
    if residual is not None:
        r = torch.full((B, Ho, Wo, N + pitch[2]), res_pad, dtype=torch.float32)
        r[..., :N] = torch.from_numpy(residual).float()
        r = r.to(DEV)
    ops.conv2d_nhwc(_dev(x, torch.bfloat16), _dev(w, torch.bfloat16), N, ks, stride, bias=_dev(bias, torch.float32) if bias is not None else None,
                    act=act, residual=r, out_f32=o32, out_bf16=o16, want_f32=False, want_bf16=False)
    torch.cuda.synchronize()
    return (o32.cpu() if o32 is not None else None), (o16.cpu() if o16 is not None else None)


def _assert_exact(o32, o16, ref, N, what):
    if o32 is not None:
        assert not _is_sent(o32[..., :N]).any(), what
        bad = o32[..., :N].double() != torch.from_numpy(ref)
        assert not bad.any(), (what, "f32", int(bad.sum()), bad.nonzero()[:4].tolist())
    if o16 is not None:
        assert not _is_sent(o16[..., :N]).any(), what
        bad = o16[..., :N].double() != _rne_bf16(ref)
        assert not bad.any(), (what, "bf16", int(bad.sum()), bad.nonzero()[:4].tolist())


# a full cross of the epilogue forms on the two geometries with the most border and tile structure, one form on each of the rest
_FULL = [cr.EXACT_GEOMS[0], cr.EXACT_GEOMS[5]]
_EXACT_CASES = [(g, a, r, o) for g in _FULL for a in ACTS for r in (False, True) for o in OUTS]
_EXACT_CASES += [(g, ACTS[i % 3], i % 2 == 0, OUTS[(i // 3 + i) % 3]) for i, g in enumerate(cr.EXACT_GEOMS) if g not in _FULL]


@pytest.mark.parametrize("geom,act,res,outs", _EXACT_CASES)
def test_conv2d_exact_integer_cases(geom, act, res, outs):
    """x in [-4, 4], w in [-2, 2], integer bias / residual: all exact in bf16, every partial sum an integer below 2^24 (checked on
    these operands by test_conv_ref_cpu.py), so the f32 output equals the float64 reference and the bf16 output is its RNE cast --
    no tolerance: a border row that reads one wrong pixel is off by a whole integer."""
    x, w, bias, residual = cr.exact_case(geom)
    ref, _ = cr.conv2d_nhwc(x, w, geom[4], geom[5], geom[6], bias, act, residual if res else None)
    o32, o16 = _conv(x, w, geom, bias, act, residual if res else None, outs)
    assert (o32 is not None) == (outs != "bf16") and (o16 is not None) == (outs != "f32")
    _assert_exact(o32, o16, ref, geom[4], (geom, act, res, outs))


@pytest.mark.parametrize("stride", [1, 2])
def test_conv2d_onehot_tap_is_a_shift_of_the_input(stride):
    """w[n, tap, c_n] = 1 only: output channel n IS input channel c_n shifted by the tap, zero where the tap leaves the image.  c_n
    covers both ends of every 64-channel K-step (C = 192: kt_per_tap = 3); the image has odd sides (7 x 5)."""
    x = cr.onehot_input()
    geom = (x.shape[0], x.shape[1], x.shape[2], cr.ONEHOT_C, cr.ONEHOT_N, 3, stride)
    for tap in range(9):
        want = cr.shifted_input(x, tap, stride)[..., cr.ONEHOT_CHANNELS]
        o32, o16 = _conv(x, cr.onehot_weights(tap).reshape(cr.ONEHOT_N, -1), geom, None, cr.ACT_NONE, None, "both")
        _assert_exact(o32, o16, want, cr.ONEHOT_N, ("tap", tap, "stride", stride))


@pytest.mark.parametrize("geom", _FULL)
def test_conv2d_strided_epilogue_operands(geom):
    """ldo32, ldo16 and ldr larger than N (and different from each other): columns 0..N equal the exact reference, columns N..ld of
    both outputs keep their bits, and the residual's padding columns hold 1e30 so a read with the wrong pitch cannot hide."""
    N = geom[4]
    x, w, bias, residual = cr.exact_case(geom, seed=1)
    ref, _ = cr.conv2d_nhwc(x, w, N, geom[5], geom[6], bias, cr.ACT_RELU_POST, residual)
    o32, o16 = _conv(x, w, geom, bias, cr.ACT_RELU_POST, residual, "both", pitch=(4, 8, 12), res_pad=1e30)
    assert o32.shape[-1] == N + 4 and o16.shape[-1] == N + 8
    assert _is_sent(o32[..., N:]).all() and _is_sent(o16[..., N:]).all()
    _assert_exact(o32, o16, ref, N, geom)


@pytest.mark.parametrize("i,geom", list(enumerate(cr.EXACT_GEOMS)))
def test_conv2d_random_operands_vs_float64(i, geom):
    """Random operands pre-rounded to bf16 at the edge geometries, against float64.  The bound is the worst case of a length-9C fp32
    sum in ANY order plus the epilogue's four roundings, |err| <= (9C + 4) 2^-24 sum(|x||w| + |bias| + |residual|): derived and valid
    whatever the K order, but LOOSE (the typical error is ~sqrt(9C) 2^-24 of the output scale) -- a tap or border mistake is caught
    by the exact cases above, not by this one; this one covers non-integer magnitudes and the bf16 rounding of the output.
    bf16 output: the RNE cast of an fp32 value inside that bound, i.e. between the casts of ref -/+ bound (rounding is monotonic) --
    the sharper form of 'within one bf16 step of the reference plus the bound'."""
    B, H, W, C, N, ks, stride = geom
    g = np.random.default_rng(50 + i)
    Ho, Wo = cr.conv_out_size(H, ks, stride), cr.conv_out_size(W, ks, stride)
    bf = lambda a: torch.from_numpy(a).float().to(torch.bfloat16).double().numpy()      # noqa: E731
    x = bf(g.standard_normal((B, H, W, C)))
    w = bf(g.standard_normal((N, ks * ks * C)) / np.sqrt(ks * ks * C))
    bias = g.standard_normal(N).astype(np.float32).astype(np.float64)
    residual = g.standard_normal((B, Ho, Wo, N)).astype(np.float32).astype(np.float64) if i % 2 == 0 else None
    act = ACTS[i % 3]
    ref, mag = cr.conv2d_nhwc(x, w, N, ks, stride, bias, act, residual)
    o32, o16 = _conv(x, w, geom, bias, act, residual, "both")
    bound = (9 * C + 4) * U * mag
    err = np.abs(o32.double().numpy() - ref)
    print(f"conv {geom}: max err / bound = {(err / bound).max():.3e}, max err {err.max():.3e}")
    assert (err <= bound).all(), (geom, float((err / bound).max()))
    lo, hi = _rne_bf16(ref - bound), _rne_bf16(ref + bound)
    got = o16.double()
    assert ((lo <= got) & (got <= hi)).all(), geom


@pytest.mark.parametrize("what", ["stride3", "1x1-stride2", "N%4", "misaligned-out"])
def test_conv2d_argument_errors_leave_the_output_alone(what):
    B, H, W, C, N, ks, stride = 1, 5, 5, 64, 8, 3, 1
    out32, out16 = _sent32((B * H * W * N + 4,)), _sent16((B, H, W, N))
    o32 = out32[:B * H * W * N].view(B, H, W, N)
    match = "3x3"
    if what == "stride3":
        stride = 3
    elif what == "1x1-stride2":
        ks, stride = 1, 2
    elif what == "N%4":
        N, match = 6, "N%4"
        o32, out16 = out32[:B * H * W * N].view(B, H, W, N), _sent16((B, H, W, N))
    else:
        o32, match = out32[1:1 + B * H * W * N].view(B, H, W, N), "alignment"      # 4 bytes off a 16-byte boundary
    x = torch.ones(B, H, W, C, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(N, ks * ks * C, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(NativeError, match=match):
        ops.conv2d_nhwc(x, w, N, ks, stride, out_f32=o32, out_bf16=out16, want_f32=False, want_bf16=False)
    torch.cuda.synchronize()
    assert _is_sent(out32).all() and _is_sent(out16).all()


# ------------------------------------------------------------------------------------------------ bicubic
# Error of the kernels' fp32 arithmetic against conv_ref.bicubic (same fp32 coordinate, float64 weights and blend), per output:
#   weights: w0 / w3 are Horner forms in x = 1 + t (or 2 - t) in [1, 2] whose intermediates are A x (<= 1.5), .. - 5A (<= 3),
#   .. * x (<= 4.5), .. + 8A (<= 3), .. * x (<= 3.1), .. - 4A (<= 0.15); a rounding of an intermediate is carried through the later
#   multiplications by x <= 2: (1.5 + 3) * 4 + (4.5 + 3) * 2 + 3.1 + 0.15 < 37 units of 2^-24, plus the rounding of x itself
#   (|w'| <= 0.75, x <= 2: 1.5) -- < 38 * 2^-24 ABSOLUTE (the result is ~0.1 out of terms of 3..6, so no relative bound exists);
#   w1 / w2 stay below 11 the same way.  (With fused multiply-adds it is half of that; the bound holds either way.)
#   blend: a value passes a product and up to four additions on each of the two levels: 10 roundings, relative.
# => |err| <= 2^-24 * sum_taps (38 |wx| + 38 |wy| + 10 |wy||wx|) |v| <= 38 * 2^-24 * wsum, wsum = sum (|wy| + |wx| + |wy||wx|) |v| as
# conv_ref.bicubic returns it.  The bicubic4x kernel evaluates the same weight forms at its four constant phases and the same
# two-level blend: the same count.
BICUBIC_C = 38
# The coordinate (dst + 0.5) * scale - 0.5 is either two fp32 roundings or one fused multiply-add (the kernel library compiles these
# files with contraction allowed); conv_ref computes both and the kernel must agree with ONE of them at every element.  They differ
# only where in/out is not exact in fp32 (here 7/3, 5/7, 1/3).


def _within_one_form(check, refs, what):
    fails = [check(*r) for r in refs]
    assert any(f is None for f in fails), (what, fails)


@pytest.mark.parametrize("h,w,H,W", cr.BICUBIC_GEOMS)
@pytest.mark.parametrize("C", [1, 4, 6, 8])
@pytest.mark.parametrize("pad", [0, 4])
def test_bicubic_edges_vs_float64(h, w, H, W, C, pad):
    """Downscale, h or w of 1 or 2, identity and exact 4x; C with and without a ragged last group of four; ldi = C rounded up to 4
    (+ 4), the padding channels hold 1e30 so a stray read shows.  f32 NCHW (always the generic kernel) and bf16 NHWC (the 4x block
    kernel when the ratio is exactly 4 and C % 4 == 0, the generic one otherwise -- C = 6 at 4x) against the same reference."""
    B = 2
    ldi = (C + 3) // 4 * 4 + pad
    ldo = (C + 3) // 4 * 4 + 4
    g = np.random.default_rng(h * 100 + w * 10 + C)
    x = np.full((B, h, w, ldi), 1e30, dtype=np.float32)
    x[..., :C] = g.standard_normal((B, h, w, C)).astype(np.float32)
    dx = torch.from_numpy(x).to(DEV)
    got32 = ops.upsample_bicubic(dx, C, H, W, nchw=True).cpu().permute(0, 2, 3, 1).double().numpy()
    out16 = _sent16((B, H, W, ldo))
    ops.upsample_bicubic(dx, C, H, W, out_bf16=out16)
    torch.cuda.synchronize()
    out16 = out16.cpu()
    assert _is_sent(out16[..., C:]).all() and not _is_sent(out16[..., :C]).any()       # columns C..ldo untouched
    got16 = out16[..., :C].double()
    refs = [cr.bicubic(x[..., :C], H, W, fma=f) for f in (False, True)]

    def check32(ref, wsum):
        bad = np.abs(got32 - ref) > BICUBIC_C * U * wsum
        return None if not bad.any() else float((np.abs(got32 - ref) / (BICUBIC_C * U * wsum + 1e-300)).max())

    def check16(ref, wsum):     # the RNE cast of an fp32 value within the bound of ref (rounding is monotonic)
        b = BICUBIC_C * U * wsum
        ok = (_rne_bf16(ref - b) <= got16) & (got16 <= _rne_bf16(ref + b))
        return None if ok.all() else int((~ok).sum())

    _within_one_form(check32, refs, ("f32", h, w, H, W, C, ldi))
    _within_one_form(check16, refs, ("bf16", h, w, H, W, C, ldi))
    if (h, w) == (H, W):        # identity: t = 0, the weights are (0, 1, 0, 0) exactly in fp32 as well
        assert np.array_equal(got32, x[..., :C].astype(np.float64))
        assert torch.equal(got16, _rne_bf16(x[..., :C].astype(np.float64)))


@pytest.mark.parametrize("h,w", [(1, 5), (2, 2), (3, 4)])
def test_bicubic_block_kernel_agrees_with_generic_kernel(h, w):
    """C = 8 at exactly 4x: the bf16 NHWC output comes from bicubic4x_kernel, the f32 NCHW output of the same data from the generic
    kernel.  The bf16 values are within one bf16 step of the float64 reference (asserted) and the cast of an fp32 value within the
    two kernels' joint bound of the generic kernel's result (asserted); the share that is not the NEAREST bf16 of the reference is
    reported (it is the share of values that sit within ~1e-6 of a rounding boundary)."""
    B, C, H, W = 3, 8, 4 * h, 4 * w
    x = np.random.default_rng(h + w).standard_normal((B, h, w, C)).astype(np.float32)
    dx = torch.from_numpy(x).to(DEV)
    gen32 = ops.upsample_bicubic(dx, C, H, W, nchw=True).cpu().permute(0, 2, 3, 1).double()
    blk16 = ops.upsample_bicubic(dx, C, H, W).cpu().double()
    ref, wsum = cr.bicubic(x, H, W)         # 4x: the scale 0.25 is exact, both coordinate forms coincide
    ref = torch.from_numpy(ref)
    nearest = _rne_bf16(ref.numpy())
    step = torch.exp2(torch.floor(torch.log2(nearest.abs().clamp_min(1e-37))) - 7.0)      # the bf16 step at the exact value
    assert ((blk16 - ref).abs() <= step).all()
    print(f"bicubic4x {h}x{w}: share of bf16 values that are not the nearest to float64 = {float((blk16 != nearest).double().mean()):.2e}")
    b = torch.from_numpy(2 * BICUBIC_C * U * wsum)                                       # each kernel is within BICUBIC_C U wsum of ref
    assert ((_rne_bf16((gen32 - b).numpy()) <= blk16) & (blk16 <= _rne_bf16((gen32 + b).numpy()))).all()


# ------------------------------------------------------------------------------------------------ bilinear
@pytest.mark.parametrize("h", cr.BILINEAR_IN)
def test_bilinear_edges_vs_float64(h):
    """h in {1, 2, 7, 37, 56} to H in {224, 5, h, h // 2}, B in {1, 3}.  The kernel's seven fp32 operations per output -- 1 - l on
    each axis, then product, sum, product, sum on the path of each of the four values: at most six roundings on any path, all
    relative, on a convex combination (the weights sum to 1 before the rounding of 1 - l, to <= 1 + 2^-24 after) -- give
    |err| <= 7 * 2^-24 * max|in|.  Coordinates: one of conv_ref's two fp32 forms (see the bicubic note).  The identity size
    returns the input exactly (l = 0, so 1 * (1 * p + 0 * p') + 0 * .. = p)."""
    for B in (1, 3):
        x = np.random.default_rng(h + B).standard_normal((B, h, h)).astype(np.float32)
        for H in cr.bilinear_out_sizes(h):
            got = ops.bilinear_up(torch.from_numpy(x).to(DEV), H).cpu().double().numpy()
            assert got.shape == (B, H, H)
            tol = 7 * U * np.abs(x).max()
            errs = [np.abs(got - cr.bilinear(x, H, fma=f)).max() for f in (False, True)]
            assert min(errs) <= tol, (h, H, B, errs, tol)
            if H == h:
                assert np.array_equal(got, x.astype(np.float64))


# ------------------------------------------------------------------------------------------------ small operators
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 65), (63, 65), (64, 64), (65, 1), (200, 3), (129, 130)])
def test_transpose_bf16_exact(rows, cols):
    t = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows)).bfloat16()
    got = ops.transpose_bf16(t.to(DEV)).cpu()
    assert got.shape == (cols, rows) and torch.equal(got.view(torch.int16), t.T.contiguous().view(torch.int16))


@pytest.mark.parametrize("B,P,C", [(1, 1, 4), (3, 1369, 768), (2, 196, 384)])
def test_vit_assemble_exact(B, P, C):
    g = torch.Generator().manual_seed(P)
    po, cls, pos = torch.randn(B * P, C, generator=g), torch.randn(C, generator=g), torch.randn(P + 1, C, generator=g)
    tok = ops.vit_assemble(po.to(DEV), cls.to(DEV), pos.to(DEV), B, P, C).cpu()
    want = torch.cat([cls.expand(B, 1, C), po.view(B, P, C)], 1) + pos       # one fp32 addition per element: exact agreement
    assert torch.equal(tok.view(B, P + 1, C), want)


@pytest.mark.parametrize("S", [8, 16, 224])
def test_im2col_patch8_exact(S):
    rgb = torch.randn(3, 3, S, S, generator=torch.Generator().manual_seed(S))
    pat = ops.im2col_patch8(rgb.to(DEV)).cpu()
    ref = torch.nn.functional.unfold(rgb, 8, stride=8).transpose(1, 2).reshape(-1, 192).to(torch.bfloat16)      # RNE
    assert pat.shape == ref.shape and torch.equal(pat.view(torch.int16), ref.view(torch.int16))


def _positive(shape, seed):
    """fp32 values in [0.5, 1.5): sums without cancellation, so 'relative to the sum' and 'relative to the sum of magnitudes' agree."""
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) + 0.5).float()


@pytest.mark.parametrize("rows", [1, 3, 15, 16, 17, 255, 256, 257, 1000])
@pytest.mark.parametrize("C,ld", [(1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (65, 72), (1, 5)])
def test_col_moments_raw_sums_vs_float64(rows, C, ld):
    """The 16-row unrolled loop, its 4-row tail and the 256-row block boundary, at column counts around the 64-column block, dense and
    with a row pitch above C (through the C entry point: ops.col_moments takes dense matrices only; the pitch columns hold 1e30).
    The kernel accumulates in double: a sum of `rows` positive terms in any order is within rows * 2^-53 of exact, relative --
    <= 1.2e-13 here, below the asserted 1e-12."""
    buf = torch.full((rows, ld), 1e30)
    buf[:, :C] = _positive((rows, C), rows * 131 + C)
    d = buf.to(DEV)
    acc = torch.zeros((2, C + 2), dtype=torch.float64, device=DEV)
    acc[:, C:] = -7.0
    ops._call("cmdiad_col_moments", ops._p(d), rows, C, ld, ops._p(acc[0]), ops._p(acc[1]), ops._stream())
    acc = acc.cpu()
    assert (acc[:, C:] == -7.0).all()
    v = buf[:, :C].double()
    assert rows * 2.0 ** -53 < 1e-12
    torch.testing.assert_close(acc[0, :C], v.sum(0), rtol=1e-12, atol=0)
    torch.testing.assert_close(acc[1, :C], (v * v).sum(0), rtol=1e-12, atol=0)
    if ld == C:     # and through the wrapper: mean and biased variance
        m, var = ops.col_moments(d)
        torch.testing.assert_close(m.cpu(), v.mean(0), rtol=1e-12, atol=0)
        # var = E[x^2] - mean^2 cancels: absolute, 1e-12 of each of the two terms, both below 1.5^2 = 2.25
        torch.testing.assert_close(var.cpu(), v.var(0, unbiased=False), rtol=0, atol=2 * 2.25e-12)


@pytest.mark.parametrize("rows", [1, 255, 257, 300_000])
def test_moments3_raw_sums_vs_float64(rows):
    """One block, two blocks, and above 1024 * 256 = 262 144 rows the grid-stride loop.  Double accumulation of positive terms: within
    rows * 2^-53 relative in the worst order (3.4e-11 at 300 000 rows); the kernel's order is a tree -- <= 2 terms per thread, 6
    shuffle levels, 3 additions over the waves, <= 1024 atomic additions over the blocks: depth <= 1035, 1035 * 2^-53 = 1.2e-13 --
    so the 1e-12 asserted here holds with room."""
    p = _positive((rows, 3), rows)
    acc = torch.zeros((9,), dtype=torch.float64, device=DEV)
    dp = p.to(DEV)
    ops._call("cmdiad_moments3", ops._p(dp), rows, ops._p(acc), ops._stream())
    d = p.double()
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    want = torch.stack([x.sum(), y.sum(), z.sum(), (x * x).sum(), (x * y).sum(), (x * z).sum(), (y * y).sum(), (y * z).sum(), (z * z).sum()])
    assert (2 + 6 + 3 + 1024) * 2.0 ** -53 < 1e-12
    torch.testing.assert_close(acc.cpu(), want, rtol=1e-12, atol=0)
    mean, cov = ops.moments3(dp)
    torch.testing.assert_close(mean.cpu(), d.mean(0), rtol=1e-12, atol=0)
    # the covariance E[ab] - E[a]E[b] cancels: absolute, 1e-12 of each of the two terms, both below 1.5^2 = 2.25
    torch.testing.assert_close(cov.cpu(), torch.cov(d.T, correction=0) if rows > 1 else torch.zeros(3, 3, dtype=torch.float64),
                               rtol=0, atol=2 * 2.25e-12)
