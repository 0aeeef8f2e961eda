"""GPU: ops.normalize_cast (normalize_cast_kernel, csrc/search_post.hip), the kernel that makes every operand of the nearest-
neighbour search, against numpy -- not against its own fp32 output, which is all the search, dedup, fakeworld and full-size tests
compare it with.

What is pinned:
  * the fp32 copy is numpy's fp32 (x - mean) * inv_std BIT FOR BIT.  The expression is a subtraction followed by a product: there
    is no product feeding an addition, so no contraction to an fma exists for it and the exact alternative of the check holds
    (search_post.hip is built with the compiler's default contraction);
  * the 16-bit row is the round-to-nearest-even cast of that fp32 copy, bit for bit (fp16: after clamping to +-65504), halfway
    cases in both directions, 16-bit subnormals, +-0 and mantissa carries included;
  * sq is the float64 sum of squares of the ROUNDED row within (D/4 + 8) * 2^-24 relative.  Squares of 16-bit values are exact in
    fp32, a lane adds at most 4 * ceil(D/256) of them and the wave reduction adds 6 + 3 levels: at most D/64 + 13 roundings on a
    sum of non-negative terms, inside the bound for every D; and it is SEPARATED from the sum over the unrounded row on inputs
    whose rounding is one-sided, by more than ten times the bound;
  * the row map of skip_leading, and that want_sq / want_f32 change nothing else."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd import ops  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def _rne_bf16_bits(f32):
    """fp32 array -> uint16 bf16 bit patterns, round to nearest, ties to even (finite input)."""
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _cast_bits(f32, dtype):
    """The 16-bit bit patterns that the fp32 values must become."""
    if dtype == torch.bfloat16:
        return _rne_bf16_bits(f32)
    return np.clip(f32, np.float32(-65504.0), np.float32(65504.0)).astype(np.float16).view(np.uint16)   # numpy: RNE


def _bits_to_f64(bits, dtype):
    if dtype == torch.bfloat16:
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float16).astype(np.float64)


def _norm_np(x, mean, inv_std):
    r = (x - np.float32(mean)) * np.float32(inv_std)
    assert r.dtype == np.float32
    return r


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _check(x, mean, inv_std, dtype, **kw):
    """One direct call against numpy; x [rows, D] fp32 numpy.  -> (bits, fp32 copy, sq) as numpy."""
    rows, D = x.shape
    o16, o32, sq = ops.normalize_cast(torch.from_numpy(x).to(DEV), mean, inv_std, want_f32=True, dtype=dtype, **kw)
    assert o16.dtype == dtype and o16.shape == (rows, D) and o32.shape == (rows, D) and sq.shape == (rows,)
    want32 = _norm_np(x, mean, inv_std)
    got32 = o32.cpu().numpy()
    np.testing.assert_array_equal(got32.view(np.uint32), want32.view(np.uint32))
    want16 = _cast_bits(want32, dtype)
    got16 = _bits(o16)
    np.testing.assert_array_equal(got16, want16)
    ref = (_bits_to_f64(want16, dtype) ** 2).sum(1)
    got = sq.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= (D / 4 + 8) * U * ref), np.max(np.abs(got - ref) / np.maximum(ref, 1e-300))
    return got16, got32, got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mean,inv_std", [(0.0, 1.0), (0.1, 1 / 1.3), (-3.7, 41.0)])
@pytest.mark.parametrize("D", [4, 132, 768, 1920])
@pytest.mark.parametrize("rows", [1, 5, 1027])
def test_bits_and_squared_norms(rows, D, mean, inv_std, dtype):
    g = np.random.default_rng(rows * 10007 + D)
    x = (g.standard_normal((rows, D)) * np.exp(g.uniform(-3, 3, (rows, 1)))).astype(np.float32)
    _check(x, mean, inv_std, dtype)


def _edge_values(dtype):
    """fp32 values (passed with mean 0, inv_std 1, i.e. unchanged: x - 0 and x * 1 are exact) on and next to the rounding
    boundaries of the 16-bit format."""
    if dtype == torch.bfloat16:
        hi = np.array([0x3F80, 0x3F81, 0x3FFF, 0x4000, 0x0001, 0x0002, 0x007F, 0x0080, 0x4F7F, 0x3EAA], np.uint32) << 16
        lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0xC000], np.uint32)     # 0x8000: the halfway case
        pos = (hi[:, None] | lo[None, :]).reshape(-1)
        pos = pos[pos < 0x7F7F0000]                                      # stays finite after rounding up
        tiny = np.array([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007F8000], np.uint32)   # -> bf16 subnormals / 0
        bits = np.concatenate([pos, tiny, np.array([0], np.uint32)])
    else:
        h = np.array([0x3C00, 0x3C01, 0x3FFF, 0x4000, 0x0001, 0x0002, 0x03FF, 0x0400, 0x7BFE, 0x3555], np.uint16).view(np.float16)
        up = np.nextafter(h, np.float16(np.inf))
        a, b = h.astype(np.float64), up.astype(np.float64)
        mid = (a + b) / 2                                                # exact in fp32: one more bit than a half
        vals = np.concatenate([a, mid, np.nextafter(mid.astype(np.float32), np.float32(0)).astype(np.float64),
                               np.nextafter(mid.astype(np.float32), np.float32(np.inf)).astype(np.float64),
                               [2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 0.0]])
        f = vals.astype(np.float32)
        assert np.array_equal(f.astype(np.float64), vals)
        bits = f.view(np.uint32)
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])          # both signs, -0 included
    return bits.view(np.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_halfway_cases_subnormals_and_signed_zero(dtype):
    v = _edge_values(dtype)
    want = _cast_bits(v, dtype)
    f32 = lambda bits: np.array([bits], np.uint32).view(np.float32)      # noqa: E731
    if dtype == torch.bfloat16:
        # the yardstick on known ties: 1 + 2^-8 -> 1 (even), 1 + 3 * 2^-8 -> 1 + 2^-6 (up to even); a subnormal tie; a carry
        assert _cast_bits(f32(0x3F808000), dtype)[0] == 0x3F80 and _cast_bits(f32(0x3F818000), dtype)[0] == 0x3F82
        assert _cast_bits(f32(0x00018000), dtype)[0] == 0x0002 and _cast_bits(f32(0x3FFFC000), dtype)[0] == 0x4000
        exp_mask = 0x7F80
    else:
        assert _cast_bits(np.float32([1 + 2.0 ** -11]), dtype)[0] == 0x3C00 and _cast_bits(np.float32([1 + 3 * 2.0 ** -11]), dtype)[0] == 0x3C02
        assert _cast_bits(np.float32([1.5 * 2.0 ** -24]), dtype)[0] == 0x0002 and _cast_bits(np.float32([2.0 ** -25]), dtype)[0] == 0x0000
        exp_mask = 0x7C00
    # the set holds what it claims: 16-bit subnormals, both zeros, results on both sides of the input
    assert np.any((want & exp_mask == 0) & (want & 0x7FFF != 0)) and np.any(want == 0x8000) and np.any(want == 0x0000)
    as64 = _bits_to_f64(want, dtype)
    assert np.any(as64 < v) and np.any(as64 > v) and np.all(np.isfinite(as64))
    D, per = 132, 100                                                    # 100 edge values and 32 ones per row: every row's sq is O(32)
    nrow = -(-len(v) // per)
    x = np.ones((nrow, D), np.float32)
    x[:, :per] = np.resize(v, nrow * per).reshape(nrow, per)
    got16, got32, _ = _check(x, 0.0, 1.0, dtype)
    assert np.array_equal(got32.view(np.uint32), x.view(np.uint32))      # the fp32 copy keeps -0 and fp32 subnormals


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [4, 132, 768, 1920])
def test_sq_is_of_the_rounded_row_not_of_the_input(D, dtype):
    """Inputs 0.45 of a 16-bit spacing above a grid point: every element rounds DOWN, so the rounded row's sum of squares is
    smaller than the input's by ~2 * 0.45 * spacing relative (1.8e-3 .. 7e-3 for bf16, 2.2e-4 .. 9e-4 for fp16) -- asserted here, on
    the CPU, to be more than ten times the bound the kernel's sq is then held to."""
    g = np.random.default_rng(D)
    frac_bits = 7 if dtype == torch.bfloat16 else 10
    m = 1.0 + g.integers(0, 2 ** (frac_bits - 1), (5, D)) / 2.0 ** frac_bits          # grid points in [1, 1.5): spacing 2^-frac_bits
    x = ((m + 0.45 * 2.0 ** -frac_bits) * 2.0 ** g.integers(-3, 4, (5, D))).astype(np.float32)
    rounded = _bits_to_f64(_cast_bits(x, dtype), dtype)
    assert np.all(rounded < x)
    s_round, s_in = (rounded ** 2).sum(1), (x.astype(np.float64) ** 2).sum(1)
    bound = (D / 4 + 8) * U
    assert np.all(s_in - s_round > 10 * bound * s_round)
    _, _, sq = _check(x, 0.0, 1.0, dtype)
    assert np.all(np.abs(sq - s_in) > 9 * bound * s_round)               # (follows from the two assertions; said for the reader)


def test_fp16_saturates_and_keeps_sq_finite():
    D = 132
    x = np.ones((3, D), np.float32)
    x[0, :6] = [65504.0, 65520.0, 70000.0, -70000.0, 1e10, -3e38]
    x[1, 5] = 65519.996                                                  # below the midpoint to 65536: rounds to 65504 anyway
    o16, o32, sq = ops.normalize_cast(torch.from_numpy(x).to(DEV), 0.0, 1.0, want_f32=True, dtype=torch.float16)
    h = o16.cpu().numpy()
    assert np.all(np.isfinite(h)) and h[0, :6].tolist() == [65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0] and h[1, 5] == 65504.0
    assert np.array_equal(o32.cpu().numpy(), x)                          # the fp32 copy is not clamped
    ref = (h.astype(np.float64) ** 2).sum(1)
    got = sq.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= (D / 4 + 8) * U * ref)
    _check(x[2:], 0.0, 1.0, torch.float16)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_whose_squares_overflow_is_taken_out_of_the_search(dtype):
    """bf16 keeps fp32's range: 1e20 squared is beyond fp32.  sq = +inf and the 16-bit row is zeroed (the search then never picks
    it), the fp32 copy keeps the values, and the neighbouring rows of the same block are untouched.  (fp16 cannot overflow by
    magnitude -- it saturates, previous test -- so its case is an infinite element, which the kernel treats the same way.)"""
    D = 260
    g = np.random.default_rng(9)
    x = g.standard_normal((6, D)).astype(np.float32)
    x[2, 7] = 1e20 if dtype == torch.bfloat16 else np.inf
    x[4, D - 1] = -1e20 if dtype == torch.bfloat16 else -np.inf
    o16, o32, sq = ops.normalize_cast(torch.from_numpy(x).to(DEV), 0.0, 1.0, want_f32=True, dtype=dtype)
    s = sq.cpu().numpy()
    assert np.isposinf(s[[2, 4]]).all() and np.isfinite(s[[0, 1, 3, 5]]).all()
    b = _bits(o16)
    assert not b[[2, 4]].any() and np.array_equal(b[[0, 1, 3, 5]], _cast_bits(x[[0, 1, 3, 5]], dtype))
    assert np.array_equal(o32.cpu().numpy().view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("G,s,R", [(1, 1, 1), (3, 1, 1), (1, 4, 1), (3, 4, 1), (1, 1, 784), (3, 1, 784), (1, 4, 784), (3, 4, 784), (3, 1, 5)])
def test_skip_leading_row_map(G, s, R, dtype):
    """x [G, s + R, D]: output row r comes from input row r + (r // R + 1) * s, and everything equals the plain call on those rows.
    (R * G is 1, 3, 15 -- not multiples of the four rows of a block -- and 784, 2352.)"""
    D, mean, inv_std = 132, 0.1, 1 / 1.3
    g = np.random.default_rng(G * 100 + s * 10 + R)
    x = g.standard_normal((G, s + R, D)).astype(np.float32)
    x[:, :s] += 1000.0                                                    # a skipped row that leaks in cannot hide
    o16, o32, sq = ops.normalize_cast(torch.from_numpy(x).to(DEV), mean, inv_std, want_f32=True, dtype=dtype, skip_leading=s)
    flat = x.reshape(-1, D)
    r = np.arange(G * R)
    src = r + (r // R + 1) * s
    assert np.array_equal(flat[src], x[:, s:].reshape(-1, D))             # the stated map is "drop the first s rows of each group"
    p16, p32, psq = ops.normalize_cast(torch.from_numpy(flat[src].copy()).to(DEV), mean, inv_std, want_f32=True, dtype=dtype)
    assert o16.shape == (G * R, D) and torch.equal(o16.view(torch.int16), p16.view(torch.int16))
    assert torch.equal(o32.view(torch.int32), p32.view(torch.int32)) and torch.equal(sq.view(torch.int32), psq.view(torch.int32))
    _check(flat[src].copy(), mean, inv_std, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_optional_outputs_change_nothing_else(dtype):
    g = np.random.default_rng(4)
    x = torch.from_numpy(g.standard_normal((1027, 132)).astype(np.float32)).to(DEV)
    x[5, 3] = float("inf")                                                # with sq this row is zeroed; without, it is only cast
    full16, full32, fullsq = ops.normalize_cast(x, 0.1, 1 / 1.3, want_f32=True, want_sq=True, dtype=dtype)
    a16, a32, asq = ops.normalize_cast(x, 0.1, 1 / 1.3, want_f32=False, want_sq=True, dtype=dtype)
    assert a32 is None and torch.equal(a16.view(torch.int16), full16.view(torch.int16)) and torch.equal(asq.view(torch.int32), fullsq.view(torch.int32))
    b16, b32, bsq = ops.normalize_cast(x, 0.1, 1 / 1.3, want_f32=True, want_sq=False, dtype=dtype)
    keep = torch.ones(1027, dtype=torch.bool, device=DEV)
    keep[5] = False
    assert bsq is None and torch.equal(b32.view(torch.int32), full32.view(torch.int32))
    assert torch.equal(b16.view(torch.int16)[keep], full16.view(torch.int16)[keep])
    assert not full16.view(torch.int16)[5].any() and bool(torch.isposinf(fullsq[5]))
