"""GPU: every instantiation of cmdiad_layernorm (float2 form C/128 = 1..8, 16-byte form C/256 = 1..4) and of
cmdiad_layernorm_skip_first against the float64 reference conv_ref.layernorm, at row counts around the four-row block, and the
agreement the two forms promise on the widths both can take."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402

from cmdiad_amd import ops  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
SENT = 0x4B3C5A69


def _ulp_check(got, ref64, what, max_ulps=1.0, frac_off=2e-3, abs_slack=None):
    """The one-step rule of tests/test_gpu_nets.py (copied: that module builds whole networks on import).  got: bf16 tensor from the
    GPU; ref64: float64 values BEFORE rounding.  Every element must be one of the (at most two) bf16 neighbours of the exact value
    -- |got - exact| <= max_ulps * ulp(exact) + abs_slack -- and all but a fraction `frac_off` must be the NEAREST one.  abs_slack
    (default 1e-5 of the mean magnitude) covers the fp32 evaluation of values that are small by cancellation."""
    got = got.detach().cpu().double()
    ref64 = ref64.detach().cpu()
    if abs_slack is None:
        abs_slack = 1e-5 * float(ref64.abs().mean())
    nearest = ref64.float().to(torch.bfloat16).double()
    ulp = torch.exp2(torch.floor(torch.log2(nearest.abs().clamp_min(1e-37))) - 7.0)       # the bf16 step at the exact value
    err = (got - ref64).abs()
    assert bool((err <= max_ulps * ulp + abs_slack).all()), (what, float(((err - abs_slack) / ulp).max()))
    off = float((got != nearest).double().mean())
    assert off <= frac_off, (what, off)
    return off


def _sent(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, SENT & 0xFFFF, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _is_sent(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32) == SENT
    return t.contiguous().view(torch.int16) == (SENT & 0xFFFF)


def _operands(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 3 + 1
    add = torch.randn(M, C, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return x, add, gamma, beta


def _misaligned(t):
    """A contiguous copy of t on the device whose first element is 8 bytes past a 16-byte boundary (C % 4 == 0: every row is):
    cmdiad_layernorm then cannot take its 16-byte form and runs the float2 form, whatever CMDIAD_LN_WIDE says."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[2:2 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def _check(y16, o32, mean, rstd, x64, gamma, beta, eps, what):
    """bf16 output: the one-step rule.  f32 output: 1e-5 relative + 1e-5 absolute (tests/test_gpu_kernels.py::test_layernorm).
    Statistics, as tests/test_gpu_train_kernels.py::test_layernorm_stats derives them: k = C/64 + 12 roundings on the path of a term
    (per-lane run, the 64-lane tree, the division) -> |mean err| <= k 2^-24 mean|x|; the two-pass variance about the fp32 mean
    carries k roundings, the mean's error dm adds dm^2 / var, rsqrt ~1 ulp (the halving by the square root is not relied on)."""
    C = x64.shape[1]
    ref, m64, r64 = cr.layernorm(x64.numpy(), gamma.double().numpy(), beta.double().numpy(), eps)
    ref, m64, r64 = torch.from_numpy(ref), torch.from_numpy(m64), torch.from_numpy(r64)
    if y16 is not None:     # (a share of 2e-3 cannot be expressed on fewer than 500 values: one value may be the other neighbour there)
        _ulp_check(y16, ref, what, frac_off=max(2e-3, 1.0 / ref.numel()))
    if o32 is not None:
        err = (o32.cpu().double() - ref).abs()
        assert (err <= 1e-5 * ref.abs() + 1e-5).all(), (what, float(err.max()))
    if mean is not None:
        k = C // 64 + 12
        dm = k * U * x64.abs().mean(1)
        assert ((mean.cpu().double() - m64).abs() <= dm).all(), (what, "mean")
        rel = k * U + 0.5 * dm * dm / (1.0 / (r64 * r64)) + 2 * U
        assert ((rstd.cpu().double() - r64).abs() <= rel * r64).all(), (what, "rstd")


@pytest.mark.parametrize("C", [128, 256, 384, 512, 640, 768, 896, 1024])
@pytest.mark.parametrize("M", [1, 3, 4, 6, 9, 1027])
def test_layernorm_every_width_vs_float64(M, C):
    """Aligned operands: C % 256 == 0 takes the 16-byte form (C/256 = 1..4), the other widths the float2 form (C/128 = 1, 3, 5, 7).
    M around the four-row block: rows M.. of sentinel-filled outputs keep their bits.  Without `add` x is left alone; with it
    x + add is written back exactly (one fp32 addition)."""
    x, add, gamma, beta = _operands(M, C, M * 7 + C)
    dg, db = gamma.to(DEV), beta.to(DEV)
    for with_add in (False, True):
        dx = x.clone().to(DEV)
        y16, o32 = _sent((M + 3, C), torch.bfloat16), _sent((M + 3, C), torch.float32)
        mean, rstd = _sent((M + 3,), torch.float32), _sent((M + 3,), torch.float32)
        ops.layernorm(dx, dg, db, 1e-6, add=add.to(DEV) if with_add else None, out_bf16=y16[:M], out_f32=o32[:M], stats=(mean[:M], rstd[:M]))
        torch.cuda.synchronize()
        xin = x + add if with_add else x
        assert torch.equal(dx.cpu(), xin)
        for t in (y16, o32, mean, rstd):
            assert _is_sent(t[M:]).all() and not _is_sent(t[:M]).any()
        _check(y16[:M], o32[:M], mean[:M], rstd[:M], xin.double(), gamma, beta, 1e-6, (M, C, with_add))


@pytest.mark.parametrize("C", [128, 256, 384, 512, 640, 768, 896, 1024])
def test_layernorm_float2_form_every_width_vs_float64(C):
    """The float2 form at EVERY width (C/128 = 1..8), reached through an x that is 8-byte but not 16-byte aligned; f32 output into a
    column block of a wider buffer (ldo32 = C + 6), whose other columns keep their bits."""
    M = 6
    x, add, gamma, beta = _operands(M, C, C + 1)
    dx = _misaligned(x)
    wide = _sent((M, C + 6), torch.float32)
    y16 = ops.layernorm(dx, gamma.to(DEV), beta.to(DEV), 1e-5, add=add.to(DEV), out_f32=wide[:, 2:2 + C])
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), x + add)
    assert _is_sent(wide[:, :2]).all() and _is_sent(wide[:, 2 + C:]).all()
    _check(y16, wide[:, 2:2 + C], None, None, (x + add).double(), gamma, beta, 1e-5, ("float2", C))


@pytest.mark.parametrize("C", [256, 512, 768, 1024])
def test_layernorm_forms_agree(C):
    """The widths both forms can take: the same rows through the 16-byte form (aligned operands) and the float2 form (x 8 bytes off).
    misc.hip promises agreement 'to fp32 rounding, not bitwise' (a lane's partial sums differ between the forms), so what is
    asserted is that BOTH meet the float64 bounds -- not torch.equal -- and that the statistics of the two are within the sum of their
    two bounds of each other."""
    M = 9
    x, _, gamma, beta = _operands(M, C, C + 2)
    dg, db = gamma.to(DEV), beta.to(DEV)
    outs = []
    for dx in (x.clone().to(DEV), _misaligned(x)):
        o32 = torch.empty((M, C), device=DEV)
        mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        y16 = ops.layernorm(dx, dg, db, 1e-5, out_f32=o32, stats=(mean, rstd))
        _check(y16, o32, mean, rstd, x.double(), gamma, beta, 1e-5, ("forms", C, dx.data_ptr() % 16))
        outs.append((o32.cpu().double(), mean.cpu().double(), rstd.cpu().double()))
    k = C // 64 + 12
    assert ((outs[0][1] - outs[1][1]).abs() <= 2 * k * U * x.double().abs().mean(1)).all()
    assert ((outs[0][0] - outs[1][0]).abs() <= 2 * (1e-5 * outs[0][0].abs() + 1e-5)).all()
    print(f"layernorm C={C}: 16-byte and float2 forms bitwise equal on {float((outs[0][0] == outs[1][0]).double().mean()):.3f} of the values")


@pytest.mark.parametrize("C", [128, 640, 1024])
@pytest.mark.parametrize("B,T", [(1, 2), (3, 5), (2, 1025)])
def test_layernorm_skip_first_matches_float2_form_bitwise(B, T, C):
    """cmdiad_layernorm_skip_first's stated contract: the arithmetic of the float2 form step for step, so rows t >= 1 of every T-row
    segment give the bits of cmdiad_layernorm (float2 form: x 8 bytes off a 16-byte boundary) on the same rows.  Output into a
    column block (ldo32 = C + 6 > C) of a sentinel-filled buffer: nothing outside the block is written."""
    g = torch.Generator().manual_seed(B * T + C)
    x = 3.0 * torch.randn(B * T, C, generator=g) + 0.5
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    rows = B * (T - 1)
    wide = _sent((rows, C + 6), torch.float32)
    ops.layernorm_skip_first(x.to(DEV), gamma, beta, 1e-5, B, T, wide[:, 2:2 + C])
    tok = x.view(B, T, C)[:, 1:].reshape(rows, C).contiguous()
    want = torch.empty((rows, C), device=DEV)
    ops.layernorm(_misaligned(tok), gamma, beta, 1e-5, out_f32=want, want_bf16=False)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 2:2 + C], want)
    assert _is_sent(wide[:, :2]).all() and _is_sent(wide[:, 2 + C:]).all()
    _check(None, want, None, None, tok.double(), gamma.cpu(), beta.cpu(), 1e-5, ("skip_first", B, T, C))
