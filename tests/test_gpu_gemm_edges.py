"""GPU: the GEMM family -- cmdiad_gemm_bf16 and the five kernels behind it (the 128 x 128 tile kernel with the general, the
residual-row and the LayerNorm-producer epilogue, the persistent 256 x 256 kernel, the residual-tiles kernel),
cmdiad_gemm_streamk_bf16 and cmdiad_gemm_tn_bf16 -- held BIT FOR BIT to the float64 references of tests/gemm_ref.py at edge shapes
and with pitches.  tests/test_gemm_ref_cpu.py checks, without a GPU, what makes a bit comparison meaningful: the operands sit on a
lattice on which fp32 accumulation is exact in every order, the bf16 outputs need rounding (truncation and half-up differ from
nearest-even), no reference holds a sentinel, and the split-K slabs follow the kernels' rule.

Every launch fills cmdiad_amd._native.GemmArgs itself (ops.gemm always passes the matrix width as the pitch).  Every output is the
leading part of a buffer of sentinel bit patterns with 128 more rows: rows past M and columns N .. ld must keep their bits.  The
pad columns of pitched A, W, residual and add2 hold 3e4: read once, they change the result.  Assertions are equality of bit
patterns except for GELU, whose pre-activation is exact and whose output is bounded by GELU_ABS (csrc/common.h) plus one rounding
of the output format; a failure names the first differing element and the tile and wave it falls in."""
import collections
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as gr  # noqa: E402
from conftest import need_ab_variants  # noqa: E402

from cmdiad_amd import _native as nat  # noqa: E402
from cmdiad_amd import ops  # noqa: E402

DEV = "cuda"
GUARD = 128                              # sentinel rows behind every output
T128 = (128, 128, 64, 64)                # block tile and wave tile of the kernels, for the failure text
T256 = (256, 256, 128, 64)
_ENV = ("CMDIAD_GEMM_PANEL_MIN", "CMDIAD_GEMM_GROUPM", "CMDIAD_GEMM_PP3", "CMDIAD_GEMM_RES_WIDE", "CMDIAD_GEMM_WIDE")


def _setting(monkeypatch, env):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _sent(rows, cols, dtype):
    if dtype == torch.float32:
        return torch.full((rows, cols), gr.SENT32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((rows, cols), gr.SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _is_sent(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32) == gr.SENT32
    return t.contiguous().view(torch.int16) == gr.SENT16


def _padded(t, extra, dtype):
    """CPU [R, C] -> device [R, C + extra] of dtype; the pad columns hold PAD_VALUE"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), gr.PAD_VALUE, dtype=torch.float32)
    buf[:, :t.shape[1]] = t
    return buf.to(dtype).to(DEV)


def _cpu(t):
    return None if t is None else t.cpu()


Run = collections.namedtuple("Run", "rc o32 o16 xb part")


def _gemm(shape, form, pitch=gr.Pitch(), ln=False, inplace=False, bad=None):
    """One cmdiad_gemm_bf16 launch of `form` on the lattice operands of `shape`; ln: with
    ln_xb, ln_part and add2; inplace: the output buffer is the residual; bad: GemmArgs fields overwritten before the call.
    Returns the return code and the WHOLE buffers, on the host."""
    M, N, K = shape
    o, S = gr.operands(*shape), form.split
    p = ops._p
    dA, dW = _padded(o.A, pitch.a, torch.bfloat16), _padded(o.W, pitch.w, torch.bfloat16)
    bias = o.bias.to(DEV) if form.bias else None
    gb = gr.group_bias_of(o, form)
    gb = gb.to(DEV) if gb is not None else None
    rs = None
    if form.row_scale:                   # readable up to M rounded up to 256 (the persistent kernel's ragged last tile)
        rs = torch.ones((M + 255) // 256 * 256)
        rs[:M] = o.rscale
        rs = rs.to(DEV)
    o32 = _sent(S * M + GUARD, N + pitch.o32, torch.float32) if form.outs in ("f32", "both") else None
    o16 = _sent(M + GUARD, N + pitch.o16, torch.bfloat16) if form.outs in ("bf16", "both") else None
    res = None
    if form.residual and inplace:
        assert pitch.r == pitch.o32
        o32[:M, :N] = o.res.to(DEV)
        res = o32
    elif form.residual:
        res = _padded(o.res, pitch.r, torch.float32)
    xb = part = add2 = None
    if ln:
        xb = _sent(M + GUARD, N + pitch.xb, torch.bfloat16)
        part = _sent(1, (N // 64) * M * 2 + 64, torch.float32)
        add2 = _padded(o.add2, pitch.add2, torch.float32)
    a = nat.GemmArgs(p(dA), K + pitch.a, p(dW), K + pitch.w, M, N, K, p(bias), p(gb), form.group_rows or 1, form.act,
                     p(res), N + pitch.r, p(o32), N + pitch.o32, p(o16), N + pitch.o16, None, None, S, None,
                     p(rs), p(xb), N + pitch.xb, p(part), p(add2), N + pitch.add2)
    for k, v in (bad or {}).items():
        setattr(a, k, v)
    rc = nat.lib().cmdiad_gemm_bf16(ctypes.byref(a), ops._stream())
    torch.cuda.synchronize()
    return Run(rc, _cpu(o32), _cpu(o16), _cpu(xb), _cpu(part))


def _guards_intact(buf, rows, N, what):
    lost = ~_is_sent(buf)
    lost[:rows, :N] = False
    if lost.any():
        r, c = (int(v) for v in lost.nonzero()[0])
        raise AssertionError(f"{what}: {int(lost.sum())} elements outside the {rows} x {N} output were written; first at ({r}, {c}), "
                             f"now {float(buf[r, c])!r} (buffer {tuple(buf.shape)})")


def _assert_bits(got, want, tiling, what):
    assert not _is_sent(got).any(), f"{what}: {int(_is_sent(got).sum())} elements were never written"
    d = gr.first_difference(got, want, tiling)
    assert d is None, f"{what}: {d}"


def _assert_within(got, ref, bound, tiling, what):
    assert not _is_sent(got).any(), f"{what}: {int(_is_sent(got).sum())} elements were never written"
    bad = ~((got.double() - ref).abs() <= bound)
    if bad.any():
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at ({r}, {c}): got {float(got[r, c])!r}, "
                             f"ref {float(ref[r, c])!r}, bound {float(bound[r, c])!r}; " + gr.locate(r, c, *tiling))


def _check(run, shape, form, tiling, what, add2=False):
    """the outputs of `run` against the float64 reference, and everything around them against the sentinel"""
    M, N, _ = shape
    assert run.rc == 0, (what, run.rc, nat.lib().cmdiad_last_error().decode())
    _, ref = gr.reference(gr.operands(*shape), form, add2=add2)
    slabs = ref if form.split > 1 else ref[None]
    assert (run.o32 is not None) == (form.outs != "bf16") and (run.o16 is not None) == (form.outs != "f32")
    for got, name in ((run.o32, "f32"), (run.o16, "bf16")):
        if got is None:
            continue
        _guards_intact(got, len(slabs) * M, N, f"{what} {name}")
        for y, want in enumerate(slabs):                          # slab y starts at row y M of the buffer (pitch ldo32)
            live, w = got[y * M:(y + 1) * M, :N], f"{what} {name}" + (f" slab {y}" if form.split > 1 else "")
            if form.act == gr.ACT_GELU:
                _assert_within(live, want, gr.gelu_bound_f32(want) if name == "f32" else gr.bf16_bound(want, gr.GELU_ABS), tiling, w)
            else:
                _assert_bits(live, want.float() if name == "f32" else gr.bf16_rne(want), tiling, w)


def _ids(v):
    if isinstance(v, dict):
        return "+".join(k.rsplit("_", 1)[-1].lower() for k in v) or "default"
    return v.name if hasattr(v, "name") else "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------ the 128 x 128 kernel
@pytest.mark.parametrize("setting", gr.SETTINGS, ids=lambda s: s[0])
@pytest.mark.parametrize("shape", gr.GENERAL_SHAPES, ids=_ids)
def test_gemm_general_kernel_is_exact_at_edge_shapes(shape, setting, monkeypatch):
    """Every epilogue form of gr.GENERAL_FORMS at 1 .. 16 K-tiles, N below one tile and 128 t +- 4, M = 128 t - 1, 128 t, 128 t + 1,
    under the default dispatch, the N-panel walk and the row-major block order."""
    _setting(monkeypatch, setting[1])
    for form in gr.GENERAL_FORMS:
        _check(_gemm(shape, form), shape, form, T128, f"{shape} {setting[0]} {form.name}")


# ------------------------------------------------------------------------------------------------ the 256-column kernels
@pytest.mark.parametrize("shape", gr.WIDE256_SHAPES, ids=_ids)
def test_gemm_256_column_kernels_are_exact_and_equal_the_default_kernel(shape, monkeypatch):
    """CMDIAD_GEMM_PP3=1 (gemm_std_pp3_kernel) and CMDIAD_GEMM_RES_WIDE=1 (gemm_residual_tiles_launch) on fewer jobs than blocks,
    M = 1 and 100 (the wr = 1 half of the 256-row tile wholly past M), 255, 257, 513: exact, nothing written past row M, and the
    whole buffers bit for bit what the default kernel leaves on the same call."""
    M, N, _ = shape
    for form in gr.PP3_FORMS:
        _setting(monkeypatch, {})
        base = _gemm(shape, form)
        _setting(monkeypatch, gr.PP3_ENV)
        run = _gemm(shape, form)
        _check(run, shape, form, T256, f"{shape} pp3 {form.name}")
        _check(base, shape, form, T128, f"{shape} default {form.name}")
        assert torch.equal(run.o16.view(torch.int16), base.o16.view(torch.int16)), f"{shape} {form.name}: pp3 differs from the default kernel"
    form = gr.BIAS_RES_F32
    for inplace in (False, True):
        _setting(monkeypatch, {})
        base = _gemm(shape, form, inplace=inplace)
        _setting(monkeypatch, gr.RES_WIDE_ENV)
        run = _gemm(shape, form, inplace=inplace)
        _check(run, shape, form, T256, f"{shape} res_wide inplace={inplace}")
        _check(base, shape, form, T128, f"{shape} default residual rows inplace={inplace}")
        assert torch.equal(run.o32.view(torch.int32), base.o32.view(torch.int32)), f"{shape} inplace={inplace}: res_wide differs from the default kernel"


# ------------------------------------------------------------------------------------------------ pitches
@pytest.mark.parametrize("kernel,env,shape,form", gr.PITCHED_CASES, ids=_ids)
def test_gemm_with_pitches(kernel, env, shape, form, monkeypatch):
    """lda = K + 8, ldw = K + 24, ldr = N + 4, ldo32 = N + 12, ldo16 = N + 8 (ld_xb = N + 4, ld_add2 = N + 8), every pitch
    different from its width and from its neighbours: operand pads poisoned, output pads and the rows past M sentinels."""
    M, N, _ = shape
    _setting(monkeypatch, env)
    ln = kernel == "ln"
    run = _gemm(shape, form, gr.PITCHED, ln=ln)
    tiling = T256 if kernel in ("pp3", "res_wide") else T128
    _check(run, shape, form, tiling, f"pitched {kernel} {shape} {form.name}", add2=ln)
    if ln:
        _, ref = gr.reference(gr.operands(*shape), form, add2=True)
        _guards_intact(run.xb, M, N, "ln_xb")
        _assert_bits(run.xb[:M, :N], gr.bf16_rne(ref), T128, "ln_xb")
        n = (N // 64) * M * 2
        _guards_intact(run.part, 1, n, "ln_part")
        part = run.part[0, :n].reshape(N // 64, M, 2)
        chunks = ref.reshape(M, N // 64, 64)
        # the sums are sums of multiples of 1/4 below 2^14: exact in any order
        _assert_bits(part[..., 0].contiguous(), chunks.sum(-1).T.float().contiguous(), (1, 128, 1, 128), "ln_part sums [chunk, row]")
        # M2 about the chunk mean: the mean and the deviations are exact (multiples of 1/256), the squares are not: 8 FMAs per lane and
        # 3 shuffle additions of non-negative partial sums, 11 roundings each below 2^-24 of the total (16: second order and margin)
        q_ref = ((chunks - chunks.mean(-1, keepdim=True)) ** 2).sum(-1).T
        _assert_within(part[..., 1], q_ref, 16 * 2.0 ** -24 * q_ref, (1, 128, 1, 128), "ln_part M2 [chunk, row]")


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.mark.parametrize("bad", [{"K": 100}, {"lda": 192 + 4}, {"ldo32": 132 + 2}], ids=["K%64", "lda%8", "ldo32%4"])
def test_gemm_argument_errors_leave_the_outputs_alone(bad, monkeypatch):
    _setting(monkeypatch, {})
    run = _gemm((129, 132, 192), gr.GENERAL_FORMS[0], bad=bad)
    assert run.rc != 0 and nat.lib().cmdiad_last_error()
    assert _is_sent(run.o32).all() and _is_sent(run.o16).all()


# ------------------------------------------------------------------------------------------------ the A/B build's 4-wave shapes
@pytest.mark.parametrize("wide", ["4", "8"])
@pytest.mark.parametrize("shape", gr.AB_WIDE_SHAPES, ids=_ids)
def test_gemm_exact_variant_wide_shapes(shape, wide, monkeypatch):
    """gemm_std_wide_kernel (csrc/ab/gemm_wide_kernels.inc, the test-only build): 256 x 128 and 256 x 256 blocks of four waves, the
    forms it takes (bias, group bias, activation, both outputs), exact."""
    need_ab_variants("gemm_std_wide_kernel")
    _setting(monkeypatch, {"CMDIAD_GEMM_WIDE": wide})
    tiling = (256, 256, 128, 128) if wide == "8" else (256, 128, 128, 64)
    for form in gr.AB_WIDE_FORMS:
        _check(_gemm(shape, form), shape, form, tiling, f"{shape} wide {wide} {form.name}")
    _check(_gemm(shape, gr.GENERAL_FORMS[3], gr.PITCHED), shape, gr.GENERAL_FORMS[3], tiling, f"{shape} wide {wide} pitched")


# ------------------------------------------------------------------------------------------------ gemm_tn
def _tn(case, want_colsum, bad=None):
    M, N1, N2, split, pitched = case
    ep, eq, eo = gr.TN_PITCH if pitched else (0, 0, 0)
    P, Q = gr.tn_operands(M, N1, N2)
    dP, dQ = _padded(P, ep, torch.bfloat16), _padded(Q, eq, torch.bfloat16)
    out = _sent(split * N1 + GUARD, N2 + eo, torch.float32)
    cs = _sent(1, split * N1 + 64, torch.float32) if want_colsum else None
    arg = {**dict(ldp=N1 + ep, ldq=N2 + eq, split=split, ldo=N2 + eo), **(bad or {})}
    rc = nat.lib().cmdiad_gemm_tn_bf16(ops._p(dP), arg["ldp"], ops._p(dQ), arg["ldq"], M, N1, N2, arg["split"], ops._p(out), arg["ldo"],
                                       ops._p(cs), ops._stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), _cpu(cs)


@pytest.mark.parametrize("case", gr.TN_CASES, ids=lambda c: "x".join(map(str, c[:4])) + ("_pitched" if c[4] else ""))
def test_gemm_tn_is_exact_slab_by_slab(case):
    """Each slab is the product over its own rows [64 kt0, 64 (kt0 + count)), an empty slab is zeros, and so are its column sums;
    the output does not depend on whether the column sums are asked for."""
    M, N1, N2, split, _ = case
    slabs, colsum = gr.tn_reference(*gr.tn_operands(M, N1, N2), split)
    outs = []
    for want_colsum in (True, False):
        rc, out, cs = _tn(case, want_colsum)
        assert rc == 0, nat.lib().cmdiad_last_error().decode()
        _guards_intact(out, split * N1, N2, f"gemm_tn {case}")
        for y in range(split):
            _assert_bits(out[y * N1:(y + 1) * N1, :N2], slabs[y].float(), T128, f"gemm_tn {case} colsum={want_colsum} slab {y}")
        if want_colsum:
            _guards_intact(cs, 1, split * N1, f"gemm_tn {case} column sums")
            _assert_bits(cs[:, :split * N1], colsum.float().reshape(1, -1), (1, N1, 1, 64), f"gemm_tn {case} column sums [slab x N1]")
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("bad", [{"ldp": 136 - 8}, {"split": 128 // 64 + 1}], ids=["ldp<N1", "split>M/64"])
def test_gemm_tn_argument_errors_leave_the_outputs_alone(bad):
    rc, out, cs = _tn((128, 136, 72, 2, False), True, bad=bad)
    assert rc != 0 and nat.lib().cmdiad_last_error()
    assert _is_sent(out).all() and _is_sent(cs).all()


# ------------------------------------------------------------------------------------------------ stream-K
_SK_COUNTERS_AT = 256 * 256 * 256 * 4    # csrc/gemm_sk.hip sk_layout: a 256 x 256 fp32 slot per block, then two counters per block


@pytest.mark.parametrize("shape", gr.STREAMK_SHAPES, ids=_ids)
def test_gemm_streamk_at_the_edges_of_its_eligibility(shape, monkeypatch):
    """257, 511 and 258 tiles on 256 blocks, three and four K-tiles (the minimum range of one tile per block: nearly every block
    both hands a piece over and takes one over), ragged and whole last M tile; tests/sk_jobs_check.cpp walks the same four launches
    on the host.  All rows against the exact reference and against the 128 x 128 kernel, in place twice on one workspace (whose
    counters return to zero) and into a separate output with sentinel rows behind it."""
    M, N, K = shape
    _setting(monkeypatch, {})
    lib = nat.lib()
    assert lib.cmdiad_gemm_streamk_eligible(M, N, K)
    g = torch.Generator().manual_seed(gr.seed_of(M, N, K))
    A = torch.randint(-4, 5, (M, K), generator=g, dtype=torch.int8)
    W = torch.randint(-2, 3, (N, K), generator=g, dtype=torch.int8)
    bias = torch.randint(-32, 33, (N,), generator=g).float() / 4
    res = torch.randint(-64, 65, (M, N), generator=g, dtype=torch.int8).float() / 2
    ref = A.float() @ W.float().T + bias + res                    # multiples of 1/4 below 2^12: fp32 on the CPU is exact in any order
    dA, dW, dbias, dres = A.to(DEV).bfloat16(), W.to(DEV).bfloat16(), bias.to(DEV), res.to(DEV)
    want = dres.clone()
    ops.gemm(dA, dW, bias=dbias, residual=want, out_f32=want, want_bf16=False)
    nbytes = int(lib.cmdiad_gemm_streamk_workspace_bytes())
    assert nbytes == _SK_COUNTERS_AT + 256 * 2 * 4
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def launch(residual, out):
        a = nat.GemmArgs(ops._p(dA), K, ops._p(dW), K, M, N, K, ops._p(dbias), None, 1, gr.ACT_NONE, ops._p(residual), N, ops._p(out), N,
                         None, 0, None, None, 1, None, None, None, 0, None, None, 0)
        rc = lib.cmdiad_gemm_streamk_bf16(ctypes.byref(a), ops._p(ws), nbytes, ops._stream())
        assert rc == 0, lib.cmdiad_last_error().decode()
        torch.cuda.synchronize()
        assert not ws[_SK_COUNTERS_AT:].any(), "hand-over counters did not return to zero"

    for rep in range(2):
        x = dres.clone()
        launch(x, x)
        assert torch.equal(x, want), f"{shape} in place, launch {rep}: " + str(gr.first_difference(x.cpu(), want.cpu(), T256))
    out = _sent(M + GUARD, N, torch.float32)
    launch(dres, out)
    out = out.cpu()
    _guards_intact(out, M, N, f"stream-K {shape} separate output")
    _assert_bits(out[:M], ref, T256, f"stream-K {shape} against the exact reference")
    assert torch.equal(want.cpu(), ref), f"{shape} 128 x 128 kernel: " + str(gr.first_difference(want.cpu(), ref, T128))
