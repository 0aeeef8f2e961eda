"""GPU: the point-group encoder's MFMA chain (cmdiad_encoder_stage1, the group-bias cmdiad_gemm_bf16, cmdiad_gemm_groupmax,
cmdiad_encoder_tail / _tail_n) against tests/encoder_ref.py, BIT FOR BIT.  The operands sit on a lattice on which every sum of
the chain is exact in fp32 in any order (tests/test_encoder_ref_cpu.py pins that, and that the inputs tell the reference from a
kernel that drops a row or a 16-row block of a group, misplaces a group boundary, seeds a maximum with 0 or rounds h2 / h3 other
than to nearest-even), so no assertion here carries a tolerance: torch.equal on fp32 and on the int16 view of bf16.  Every
output lands in an oversized buffer with 128 guard rows of a position-dependent bit pattern before and after it.

(groups, Mg) -> rows: (1,32) 32, (1,64) 64 below one tile, once-per-block stage 1 | (1,128) one tile | (4,32), (2,64) one tile of
four / two groups | (3,32) 96, (7,32) 224, (9,64) 576 ragged | (5,32) 160 tile + ragged 32 | (3,64) 192 tile + one group |
(257,128) 32 896: block 0 of the persistent kernels walks two tiles, the rest one | (1030,32) 32 960: 258 blocks of the once
kernel, ragged | (2052,32) 65 664: 513 tiles, three for block 0, two for the others."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ref as er  # noqa: E402
from conftest import need_ab_variants  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 128
IDS = [f"{g}x{m}" for g, m in er.GRID]


@pytest.fixture(scope="module")
def ops():
    from cmdiad_amd import ops as o
    return o


_W = {}


def _weights():
    """the lattice weights on the device, as the kernels take them"""
    if not _W:
        w = er.weights()
        bf = lambda t: t.to(torch.bfloat16).to(DEV).contiguous()      # noqa: E731 -- exact: integers of at most two bits
        _W.update(w1b1=w["w1b1"].to(DEV), W2=bf(w["W2"]), b2=w["b2"].to(DEV), W3a=bf(w["W3a"]), W3b=bf(w["W3b"]), b3=w["b3"].to(DEV),
                  W4=bf(w["W4"]), b4=w["b4"].to(DEV))
        _W[384] = (_W["W4"], _W["b4"])
        _W[256] = (_W["W4"][:256], _W["b4"][:256])                    # (leading rows of a contiguous tensor: contiguous, aligned)
    return _W


def _case(groups, Mg):
    c = er.case(groups, Mg)
    er.check_preconditions(c["stats"], Mg)
    return c


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _guarded(rows, cols, dtype):
    """-> (buffer [GUARD + rows + GUARD, cols] on the device, filled with a position-dependent finite bit pattern; its copy)"""
    i = torch.arange((rows + 2 * GUARD) * cols, dtype=torch.int64)
    if dtype == torch.float32:
        pat = (0x4B3C0000 | ((i * 40503) & 0xFFFF)).to(torch.int32).view(torch.float32)
    else:
        pat = (0x4B00 | ((i * 157) & 0xFF)).to(torch.int16).view(torch.bfloat16)
    buf = pat.reshape(-1, cols).to(DEV)
    return buf, buf.clone()


def _body(buf):
    return buf[GUARD:buf.shape[0] - GUARD]


def _same(got, want, what):
    """bit for bit; `want` from the CPU reference"""
    want = want.to(got.dtype).to(got.device) if want.dtype != got.dtype else want.to(got.device)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(_bits(got.contiguous()), _bits(want.contiguous())):
        bad = (_bits(got.contiguous()) != _bits(want.contiguous())).nonzero()
        r, c = bad[0].tolist()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at [{r}, {c}]: "
                             f"got {float(got[r, c])}, want {float(want[r, c])}; rows {sorted(set(bad[:, 0].tolist()))[:8]}")


def _guards_intact(buf, orig, what, untouched_rows=None):
    """the guard rows (and `untouched_rows` of the body) still hold the pattern"""
    n = buf.shape[0]
    assert torch.equal(_bits(buf[:GUARD]), _bits(orig[:GUARD])), f"{what}: a store in the {GUARD} rows BEFORE the output"
    assert torch.equal(_bits(buf[n - GUARD:]), _bits(orig[n - GUARD:])), f"{what}: a store in the {GUARD} rows AFTER the output"
    if untouched_rows is not None:
        assert torch.equal(_bits(_body(buf)[untouched_rows]), _bits(_body(orig)[untouched_rows])), f"{what}: a row that is not the kernel's was written"


# ------------------------------------------------------------------------------------------------ the checks
def _check_stage1(ops, groups, Mg):
    c, w = _case(groups, Mg), _weights()
    M = groups * Mg
    (h2, h2o), (g32, g32o), (g16, g16o) = _guarded(M, 256, torch.bfloat16), _guarded(groups, 256, torch.float32), _guarded(groups, 256, torch.bfloat16)
    xyz = c["xyz"].to(DEV)
    ops._call("cmdiad_encoder_stage1", ops._p(xyz), ops._p(w["w1b1"]), ops._p(w["W2"]), ops._p(w["b2"]), groups, Mg,
              ops._p(_body(h2)), ops._p(_body(g32)), ops._p(_body(g16)), ops._stream())
    torch.cuda.synchronize()
    _same(_body(g32), c["g32"], "stage-1 maxima (fp32)")
    _same(_body(g16), c["g16"], "stage-1 maxima (bf16)")
    _same(_body(h2), c["h2"], "h2")
    for b, o, what in ((h2, h2o, "h2"), (g32, g32o, "g32"), (g16, g16o, "g16")):
        _guards_intact(b, o, what)


def _check_two_kernel_path(ops, groups, Mg):
    """each kernel fed the REFERENCE's inputs, so that a defect upstream does not mask one here"""
    c, w = _case(groups, Mg), _weights()
    M = groups * Mg
    gb, gbo = _guarded(groups, 512, torch.float32)
    ops.gemm(c["g16"].to(DEV), w["W3a"], bias=w["b3"], out_f32=_body(gb), want_bf16=False)
    _same(_body(gb), c["gb"], "group bias")
    _guards_intact(gb, gbo, "group bias")
    h3, h3o = _guarded(M, 512, torch.bfloat16)
    ops.gemm(c["h2"].to(DEV), w["W3b"], act=ops.ACT_RELU, group_bias=c["gb"].to(DEV), group_rows=Mg, out_bf16=_body(h3))
    _same(_body(h3), c["h3"], "h3")
    _guards_intact(h3, h3o, "h3")
    h3r = c["h3"].to(DEV)
    for n_out in er.N_OUT:
        W4, b4 = w[n_out]
        want = c["tok"][:, :n_out]
        for want16 in (False, True):
            (t32, t32o), (t16, t16o) = _guarded(groups, n_out, torch.float32), _guarded(groups, n_out, torch.bfloat16)
            ops._call("cmdiad_gemm_groupmax", ops._p(h3r), ops._p(W4), ops._p(b4), groups, Mg, n_out, 512, ops._p(_body(t32)),
                      ops._p(_body(t16)) if want16 else None, ops._stream())
            _same(_body(t32), want, f"tokens {n_out} (fp32)")
            _guards_intact(t32, t32o, f"tokens {n_out} (fp32)")
            if want16:
                _same(_body(t16), want.to(torch.bfloat16), f"tokens {n_out} (bf16)")
            _guards_intact(t16, t16o, f"tokens {n_out} (bf16)", None if want16 else slice(None))


def _segs(groups):
    proper = [d for d in range(2, groups) if groups % d == 0]
    return sorted({0, 1, groups, *proper[:1]})


def _check_tail(ops, groups, Mg, n_out):
    c, w = _case(groups, Mg), _weights()
    W4, b4 = w[n_out]
    h2, gb, want = c["h2"].to(DEV), c["gb"].to(DEV), c["tok"][:, :n_out]
    for seg in (_segs(groups) if n_out == 256 else [0]):
        rows = groups + (groups // seg if seg else 0)
        tok, toko = _guarded(rows, n_out, torch.float32)
        ops.encoder_tail_n(h2, gb, w["W3b"], W4, b4, groups, Mg, seg=seg, out=_body(tok))
        gi = torch.arange(groups)
        dst = (gi + gi // seg + 1) if seg else gi
        _same(_body(tok)[dst.to(DEV)], want, f"tail {n_out} seg {seg}")
        cls = torch.ones(rows, dtype=torch.bool)
        cls[dst] = False
        _guards_intact(tok, toko, f"tail {n_out} seg {seg}", cls.to(DEV))
        assert int(cls.sum()) == (groups // seg if seg else 0)


# ------------------------------------------------------------------------------------------------ production library
@pytest.mark.parametrize("groups,Mg", er.GRID, ids=IDS)
def test_encoder_stage1_exact(ops, groups, Mg):
    """h2, the fp32 group maxima (taken before h2's rounding) and their bf16 copy: persistent kernel at whole tiles, the
    once-per-block kernel at ragged row counts"""
    _check_stage1(ops, groups, Mg)


@pytest.mark.parametrize("panel_min", [None, "1"], ids=["tiles", "panel"])
@pytest.mark.parametrize("groups,Mg", er.GRID, ids=IDS)
def test_encoder_two_kernel_path_exact(ops, groups, Mg, panel_min, monkeypatch):
    """gb = gemm(g16, W3a, b3); h3 = gemm(h2, W3b, ReLU, group bias, group_rows = Mg); tokens = gemm_groupmax(h3, W4, b4) at both
    widths, fp32 and bf16; again with one block walking every N tile of its M panel"""
    if panel_min:
        monkeypatch.setenv("CMDIAD_GEMM_PANEL_MIN", panel_min)
    _check_two_kernel_path(ops, groups, Mg)


@pytest.mark.parametrize("n_out", er.N_OUT)
@pytest.mark.parametrize("groups,Mg", er.GRID, ids=IDS)
def test_encoder_tail_exact(ops, groups, Mg, n_out):
    """cmdiad_encoder_tail_n at 384 and 256 columns; at 256 also scattered behind one leading row per cloud of `seg` groups
    (seg = 1, a proper divisor, all groups): those rows and the guard rows keep their pattern"""
    _check_tail(ops, groups, Mg, n_out)


@pytest.mark.parametrize("n_out", er.N_OUT)
@pytest.mark.parametrize("groups,Mg", er.CHAIN, ids=[f"{g}x{m}" for g, m in er.CHAIN])
def test_encoder_chain_exact(ops, groups, Mg, n_out):
    """coordinates -> tokens as PackedPointMAE.encode / PackedPointBERT.encode string the kernels: stage 1, the group-bias
    product on stage 1's bf16 maxima, the tail on stage 1's h2"""
    c, w = _case(groups, Mg), _weights()
    W4, b4 = w[n_out]
    h2, _, g16 = ops.encoder_stage1(c["xyz"].to(DEV), w["w1b1"], w["W2"], w["b2"], groups, Mg)
    gb, _ = ops.gemm(g16, w["W3a"], bias=w["b3"], want_f32=True, want_bf16=False)
    if n_out == 384:
        tok = ops.encoder_tail(h2, gb, w["W3b"], W4, b4, groups, Mg)
        _same(tok, c["tok"], "tokens")
    else:
        out = torch.full((groups + 1, 256), 7.0, dtype=torch.float32, device=DEV)
        ops.encoder_tail_n(h2, gb, w["W3b"], W4, b4, groups, Mg, seg=groups, out=out)
        _same(out[1:], c["tok"][:, :256], "tokens")
        assert bool((out[0] == 7.0).all())


def _check_groupmax(ops, N, K, groups, Mg):
    c = er.groupmax_case(N, K, groups, Mg)
    er.check_groupmax_preconditions(c["stats"], N, Mg)
    er.check_groupmax_preconditions(c["stats_nb"], N, Mg)
    A, W, bias = c["A"].to(torch.bfloat16).to(DEV), c["W"].to(torch.bfloat16).to(DEV), c["bias"].to(DEV)
    assert torch.equal(A.float().cpu(), c["A"])
    for with_bias in (True, False):
        want = c["out"] if with_bias else c["out_nb"]
        for want16 in (True, False):
            (t32, t32o), (t16, t16o) = _guarded(groups, N, torch.float32), _guarded(groups, N, torch.bfloat16)
            ops._call("cmdiad_gemm_groupmax", ops._p(A), ops._p(W), ops._p(bias) if with_bias else None, groups, Mg, N, K,
                      ops._p(_body(t32)), ops._p(_body(t16)) if want16 else None, ops._stream())
            what = f"groupmax N={N} K={K} bias={with_bias}"
            _same(_body(t32), want, what)
            _guards_intact(t32, t32o, what)
            if want16:
                _same(_body(t16), want.to(torch.bfloat16), what + " (bf16)")
            _guards_intact(t16, t16o, what + " (bf16)", None if want16 else slice(None))


@pytest.mark.parametrize("N,K,groups,Mg", er.GROUPMAX_GRID)
def test_gemm_groupmax_off_the_encoder_shape_exact(ops, N, K, groups, Mg):
    """cmdiad_gemm_groupmax at what its entry point accepts (N % 4 == 0, K % 64 == 0) beyond the encoder's 384 / 256 x 512: one
    column group, a ragged second N tile, one and three K-steps; with and without bias, with and without the bf16 output"""
    _check_groupmax(ops, N, K, groups, Mg)


# ------------------------------------------------------------------------------------------------ test-only build
# The superseded formulations (csrc/ab/*.inc) must give the same bits; the switches are read per call.  tests/test_gpu_variants.py
# runs these (-k exact_variant) in a child process that loads the test-only library.
@pytest.mark.parametrize("switch", ["CMDIAD_STAGE1_PERSIST", "CMDIAD_STAGE1_ONCE"])
@pytest.mark.parametrize("groups,Mg", er.GRID, ids=IDS)
def test_encoder_stage1_exact_variant(ops, groups, Mg, switch, monkeypatch):
    need_ab_variants(f"{switch}=0")
    monkeypatch.setenv(switch, "0")
    _check_stage1(ops, groups, Mg)


@pytest.mark.parametrize("wide", ["4", "8"])
@pytest.mark.parametrize("groups,Mg", er.GRID, ids=IDS)
def test_encoder_two_kernel_path_exact_variant(ops, groups, Mg, wide, monkeypatch):
    need_ab_variants(f"CMDIAD_GEMM_WIDE={wide}")
    monkeypatch.setenv("CMDIAD_GEMM_WIDE", wide)
    _check_two_kernel_path(ops, groups, Mg)


@pytest.mark.parametrize("wide", ["4", "8"])
@pytest.mark.parametrize("N,K,groups,Mg", er.GROUPMAX_GRID)
def test_gemm_groupmax_off_the_encoder_shape_exact_variant(ops, N, K, groups, Mg, wide, monkeypatch):
    need_ab_variants(f"CMDIAD_GEMM_WIDE={wide}")
    monkeypatch.setenv("CMDIAD_GEMM_WIDE", wide)
    _check_groupmax(ops, N, K, groups, Mg)


@pytest.mark.parametrize("pp", ["0", "1"])
@pytest.mark.parametrize("groups,Mg", er.GRID, ids=IDS)
def test_encoder_tail_exact_variant(ops, groups, Mg, pp, monkeypatch):
    need_ab_variants(f"CMDIAD_TAIL_PP={pp}")
    monkeypatch.setenv("CMDIAD_TAIL_PP", pp)
    _check_tail(ops, groups, Mg, 384)
