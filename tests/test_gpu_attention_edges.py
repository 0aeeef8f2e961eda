"""LayerNorm -> cmdiad_gemm_qkv -> cmdiad_attention -> proj / fc1 / fc2 (csrc/blocks.cpp) at the token counts the production
geometries never reach: single-token images, T below one key tile, T that is no multiple of 64 or 32, M below one 128-row tile,
a 128-row tile that spans many images.

  QKV head-split     exact: integer operands for which acc, acc + bias and fma(acc, row_scale, bias) are exact in fp32 in any
                     order, against a float32 CPU reference, bit for bit; the padding holds 7.0 before and after.
  attention routing  exact: every query selects one key (or two tied ones) by an 11-bit +-1 code of the key index; all scores are
                     integers, P is 1 or <= 2^-40, l is 1 or 2: the output is v[perm(t)] (or the mean of two rows) bit for bit,
                     also with poisoned padding in q, k and v^T.
  attention, random  operands with a planted spike against the float64 tile model (tests/attn_ref.py), one bf16 step per
                     element, the share of not-nearest roundings pooled over the grid.
  block entry point  cmdiad_transformer_block_fwd against its separate launches, bit for bit, unfolded and folded; the stage by
                     stage float64 check of tests/test_gpu_nets.py on three small geometries.
The CPU side (the model, the fp32 emulation of the kernel's loop, the routing inputs) is pinned by tests/test_attn_ref_cpu.py."""
import functools
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import attn_ref as ar  # noqa: E402
from block_stages import FRAC_OFF, STAGES, stage_by_stage  # noqa: E402
from cmdiad_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ QKV head-split, exact
@functools.lru_cache(maxsize=None)
def _qkv_case(B, T, C):
    """operands on the device and the three references (with bias / without / with bias and row_scale), computed once"""
    A, W, bias, rs = ar.qkv_exact_operands(B, T, C)
    refs = {"bias": ar.qkv_exact_reference(A, W, bias, None, B, T), "nobias": ar.qkv_exact_reference(A, W, None, None, B, T),
            "rowscale": ar.qkv_exact_reference(A, W, bias, rs, B, T)}
    return A.to(DEV), W.to(DEV), bias.to(DEV), rs.to(DEV), refs


def _check_qkv(bufs, ref, T, what):
    """the valid part equals the reference bit for bit; every padding element still holds the fill value"""
    (q, k, vt), (rq, rk, rvt) = bufs, ref
    assert torch.equal(q[:, :, :T].cpu(), rq), (what, "q")
    assert torch.equal(k[:, :, :T].cpu(), rk), (what, "k")
    assert torch.equal(vt[:, :, :, :T].cpu(), rvt), (what, "v^T")
    for name, pad in (("q", q[:, :, T:]), ("k", k[:, :, T:]), ("v^T", vt[:, :, :, T:])):
        assert bool((pad == ar.PAD_FILL).all()), (what, name, "padding was written")


@pytest.fixture(scope="module")
def vrows0_outputs(tmp_path_factory):
    """{(B, T, C): (q, k, vt)} of the with-bias form from a process that runs with CMDIAD_QKV_VROWS=0 (the switch is read once
    per process): tests/qkv_vrows_worker.py, one run for the whole grid"""
    path = str(tmp_path_factory.mktemp("qkv_vrows0") / "out.pt")
    env = dict(os.environ, CMDIAD_QKV_VROWS="0")
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "qkv_vrows_worker.py"), path], capture_output=True, text=True,
                         timeout=300, env=env, cwd=REPO)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return torch.load(path)


@pytest.mark.parametrize("B,T,C", ar.QKV_GRID)
@pytest.mark.parametrize("form", ["bias", "nobias", "rowscale"])
def test_qkv_head_split_exact(form, B, T, C):
    """Integer A in [-4, 4], integer W in [-2, 2], bias in quarters, row_scale in powers of two: k = bf16(acc + bias), v likewise
    and transposed, q = bf16((acc + bias) * fp32(0.125 log2 e)), equal to the float32 CPU reference in every bit; rows / columns
    T .. Tp-1 of the three buffers are never written."""
    assert os.environ.get("CMDIAD_QKV_VROWS") != "0"            # this process runs the default (row-store) V^T form
    A, W, bias, rs, refs = _qkv_case(B, T, C)
    bufs = ar.qkv_filled_buffers(B, C // 64, T, DEV)
    ops.gemm_qkv(A, W, None if form == "nobias" else bias, B, T, *bufs, row_scale=rs if form == "rowscale" else None)
    _check_qkv(bufs, refs[form], T, (form, B, T, C))


@pytest.mark.parametrize("B,T,C", ar.QKV_GRID)
def test_qkv_head_split_exact_direct_v_stores(B, T, C, vrows0_outputs):
    """CMDIAD_QKV_VROWS=0 (V^T tiles stored in the direct form everywhere): the reference's bits, hence the default form's,
    padding included."""
    A, W, bias, _, refs = _qkv_case(B, T, C)
    got = vrows0_outputs[(B, T, C)]
    _check_qkv(got, refs["bias"], T, ("vrows0", B, T, C))
    bufs = ar.qkv_filled_buffers(B, C // 64, T, DEV)
    ops.gemm_qkv(A, W, bias, B, T, *bufs)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(got, bufs))


# ------------------------------------------------------------------------------------------------ attention routing, exact
def _head_layout(q, k, v, T):
    """[B,H,T,64] float32 -> q, k [B,H,Tp,64] and v^T [B,H,64,Tp] bf16 on the device, zero padding"""
    B, H = q.shape[:2]
    Tp = (T + 63) // 64 * 64
    qd = torch.zeros((B, H, Tp, 64), dtype=torch.bfloat16, device=DEV)
    kd = torch.zeros_like(qd)
    vtd = torch.zeros((B, H, 64, Tp), dtype=torch.bfloat16, device=DEV)
    qd[:, :, :T], kd[:, :, :T], vtd[:, :, :, :T] = q.to(DEV), k.to(DEV), v.transpose(-1, -2).to(DEV)
    return qd, kd, vtd


def _poison_padding(qd, kd, vtd, T, seed):
    """k padding: 4 x the key rows of indices 0, 1, ... (index 0 and T-1 are hot for some query by construction: unmasked, such a
    row scores 800 or more against 220); q padding: random +-1 codes; v^T padding: 3.0 (finite: it is multiplied by exact zeros)"""
    Tp = qd.shape[2]
    if Tp == T:
        return
    g = torch.Generator().manual_seed(seed)
    B, H = qd.shape[:2]
    kd[:, :, T:, :ar.CODE_BITS] = (80.0 * ar.code(torch.arange(Tp - T) % T)).to(torch.bfloat16).to(DEV)
    qd[:, :, T:, :ar.CODE_BITS] = (torch.randint(0, 2, (B, H, Tp - T, ar.CODE_BITS), generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    vtd[:, :, :, T:] = 3.0


@pytest.mark.parametrize("B,H,T,kind", ar.routing_cases(), ids=lambda v: str(v))
def test_attention_routing_exact(B, H, T, kind):
    """out[b*T + t, h*64 + d] = v[b, h, perm(t), d] (one_hot) or the mean of the two tied rows (two_hot<bit>: bit 2 puts the pair on
    the two lane halves, 5 on the two 32-key sub-tiles, 6 and 7 in different key tiles), bit for bit; and the same bits with
    poisoned padding.  A key mask off by one, a swapped head / batch stride, a transposed V index or a dropped lane half in the
    row sum each fail this by whole values."""
    q, k, v, want = ar.routing_inputs(B, H, T, kind, ar.routing_seed(B, H, T))
    qd, kd, vtd = _head_layout(q, k, v, T)
    out = ops.attention(qd, kd, vtd, B, H, T)
    want = want.permute(0, 2, 1, 3).reshape(B * T, H * 64).to(torch.bfloat16)
    got = out.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"
    _poison_padding(qd, kd, vtd, T, 5 + T)
    again = ops.attention(qd, kd, vtd, B, H, T).cpu()
    assert torch.equal(again, got), f"poisoned padding changed {int((again != got).sum())} elements"


# ------------------------------------------------------------------------------------------------ attention, random operands
@functools.lru_cache(maxsize=None)
def _edge_case(B, H, T):
    """one case of the random-operand grid: the per-element bound asserted, -> (elements not nearest, elements)"""
    q, k, v = ar.spiked_operands(B, H, T, ar.edge_seed(B, H, T))
    a_ref, peak, _ = ar.attention_tile_model(q, k, v, T)
    out = ops.attention(*_head_layout(q, k, v, T), B, H, T)
    to_rows = lambda t: t.transpose(1, 2).reshape(B * T, H * 64)            # noqa: E731
    off = ar._ulp_check(out, to_rows(a_ref), f"attention B={B} H={H} T={T}", max_ulps=1.05, frac_off=1.0,
                        abs_slack=to_rows(ar.attention_slack(peak, v.double(), a_ref)))
    return off * a_ref.numel(), a_ref.numel()


@pytest.mark.parametrize("T", ar.EDGE_T)
@pytest.mark.parametrize("B,H", ar.EDGE_BH)
def test_attention_random_operands_edge_lengths(B, H, T):
    """q = 0.3 randn, k, v = randn with one planted spike per head in the last key tile: every output within 1.05 bf16 steps (+ the
    stage test's slack) of the float64 tile model."""
    _edge_case(B, H, T)


def test_attention_random_operands_pooled_share():
    """The share of outputs that are not the nearest bf16 of the model's value, pooled over the whole grid, against the
    stage's threshold (tests/block_stages.py FRAC_OFF).  tests/test_attn_ref_cpu.py prints the same figure for the fp32
    emulation of the kernel's loop on the same operands."""
    cases = [_edge_case(B, H, T) for B, H in ar.EDGE_BH for T in ar.EDGE_T]
    miss, total = sum(c[0] for c in cases), sum(c[1] for c in cases)
    print(f"attention, not the nearest bf16 of the model's value, pooled over the grid: {miss / total:.2e} ({round(miss)} of {total})")
    assert miss / total <= FRAC_OFF["attention"]


# ------------------------------------------------------------------------------------------------ block entry point
def block_state_dict(C, hidden, qkv_bias, seed):
    """One random pre-LN block under the key names runtime._pack_block reads (prefix ""), scaled as oracle.nets.synth_state_dict
    scales its blocks: matrices randn / sqrt(fan_in), biases 0.02 randn, LayerNorm gamma 1 + 0.1 randn."""
    g = torch.Generator().manual_seed(seed)
    mat = lambda n, k: torch.randn((n, k), generator=g) / k ** 0.5          # noqa: E731
    vec = lambda n: 0.02 * torch.randn((n,), generator=g)                   # noqa: E731
    sd = {"norm1.weight": 1.0 + 0.1 * torch.randn((C,), generator=g), "norm1.bias": vec(C),
          "norm2.weight": 1.0 + 0.1 * torch.randn((C,), generator=g), "norm2.bias": vec(C),
          "attn.qkv.weight": mat(3 * C, C), "attn.proj.weight": mat(C, C), "attn.proj.bias": vec(C),
          "mlp.fc1.weight": mat(hidden, C), "mlp.fc1.bias": vec(hidden), "mlp.fc2.weight": mat(C, hidden), "mlp.fc2.bias": vec(C)}
    if qkv_bias:
        sd["attn.qkv.bias"] = vec(3 * C)
    return sd


@pytest.mark.parametrize("B,T,C,hidden", [(1, 1, 128, 512), (3, 43, 128, 512), (1, 65, 384, 1536), (2, 197, 384, 1536),
                                          (1, 257, 768, 3072), (40, 5, 128, 256)])
@pytest.mark.parametrize("fold", ["0", "1"])
def test_block_entry_point_equals_separate_launches(fold, B, T, C, hidden, monkeypatch):
    """Three blocks on one residual stream through cmdiad_transformer_block_fwd and as separate entry-point calls: identical
    bits, finite.  Folded: with pos and the flags chained as PackedPointMAE chains them (block 1's output is read, so block 0
    prepares block 1's LayerNorm, block 1 prepares nothing)."""
    from cmdiad_amd.runtime import _QkvBuffers, _pack_block, block_flags, transformer_block, transformer_block_unfused
    monkeypatch.setenv("CMDIAD_LN_FOLD", fold)
    monkeypatch.delenv("CMDIAD_PMAE_MLP", raising=False)
    qkv_bias, eps, n = C != 384, 1e-5 if C == 384 else 1e-6, 3
    blocks = [_pack_block(block_state_dict(C, hidden, qkv_bias, 40 + i), "", DEV, qkv_bias) for i in range(n)]
    assert ("qkv_wf" in blocks[0]) == (fold == "1")
    g = torch.Generator().manual_seed(B * T + C)
    x0 = torch.randn((B * T, C), generator=g).to(DEV)
    pos = (0.1 * torch.randn((B * T, C), generator=g)).to(DEV) if fold == "1" or C == 384 else None
    xa, xb, ba, bb, state = x0.clone(), x0.clone(), _QkvBuffers(), _QkvBuffers(), {}
    for i, blk in enumerate(blocks):
        fl = block_flags(i, n, fold == "1", (1,))
        transformer_block(xa, blk, B, T, C // 64, eps, ba, pos=pos, flags=fl)
        transformer_block_unfused(xb, blk, B, T, C // 64, eps, bb, pos=pos, flags=fl, state=state)
        assert torch.equal(xa, xb), (i, float((xa - xb).abs().max()))
    assert bool(torch.isfinite(xa).all()) and not torch.equal(xa, x0)


STAGE_GEOMETRIES = ((2, 65, 128), (3, 43, 384), (1, 257, 768))


@functools.lru_cache(maxsize=None)
def _stage_case(B, T, C):
    qkv_bias = C != 384                      # 384 as Point-MAE runs it: no qkv bias, the positional re-add, eps 1e-5
    sd = block_state_dict(C, 4 * C, qkv_bias, 60 + C)
    g = torch.Generator().manual_seed(B * T + C)
    x0 = torch.randn((B * T, C), generator=g)
    pos = None if qkv_bias else 0.1 * torch.randn((B * T, C), generator=g)
    return stage_by_stage(sd, "", B, T, C, C // 64, 1e-6 if qkv_bias else 1e-5, qkv_bias, x0, pos, f"(B, T, C) = {(B, T, C)}", pooled=True)


@pytest.mark.parametrize("B,T,C", STAGE_GEOMETRIES)
def test_block_stage_by_stage_small_geometries(B, T, C):
    """The body of test_transformer_block_stage_by_stage_vs_fp64 (tests/block_stages.py) with its per-element bounds."""
    _stage_case(B, T, C)


def test_block_stage_by_stage_small_geometries_pooled_shares():
    """... and its per-stage shares of not-nearest roundings, pooled over the three geometries, against the same thresholds."""
    cases = [_stage_case(*geo) for geo in STAGE_GEOMETRIES]
    for stage in STAGES:
        miss, total = sum(c[stage][0] * c[stage][1] for c in cases), sum(c[stage][1] for c in cases)
        print(f"{stage}: not nearest, pooled over {STAGE_GEOMETRIES}: {miss / total:.2e} ({round(miss)} of {total})")
        assert miss / total <= FRAC_OFF[stage], stage
