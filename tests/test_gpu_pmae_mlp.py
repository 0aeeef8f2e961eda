"""The fused Point-MAE MLP (csrc/mlp_fused.hip: fc1 + GELU + fc2 in one kernel, hidden kept on chip) against the same blocks issued
as separate entry-point launches: bit for bit, on the production shape, a ragged row count, every LayerNorm-fold flag combination
of a Point-MAE chain (PREP_NEXT with pos, LN1_READY, a fetch layer without PREP_NEXT), heavy-tailed operands, and on both sides
of the dispatch threshold (CMDIAD_PMAE_MLP unset)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cmdiad_amd import runtime  # noqa: E402
from oracle import nets  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, H, EPS, READ_AFTER = 384, 6, 1e-5, (1,)
_SENTINEL = 0x7FC5A5A5   # a quiet NaN with a payload no computation produces


def _heavy_tailed(sd, n_blocks):
    """Massive-activation style operands: a few fc1 / fc2 rows and columns at 20-40x (the products then see hidden values and
    partial sums far outside O(1), where any change of the accumulation order would show in the low bits)."""
    sd = dict(sd)
    for i in range(n_blocks):
        p = f"blocks.blocks.{i}.mlp."
        w1, w2 = sd[p + "fc1.weight"].clone(), sd[p + "fc2.weight"].clone()
        w1[[5, 700, 1535]] *= 30.0
        w1[:, 37] *= 20.0
        w2[:, [3, 900]] *= 40.0
        w2[200] *= 25.0
        sd[p + "fc1.weight"], sd[p + "fc2.weight"] = w1, w2
    return sd


def _chain(B, T, fused, monkeypatch, heavy=False, n_blocks=4):
    """n consecutive Point-MAE blocks on one residual stream, flags chained as PackedPointMAE does (block 1 is a fetch layer).
    fused: "1" / "0" / None (CMDIAD_PMAE_MLP forced on / off / unset) for cmdiad_transformer_block_fwd; "ref": the same blocks
    as separate launches (runtime.transformer_block_unfused)."""
    from cmdiad_amd.runtime import _QkvBuffers, _pack_block, block_flags, transformer_block, transformer_block_unfused
    monkeypatch.setenv("CMDIAD_LN_FOLD", "1")
    if fused in ("0", "1"):
        monkeypatch.setenv("CMDIAD_PMAE_MLP", fused)
    else:
        monkeypatch.delenv("CMDIAD_PMAE_MLP", raising=False)
    sd = nets.outlier_pointmae(21) if heavy else nets.synth_state_dict("pointmae", 21)
    if heavy:
        sd = _heavy_tailed(sd, n_blocks)
    blocks = [_pack_block(sd, f"blocks.blocks.{i}.", DEV, False) for i in range(n_blocks)]
    assert "fc1_wf" in blocks[0]
    g = torch.Generator().manual_seed(B * T)
    x = torch.randn(B * T, C, generator=g)
    if heavy:
        x[:, [7, 100]] *= 60.0              # residual channels two orders of magnitude above the rest
        x[::97] *= 8.0                      # and high-norm tokens
    # the residual stream is the leading B * T rows of a buffer with 16 guard rows behind it, which no launch may touch
    buf = torch.full((B * T + 16, C), _SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    x, x_cpu = buf[:B * T], x
    x.copy_(x_cpu)
    pos = (0.1 * torch.randn(B * T, C, generator=g)).to(DEV)
    bufs, state, taps = _QkvBuffers(), {}, []
    for i, blk in enumerate(blocks):
        fl = block_flags(i, n_blocks, True, READ_AFTER)
        if fused == "ref":
            transformer_block_unfused(x, blk, B, T, H, EPS, bufs, pos=pos, flags=fl, state=state)
        else:
            transformer_block(x, blk, B, T, H, EPS, bufs, pos=pos, flags=fl)
        if i in READ_AFTER:
            taps.append(x.clone())
    torch.cuda.synchronize()
    assert bool((buf[B * T:].view(torch.int32) == _SENTINEL).all()), "rows past M were written"
    return x, taps


def _same(a, b):
    xa, ta = a
    xb, tb = b
    assert torch.isfinite(xa).all()
    assert torch.equal(xa, xb), float((xa - xb).abs().max())
    assert len(ta) == len(tb) and all(torch.equal(u, v) for u, v in zip(ta, tb))


@pytest.mark.parametrize("B,T", [(32, 1024), (3, 1000), (1, 1024), (2, 200), (1, 1), (1, 65), (3, 43), (1, 127), (1, 9), (1, 120), (1, 137)])
def test_fused_mlp_block_equals_separate_launches(B, T, monkeypatch):
    """CMDIAD_PMAE_MLP=1: every row count, ragged ones included (M = 3 000, 400: the last 128-row tile is partial, the last
    waves of it have no live row at all; M = 1, 65, 127: a single partial tile; M = 129: one row in the second; M = 9, 120, 137:
    a wave with exactly one of its upper eight rows live, the tile's last wave with its upper eight dead, and the first case
    again in a second tile).  The residual
    stream has guard rows behind it (_chain): the epilogue's row test must keep every store below M."""
    _same(_chain(B, T, "1", monkeypatch), _chain(B, T, "ref", monkeypatch))


def test_fused_mlp_heavy_tailed_operands(monkeypatch):
    _same(_chain(3, 1024, "1", monkeypatch, heavy=True), _chain(3, 1024, "ref", monkeypatch, heavy=True))


@pytest.mark.parametrize("B", [23, 24])
def test_dispatch_threshold_both_sides(B, monkeypatch):
    """Unset switch: M = 23 552 runs the two launches, M = 24 576 the fused kernel; both give the bits of the separate launches
    and of the forced forms."""
    got = _chain(B, 1024, None, monkeypatch, n_blocks=2)
    _same(got, _chain(B, 1024, "ref", monkeypatch, n_blocks=2))
    _same(got, _chain(B, 1024, "1" if B == 23 else "0", monkeypatch, n_blocks=2))


def test_fused_mlp_is_not_used_for_the_unfolded_or_vit_blocks(monkeypatch):
    """CMDIAD_PMAE_MLP=1 leaves the blocks it cannot serve on their launches: the unfolded form and the ViT geometry still agree
    with their separate-launch forms."""
    from cmdiad_amd.runtime import _QkvBuffers, _pack_block, transformer_block, transformer_block_unfused
    monkeypatch.setenv("CMDIAD_PMAE_MLP", "1")
    for kind, fold, B, T, c, h, eps, fmt, qkv_bias in (("pointmae", "0", 2, 1024, 384, 6, 1e-5, "blocks.blocks.0.", False),
                                                        ("vit", "1", 2, 785, 768, 12, 1e-6, "blocks.0.", True)):
        monkeypatch.setenv("CMDIAD_LN_FOLD", fold)
        blk = _pack_block(nets.synth_state_dict(kind, 31), fmt, DEV, qkv_bias)
        x0 = torch.randn(B * T, c, generator=torch.Generator().manual_seed(5)).to(DEV)
        xa, xb = x0.clone(), x0.clone()
        transformer_block(xa, blk, B, T, h, eps, _QkvBuffers())
        transformer_block_unfused(xb, blk, B, T, h, eps, _QkvBuffers())
        torch.cuda.synchronize()
        assert torch.equal(xa, xb), kind
