"""One transformer block kernel by kernel against float64 arithmetic on the GPU's own input of every stage: the body shared by
tests/test_gpu_nets.py (production geometries) and tests/test_gpu_attention_edges.py (small ones).  Needs a GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_ref import _ulp_check, attention_tile_model  # noqa: E402

DEV = "cuda"
STAGES = ("LayerNorm 1", "q", "k", "v", "attention", "LayerNorm 2", "fc1 + GELU")
# the share of a stage's bf16 outputs that may be a neighbour of the float64 value's nearest bf16 instead of the nearest itself
FRAC_OFF = {"LayerNorm 1": 2e-3, "q": 2e-3, "k": 2e-3, "v": 2e-3, "attention": 5e-3, "LayerNorm 2": 2e-3, "fc1 + GELU": 3e-2}


def stage_by_stage(sd, prefix, B, T, C, H, eps, qkv_bias, x0, pos, label, pooled=False):
    """models/models.py:126-180 kernel by kernel on the residual stream x0 [B*T, C] (pos [B*T, C] or None: the positional re-add):
    LayerNorm, qkv projection with head-split stores, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual.  bf16
    outputs: within one bf16 step of the exact value everywhere, and all but FRAC_OFF[stage] of them the nearest bf16; fp32
    outputs (the residual stream): 2e-5 of the feature scale.  -> {stage: (share not nearest, elements)}.  pooled: the per-element
    bounds only; the caller holds the shares, summed over its geometries, to FRAC_OFF."""
    from cmdiad_amd import ops
    from cmdiad_amd.runtime import _QkvBuffers, _pack_block, transformer_block_unfused
    from oracle.nets_rounded import LOG2E, r16
    with_pos = pos is not None
    blk = _pack_block(sd, prefix, DEV, qkv_bias)          # (no fold: this test pins the separate launches)
    W = lambda k: sd[prefix + k].double()                                  # noqa: E731
    Wb = lambda k: r16(sd[prefix + k])                                     # noqa: E731  (weights as the kernels hold them)
    frac = lambda stage: 1.0 if pooled else FRAC_OFF[stage]                # noqa: E731
    x = x0.to(DEV)
    M, hd = B * T, 64
    off = {}
    # ---- LayerNorm 1 (+ pos): x <- x + pos in place, h = bf16(LN(x))
    h = ops.layernorm(x, blk["ln1_w"], blk["ln1_b"], eps, add=pos.to(DEV) if with_pos else None)
    x_ref = x0.double() + (pos.double() if with_pos else 0.0)
    np.testing.assert_allclose(x.cpu().double().numpy(), x_ref.float().double().numpy(), rtol=0, atol=0)      # one fp32 add: exact
    ln = lambda v, n: torch.nn.functional.layer_norm(v, (C,), W(n + ".weight"), W(n + ".bias"), eps)   # noqa: E731
    off["LayerNorm 1"] = (_ulp_check(h, ln(x.cpu().double(), "norm1"), "LayerNorm 1", frac_off=frac("LayerNorm 1")), h.numel())
    # ---- qkv: q = bf16((h.Wq^T + b) * hd^-0.5 * log2 e), k, v = bf16(h.W^T + b), head-split, v transposed
    q, k, vt = _QkvBuffers().get(B, H, T, DEV)
    ops.gemm_qkv(h, blk["qkv_w"], blk["qkv_b"], B, T, q, k, vt)
    qkv = h.cpu().double() @ Wb("attn.qkv.weight").T + (W("attn.qkv.bias") if qkv_bias else 0.0)
    qkv = qkv.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)               # [3,B,H,T,64]
    scale = float(torch.tensor(hd ** -0.5 * LOG2E, dtype=torch.float32))
    n_head = B * H * T * hd
    off["q"] = (_ulp_check(q[:, :, :T], qkv[0].float().double() * scale, "q", max_ulps=1.01, frac_off=frac("q")), n_head)   # (the scale multiplies the fp32 value)
    off["k"] = (_ulp_check(k[:, :, :T], qkv[1], "k", frac_off=frac("k")), n_head)
    off["v"] = (_ulp_check(vt[:, :, :, :T].transpose(-1, -2), qkv[2], "v", frac_off=frac("v")), n_head)
    assert not bool(q[:, :, T:].any()) and not bool(k[:, :, T:].any()) and not bool(vt[:, :, :, T:].any())   # padding stays zero
    # ---- attention on the GPU's own q, k, v: keys in tiles of 64, P = bf16(exp2(S - reference)), row sum of the unrounded exp2.
    # The reference is the first tile's maximum and moves up only when some query of the WAVE (32 consecutive queries) meets a
    # score more than 8 (log2 units) above its own; then every query of that wave moves to its running maximum (csrc/attention.hip;
    # the model is tests/attn_ref.py attention_tile_model)
    a = ops.attention(q, k, vt, B, H, T)
    vd = vt[:, :, :, :T].transpose(-1, -2).cpu().double()
    stats = {}
    o64, peak, _ = attention_tile_model(q, k, vt.transpose(-1, -2), T, stats)
    print(f"  [attention model: the reference moved in {stats['moved']} of {(T // 64) * B * H} (head, later tile) pairs]")
    a_ref = o64.transpose(1, 2).reshape(M, C)
    # A P element whose rounding falls the other way (1 in ~3 000: the fp32 scores carry ~1e-6 of absolute error) moves every output
    # of its query by one bf16 step of that weight times the value: <= 2^-8 (p_i / l) |v_i|.  Under uniform attention that is 4e-5
    # of the output scale, with a dominant key (weight 0.1 ... 0.6) up to 1.5e-2 of it -- whole rows then sit one P step away
    # (tools/attn_diag.py lists them).  The slack is exactly that bound per (query, column): 2^-7 x the query's largest weight x
    # the column's largest |v| (two such flips).  With THIS model of the P rounding 99.94 % of the outputs are the nearest bf16 of
    # the float64 value; with P rounded against the final maximum, or not rounded, only 75-79 % are (same tool).
    slack = 2.0 ** -7 * peak[..., None] * vd.abs().amax(2)[:, :, None, :]                      # [B,H,T,64]
    slack = slack.transpose(1, 2).reshape(M, C) + 1e-5 * float(a_ref.abs().mean())
    off["attention"] = (_ulp_check(a, a_ref, "attention", max_ulps=1.05, frac_off=frac("attention"), abs_slack=slack), a.numel())
    # ---- proj + residual (fp32, in place)
    ops.gemm(a, blk["proj_w"], bias=blk["proj_b"], residual=x, out_f32=x, want_bf16=False)
    x_ref = x_ref.float().double() + (a.cpu().double() @ Wb("attn.proj.weight").T + W("attn.proj.bias"))
    scale_x = float(x_ref.abs().mean())
    # fp32 outputs: 2e-5 of the feature scale -- plus, for the heavy-tailed stream, fp32's own relative step on the 100x elements
    # (a value of 4 000 carries 2.4e-4 of absolute rounding per fp32 operation: 1e-6 of ITS size)
    assert bool(((x.cpu().double() - x_ref).abs() <= 2e-5 * scale_x + 1e-6 * x_ref.abs()).all())
    # ---- LayerNorm 2, fc1 + GELU, fc2 + residual
    h2 = ops.layernorm(x, blk["ln2_w"], blk["ln2_b"], eps)
    off["LayerNorm 2"] = (_ulp_check(h2, ln(x.cpu().double(), "norm2"), "LayerNorm 2", frac_off=frac("LayerNorm 2")), h2.numel())
    _, mid = ops.gemm(h2, blk["fc1_w"], bias=blk["fc1_b"], act=ops.ACT_GELU)
    z = h2.cpu().double() @ Wb("mlp.fc1.weight").T + W("mlp.fc1.bias")
    # erf-GELU with one transcendental (|error| <= 5.3e-7 ABSOLUTE, csrc/common.h): a visible share of a bf16 step only for the
    # small outputs, hence the absolute slack and the larger share of not-nearest roundings
    off["fc1 + GELU"] = (_ulp_check(mid, torch.nn.functional.gelu(z), "fc1 + GELU", max_ulps=1.0, frac_off=frac("fc1 + GELU"), abs_slack=1e-6), mid.numel())
    x_before = x.cpu().double()
    ops.gemm(mid, blk["fc2_w"], bias=blk["fc2_b"], residual=x, out_f32=x, want_bf16=False)
    x_ref2 = x_before + (mid.cpu().double() @ Wb("mlp.fc2.weight").T + W("mlp.fc2.bias"))
    assert bool(((x.cpu().double() - x_ref2).abs() <= 2e-5 * float(x_ref2.abs().mean()) + 1e-6 * x_ref2.abs()).all())
    print(f"{label}: fraction of bf16 outputs that are not the nearest bf16 of the float64 value, per stage: {['%.1e' % off[s][0] for s in STAGES]}")
    # the chained production entry point gives the same block output as these separate calls (bit for bit: same kernels)
    xb = x0.to(DEV)
    transformer_block_unfused(xb, blk, B, T, H, eps, _QkvBuffers(), pos=pos.to(DEV) if with_pos else None)
    assert torch.equal(xb, x)
    return off
