"""GPU parity of the three networks (bf16 MFMA, fp32 accumulate / residual stream) against the fp32
CPU oracle (oracle/nets.py, itself pinned to the reference by tests/test_oracle_golden.py) and
against the committed golden vectors.

Tolerance model: every GEMM operand is rounded to bf16 (relative 2^-9 per element); after L chained
layers the feature error is ~ sqrt(L) * 2^-8 of the feature scale.  The assertions therefore bound the
error relative to the mean absolute feature value: mean |err| <= 1.5 %, max |err| <= 12 %."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd import ops, runtime  # noqa: E402
from oracle import kernels as ok  # noqa: E402
from oracle import nets  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from block_stages import stage_by_stage  # noqa: E402

DEV = "cuda"


def _rel(got, ref):
    scale = ref.abs().mean().item()
    err = (got - ref).abs()
    return err.mean().item() / scale, err.max().item() / scale


@pytest.mark.parametrize("fold", ["0", "1"])   # LayerNorms as launches (default for the ViT) / folded into the products
def test_vit_b8_forward_vs_oracle(fold, monkeypatch):
    monkeypatch.setenv("CMDIAD_LN_FOLD", fold)
    sd = nets.synth_state_dict("vit", 31)
    rgb = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = nets.vit_forward(sd, rgb)
    got = runtime.PackedViT(sd, device=DEV).forward(rgb.to(DEV)).cpu()
    assert got.shape == (2, 768, 28, 28)
    mean_rel, max_rel = _rel(got, ref)
    assert mean_rel < 0.015 and max_rel < 0.12, (mean_rel, max_rel)


def _rel_by_channel(got, ref, ch_dim):
    """mean |err| over the mean |ref| (as _rel), and the max |err| against the mean |ref| OF ITS CHANNEL: with heavy-tailed weights
    a few channels are 50-100x the others, and an error bound in units of the global mean would measure those channels' size."""
    err = (got - ref).abs()
    dims = [d for d in range(ref.dim()) if d != ch_dim]
    scale_c = ref.abs().mean(dim=dims, keepdim=True).clamp_min(ref.abs().mean() * 0.25)    # (a near-zero channel is measured on the global scale)
    return err.mean().item() / ref.abs().mean().item(), (err / scale_c).max().item()


def test_vit_b8_forward_heavy_tailed_weights_vs_oracle():
    """the parity tests above run on O(1) synthetic weights; a real DINO ViT-B/8 has massive-activation
    channels (~100x) and high-norm tokens.  oracle.nets.outlier_vit plants both; the same bounds must hold through the bf16
    operand casts (LayerNorm -> bf16, q pre-scale, GELU hidden rows), per channel: mean <= 1.5 %, max <= 12 % of the channel's
    own scale.  The fp32 residual stream is what carries the outliers; every 16-bit operand is a LayerNorm output or an
    activation, whose rounding is RELATIVE (2^-9 of the element), so a 100x channel costs the others nothing."""
    sd = nets.outlier_vit(31)
    rgb = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = nets.vit_forward(sd, rgb)
        # the premise: the residual stream in front of the last LayerNorm really has the outliers
        x = torch.nn.functional.conv2d(rgb, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=8).flatten(2).transpose(1, 2)
        x = torch.cat([sd["cls_token"].expand(2, -1, -1), x], 1) + sd["pos_embed"]
        assert float(x[:, 400].norm()) > 5 * float(x[:, 100].norm())          # one token enters with ~8x the norm of the others
        for i in range(12):
            x = nets._block(x, sd, f"blocks.{i}", 12, 1e-6)
    typical = float(x.abs().median())
    assert float(x[:, :, 7].abs().mean()) > 60 * typical                      # ... and three channels carry ~100x the typical value
    for fold in ("0", "1"):
        os.environ["CMDIAD_LN_FOLD"] = fold
        try:
            got = runtime.PackedViT(sd, device=DEV).forward(rgb.to(DEV)).cpu()
        finally:
            del os.environ["CMDIAD_LN_FOLD"]
        mean_rel, max_rel = _rel_by_channel(got, ref, 1)
        print(f"heavy-tailed ViT, LN fold {fold}: mean {mean_rel:.4f}, max (per channel scale) {max_rel:.4f}")
        assert mean_rel < 0.015 and max_rel < 0.12, (fold, mean_rel, max_rel)


def test_pointmae_heavy_tailed_weights_vs_oracle():
    """The same for Point-MAE with one BatchNorm channel of the encoder at 50x (oracle.nets.outlier_pointmae)."""
    from cmdiad_amd.synth import synth_cloud
    from oracle import scoring
    sd = nets.outlier_pointmae(21)
    pc, _ = scoring.unorganize_no_zeros(synth_cloud(2, 0.3))
    xyz = np.ascontiguousarray(pc[0].T.numpy())[None]
    pm = runtime.PackedPointMAE(sd, device=DEV)
    feats, center, ori_idx, center_idx = pm.forward(torch.from_numpy(xyz).to(DEV))
    cidx, cen = ok.fps(xyz, 1024)
    idx, nb = ok.knn_group(xyz, cen, 128)
    np.testing.assert_array_equal(ori_idx.cpu().numpy(), idx)
    with torch.no_grad():
        ref = nets.pointmae_forward(sd, torch.from_numpy(nb), torch.from_numpy(cen))
    got = feats.transpose(1, 2).cpu()
    mean_rel, max_rel = _rel_by_channel(got, ref, 1)
    g_mean, g_max = _rel(got, ref)
    err = (got - ref).abs()
    flat = int(err.argmax())
    c, t = (flat // ref.shape[2]) % ref.shape[1], flat % ref.shape[2]
    print(f"heavy-tailed Point-MAE: mean {mean_rel:.4f}, max (per channel scale) {max_rel:.4f}; global-scale max {g_max:.4f}; largest |err| {float(err.max()):.4f} at "
          f"channel {c}, token {t}: ref {float(ref[0, c, t]):.4f} got {float(got[0, c, t]):.4f}; channel mean |ref| {float(ref[0, c].abs().mean()):.4f}, "
          f"global mean |ref| {float(ref.abs().mean()):.4f}; token error norm / token norm {float(err[0, :, t].norm() / ref[0, :, t].norm()):.4f}")
    assert mean_rel < 0.015 and max_rel < 0.12, (mean_rel, max_rel)


def test_vit_blocks_vs_reference_golden(golden):
    # the block stack against the vector produced by the reference's own Block class (GV)
    g = golden("gv_vit_blocks.npz")
    sd = nets.synth_state_dict("vit", 31)
    vit = runtime.PackedViT(sd, device=DEV)
    x = torch.randn(1, 785, 768, generator=torch.Generator().manual_seed(int(g["x_seed"]))).to(DEV).reshape(785, 768).contiguous()
    for i, blk in enumerate(vit.blocks):   # the LayerNorm fold chained across the blocks, as PackedViT.forward_tokens does
        runtime.transformer_block(x, blk, 1, 785, 12, 1e-6, vit.bufs, flags=runtime.block_flags(i, len(vit.blocks), "qkv_wf" in blk))
    ref = torch.from_numpy(g["y_sub"])
    mean_rel, max_rel = _rel(x.cpu()[::8, ::4], ref)
    assert mean_rel < 0.015 and max_rel < 0.12, (mean_rel, max_rel)


def test_pointmae_vs_reference_golden(golden):
    g = golden("g2_pointmae.npz")
    sd = nets.synth_state_dict("pointmae", 21)
    pm = runtime.PackedPointMAE(sd, device=DEV, group_size=32, num_group=64)
    xyz = torch.from_numpy(np.ascontiguousarray(g["pc"][0].T)[None]).to(DEV)
    feats, center, ori_idx, center_idx = pm.forward(xyz)
    np.testing.assert_array_equal(center_idx.cpu().numpy(), g["center_idx"])
    np.testing.assert_array_equal(center.cpu().numpy(), g["center"])
    np.testing.assert_array_equal(ori_idx.cpu().numpy().astype(np.int32), g["ori_idx"])
    ref = torch.from_numpy(g["feats_eval"])  # [1,768,64]
    mean_rel, max_rel = _rel(feats.transpose(1, 2).cpu(), ref)
    assert mean_rel < 0.015 and max_rel < 0.12, (mean_rel, max_rel)


@pytest.mark.parametrize("fold", ["pmae", "0"])   # folded (default for Point-MAE) / LayerNorms as launches
def test_pointmae_full_size_vs_oracle(fold, monkeypatch):
    monkeypatch.setenv("CMDIAD_LN_FOLD", fold)
    from cmdiad_amd.synth import synth_cloud
    from oracle import scoring
    sd = nets.synth_state_dict("pointmae", 21)
    pc, _ = scoring.unorganize_no_zeros(synth_cloud(2, 0.3))
    xyz = np.ascontiguousarray(pc[0].T.numpy())[None]
    pm = runtime.PackedPointMAE(sd, device=DEV)
    feats, center, ori_idx, center_idx = pm.forward(torch.from_numpy(xyz).to(DEV))
    cidx, cen = ok.fps(xyz, 1024)
    np.testing.assert_array_equal(center_idx.cpu().numpy(), cidx)
    idx, nb = ok.knn_group(xyz, cen, 128)
    np.testing.assert_array_equal(ori_idx.cpu().numpy(), idx)
    with torch.no_grad():
        ref = nets.pointmae_forward(sd, torch.from_numpy(nb), torch.from_numpy(cen))
    mean_rel, max_rel = _rel(feats.transpose(1, 2).cpu(), ref)
    assert mean_rel < 0.015 and max_rel < 0.12, (mean_rel, max_rel)


def test_hallucination_generate_vs_golden(golden):
    g = golden("g5_halluc.npz")
    sd = nets.synth_state_dict("halluc", 51)
    hn = runtime.PackedHallucination(sd, device=DEV)
    s = torch.randn(2, 64, 1536, generator=torch.Generator().manual_seed(int(g["samples_seed"])))
    xyz, rgb = s[:, :, :768].contiguous(), s[:, :, 768:].contiguous()
    for src, x, key in (("xyz", xyz, "gen_xyz2rgb"), ("rgb", rgb, "gen_rgb2xyz")):
        got = hn.generate(x.to(DEV), src).cpu()
        ref = torch.from_numpy(g[key])
        err = (got - ref).abs()
        # three chained bf16 GEMMs; outputs are GELU values of O(0.1..1)
        assert err.mean().item() < 4e-3 and err.max().item() < 4e-2, (err.mean().item(), err.max().item())


def test_transformer_block_entry_point_equals_its_seven_launches():
    """cmdiad_transformer_block_fwd (one FFI call per block) against the same block issued as seven separate entry-point
    calls: identical bits, for the ViT geometry and for the Point-MAE geometry with the positional re-add."""
    from cmdiad_amd.runtime import _QkvBuffers, _pack_block, transformer_block, transformer_block_unfused
    for kind, seed, prefix, B, T, C, H, eps, qkv_bias, with_pos in (("vit", 31, "blocks.3.", 2, 785, 768, 12, 1e-6, True, False),
                                                                      ("pointmae", 21, "blocks.blocks.5.", 3, 1024, 384, 6, 1e-5, False, True)):
        sd = nets.synth_state_dict(kind, seed)
        blk = _pack_block(sd, prefix, DEV, qkv_bias)
        g = torch.Generator().manual_seed(B * T)
        x0 = torch.randn(B * T, C, generator=g).to(DEV)
        pos = 0.1 * torch.randn(B * T, C, generator=g).to(DEV) if with_pos else None
        xa, xb = x0.clone(), x0.clone()
        transformer_block(xa, blk, B, T, H, eps, _QkvBuffers(), pos=pos)
        transformer_block_unfused(xb, blk, B, T, H, eps, _QkvBuffers(), pos=pos)
        assert torch.equal(xa, xb) and not torch.equal(xa, x0)


def test_pointmae_batch_statistics_bn_vs_reference_golden(golden):
    """the reference as shipped never calls .eval() on the extractor, so Point-MAE's two BatchNorm1d layers
    (models/models.py:189,195) normalise with the statistics of the sample.  bn_batch_stats=True reproduces that mode on
    the GPU; golden G2 `tokens_train` / `feats_train` are the REFERENCE's own PointTransformer in .train() (DropPath
    stubbed to identity).  Also: per-sample statistics (a batch of two gives each sample's B = 1 result) and the moment
    kernels against torch."""
    g = golden("g2_pointmae.npz")
    sd = nets.synth_state_dict("pointmae", 21)
    pm = runtime.PackedPointMAE(sd, device=DEV, group_size=32, num_group=64, bn_batch_stats=True)
    xyz = torch.from_numpy(np.ascontiguousarray(g["pc"][0].T)[None]).to(DEV)
    feats, center, ori_idx, center_idx = pm.forward(xyz)
    np.testing.assert_array_equal(center_idx.cpu().numpy(), g["center_idx"])
    ref = torch.from_numpy(g["feats_train"])
    mean_rel, max_rel = _rel(feats.transpose(1, 2).cpu(), ref)
    assert mean_rel < 0.015 and max_rel < 0.12, (mean_rel, max_rel)
    # encoder tokens alone (models.py:200-215)
    _, nb = ops.knn_group(xyz, center, 32)
    tok = pm.encode(nb).cpu()
    ref_tok = torch.from_numpy(g["tokens_train"]).reshape(-1, 384)
    mt, xt = _rel(tok, ref_tok)
    assert mt < 0.01 and xt < 0.08, (mt, xt)
    # ... and it IS a different function from the eval-mode contract
    ev = runtime.PackedPointMAE(sd, device=DEV, group_size=32, num_group=64, bn_batch_stats=False).encode(nb).cpu()
    assert _rel(ev, ref_tok)[0] > 5 * mt
    assert _rel(ev, torch.from_numpy(g["tokens_eval"]).reshape(-1, 384))[0] < 0.01
    # per-sample statistics: sample 0 of a batch of two == the B = 1 result
    two = torch.cat([nb, nb.flip(1) * 1.3], 0).contiguous()
    tok2 = pm.encode(two).cpu()
    torch.testing.assert_close(tok2[:64], tok, rtol=0, atol=0)
    # moment kernels
    x = torch.randn(5000, 37, generator=torch.Generator().manual_seed(2)).to(DEV)
    m, v = ops.col_moments(x)
    np.testing.assert_allclose(m.cpu().numpy(), x.double().mean(0).cpu().numpy(), atol=1e-12)
    np.testing.assert_allclose(v.cpu().numpy(), x.double().var(0, unbiased=False).cpu().numpy(), rtol=1e-10)
    p3 = torch.randn(7001, 3, generator=torch.Generator().manual_seed(3)).to(DEV) * 0.01 + 0.5
    mu, cov = ops.moments3(p3)
    np.testing.assert_allclose(mu.cpu().numpy(), p3.double().mean(0).cpu().numpy(), atol=1e-12)
    np.testing.assert_allclose(cov.cpu().numpy(), torch.cov(p3.double().T, correction=0).cpu().numpy(), rtol=1e-7, atol=1e-14)


# ------------------------------------------------------------------------------------------ operand-rounded fp64 oracle
# Rounding to bf16 AMPLIFIES a difference d between two computations to ~sqrt(d * 2^-8) (a fraction d / 2^-8 of the elements
# lands on the other side of a rounding boundary, each by a whole 2^-8 step), so two implementations that round at the same
# places still decorrelate to the full bf16 noise level after four or five rounding points in sequence: measured, the 12-block
# ViT against oracle/nets_rounded.py differs by 2.7e-3 mean / 1.9e-2 max of the feature scale -- little better than against the
# unrounded fp32 oracle (4.5e-3 / 3.1e-2).  A tight end-to-end bound therefore does not exist for a 16-bit chain.  What CAN be
# tight is every kernel of a block on ITS OWN inputs: one rounding point per comparison, so the two sides differ by at most one
# bf16 step on the few elements that sit on a boundary, and by fp32 accumulation noise (1e-6) elsewhere.
@pytest.mark.parametrize("kind", ["vit", "pointmae", "vit-heavy-tailed"])
def test_transformer_block_stage_by_stage_vs_fp64(kind):
    """models/models.py:126-180 (and timm's block, same algebra) kernel by kernel at full size, B = 2: LayerNorm (+ the
    positional re-add), qkv projection with head-split stores, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual
    -- each against float64 arithmetic on the GPU's OWN input of that stage (oracle/nets_rounded.py's model of where operands are
    rounded).  bf16 outputs: within one bf16 step of the exact value everywhere, the nearest bf16 for >= 99.8 % of the elements;
    fp32 outputs (the residual stream): 2e-5 of the feature scale.  A wrong bias element, a mis-scaled head or a transposed tile
    fails by orders of magnitude.  The body is tests/block_stages.py (tests/test_gpu_attention_edges.py runs it on small
    geometries); _ulp_check and the float64 model of the attention kernel's tile loop are tests/attn_ref.py."""
    heavy = kind.endswith("heavy-tailed")
    kind = kind.split("-")[0]
    if kind == "vit":
        seed, prefix, B, T, C, H, eps, qkv_bias, with_pos = 31, "blocks.5.", 2, 785, 768, 12, 1e-6, True, False
    else:
        seed, prefix, B, T, C, H, eps, qkv_bias, with_pos = 21, "blocks.blocks.7.", 2, 1024, 384, 6, 1e-5, False, True
    sd = nets.synth_state_dict(kind, seed)
    g = torch.Generator().manual_seed(B * T + C)
    x0 = torch.randn(B * T, C, generator=g)
    if heavy:     # a residual stream as a DINO checkpoint has it: three channels at ~100x on every token, one token at ~40x
        x0[:, 7] += 100.0
        x0[:, 300] -= 80.0
        x0[:, 555] += 100.0
        x0[400] *= 40.0
        x0[T + 400] *= 40.0
    pos = 0.1 * torch.randn(B * T, C, generator=g) if with_pos else None
    stage_by_stage(sd, prefix, B, T, C, H, eps, qkv_bias, x0, pos, kind)


def _tight(got, ref):
    """(mean, max) |error| relative to the mean absolute feature value, against the operand-rounded float64 oracle."""
    scale = ref.abs().mean().item()
    err = (got.double() - ref).abs()
    return err.mean().item() / scale, err.max().item() / scale


def test_networks_end_to_end_vs_operand_rounded_fp64_oracle(monkeypatch):
    """ViT-B/8 and Point-MAE (encoder + transformer) at full size against oracle/nets_rounded.py end to end.  Because rounding
    decorrelates the two sides (comment above) the bound is the bf16 noise level, like the fp32-oracle tests -- but the operand-
    rounded oracle removes the systematic part of the difference, so mean / max are asserted at about half of those tests'
    tolerances, and a 0.02 error in ONE bias element of ONE block is still caught (it exceeds the max bound)."""
    from cmdiad_amd.synth import synth_cloud
    from oracle import nets_rounded as nr
    from oracle import scoring
    monkeypatch.setenv("CMDIAD_LN_FOLD", "0")          # the LayerNorms as launches: LN(x) is what gets rounded (nets_rounded's model)
    sd = nets.synth_state_dict("vit", 31)
    rgb = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = nr.vit_forward_rounded(sd, rgb)
    got = runtime.PackedViT(sd, device=DEV).forward(rgb.to(DEV)).cpu()
    mean_rel, max_rel = _tight(got, ref)
    print(f"ViT-B/8 vs operand-rounded fp64: mean {mean_rel:.2e}, max {max_rel:.2e} of the feature scale")
    assert mean_rel < 6e-3 and max_rel < 5e-2, (mean_rel, max_rel)
    sd = nets.synth_state_dict("pointmae", 21)
    pm = runtime.PackedPointMAE(sd, device=DEV)
    pc, _ = scoring.unorganize_no_zeros(synth_cloud(2, 0.3))
    xyz = np.ascontiguousarray(pc[0].T.numpy())[None]
    feats, center, ori_idx, center_idx = pm.forward(torch.from_numpy(xyz).to(DEV))
    cidx, cen = ok.fps(xyz, 1024)
    idx, nb = ok.knn_group(xyz, cen, 128)
    np.testing.assert_array_equal(ori_idx.cpu().numpy(), idx)
    tok_gpu = pm.encode(torch.from_numpy(nb).to(DEV)).cpu().view(1, 1024, -1)
    with torch.no_grad():
        tok = nr.pointmae_encoder_rounded(sd, torch.from_numpy(nb))
        ref = nr.pointmae_transformer_rounded(sd, tok, torch.from_numpy(cen))
    t_mean, t_max = _tight(tok_gpu, tok)
    f_mean, f_max = _tight(feats.transpose(1, 2).cpu(), ref)
    print(f"Point-MAE vs operand-rounded fp64: tokens mean {t_mean:.2e} max {t_max:.2e}; features mean {f_mean:.2e} max {f_max:.2e}")
    # the encoder has three rounding points in sequence (h1, h2, h3): tight; the 12-block transformer behind it is not
    assert t_mean < 1e-3 and t_max < 1e-2, (t_mean, t_max)
    assert f_mean < 6e-3 and f_max < 5e-2, (f_mean, f_max)
