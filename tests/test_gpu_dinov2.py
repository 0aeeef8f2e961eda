"""DINOv2 ViT-B/14 on the GPU (vit_base_patch14_dinov2.lvd142m, models/models.py:36-39): the patch-14 operand and the adaptive
pooling of the 37 x 37 token grid (exact), the LayerScale fold (float64, rounding bound), the whole backbone at 518 against the
float64 restatement (a2's bar), the scoring tail on the 37 x 37 grid against the reference's golden, and the drop-in / batched
predictor at rgb_size 518."""
import functools
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cmdiad_amd import engine as eng  # noqa: E402
from cmdiad_amd import ops, runtime  # noqa: E402
from cmdiad_amd.predictor import BatchPredictor  # noqa: E402
from cmdiad_amd.synth import synth_cloud, synth_rgb  # noqa: E402
from dinov2_synth import dinov2_tokens64, synth_dinov2_state_dict  # noqa: E402
from oracle import nets  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_dinov2 import inputs  # noqa: E402

DEV = "cuda"
DINO = "vit_base_patch14_dinov2.lvd142m"


@functools.lru_cache(maxsize=None)
def _sd():
    return synth_dinov2_state_dict(31)


def test_im2col_patch14_is_the_unfold_rounded_to_bf16():
    """[B*1369, 640]: columns 0..587 the bf16 of torch's unfold (c, dy, dx order = the flattened conv weight), 588..639 zero; a
    NaN-filled output, so a missing or stray write fails."""
    B, S = 3, 518
    rgb = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(5)) * 3.0
    out = torch.full((B * 37 * 37, 640), float("nan"), dtype=torch.bfloat16, device=DEV)
    r = rgb.to(DEV)
    ops._call("cmdiad_im2col_patch14", ops._p(r), B, S, ops._p(out), ops._stream())
    want = F.unfold(rgb, 14, stride=14).transpose(1, 2).reshape(B * 1369, 588).bfloat16()
    got = out.cpu()
    assert torch.equal(got[:, :588], want)
    assert torch.equal(got[:, 588:], torch.zeros(B * 1369, 52, dtype=torch.bfloat16))
    assert torch.equal(ops.im2col_patch14(r).cpu(), got)


@pytest.mark.parametrize("s,C", [(37, 768), (28, 768), (37, 12), (23, 8)])
def test_token_pool56_is_torch_adaptive_avg_pool2d_bit_for_bit(s, C):
    """cmdiad_token_pool56 on [B, 1 + s*s, C] tokens (cls row skipped) against torch's CPU adaptive_avg_pool2d of the s x s grid:
    identical bits (the header's bar).  At s = 28 it also equals Engine.rgb_patch56's replication view."""
    B = 2
    g = torch.Generator().manual_seed(s * 1000 + C)
    tok = torch.randn(B, 1 + s * s, C, generator=g) * 4.0
    tok[:, 0] = float("nan")                       # the cls row must never be read
    out = torch.full((B, 3136, C), float("nan"), device=DEV)
    t = tok.to(DEV)
    ops._call("cmdiad_token_pool56", ops._p(t), B, s, C, ops._p(out), ops._stream())
    grid = tok[:, 1:].transpose(1, 2).reshape(B, C, s, s)
    want = F.adaptive_avg_pool2d(grid, (56, 56)).reshape(B, C, 3136).transpose(1, 2)
    assert torch.equal(out.cpu(), want)
    ex = eng.Extraction()
    ex.rgb_tokens = t
    view = eng.Engine.rgb_patch56(ex)
    assert view.shape == (B, 3136, C) and torch.equal(view.cpu(), want)
    if s == 28:
        p = t[:, 1:]
        assert torch.equal(view, p.reshape(B, 28, 1, 28, 1, C).expand(B, 28, 2, 28, 2, C).reshape(B, 3136, C))


def _fold_case(sd, p, linear, ls, M, K, heavy, seed):
    """One LayerScale'd product (proj + residual, or fc2 + residual) on its own inputs: the packed weight is bf16(fp32(g W)) and
    the bias fp32(g b); the fp32 residual output against the UNFOLDED float64 definition x + g (a W^T + b), within the exact bound
    of the weight's one rounding (sum_k |a_k| |bf16(g W) - g W|) plus the fp32 bar of the unfolded products (2e-5 of the scale)."""
    blk = runtime._pack_block(sd, p, DEV, True)
    name = "proj" if linear == "attn.proj" else "fc2"
    W, b, gam = sd[p + linear + ".weight"].double(), sd[p + linear + ".bias"].double(), sd[p + ls + ".gamma"].double()
    gw32 = (sd[p + linear + ".weight"].float() * sd[p + ls + ".gamma"].float()[:, None])
    assert torch.equal(blk[name + "_w"].cpu(), gw32.bfloat16())
    assert torch.equal(blk[name + "_b"].cpu(), sd[p + linear + ".bias"].float() * sd[p + ls + ".gamma"].float())
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    x0 = torch.randn(M, 768, generator=g)
    if heavy:   # as a DINO checkpoint's stream has it: a few channels at ~100x, one token at ~40x, some 30x hidden values
        x0[:, 7] += 100.0
        x0[:, 555] -= 80.0
        x0[400] *= 40.0
        a[:, 11] *= 30.0
    a16 = a.bfloat16()
    x = x0.to(DEV)
    ops.gemm(a16.to(DEV), blk[name + "_w"], bias=blk[name + "_b"], residual=x, out_f32=x, want_bf16=False)
    ad = a16.double()
    want = x0.double() + gam * (ad @ W.T + b)
    delta = (gw32.bfloat16().double() - gam[:, None] * W).abs()
    bound = ad.abs() @ delta.T
    scale = (gam * (ad @ W.T)).abs().mean().item() + x0.abs().mean().item()
    err = (x.cpu().double() - want).abs()
    ulp = 2.0 ** -23 * want.abs()           # (the one rounding of the fp32 result itself, large on the ~40x token)
    assert bool((err <= bound + ulp + 2e-5 * scale).all()), (name, heavy, (err - bound - ulp).max().item(), scale)
    # ... and >= 99.8 % of the elements within the fp32 bar of the FOLDED weights as held (the kernel's own rounding only)
    near = (x.cpu().double() - (x0.double() + ad @ gw32.bfloat16().double().T + (b.float() * gam.float()).double())).abs()
    assert (near <= ulp + 2e-5 * scale).double().mean().item() >= 0.998, (name, heavy)
    # an unfolded block (g = 1) would be off by far more than the (worst-case) bound and than the error seen: the test sees the fold
    off = ((gam - 1.0).abs()[None, :] * (ad @ W.T + b).abs()).mean().item()
    assert off > 10 * (bound.mean().item() + 2e-5 * scale) and off > 100 * err.mean().item(), (off, bound.mean().item(), err.mean().item())


@pytest.mark.parametrize("heavy", [False, True], ids=["plain", "heavy-tailed"])
def test_layerscale_fold_vs_fp64(heavy):
    sd = _sd()
    M = 2 * 1370
    _fold_case(sd, "blocks.5.", "attn.proj", "ls1", M, 768, heavy, 11)
    _fold_case(sd, "blocks.5.", "mlp.fc2", "ls2", M, 3072, heavy, 12)


def test_backbone_at_518_vs_fp64():
    """Model(DINOv2).forward_rgb_features at B = 2 against the float64 restatement: a2's bar (mean <= 1.5 %, max <= 12 % of the
    feature scale), [B, 768, 37, 37], tokens [B, 1370, 768]."""
    from cmdiad_amd.models.models import Model
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = Model(device=DEV, rgb_backbone_name=DINO, group_size=32, num_group=64)
    m.rgb_backbone.load_state_dict(_sd())
    m.to(DEV)
    rgb = torch.cat([synth_rgb(40 + i, size=518) for i in range(2)])
    with torch.no_grad():
        tok = m.forward_rgb_tokens(rgb.to(DEV))
        fmap = m.forward_rgb_features(rgb.to(DEV))
    assert tok.shape == (2, 1370, 768) and fmap.shape == (2, 768, 37, 37)
    ref = dinov2_tokens64(_sd(), rgb)
    assert torch.equal(fmap.cpu(), tok[:, 1:].permute(0, 2, 1).reshape(2, 768, 37, 37).cpu())
    scale = ref.abs().mean().item()
    err = (tok.cpu().double() - ref).abs()
    print(f"DINOv2 B=2: mean {err.mean().item() / scale:.4%}, max {err.max().item() / scale:.4%} of the feature scale {scale:.3f}")
    assert err.mean().item() <= 0.015 * scale and err.max().item() <= 0.12 * scale


def test_scoring_tail_on_the_37_grid_vs_reference_golden(golden):
    """engine.score_patches with dims (37, 37) against the reference's compute_single_s_s_map (make_golden_dinov2.py): s rtol 1e-4,
    nearest-neighbour indices exact, the pre-blur map as G4 holds it."""
    g = golden("gdv_dinov2.npz")
    _, bank, patch = inputs()
    r = eng.score_patches(patch.to(DEV).unsqueeze(0).contiguous(), eng.Bank(bank.to(DEV)), (37, 37), 224)
    np.testing.assert_array_equal(r["min_idx"][0].cpu().numpy(), g["min_idx"])
    np.testing.assert_allclose(r["min_val"][0].cpu().numpy(), g["min_val"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(float(r["s"][0]), float(g["s"]), rtol=1e-4)
    np.testing.assert_allclose(r["s_map_pre"].cpu().numpy()[:, ::4, ::4], g["s_map"], rtol=1e-5, atol=1e-5)
    blurred = ops.blur8_maps(r["s_map_pre"].contiguous())
    assert blurred.shape == (1, 224, 224) and bool(torch.isfinite(blurred).all())


def _args(**kw):
    a = dict(rgb_backbone_name=DINO, xyz_backbone_name='Point_MAE', group_size=128, num_group=1024, rgb_size=518, xyz_size=224,
             gt_size=224, f_coreset=1.0, coreset_eps=0.9, coreset_dtype='FP16', random_state=None, dist_method_s='l2',
             dist_method_coreset='l2', main_modality='', use_hn=False, fusion_module_path='', ocsvm_nu=0.5, ocsvm_maxiter=1000,
             xyz_s_lambda=1.0, xyz_smap_lambda=1.0, rgb_s_lambda=0.1, rgb_smap_lambda=0.1, fusion_s_lambda=1.0,
             fusion_smap_lambda=1.0, save_feature_for_fusion=False, save_seg_results=False, use_depth=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _sample(i, anomalous=False):
    pc = synth_cloud(700 + i, 0.40 + 0.03 * (i % 4), texture=0.004)
    rgb = synth_rgb(700 + i, size=518)
    mask = torch.zeros(1, 224, 224)
    if anomalous:
        pc[0, 2, 80:100, 90:110] -= 0.015 * (pc[0, 2, 80:100, 90:110] != 0)
        rgb[0, :, 185:231, 206:252] += 4.0
        mask[0, 80:100, 90:110] = 1
    return rgb, pc, mask


@pytest.mark.parametrize("kind", ["DINO", "DINO+Point_MAE"])
def test_dropin_at_518_and_batch_predictor(kind):
    """RGBFeatures / DoubleRGBPointFeatures at rgb_size 518 (xyz 224): fit, late fusion and predict complete with 1 369-row rgb
    libraries; for DINO+Point_MAE the batched predictor with the same engine agrees with the drop-in's per-sample predict within
    test_gpu_predictor.py's tolerances (image score rtol 1e-4, map within 2.5 8-bit blur levels)."""
    from cmdiad_amd.feature_extractors import multiple_features as mf
    cls = mf.RGBFeatures if kind == "DINO" else mf.DoubleRGBPointFeatures
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = cls(_args())
    m.deep_feature_extractor.rgb_backbone.load_state_dict(_sd())
    m.deep_feature_extractor.xyz_backbone.load_state_dict(nets.sharpen_pointmae(nets.synth_state_dict("pointmae", 21)))
    train = [_sample(i) for i in range(3)]
    for rgb, pc, _ in train:
        m.add_sample_to_mem_bank((rgb, pc, pc.clone()), class_name="synthetic")
    m.run_coreset()
    assert m.patch_rgb_lib.shape == (3 * 1369, 768)
    for rgb, pc, _ in train:
        m.add_sample_to_late_fusion_mem_bank((rgb, pc, pc.clone()))
    m.run_late_fusion()
    test = [_sample(10 + i, anomalous=(i % 2 == 1)) for i in range(4)]
    for rgb, pc, mask in test:
        m.predict((rgb, pc, pc.clone()), mask, np.array([int(mask.any())]), ["x.png"])
    img = np.concatenate(m.image_preds).ravel()
    maps = np.stack(m.predictions)
    assert img.shape == (4,) and maps.shape == (4, 224, 224) and np.isfinite(img).all() and np.isfinite(maps).all()
    if kind == "DINO":
        return
    stats = dict(xyz_mean=float(m.xyz_mean), xyz_std=float(m.xyz_std), rgb_mean=float(m.rgb_mean), rgb_std=float(m.rgb_std))
    p = BatchPredictor(m._engine, eng.Bank(m.patch_xyz_lib.to(DEV)), eng.Bank(m.patch_rgb_lib.to(DEV)), stats, m.detect_fuser,
                       m.seg_fuser, lambdas=(1.0, 1.0, 0.1, 0.1), batch=4, use_graph=False, rgb_size=518)
    assert p.inputs[0]["rgb"].shape == (4, 3, 518, 518) and p.inputs[0]["pcs"].shape == (4, 3, 224, 224)
    bi, bm = p.predict_batch(torch.cat([t[0] for t in test]).to(DEV), torch.cat([t[1] for t in test]).to(DEV))
    for b in range(4):
        np.testing.assert_allclose(bi[b], img[b], rtol=1e-4, atol=1e-6)
        assert np.abs(bm[b] - maps[b]).max() <= 2.5 * np.ptp(maps[b]) / 255.0 + 1e-9, b
