"""DINOv2 ViT-B/14 RGB backbone (vit_base_patch14_dinov2.lvd142m, models/models.py:36-39): module surface, checkpoint rules, the
refusals of configurations the reference cannot run, and the reference's 37 x 37 grid downstream (golden: make_golden_dinov2.py)
against a float64 restatement -- everything that needs no GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from cmdiad_amd.models import models as M
from dinov2_synth import TOKENS, rgb_patches64, synth_dinov2_state_dict

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_dinov2 import inputs  # noqa: E402
from oracle import scoring  # noqa: E402

DINO = "vit_base_patch14_dinov2.lvd142m"


def timm_dinov2_layout():
    """timm's VisionTransformer(img_size=518, patch_size=14, embed_dim=768, depth=12, num_heads=12, init_values=1e-5,
    num_classes=0) state_dict, written out: (name, shape) in registration order [external]."""
    out = [("cls_token", (1, 1, 768)), ("pos_embed", (1, 1370, 768)),
           ("patch_embed.proj.weight", (768, 3, 14, 14)), ("patch_embed.proj.bias", (768,))]
    for i in range(12):
        b = f"blocks.{i}."
        out += [(b + "norm1.weight", (768,)), (b + "norm1.bias", (768,)),
                (b + "attn.qkv.weight", (2304, 768)), (b + "attn.qkv.bias", (2304,)),
                (b + "attn.proj.weight", (768, 768)), (b + "attn.proj.bias", (768,)), (b + "ls1.gamma", (768,)),
                (b + "norm2.weight", (768,)), (b + "norm2.bias", (768,)),
                (b + "mlp.fc1.weight", (3072, 768)), (b + "mlp.fc1.bias", (3072,)),
                (b + "mlp.fc2.weight", (768, 3072)), (b + "mlp.fc2.bias", (768,)), (b + "ls2.gamma", (768,))]
    return out + [("norm.weight", (768,)), ("norm.bias", (768,))]


def _model(name=DINO, **kw):
    return M.Model(device="cpu", rgb_backbone_name=name, group_size=32, num_group=64, **kw)


def test_dinov2_state_dict_matches_timm_layout():
    sd = M.rgb_backbone(DINO).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == timm_dinov2_layout()
    assert TOKENS == 1370
    # timm's init_values: every LayerScale starts at 1e-5
    assert all(torch.equal(v, torch.full((768,), 1e-5)) for k, v in sd.items() if k.endswith(".gamma"))
    M.rgb_backbone(DINO).load_state_dict(synth_dinov2_state_dict(3), strict=True)


def test_vit_b8_module_is_unchanged():
    """ViT-B/8's names (no LayerScale) and its seeded init: the checksums of the tree before the DINOv2 option."""
    from oracle import nets
    for name in M.VIT_B8_NAMES:
        assert set(M.rgb_backbone(name).state_dict()) == set(nets.synth_state_dict("vit", 0))
    torch.manual_seed(5)
    sd = M.VisionTransformer().state_dict()
    assert len(sd) == 150 and not any(".ls" in k for k in sd)
    got = [sum(v.double().sum().item() for v in sd.values()), sum(v.double().abs().sum().item() for v in sd.values())]
    np.testing.assert_allclose(got, [19176.056890151554, 1389520.5397423469], rtol=1e-9)


def _save(path, sd, wrap=True):
    torch.save({"model": {f"module.{k}": v for k, v in sd.items()}} if wrap else sd, path)


def test_checkpoint_loads_ignores_mask_token_and_fails_on_missing_gamma(tmp_path, monkeypatch):
    monkeypatch.delenv("CMDIAD_VIT_CHECKPOINT", raising=False)
    monkeypatch.setenv("CMDIAD_POINTMAE_CHECKPOINT", str(tmp_path / "none.pth"))
    monkeypatch.setenv("CMDIAD_ALLOW_RANDOM_INIT", "1")   # (for the Point-MAE side only: the ViT gets its file)
    want = synth_dinov2_state_dict(4)
    meta = dict(want, mask_token=torch.zeros(1, 768))     # Meta's dinov2_vitb14 file carries the masked-modelling token
    path = str(tmp_path / "dinov2.pth")
    _save(path, meta, wrap=False)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        warnings.filterwarnings("ignore", message=".*Point-MAE keeps its seeded random init")
        m = _model(checkpoint_path=path)
    got = m.rgb_backbone.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    for drop in ("blocks.7.ls1.gamma", "blocks.0.ls2.gamma"):
        _save(path, {k: v for k, v in want.items() if k != drop})
        with pytest.raises(RuntimeError, match="lacks 1 backbone tensors"):
            _model(checkpoint_path=path)


def test_model_without_weights_names_the_backbone(monkeypatch, tmp_path):
    monkeypatch.delenv("CMDIAD_VIT_CHECKPOINT", raising=False)
    monkeypatch.setenv("CMDIAD_ALLOW_RANDOM_INIT", "0")
    with pytest.raises(RuntimeError, match=DINO.replace(".", r"\.")):
        _model()
    monkeypatch.setenv("CMDIAD_ALLOW_RANDOM_INIT", "1")
    monkeypatch.setenv("CMDIAD_POINTMAE_CHECKPOINT", str(tmp_path / "none.pth"))
    with pytest.warns(UserWarning):
        m = _model()
    assert m.rgb_backbone.pos_embed.shape == (1, 1370, 768) and m.rgb_backbone.patch_embed.proj.kernel_size == (14, 14)
    with pytest.raises(NotImplementedError, match="vit_small_patch8_224_dino"):
        _model("vit_small_patch8_224_dino")


def _args(**kw):
    a = dict(rgb_backbone_name=DINO, xyz_backbone_name='Point_MAE', group_size=128, num_group=1024, rgb_size=518, xyz_size=224,
             gt_size=224, main_modality='', use_hrnet=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_refusals_name_their_reason():
    from cmdiad_amd.feature_extractors import multiple_features as mf
    for cls in (mf.RGBFeatures, mf.DoubleRGBPointFeatures, mf.RGBorXYZWithOneHallucination,
                mf.RGBorXYZWithOneHallucinationFromFeature):
        with pytest.raises(NotImplementedError, match="--rgb_size 518"):
            cls(_args(rgb_size=224))
    with pytest.raises(NotImplementedError, match="use_hrnet"):
        mf.RGBorXYZWithOneHallucination(_args(use_hrnet=True, main_modality='rgb'))
    with pytest.raises(NotImplementedError, match="main_modality 'xyz'"):
        mf.RGBorXYZWithOneHallucinationFromFeature(_args(main_modality='xyz'))
    # what the reference does run is not refused (the refusal hooks alone; building the objects needs the GPU)
    mf.RGBorXYZWithOneHallucination._refuse(_args(use_hrnet=True, main_modality='xyz'))
    mf.RGBorXYZWithOneHallucination._refuse(_args(use_hn=True, main_modality='rgb'))
    mf.RGBorXYZWithOneHallucinationFromFeature._refuse(_args(main_modality='rgb'))
    mf.RGBorXYZWithOneHallucinationFromFeature._refuse(_args(rgb_backbone_name="vit_base_patch8_224_dino", rgb_size=224,
                                                             main_modality='xyz'))


def test_reference_golden_against_float64(golden):
    """The fixture (the reference's get_rgb_patch / compute_single_s_s_map on the 37 x 37 grid) against this test's float64
    restatement: pins the fixture and the grid arithmetic the GPU tests hold the kernels to."""
    g = golden("gdv_dinov2.npz")
    fmap, bank, patch = inputs()
    p, p2 = rgb_patches64(fmap)
    np.testing.assert_array_equal(g["rgb_patch"], p.float().numpy())                    # a reshape: exact
    np.testing.assert_allclose(g["rgb_patch2"], p2.numpy(), rtol=1e-6, atol=1e-6)      # 1, 2 or 4 cells per window
    # the reference's own fp32 pooling (torch's CPU kernel) is what cmdiad_token_pool56 reproduces bit for bit
    ref32 = torch.nn.functional.adaptive_avg_pool2d(fmap[0], (56, 56)).reshape(fmap.shape[1], -1).T
    np.testing.assert_array_equal(g["rgb_patch2"], ref32.numpy())
    d = torch.cdist(patch.double(), bank.double())
    r = scoring.single_s_s_map(patch.double(), d, bank.double(), (37, 37), blur=False)
    np.testing.assert_array_equal(g["min_idx"], r["min_idx"].numpy())
    # (the reference's fp32 cdist forms |q|^2 + |b|^2 - 2 q.b: ~1e-5 relative against float64)
    np.testing.assert_allclose(g["min_val"], r["min_val"].numpy(), rtol=1e-4)
    np.testing.assert_allclose(float(g["s"]), float(r["s"]), rtol=1e-4)
    np.testing.assert_allclose(g["s_map"], r["s_map"].numpy()[:, ::4, ::4], rtol=1e-4, atol=1e-5)
