"""Point-BERT backbone (models/models.py:31-33, 246-352 with encoder_dims=256): module surface, seeded init, checkpoint loading and
the Model's backbone selection -- everything that needs no GPU.  Fixture: tests/golden/make_golden_pointbert.py."""
import inspect
import os

import numpy as np
import pytest
import torch

from cmdiad_amd.models import models as M
from pointbert_synth import synth_pointbert_state_dict


def test_pointbert_state_dict_names_and_shapes_match_reference(golden):
    g = golden("gpb_pointbert.npz")
    sd = M.PointTransformer(group_size=32, num_group=64, encoder_dims=256).state_dict()
    assert list(sd) == [str(n) for n in g["names"]]     # same names in the same registration order
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    # ... and the synthetic weights the GPU tests use fit it exactly
    M.PointTransformer(group_size=32, num_group=64, encoder_dims=256).load_state_dict(synth_pointbert_state_dict(21), strict=True)


def test_pointbert_seeded_init_matches_reference_checksums(golden):
    """Same construction order => same RNG consumption (cls_pos's randn and reduce_dim's init before the encoder)."""
    g = golden("gpb_pointbert.npz")
    torch.manual_seed(123)
    sd = M.PointTransformer(group_size=128, num_group=1024, encoder_dims=256).state_dict()
    assert list(sd) == [str(n) for n in g["init_names"]]
    got = np.array([[v.double().sum().item(), v.double().abs().sum().item()] for v in sd.values()])
    np.testing.assert_allclose(got, g["init_checksums"], rtol=1e-9, atol=1e-9)


def test_point_mae_module_is_unchanged_by_the_pointbert_option():
    names = list(M.PointTransformer(group_size=32, num_group=64).state_dict())
    assert not any(n.startswith(("cls_", "reduce_dim")) for n in names)
    with pytest.raises(NotImplementedError):
        M.PointTransformer(encoder_dims=512)


def _pb_checkpoint(path, seed=5, drop=None):
    """A Point-BERT pretrain file as the reference's loader sees it: DataParallel `module.` prefix, the online transformer under
    `transformer_q.` with its classification heads, a momentum copy `transformer_k.`, the dVAE, and the masked model's extras."""
    sd = synth_pointbert_state_dict(seed)
    base = {}
    for k, v in sd.items():
        if k != drop:
            base[f"module.transformer_q.{k}"] = v
        base[f"module.transformer_k.{k}"] = v + 1.0
    base["module.transformer_q.cls_head_finetune.0.weight"] = torch.ones(256, 768)
    base["module.transformer_q.cls_head.weight"] = torch.ones(3, 3)
    base["module.transformer_q.mask_token"] = torch.ones(1, 1, 384)
    base["module.transformer_q.lm_head.weight"] = torch.ones(8192, 384)
    base["module.dvae.encoder.first_conv.0.weight"] = torch.ones(128, 3, 1)
    base["module.dvae.dgcnn_1.input_trans.weight"] = torch.ones(4, 4)
    base["module.pos_drop.weight"] = torch.ones(3)      # a top-level key: the rewrite drops it
    torch.save({"base_model": base, "epoch": 300}, path)
    return sd


def test_load_model_from_pb_ckpt_keeps_exactly_the_backbone(tmp_path):
    assert list(inspect.signature(M.PointTransformer.load_model_from_pb_ckpt).parameters) == ["self", "bert_ckpt_path"]
    path = str(tmp_path / "Point-BERT.pth")
    want = _pb_checkpoint(path)
    pt = M.PointTransformer(group_size=32, num_group=64, encoder_dims=256)
    pt.load_model_from_pb_ckpt(path)
    got = pt.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v.to(got[k].dtype)), k   # transformer_q, never transformer_k / dvae / the heads


def test_load_model_from_pb_ckpt_fails_on_a_missing_backbone_tensor(tmp_path):
    path = str(tmp_path / "Point-BERT.pth")
    _pb_checkpoint(path, drop="reduce_dim.weight")
    pt = M.PointTransformer(group_size=32, num_group=64, encoder_dims=256)
    with pytest.raises(RuntimeError, match="reduce_dim.weight"):
        pt.load_model_from_pb_ckpt(path)


def _model(name, **kw):
    return M.Model(device="cpu", rgb_backbone_name="vit_base_patch8_224_dino", xyz_backbone_name=name, group_size=32, num_group=64,
                   **kw)


def test_model_point_bert_checkpoint_and_random_init_rule(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                       # checkpoints/Point-BERT.pth relative to the working directory, as main.py
    monkeypatch.delenv("CMDIAD_POINTBERT_CHECKPOINT", raising=False)
    monkeypatch.setenv("CMDIAD_ALLOW_RANDOM_INIT", "1")   # (the ViT has no checkpoint here either)
    with pytest.warns(UserWarning, match="Point-BERT keeps its seeded random init"):
        m = _model("Point_Bert")
    assert isinstance(m.xyz_backbone, M.PointTransformer) and m.xyz_backbone.encoder_dims == 256
    assert m.xyz_backbone.reduce_dim.weight.shape == (384, 256)
    # the default file, then the environment override
    os.makedirs("checkpoints")
    want = _pb_checkpoint(os.path.join("checkpoints", "Point-BERT.pth"), seed=7)
    m = _model("Point_Bert")
    assert torch.equal(m.xyz_backbone.state_dict()["cls_pos"], want["cls_pos"])
    other = str(tmp_path / "other.pth")
    want2 = _pb_checkpoint(other, seed=8)
    monkeypatch.setenv("CMDIAD_POINTBERT_CHECKPOINT", other)
    m = _model("Point_Bert")
    assert torch.equal(m.xyz_backbone.state_dict()["cls_pos"], want2["cls_pos"])
    # a missing file without the opt-in is an error, as for Point-MAE
    monkeypatch.setenv("CMDIAD_POINTBERT_CHECKPOINT", str(tmp_path / "nope.pth"))
    monkeypatch.setenv("CMDIAD_VIT_CHECKPOINT", "")
    monkeypatch.setenv("CMDIAD_ALLOW_RANDOM_INIT", "0")
    with pytest.raises((FileNotFoundError, RuntimeError)):
        _model("Point_Bert")
    pt = M.PointTransformer(group_size=32, num_group=64, encoder_dims=256)
    with pytest.raises(FileNotFoundError, match="CMDIAD_POINTBERT_CHECKPOINT"):
        pt.load_model_from_pb_ckpt(str(tmp_path / "nope.pth"))


def test_other_xyz_backbones_still_raise(monkeypatch):
    monkeypatch.setenv("CMDIAD_ALLOW_RANDOM_INIT", "1")
    for name in ("Point_BERT", "PointNet", ""):
        with pytest.raises(NotImplementedError):
            _model(name)
