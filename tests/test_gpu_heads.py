"""GPU parity of the conv / feature-to-input / HRNet distillation heads against the outputs of the
reference's own modules (tests/golden/g10_heads.npz: eval mode, synthetic weights of oracle.heads) and against the fp32
CPU oracle at a second batch size.

Tolerance model as tests/test_gpu_nets.py: every convolution / GEMM operand is rounded to bf16 (2^-9 relative), fp32
accumulation; after L chained layers the error is ~ sqrt(L) 2^-8 of the activation scale -> mean |err| <= 1.5 %,
max |err| <= 12 % of the mean absolute output; the scalar losses (means over 3136+ rows) to 0.5 %."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd.models import hallucination_network as hn  # noqa: E402
from cmdiad_amd.models.hrnet import HRNet  # noqa: E402
from oracle import heads  # noqa: E402

DEV = "cuda"


def _rel(got, ref):
    got, ref = torch.as_tensor(got).float(), torch.as_tensor(ref).float()
    scale = ref.abs().mean().item()
    err = (got - ref).abs()
    return err.mean().item() / scale, err.max().item() / scale


def _inputs(g):
    gen = torch.Generator().manual_seed(int(g["tok_seed"]))
    xyz_tok, rgb_tok = torch.randn(1, 3136, 768, generator=gen), torch.randn(1, 3136, 768, generator=gen)
    return xyz_tok, rgb_tok, torch.randn(1, 3, 224, 224, generator=gen)


def _load(module, kind):
    module.load_state_dict(heads.synth_head_state_dict(kind, 41))
    return module.to(DEV).eval()


def _check(got, ref, what):
    mean_rel, max_rel = _rel(got, ref)
    assert mean_rel < 0.015 and max_rel < 0.12, (what, mean_rel, max_rel)


def test_conv_ftof_vs_reference_golden(golden):
    g = golden("g10_heads.npz")
    xyz_tok, rgb_tok, _ = _inputs(g)
    m = _load(hn.HallucinationCrossModalityConv(None, 768, 768), "conv_ftof")
    xh, rh = m.hallucination_generation(xyz_tok.to(DEV), rgb_tok.to(DEV), "train")
    assert xh.shape == (1, 3136, 768) and xh.is_cuda and xh.dtype == torch.float32
    _check(xh[0, ::7, ::8].cpu(), g["conv_ftof/xyz_h"], "xyz_h")
    _check(rh[0, ::7, ::8].cpu(), g["conv_ftof/rgb_h"], "rgb_h")
    assert torch.equal(m.hallucination_generation(None, rgb_tok.to(DEV), "xyz"), xh)
    assert torch.equal(m.hallucination_generation(xyz_tok.to(DEV), None, "rgb"), rh)
    np.testing.assert_allclose([float(v) for v in m(xyz_tok.to(DEV), rgb_tok.to(DEV), False, "l2")], g["conv_ftof/loss"], rtol=5e-3)
    np.testing.assert_allclose([float(v) for v in m(xyz_tok.to(DEV), rgb_tok.to(DEV), True, "l2")], g["conv_ftof/loss_sigmoid"], rtol=5e-3)


def test_ftoi_heads_vs_reference_golden(golden):
    g = golden("g10_heads.npz")
    xyz_tok, rgb_tok, img = _inputs(g)
    m = _load(hn.HallucinationRGBFeatureToXYZInputMLP(types.SimpleNamespace(estimate_depth=False), 768), "ftoi_mlp")
    y = m.hallucination_generation(rgb_tok.to(DEV))
    assert y.shape == (1, 3, 224, 224)
    _check(y[0, :, ::4, ::4].cpu(), g["ftoi_mlp/y"], "ftoi_mlp")
    np.testing.assert_allclose(float(m(rgb_tok.to(DEV), img.to(DEV))), float(g["ftoi_mlp/loss"]), rtol=5e-3)
    m = _load(hn.HallucinationFeatureToInputConv(None, 768), "ftoi_conv")
    y = m.hallucination_generation(xyz_tok.to(DEV))
    assert y.shape == (1, 3, 224, 224) and y.is_contiguous()
    _check(y[0, :, ::4, ::4].cpu(), g["ftoi_conv/y"], "ftoi_conv")
    np.testing.assert_allclose(float(m(xyz_tok.to(DEV), img.to(DEV))), float(g["ftoi_conv/loss"]), rtol=5e-3)


def test_hrnet_vs_reference_golden(golden):
    g = golden("g10_heads.npz")
    xyz_tok, _, img = _inputs(g)
    m = _load(HRNet(512, 768, 0.1), "hrnet")
    y = m.hallucination_generation(img.to(DEV))
    assert y.shape == (1, 768, 56, 56)
    _check(y[0, ::8, ::2, ::2].cpu(), g["hrnet/y"], "hrnet")
    # the callers' reshape (multiple_features.py:330-331) of the NCHW view gives the token matrix back
    tok = y.reshape(1, 768, -1).transpose(-1, -2)
    assert torch.equal(tok, m.hallucination_tokens(img.to(DEV)))
    np.testing.assert_allclose(float(m(img.to(DEV), xyz_tok.to(DEV))), float(g["hrnet/loss"]), rtol=5e-3)
    with pytest.raises(ValueError, match="c=512"):
        HRNet(48, 768, 0.1).to(DEV).eval().hallucination_generation(img.to(DEV))


def test_heads_batched_vs_oracle_and_depth_variant():
    gen = torch.Generator().manual_seed(9)
    tok, img = torch.randn(3, 3136, 768, generator=gen), torch.randn(3, 3, 224, 224, generator=gen)
    with torch.no_grad():
        sd = heads.synth_head_state_dict("hrnet", 5)
        m = HRNet(512, 768, 0.1)
        m.load_state_dict(sd)
        _check(m.to(DEV).eval().hallucination_generation(img.to(DEV)).cpu(), heads.hrnet(sd, img), "hrnet B=3")
        sd = heads.synth_head_state_dict("ftoi_mlp", 5, out_dim=1)
        m = hn.HallucinationRGBFeatureToXYZInputMLP(types.SimpleNamespace(estimate_depth=True), 768)
        m.load_state_dict(sd)
        y = m.to(DEV).eval().hallucination_generation(tok.to(DEV))
        assert y.shape == (3, 1, 224, 224)
        _check(y.cpu(), heads.ftoi_mlp(sd, tok), "ftoi_mlp depth B=3")
        sd = heads.synth_head_state_dict("ftoi_conv", 5)
        m = hn.HallucinationFeatureToInputConv(None, 768)
        m.load_state_dict(sd)
        _check(m.to(DEV).eval().hallucination_generation(tok[:2].to(DEV)).cpu(), heads.ftoi_conv(sd, tok[:2]), "ftoi_conv B=2")


def test_head_repacks_after_weight_update():
    m = _load(hn.HallucinationFeatureToInputConv(None, 768), "ftoi_conv")
    tok = torch.randn(1, 3136, 768, generator=torch.Generator().manual_seed(1)).to(DEV)
    a = m.hallucination_generation(tok)
    with torch.no_grad():
        m.conv4.bias.add_(1.0)
    b = m.hallucination_generation(tok)
    torch.testing.assert_close(b, a + 1.0, rtol=0, atol=1e-5)
    m.train()   # training mode with gradients builds a graph (the pretraining loop); the inference kernels serve no_grad
    loss = m(tok, torch.zeros(1, 3, 224, 224, device=DEV))
    assert loss.requires_grad
    with torch.no_grad():
        assert not m(tok, torch.zeros(1, 3, 224, 224, device=DEV)).requires_grad


@pytest.mark.parametrize("kind", ["ftoi_mlp", "ftoi_conv", "hrnet", "hrnet_hip", "conv_ftof"])
def test_head_training_follows_the_reference_loss_curve(kind, golden):
    """hallucination_network_pretrain.py:106-147 for the conv / feature-to-input / HRNet heads: three Adam steps (lr 1e-3) in
    train() mode from the synthetic weights on one seeded batch of two, against the same three steps of the REFERENCE's own
    modules on the CPU (tests/golden/g12_heads_train.npz, make_golden.py g12): the loss before every step, and sum / abs-sum of
    every tensor of the state_dict afterwards (weights, biases, BatchNorm running statistics).  The conv FtoF and the two
    feature-to-input heads run their hand-written forward + backward (cmdiad_amd/conv_train.py: bf16 GEMM operands, fp32
    accumulation), and so does the HRNet trunk ("hrnet" and "hrnet_hip" are the same run since that path became its only one)."""
    from cmdiad_amd.models.hrnet import HRNet
    if kind == "hrnet_hip":   # (the third step is the HIP-graph capture + replay)
        kind = "hrnet"
    g12 = golden("g12_heads_train.npz")
    gen = torch.Generator().manual_seed(int(g12["input_seed"]))
    a, b = torch.randn(2, 3136, 768, generator=gen), torch.randn(2, 3136, 768, generator=gen)
    img = torch.randn(2, 3, 224, 224, generator=gen)
    x = {"conv_ftof": (a, b), "ftoi_mlp": (a, img), "ftoi_conv": (a, img), "hrnet": (img, b)}[kind]
    make = {"conv_ftof": lambda: hn.HallucinationCrossModalityConv(None, 768, 768),
            "ftoi_mlp": lambda: hn.HallucinationRGBFeatureToXYZInputMLP(types.SimpleNamespace(estimate_depth=False), 768),
            "ftoi_conv": lambda: hn.HallucinationFeatureToInputConv(None, 768),
            "hrnet": lambda: HRNet(512, 768, 0.1)}[kind]
    m = make()
    m.load_state_dict(heads.synth_head_state_dict(kind, int(g12["weight_seed"])))
    m.to(DEV).train()
    opt = torch.optim.Adam(m.parameters(), lr=float(g12["lr"]))
    want = g12[f"{kind}/loss"]
    for step in range(int(g12["steps"])):
        opt.zero_grad()
        if kind == "conv_ftof":
            lx, lr_ = m(x[0], x[1], False, "l2")
            loss, got = lx + lr_, [float(lx.detach()), float(lr_.detach())]
        else:
            loss = m(x[0], x[1])
            got = [float(loss.detach())]
        np.testing.assert_allclose(got, want[step], rtol=3e-3, err_msg=f"{kind} step {step}")
        loss.backward()
        opt.step()
    for k, v in m.state_dict().items():
        if not v.dtype.is_floating_point:
            continue
        ref = g12[f"{kind}/after/{k}"]
        got = np.array([v.double().sum().item(), v.double().abs().sum().item()])
        # abs-sum pins the magnitudes; the plain sum of a zero-mean tensor is compared against the abs-sum's scale
        assert abs(got[1] - ref[1]) <= 2e-3 * ref[1] + 1e-6, (kind, k, got, ref)
        assert abs(got[0] - ref[0]) <= 2e-3 * ref[1] + 1e-6, (kind, k, got, ref)
    # the inference kernels pick the trained weights up (repack on version change) and agree with the module's own layers
    m.eval()
    with torch.no_grad():
        if kind == "conv_ftof":
            lx, lr_ = m(x[0], x[1], False, "l2")
            ref = [float(v) for v in hn.HallucinationCrossModalityConv._losses(
                m, hn.feature_reshape_back(m.rgb_conv(hn.feature_reshape(x[1].to(DEV)))),
                hn.feature_reshape_back(m.xyz_conv(hn.feature_reshape(x[0].to(DEV)))), x[0].to(DEV), x[1].to(DEV), False)]
            np.testing.assert_allclose([float(lx), float(lr_)], ref, rtol=2e-2)


@pytest.mark.parametrize("flags,cls_name,head_kind", [
    (dict(use_hrnet=True, c_hrnet=512, main_modality='rgb'), "RGBorXYZWithOneHallucination", "hrnet"),
    (dict(use_hrnet=True, c_hrnet=512, main_modality='xyz'), "RGBorXYZWithOneHallucination", "hrnet"),
    (dict(use_hn=True, use_hn_conv=True, main_modality='xyz'), "RGBorXYZWithOneHallucination", "conv_ftof"),
    (dict(use_hn_from_rgb_conv=True, main_modality='xyz'), "RGBorXYZWithOneHallucinationFromFeature", "ftoi_conv"),
    (dict(use_hn_from_rgb_mlp=True, main_modality='rgb'), "RGBorXYZWithOneHallucinationFromFeature", "ftoi_mlp"),
])
def test_method_classes_run_the_protocol_with_each_head(flags, cls_name, head_kind):
    """cmdiad_runner.py:44-92 (fit, coreset, late fusion, predict, metrics) through the ItoF / conv FtoF / FtoI variants of the
    one-hallucination method classes (multiple_features.py:312-797): runs on the GPU path and produces finite, well-formed
    results; the hallucination bank has the modality's row count."""
    import warnings
    from test_gpu_engine import make_args, synth_sample
    from cmdiad_amd.feature_extractors import multiple_features as mf
    from oracle import nets
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = getattr(mf, cls_name)(make_args(**flags))
    m.deep_feature_extractor.rgb_backbone.load_state_dict(nets.synth_state_dict("vit", 31))
    m.deep_feature_extractor.xyz_backbone.load_state_dict(nets.synth_state_dict("pointmae", 21))
    sd = heads.synth_head_state_dict(head_kind, 7)
    if head_kind == "ftoi_mlp":  # a usable synthetic point map: metres-scale coordinates around a plane
        sd["mlp.6.bias"] = torch.tensor([0.0, 0.0, 0.5])
        sd["mlp.6.weight"] = sd["mlp.6.weight"] * 0.05
    m.fusion.load_state_dict(sd)
    m.fusion.eval()
    train = [synth_sample(60 + i) for i in range(2)]
    for rgb, pc in train:
        m.add_sample_to_mem_bank((rgb, pc, pc), class_name="synth")
    rows = 784 if (cls_name.endswith("FromFeature") and flags["main_modality"] == "xyz") else 3136
    assert sum(p.shape[0] for p in m.patch_fusion_lib) == 2 * rows
    m.run_coreset()
    for rgb, pc in train:
        m.add_sample_to_late_fusion_mem_bank((rgb, pc, pc))
    m.run_late_fusion()
    for i, anomalous in ((70, False), (71, True)):
        rgb, pc = synth_sample(i, anomalous)
        mask = torch.zeros(1, 1, 224, 224)
        if anomalous:
            mask[..., 100:120, 100:120] = 1
        m.predict((rgb, pc, pc), mask, np.array([int(anomalous)]), [f"synth/{i}.png"])
    m.calculate_metrics()
    assert np.isfinite([m.image_rocauc, m.pixel_rocauc, m.au_pro]).all()
    assert m.predictions[0].shape == (224, 224) and np.isfinite(m.predictions[0]).all()


def test_dumped_pairs_round_trip_into_the_head_trainers(tmp_path):
    """the input side of the feature-to-input / input-to-feature trainers, end to end on the device.
    DoubleRGBPointFeatures with --save_frgb_xyz --save_rgb_fxyz dumps its samples while the memory bank is built and in predict
    (multiple_features.py:827-867, 947-962); the pair datasets (dataset.py:268-362) read them back; a batch of them drives one
    training step of the FtoI conv head (hand-written forward + backward, conv_train.ftoi_conv_loss) and of the HRNet trunk
    (conv_train.hrnet_loss): finite loss, gradients on every parameter.  The dumped features are what the extractor returns."""
    import os
    import warnings
    from cmdiad_amd import dataset as ds
    from cmdiad_amd import engine as eng
    from oracle import nets
    from cmdiad_amd.feature_extractors.multiple_features import DoubleRGBPointFeatures
    from cmdiad_amd.models.hallucination_network import HallucinationFeatureToInputConv
    from cmdiad_amd.synth import synth_cloud, synth_rgb
    a = dict(rgb_backbone_name='vit_base_patch8_224_dino', xyz_backbone_name='Point_MAE', group_size=128, num_group=1024,
             rgb_size=224, xyz_size=224, gt_size=224, f_coreset=1.0, coreset_eps=0.9, coreset_dtype='FP16',
             random_state=None, dist_method_s='l2', dist_method_coreset='l2', main_modality='', use_hn=False,
             fusion_module_path='', ocsvm_nu=0.5, ocsvm_maxiter=1000, xyz_s_lambda=1.0, xyz_smap_lambda=1.0,
             rgb_s_lambda=0.1, rgb_smap_lambda=0.1, fusion_s_lambda=1.0, fusion_smap_lambda=1.0,
             save_feature_for_fusion=False, save_seg_results=False, use_depth=False,
             save_frgb_xyz=True, save_rgb_fxyz=True, save_path_frgb_xyz=str(tmp_path / "frgb_xyz"), save_path_rgb_fxyz=str(tmp_path / "rgb_fxyz"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = DoubleRGBPointFeatures(types.SimpleNamespace(**a))
    m.deep_feature_extractor.rgb_backbone.load_state_dict(nets.synth_state_dict("vit", 31))
    m.deep_feature_extractor.xyz_backbone.load_state_dict(nets.synth_state_dict("pointmae", 21))
    train = [(synth_rgb(i), synth_cloud(200 + i, 0.30, texture=0.004)) for i in range(3)]
    for rgb, pc in train:
        m.add_sample_to_mem_bank((rgb, pc, pc), class_name="synth")
    m.run_coreset()
    for sub, names in (("frgb_xyz/train/frgb", ["synth0_frgb.pt", "synth1_frgb.pt", "synth2_frgb.pt"]),
                       ("frgb_xyz/train/xyz", ["synth0_xyz.pt", "synth1_xyz.pt", "synth2_xyz.pt"]),
                       ("rgb_fxyz/train/rgb", ["synth0_rgb.pt", "synth1_rgb.pt", "synth2_rgb.pt"])):
        assert sorted(os.listdir(tmp_path / sub)) == names
    assert len(os.listdir(tmp_path / "rgb_fxyz" / "train" / "fxyz")) == 6          # _hfxyz + _lfxyz per sample
    # what was dumped IS the extractor's output for that sample
    ex = m._extract_batch([(train[1][0], train[1][1], train[1][1])])
    d1 = ds.FeatureToInputPreTrainTensorDataset(str(tmp_path / "frgb_xyz" / "train"), "xyz_frgb")
    frgb, xyz = d1[1]
    assert frgb.is_cuda and tuple(frgb.shape) == (3136, 768) and tuple(xyz.shape) == (3, 224, 224)
    assert torch.equal(frgb, eng.Engine.rgb_patch56(ex)[0]) and torch.equal(xyz.cpu(), train[1][1][0])
    d2 = ds.InputToFeaturePreTrainTensorDataset(str(tmp_path / "rgb_fxyz" / "train"), "rgb_fxyz")
    rgb, fxyz = d2[1]
    assert not rgb.is_cuda and torch.equal(rgb, train[1][0][0]) and torch.equal(fxyz.to(DEV), m._engine.xyz_patch(ex, P=56)[0])
    lo = torch.load(tmp_path / "rgb_fxyz" / "train" / "fxyz" / "synth1_lfxyz.pt")
    assert torch.equal(lo.to(DEV), m._engine.xyz_patch(ex, P=28)[0])
    # one training step of each head from a batch of the dumped pairs
    torch.manual_seed(0)
    ring = ds.PairRing(d1, 2, shuffle=True, drop_last=True, device=DEV)
    feat, img = next(iter(ring))
    head = HallucinationFeatureToInputConv(None, 768).to(DEV).train()
    loss = head(feat, img)
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in head.named_parameters() if not n.startswith("norm"))
    ring2 = ds.PairRing(d2, 2, shuffle=False, drop_last=True, device=DEV)
    img2, feat2 = next(iter(ring2))
    trunk = HRNet(512, 768, 0.1).to(DEV).train()
    loss2 = trunk(img2, feat2)
    loss2.backward()
    grads = {n: p.grad for n, p in trunk.named_parameters()}
    assert torch.isfinite(loss2) and all(grads[n] is not None and torch.isfinite(grads[n]).all() and float(grads[n].abs().sum()) > 0
                                         for n in ("conv1.weight", "layer2.1.conv2.weight", "final_layer.weight"))
    # (layer4 exists in the state_dict but the reference's forward stops after layer3, hrnet.py:251-288: no gradient there)
    # predict dumps under test/
    for rgb, pc in train:
        m.add_sample_to_late_fusion_mem_bank((rgb, pc, pc))
    m.run_late_fusion()
    m.predict((train[0][0], train[0][1], train[0][1]), torch.zeros(1, 224, 224), 0, ["x.png"])
    _ = m.image_preds            # (reading a result attribute runs the deferred micro-batch)
    assert sorted(os.listdir(tmp_path / "frgb_xyz" / "test" / "frgb")) == ["synth3_frgb.pt"]
