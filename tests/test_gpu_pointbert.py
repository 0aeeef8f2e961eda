"""Point-BERT on the GPU (PackedPointBERT; models/models.py:246-352 with encoder_dims=256): the 256-wide encoder tail, the
cls-row token layout and the fetch LayerNorm that skips it, against the reference's golden (tests/golden/make_golden_pointbert.py)
and against a float64 restatement at full size.  Tolerances as for Point-MAE (tests/test_gpu_nets.py)."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd import ops, runtime  # noqa: E402
from oracle import kernels as ok  # noqa: E402
from pointbert_synth import pointbert_forward64, synth_pointbert_state_dict  # noqa: E402

DEV = "cuda"


def _rel(got, ref):
    scale = ref.abs().mean().item()
    err = (got.double() - ref.double()).abs()
    return err.mean().item() / scale, err.max().item() / scale


@pytest.mark.parametrize("Mg,groups", [(128, 24), (64, 9), (32, 7), (32, 50), (128, 300), (128, 770), (64, 1031), (32, 2051)])
def test_encoder_tail_256_equals_two_kernel_path(Mg, groups):
    """cmdiad_encoder_tail_n at 256 output columns against cmdiad_gemm_bf16(ReLU, group bias) + cmdiad_gemm_groupmax: identical
    tokens over the grid of the 384-wide test; with seg the same tokens land one row further per cloud and the cls rows stay
    untouched."""
    w = runtime.fold_pointmae_encoder(synth_pointbert_state_dict(21), "encoder.", DEV)
    assert w["W4"].shape == (256, 512)
    g = torch.Generator().manual_seed(Mg + groups)
    h2 = torch.randn(groups * Mg, 256, generator=g).to(DEV).bfloat16()
    gb = torch.randn(groups, 512, generator=g).to(DEV)
    _, h3 = ops.gemm(h2, w["W3b"], act=ops.ACT_RELU, group_bias=gb, group_rows=Mg)
    want, _ = ops.gemm_groupmax(h3, w["W4"], w["b4"], groups, Mg)
    got = ops.encoder_tail_n(h2, gb, w["W3b"], w["W4"], w["b4"], groups, Mg)
    assert got.shape == (groups, 256) and torch.equal(got, want)
    for seg in {1, groups} | ({groups // 7} if groups % 7 == 0 and groups > 7 else set()):
        out = torch.full((groups + groups // seg, 256), float("nan"), device=DEV)
        ops.encoder_tail_n(h2, gb, w["W3b"], w["W4"], w["b4"], groups, Mg, seg=seg, out=out)
        rows = torch.arange(groups, device=DEV)
        rows = rows + rows // seg + 1
        assert torch.equal(out[rows], want)
        lead = torch.arange(groups // seg, device=DEV) * (seg + 1)
        assert torch.isnan(out[lead]).all()


def test_lead_rows_and_layernorm_skip_first_are_exact():
    """cmdiad_lead_rows writes exactly the B cls rows of both streams; cmdiad_layernorm_skip_first writes exactly the token rows'
    LayerNorm into its column block of the centre-major features (NaN-filled outputs: a missing or stray write fails)."""
    B, G, C = 3, 37, 384
    T = G + 1
    g = torch.Generator().manual_seed(4)
    cls, cls_pos = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    x = torch.full((B * T, C), float("nan"), device=DEV)
    pos = torch.full((B * T, C), float("nan"), device=DEV)
    ops.lead_rows(x, pos, cls, cls_pos, B, T)
    want_x = torch.full_like(x, float("nan"))
    want_p = torch.full_like(pos, float("nan"))
    want_x[::T], want_p[::T] = cls, cls_pos
    torch.testing.assert_close(x, want_x, rtol=0, atol=0, equal_nan=True)
    torch.testing.assert_close(pos, want_p, rtol=0, atol=0, equal_nan=True)

    x = (3.0 * torch.randn(B * T, C, generator=g) + 0.5).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    feats = torch.full((B * G, 2 * C), float("nan"), device=DEV)
    ops.layernorm_skip_first(x, gamma, beta, 1e-5, B, T, feats[:, C:])
    tok = x.view(B, T, C)[:, 1:].reshape(B * G, C).contiguous()
    want = torch.empty((B * G, C), device=DEV)
    ops.layernorm(tok.clone(), gamma, beta, 1e-5, out_f32=want, want_bf16=False)
    assert torch.equal(feats[:, C:], want)                 # the same bits as cmdiad_layernorm on the same rows
    assert torch.isnan(feats[:, :C]).all()
    torch.testing.assert_close(want, torch.nn.functional.layer_norm(tok, (C,), gamma, beta, 1e-5), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("batch_stats", [False, True])
def test_pointbert_vs_reference_golden(golden, batch_stats):
    g = golden("gpb_pointbert.npz")
    mode = "train" if batch_stats else "eval"
    pm = runtime.PackedPointBERT(synth_pointbert_state_dict(int(g["seed"])), device=DEV, group_size=32, num_group=64,
                                 bn_batch_stats=batch_stats)
    xyz = torch.from_numpy(np.ascontiguousarray(g["pc"][0].T)[None]).to(DEV)
    feats, center, ori_idx, center_idx = pm.forward(xyz)
    np.testing.assert_array_equal(center_idx.cpu().numpy(), g["center_idx"])
    np.testing.assert_array_equal(center.cpu().numpy(), g["center"])
    np.testing.assert_array_equal(ori_idx.cpu().numpy().astype(np.int32), g["ori_idx"])
    mean_rel, max_rel = _rel(feats.transpose(1, 2).cpu(), torch.from_numpy(g[f"feats_{mode}"]))
    assert mean_rel < 0.015 and max_rel < 0.12, (mean_rel, max_rel)
    _, nb = ops.knn_group(xyz, center, 32)
    tok = pm.encode(nb).cpu()                              # [65, 256]: row 0 is the (unwritten) cls row
    mt, xt = _rel(tok[1:], torch.from_numpy(g[f"tokens_{mode}"]).reshape(-1, 256))
    assert mt < 0.01 and xt < 0.08, (mt, xt)


def _clouds(B, N=24576):
    """B clouds of N points; cloud i depends on i alone (the first two are the same in every batch)."""
    out = []
    for i in range(B):
        g = torch.Generator().manual_seed(77 + i)
        base = torch.rand(N, 3, generator=g) * torch.tensor([0.08, 0.08, 0.01])
        out.append(base + 0.002 * torch.randn(N, 3, generator=g))
    return torch.stack(out).contiguous()


@functools.lru_cache(maxsize=None)
def _ref_full(i):
    """float64 restatement of cloud i of _clouds (the first two clouds are the same in every batch built by _clouds)."""
    xyz = np.ascontiguousarray(_clouds(2)[i:i + 1].numpy())
    cidx, cen = ok.fps(xyz, 1024)
    idx, nb = ok.knn_group(xyz, cen, 128)
    with torch.no_grad():
        ref = pointbert_forward64(synth_pointbert_state_dict(21), torch.from_numpy(nb), torch.from_numpy(cen))
    return cidx, idx, ref


@pytest.mark.parametrize("B", [2, 24])
@pytest.mark.parametrize("fold", ["pmae", "0"])
def test_pointbert_full_size_vs_float64(B, fold, monkeypatch):
    """G = 1024, Mg = 128, N = 24 576: T = 1025 tokens per cloud (attention pads to 1088).  At B = 24, B * 1025 >= 24 576 rows, so
    with the LayerNorm fold the fused MLP kernel runs; it must give the same bits as the two launches."""
    monkeypatch.setenv("CMDIAD_LN_FOLD", fold)
    sd = synth_pointbert_state_dict(21)
    pm = runtime.PackedPointBERT(sd, device=DEV)
    xyz = _clouds(B).to(DEV)
    monkeypatch.setenv("CMDIAD_PMAE_MLP", "1" if B == 24 else "0")
    feats, center, ori_idx, center_idx = pm.forward(xyz)
    assert feats.shape == (B, 1024, 768)
    for i in range(2):
        cidx, idx, ref = _ref_full(i)
        np.testing.assert_array_equal(center_idx[i:i + 1].cpu().numpy(), cidx)
        np.testing.assert_array_equal(ori_idx[i:i + 1].cpu().numpy(), idx)
        mean_rel, max_rel = _rel(feats[i:i + 1].transpose(1, 2).cpu(), ref)
        assert mean_rel < 0.015 and max_rel < 0.12, (i, mean_rel, max_rel)
    if B == 24:
        monkeypatch.setenv("CMDIAD_PMAE_MLP", "0")
        feats0 = pm.forward(xyz)[0]
        assert torch.equal(feats, feats0)


def test_pointbert_batch_equals_single_clouds():
    """What the micro-batched drivers rely on: a cloud's features do not depend on the batch around it, bit for bit."""
    pm = runtime.PackedPointBERT(synth_pointbert_state_dict(21), device=DEV, group_size=32, num_group=64)
    xyz = _clouds(3, 3000).to(DEV)
    batch = pm.forward(xyz)
    for i in range(3):
        one = pm.forward(xyz[i:i + 1].contiguous())
        for a, b in zip(batch, one):
            assert torch.equal(a[i:i + 1], b), i


def test_features_call_with_point_bert_returns_reference_shapes():
    from cmdiad_amd.feature_extractors.features import Features
    from cmdiad_amd.synth import synth_rgb
    args = types.SimpleNamespace(rgb_backbone_name='vit_base_patch8_224_dino', xyz_backbone_name='Point_Bert', group_size=32,
                                 num_group=64, rgb_size=224, xyz_size=224, gt_size=224, f_coreset=1.0, coreset_eps=0.9,
                                 coreset_dtype='FP16', random_state=None, ocsvm_nu=0.5, ocsvm_maxiter=1000)
    f = Features(args)
    assert isinstance(f._engine.pm, runtime.PackedPointBERT)
    xyz = _clouds(1, 3000).transpose(1, 2).contiguous()           # [1, 3, N] as the reference's callers pass it
    rgb_maps, xyz_maps, center, ori_idx, center_idx, _ = f(synth_rgb(1), xyz)
    assert rgb_maps[0].shape == (1, 768, 28, 28)
    assert xyz_maps[0].shape == (1, 768, 64)                       # models/models.py:350: [B, 2 x 384, G]
    assert center.shape == (1, 64, 3) and ori_idx.shape == (1, 64, 32) and center_idx.shape == (1, 64)
    ref = runtime.PackedPointBERT(f.deep_feature_extractor.xyz_backbone.state_dict(), device=DEV, group_size=32, num_group=64)
    assert torch.equal(xyz_maps[0], ref.forward(xyz.transpose(1, 2).contiguous().to(DEV))[0].transpose(1, 2).cpu())
