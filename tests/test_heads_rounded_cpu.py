"""oracle/heads_rounded.py, the float64 restatement the GPU tests of the HRNet trunk's and the FtoI conv head's training steps
compare against (tests/test_gpu_heads_rounded.py): with its bf16 roundings switched off it must BE float64 autograd through the
modules' own torch layers -- loss, every gradient, every BatchNorm's batch statistics -- at a small image size.  Also pins what
its two straight-through helpers do."""
import numpy as np
import torch
import torch.nn.functional as F

from cmdiad_amd.models.hallucination_network import HallucinationFeatureToInputConv
from cmdiad_amd.models.hrnet import HRNet
from oracle import heads, heads_rounded


def _assert_close(got, want, what):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, what
    err = float((got - want).norm() / want.norm())
    assert err < 1e-10, (what, err)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-9, atol=1e-12 * float(want.abs().max()), err_msg=what)


def test_straight_through_helpers():
    g = torch.Generator().manual_seed(3)
    v = (torch.randn(1000, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    w = torch.randn(1000, generator=g, dtype=torch.float64)
    r = heads_rounded.rb(v)
    assert torch.equal(r, v.detach().float().bfloat16().double()) and not torch.equal(r, v.detach())
    (r * w).sum().backward()
    assert torch.equal(v.grad, w)                                           # rb: the gradient passes unchanged
    v.grad = None
    q = heads_rounded.gb(v)
    assert torch.equal(q, v.detach())
    (q * w).sum().backward()
    assert torch.equal(v.grad, w.float().bfloat16().double()) and not torch.equal(v.grad, w)   # gb: the gradient is rounded


def test_hrnet_restatement_unrounded_equals_autograd_through_the_module():
    """HRNet trunk at 32 x 32 (an 8 x 8 token map), B = 2.  Every BatchNorm of the module runs with momentum 1, so after one step
    its running buffers ARE the batch statistics (mean; unbiased variance): nn.BatchNorm2d's own bookkeeping pins the restatement's."""
    sd = heads.synth_head_state_dict("hrnet", 41)
    g = torch.Generator().manual_seed(5)
    B, S = 2, 32
    img = torch.randn(B, 3, S, S, generator=g, dtype=torch.float64)
    feat = torch.randn(B, (S // 4) ** 2, 768, generator=g, dtype=torch.float64)
    m = HRNet(512, 768, 0.1)
    m.load_state_dict(sd)
    m.double().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 1.0          # (Bottleneck's BatchNorms do not take HRNet's bn_momentum, as in the reference)
    x = torch.relu(m.bn1(m.conv1(img)))
    x = torch.relu(m.bn2(m.conv2(x)))
    x = m.final_layer(m.layer3(m.layer2(m.layer1(x))))
    want_loss = heads.mean_row_norm(x.flatten(2).transpose(1, 2), feat, 2)
    want_loss.backward()
    loss, grads, stats = heads_rounded.hrnet_train_rounded(sd, img, feat, rounded=False)
    _assert_close(loss, want_loss.detach(), "loss")
    params = dict(m.named_parameters())
    assert set(grads) == {n for n in params if not n.startswith("layer4.")}
    for n, gr in grads.items():
        _assert_close(gr, params[n].grad, n)
    mods = dict(m.named_modules())
    assert len(stats) == 39
    for n, (mean, var) in stats.items():
        count = B * (S // 2) ** 2 if n == "bn1" else B * (S // 4) ** 2
        _assert_close(mean, mods[n].running_mean, n + " mean")
        _assert_close(var * count / (count - 1), mods[n].running_var, n + " var")
    # with the roundings on it is a different function: the pin above is not vacuous
    loss_r, grads_r, _ = heads_rounded.hrnet_train_rounded(sd, img, feat)
    assert 0 < abs(float(loss_r - loss)) < 1e-2 * float(loss)
    assert float((grads_r["conv1.weight"] - grads["conv1.weight"]).norm()) > 0


def test_ftoi_conv_restatement_unrounded_equals_autograd_through_the_module():
    """FtoI conv head on a 4 x 4 token map upsampled to 16 x 16, B = 2: conv1, bicubic, conv2 + ReLU, conv3 + ReLU, conv4."""
    sd = heads.synth_head_state_dict("ftoi_conv", 41)
    g = torch.Generator().manual_seed(6)
    B, s, S = 2, 4, 16
    feat = torch.randn(B, s * s, 768, generator=g, dtype=torch.float64)
    img = torch.randn(B, 3, S, S, generator=g, dtype=torch.float64)
    m = HallucinationFeatureToInputConv(None, 768)
    m.load_state_dict(sd)
    m.double().train()
    h = m.conv1(feat.transpose(1, 2).reshape(B, 768, s, s))
    h = F.interpolate(h, size=(S, S), mode="bicubic")
    h = m.conv4(torch.relu(m.conv3(torch.relu(m.conv2(h)))))
    want_loss = heads.mean_row_norm(h, img, 1)
    want_loss.backward()
    loss, grads = heads_rounded.ftoi_conv_train_rounded(sd, feat, img, rounded=False)
    _assert_close(loss, want_loss.detach(), "loss")
    params = dict(m.named_parameters())
    assert set(grads) == set(heads_rounded.FTOI_PARAMS)
    for n, gr in grads.items():
        _assert_close(gr, params[n].grad, n)
    loss_r, grads_r = heads_rounded.ftoi_conv_train_rounded(sd, feat, img)
    assert 0 < abs(float(loss_r - loss)) < 1e-2 * float(loss)
    assert float((grads_r["conv1.weight"] - grads["conv1.weight"]).norm()) > 0
