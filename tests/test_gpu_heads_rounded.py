"""Hand-written training steps of the HRNet trunk (conv_train.hrnet_forward_backward) and the feature-to-input conv head
(conv_train.ftoi_forward_backward) at the production shapes -- 224 x 224 images, 3136 tokens -- against their float64
restatement with the same bf16 roundings (oracle/heads_rounded.py, pinned to the modules' own layers by
tests/test_heads_rounded_cpu.py), run in float64 on the device.  Both sides round the same operands, so every gradient is held
to its relative L2 error and its norm ratio (a gradient wrong by a constant factor fails here; a cosine cannot see it), besides
its cosine, the loss and every BatchNorm's batch statistics.  The split-K and chunk choices of the step (_split_for, bn_relu_bwd) depend on the token
count, so only these shapes test the code that runs.

What is left is fp32 accumulation order and the bf16 roundings that flip on a last-bit difference.  In the FtoI head (three
rounded stages) that stays small.  The HRNet trunk is 36 rounded BatchNorm + ReLU stages deep, and there the flips cascade:
the batch statistics agree to 1e-9 at bn1 and to ~4e-4 of the batch std at layer3.3, and the gradients below layer3.3.bn3
differ by 10-20 % in relative L2 (1 - cos ~0.02), while the final layer's agree to 3e-4.  That is the restatement's own
sensitivity, not the kernels': multiplying every convolution output of the float64 restatement by (1 + 1e-7 N(0,1)) -- less
than fp32 rounding -- moves it from itself by the same amounts, parameter by parameter.  A constant factor does not hide in that
noise: the norm ratio |‖g‖ / ‖ref‖ - 1| of a convolution weight's gradient stays below 6e-3, so every tensor's ratio is bounded
too.  Measured on an MI355X, worst over 5 input seeds per batch size (gradients: worst parameter):
              grad rel L2   |norm ratio - 1|   1 - cos    loss       mean / std   var (rel)
  HRNet B=1   2.2e-1        3.9e-2             2.3e-2     4.7e-6     4.8e-4       2.4e-3
  HRNet B=3   1.9e-1        3.8e-2             1.8e-2     8.7e-6     2.7e-4       1.2e-3
  FtoI  B=1   5.0e-3        1.0e-4             1.3e-5     3.9e-6
  FtoI  B=2   4.5e-3        5.0e-5             9.9e-6     3.6e-6
The bounds (HRNET_BOUNDS, FTOI_BOUNDS: per stage and kind for HRNet, per layer for FtoI) are 2x the worst value of their group
for relative L2 and cosine, 4x for the norm ratio, the loss and the statistics.  The running statistics that hrnet_loss
writes are checked separately against nn.BatchNorm2d's update rule applied to the step's own batch statistics."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd import conv_train  # noqa: E402
from oracle import heads, heads_rounded  # noqa: E402

DEV = "cuda"

# (relative L2, |norm ratio - 1|, 1 - cosine) of every gradient of a group; group maxima measured in the module docstring's runs
HRNET_BOUNDS = {
    "final": (7e-4, 4e-5, 1.2e-7),                # measured 3.4e-4, 1.0e-5, 5.8e-8
    "layer3/conv": (0.3, 8e-3, 2.5e-2),           # 1.5e-1, 2.2e-3, 1.2e-2
    "layer3/bn": (0.36, 0.1, 3.3e-2),             # 1.8e-1, 2.5e-2, 1.6e-2
    "layer2/conv": (0.36, 8e-3, 3.2e-2),          # 1.8e-1, 2.1e-3, 1.6e-2
    "layer2/bn": (0.44, 0.14, 4.6e-2),            # 2.2e-1, 3.5e-2, 2.3e-2
    "layer1/conv": (0.36, 1.5e-2, 3.3e-2),        # 1.8e-1, 3.9e-3, 1.7e-2
    "layer1/bn": (0.44, 0.14, 4.4e-2),            # 2.2e-1, 3.7e-2, 2.2e-2
    "stem/conv": (0.35, 2.2e-2, 3.1e-2),          # 1.8e-1, 5.6e-3, 1.6e-2
    "stem/bn": (0.42, 0.15, 4.5e-2),              # 2.1e-1, 3.9e-2, 2.3e-2
}
HRNET_LOSS, HRNET_MEAN, HRNET_VAR = 3e-5, 1.9e-3, 9e-3   # measured 8.7e-6, 4.8e-4, 2.4e-3
FTOI_BOUNDS = {
    "conv1.weight": (1e-2, 8e-5, 2.5e-5),        # 5.0e-3, 1.9e-5, 1.3e-5
    "conv2.weight": (6e-3, 1.6e-4, 8.5e-6),      # 2.9e-3, 3.9e-5, 4.3e-6
}
FTOI_OTHER = (7e-4, 4e-4, 1.2e-7)                # every bias, conv3 / conv4 weights: 3.6e-4, 1.0e-4, 6.2e-8
FTOI_LOSS = 1.5e-5                               # 3.9e-6


def hrnet_group(name):
    if name.startswith("final_layer."):
        return "final"
    stage = name.split(".")[0] if name.startswith("layer") else "stem"
    return stage + ("/bn" if name.split(".")[-2].startswith("bn") or ".downsample.1." in name else "/conv")


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _ratio(a, b):
    return abs(float(a.double().norm() / b.double().norm()) - 1)


def _one_minus_cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return 1.0 - float((a @ b) / (a.norm() * b.norm()))


def hrnet_errors(B, seed):
    """-> (loss rel error, worst |d mean| / batch std, worst |d var| / var, {parameter: (rel L2, |norm ratio - 1|, 1 - cos)})."""
    sd = heads.synth_head_state_dict("hrnet", 41)
    names = heads_rounded.hrnet_param_names(sd)
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    feat = torch.randn(B, 3136, 768, generator=g).to(DEV)
    P = {n: sd[n].to(DEV) for n in names}
    loss, G, stats = conv_train.hrnet_forward_backward(img, feat, P, B)
    ref_loss, ref_G, ref_stats = heads_rounded.hrnet_train_rounded(sd, img, feat)
    assert set(G) == set(ref_G) == set(names)
    assert set(stats) == set(ref_stats) and len(stats) == 39
    per = {}
    for n in names:
        assert G[n].shape == ref_G[n].shape, n
        per[n] = (_rel(G[n], ref_G[n]), _ratio(G[n], ref_G[n]), _one_minus_cos(G[n], ref_G[n]))
    dmean = max(float(((m - rm).abs() / (rv + 1e-5).sqrt()).max()) for (m, _), (rm, rv) in
                ((stats[k], ref_stats[k]) for k in stats))
    dvar = max(float(((v - rv).abs() / rv).max()) for (_, v), (_, rv) in ((stats[k], ref_stats[k]) for k in stats))
    return abs(float(loss) / float(ref_loss) - 1), dmean, dvar, per


def ftoi_errors(B, seed):
    """-> (loss rel error, {parameter: (rel L2, |norm ratio - 1|, 1 - cos)})."""
    sd = heads.synth_head_state_dict("ftoi_conv", 41)
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, 3136, 768, generator=g).to(DEV)
    img = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    params = tuple(sd[n].to(DEV) for n in heads_rounded.FTOI_PARAMS)
    loss, grads = conv_train.ftoi_forward_backward(feat, img, params, B)
    ref_loss, ref_G = heads_rounded.ftoi_conv_train_rounded(sd, feat, img)
    per = {}
    for n, gr in zip(heads_rounded.FTOI_PARAMS, grads):
        assert gr.shape == ref_G[n].shape, n
        per[n] = (_rel(gr, ref_G[n]), _ratio(gr, ref_G[n]), _one_minus_cos(gr, ref_G[n]))
    return abs(float(loss) / float(ref_loss) - 1), per


@pytest.mark.parametrize("B", [1, 3])
def test_hrnet_step_vs_rounded_float64(B):
    dloss, dmean, dvar, per = hrnet_errors(B, 100 + B)
    bad = {n: v for n, v in per.items() if any(x >= b for x, b in zip(v, HRNET_BOUNDS[hrnet_group(n)]))}
    assert not bad, bad
    assert dloss < HRNET_LOSS, dloss
    assert dmean < HRNET_MEAN and dvar < HRNET_VAR, (dmean, dvar)


@pytest.mark.parametrize("B", [1, 2])
def test_ftoi_conv_step_vs_rounded_float64(B):
    dloss, per = ftoi_errors(B, 200 + B)
    bad = {n: v for n, v in per.items() if any(x >= b for x, b in zip(v, FTOI_BOUNDS.get(n, FTOI_OTHER)))}
    assert not bad, bad
    assert dloss < FTOI_LOSS, dloss


@pytest.mark.parametrize("momentum", [0.1, None])
def test_hrnet_running_statistics_follow_batchnorm2d(momentum, monkeypatch):
    """Two eager steps of HRNet.forward (the hand-written path, no graph) with every BatchNorm at `momentum` (None: the cumulative
    average).  The buffers must be nn.BatchNorm2d's update -- running = (1 - m) running + m stat, the variance made unbiased by
    n / (n - 1) with n = B x 112^2 for bn1 and B x 56^2 for every other BatchNorm, m = momentum or 1 / num_batches_tracked --
    applied to the batch statistics that hrnet_forward_backward returns for the same inputs.  To rtol 1e-6: the unbiased
    correction alone is 1 + 4e-5 at bn1 (B = 2)."""
    from cmdiad_amd.models.hrnet import HRNet
    monkeypatch.setenv("CMDIAD_HRNET_GRAPH", "0")
    B = 2
    sd = heads.synth_head_state_dict("hrnet", 41)
    m = HRNet(512, 768, 0.1)
    m.load_state_dict(sd)
    bns = {n: mod for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)}
    for mod in bns.values():
        mod.momentum = momentum
    m.to(DEV).train()
    gen = torch.Generator().manual_seed(23)
    batches = [(torch.randn(B, 3, 224, 224, generator=gen).to(DEV), torch.randn(B, 3136, 768, generator=gen).to(DEV)) for _ in range(2)]
    for img, feat in batches:
        m(img, feat).backward()                  # no optimizer step: the parameters stay those of the recomputation below
    P = {n: p.detach() for n, p in m.named_parameters() if not n.startswith("layer4.")}
    want = {n: [sd[n + ".running_mean"].double(), sd[n + ".running_var"].double(), sd[n + ".running_mean"].double().abs()]
            for n in bns if not n.startswith("layer4.")}
    assert len(want) == 39
    for k, (img, feat) in enumerate(batches):
        _, _, stats = conv_train.hrnet_forward_backward(img, feat, P, B)
        mom = momentum if momentum is not None else 1.0 / (k + 1)
        for n, (mean, var) in stats.items():
            cnt = B * 112 * 112 if n == "bn1" else B * 56 * 56
            w = want[n]
            w[0] = (1 - mom) * w[0] + mom * mean.cpu()
            w[1] = (1 - mom) * w[1] + mom * var.cpu() * (cnt / (cnt - 1))
            w[2] = (1 - mom) * w[2] + mom * mean.cpu().abs()      # scale of the mean's sum, for its cancellation
    for n, mod in bns.items():
        if n.startswith("layer4."):
            assert int(mod.num_batches_tracked) == 0 and torch.equal(mod.running_mean.cpu(), sd[n + ".running_mean"]), n
            continue
        assert int(mod.num_batches_tracked) == 2, n
        rm, rv, scale = want[n]
        got_m, got_v = mod.running_mean.cpu().double(), mod.running_var.cpu().double()
        assert float(((got_m - rm).abs() / scale).max()) < 1e-6, (n, float(((got_m - rm).abs() / scale).max()))
        np.testing.assert_allclose(got_v.numpy(), rv.numpy(), rtol=1e-6, atol=0, err_msg=n)
