"""CPU: the host plumbing that the five training heads share (cmdiad_amd/train.py) -- the one autograd function behind every
head's loss, the BatchNorm running-statistics update against nn.BatchNorm2d itself -- and the routing of the head modules'
forward(): training with gradients goes to the hand-written path, whatever the environment says.  No GPU, no native library."""
import types

import pytest
import torch
import torch.nn as nn

from cmdiad_amd import conv_train, train


# ---------------------------------------------------------------------------------------------------------------- step_loss
def _fake_step(grads, check=None):
    """A step over CPU tensors: loss = sum of the parameters' sums, `grads` as its stored gradients; records how it was called."""
    calls = []

    def step(ps, need_grad):
        assert not torch.is_grad_enabled() and not any(p.requires_grad for p in ps)      # detached parameters, inside Function.forward
        calls.append(need_grad)
        return sum(p.sum() for p in ps), (grads if need_grad else None), check
    return step, calls


def test_step_loss_scales_the_stored_gradients_by_the_upstream_factor():
    a, b, c = (nn.Parameter(torch.randn(s)) for s in ((3,), (2, 2), (4,)))
    ga, gc = torch.randn(3), torch.randn(4)
    step, calls = _fake_step((ga, None, gc))
    loss = train.step_loss(step, (a, b, c))
    assert calls == [True] and loss.requires_grad
    (3 * loss).backward()
    assert torch.equal(a.grad, 3 * ga) and torch.equal(c.grad, 3 * gc)
    assert b.grad is None                                       # a None gradient stays None


def test_step_loss_needs_no_gradient_without_grad_mode_or_trainable_parameters():
    a = nn.Parameter(torch.randn(3))
    frozen = torch.randn(3)

    def never():
        raise AssertionError("backward() reached")
    step, calls = _fake_step((torch.randn(3),), check=never)
    with torch.no_grad():
        assert not train.step_loss(step, (a,)).requires_grad
    assert not train.step_loss(step, (frozen,)).requires_grad
    assert calls == [False, False]
    # one trainable parameter among frozen ones is enough
    step, calls = _fake_step((None, torch.ones(3)))
    loss = train.step_loss(step, (frozen, a))
    assert calls == [True] and loss.requires_grad
    loss.backward()
    assert torch.equal(a.grad, torch.ones(3))


def test_step_loss_runs_the_check_at_the_start_of_backward():
    a = nn.Parameter(torch.randn(3))
    state = {"valid": True}

    def check():
        if not state["valid"]:
            raise RuntimeError("gradients have been overwritten")
    step, _ = _fake_step((torch.ones(3),), check=check)
    train.step_loss(step, (a,)).backward()
    assert torch.equal(a.grad, torch.ones(3))
    loss = train.step_loss(step, (a,))
    state["valid"] = False
    with pytest.raises(RuntimeError, match="overwritten"):
        loss.backward()


# ---------------------------------------------------------------------------------------------------------------- running statistics
@pytest.mark.parametrize("momentum", [0.1, 0.37, None])
def test_update_running_stats_is_batchnorm2d_in_train_mode(momentum):
    g = torch.Generator().manual_seed(3)
    C = 5
    ref = nn.BatchNorm2d(C, momentum=momentum).double().train()
    mine = nn.BatchNorm2d(C, momentum=momentum).double().train()
    for k in range(3):                                          # three batches: the cumulative average changes its factor every step
        x = (torch.randn(4, C, 3, 2, generator=g, dtype=torch.float64) * (1 + k) + k)
        ref(x)
        rows = x.transpose(0, 1).reshape(C, -1)
        train.update_running_stats(mine, rows.mean(1), rows.var(1, unbiased=False), rows.shape[1])
        assert int(mine.num_batches_tracked) == int(ref.num_batches_tracked) == k + 1
        assert (mine.running_mean - ref.running_mean).abs().max() <= 1e-12
        assert (mine.running_var - ref.running_var).abs().max() <= 1e-12


def test_update_running_stats_leaves_a_module_without_them_untouched():
    bn = nn.BatchNorm2d(4, track_running_stats=False).double()
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    train.update_running_stats(bn, torch.randn(4, dtype=torch.float64), torch.rand(4, dtype=torch.float64), 24)
    assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
    after = bn.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)


# ---------------------------------------------------------------------------------------------------------------- routing
def test_training_forward_goes_to_the_hand_written_path_whatever_the_environment_says(monkeypatch):
    """The modules used to select their own torch layers under CMDIAD_CONV_TRAIN=torch / CMDIAD_HRNET_TRAIN=torch: the variables
    select nothing any more -- forward() in train() mode with gradients returns what conv_train's loss functions return."""
    from cmdiad_amd.models import hallucination_network as hn
    from cmdiad_amd.models.hrnet import HRNet
    monkeypatch.setenv("CMDIAD_CONV_TRAIN", "torch")
    monkeypatch.setenv("CMDIAD_HRNET_TRAIN", "torch")
    seen = []

    def sentinel(name):
        def fn(module, *args):
            seen.append((name, module))
            return name
        return fn
    for name in ("tower_loss", "ftoi_conv_loss", "ftoi_mlp_loss", "hrnet_loss"):
        monkeypatch.setattr(conv_train, name, sentinel(name))
    tok, img = torch.zeros(1, 3136, 768), torch.zeros(1, 3, 224, 224)
    hr = HRNet(512, 768).train()
    assert hr(img, tok) == "hrnet_loss"
    conv = hn.HallucinationCrossModalityConv(None, 768, 768).train()
    assert conv(tok, tok, False, "l2") == ("tower_loss", "tower_loss")
    ftoi = hn.HallucinationFeatureToInputConv(None, 768).train()
    assert ftoi(tok, img) == "ftoi_conv_loss"
    mlp = hn.HallucinationRGBFeatureToXYZInputMLP(types.SimpleNamespace(estimate_depth=False), 768).train()
    assert mlp(tok, img) == "ftoi_mlp_loss"
    assert seen == [("hrnet_loss", hr), ("tower_loss", conv.rgb_conv), ("tower_loss", conv.xyz_conv), ("ftoi_conv_loss", ftoi),
                    ("ftoi_mlp_loss", mlp)]
