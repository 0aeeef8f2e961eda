"""Operand-rounded float64 restatement of two hand-written TRAINING steps: the HRNet trunk (conv_train.hrnet_forward_backward)
and the feature-to-input conv head (conv_train.ftoi_forward_backward).  Train-mode algebra of ``oracle/heads.py`` (BatchNorm on
batch statistics), differentiated by torch autograd in float64, with bf16 rounding at the places where the HIP path rounds.

TEST INFRASTRUCTURE ONLY (see oracle/README.md): imported by tests/ alone.

Why: against the module's own fp32 layers the HIP step differs by a few % of gradient norm (bf16 operands flip ~0.2 % of every
ReLU mask), so those tests check gradients by cosine alone -- blind to a gradient that is wrong by a constant factor.  With the
same roundings on both sides both open the same ReLUs, and what is left is fp32 accumulation order plus the odd bf16 rounding
that flips on a last-bit difference: small enough to bound the relative L2 error of every gradient.

Two straight-through helpers carry the roundings (``rounded=False`` makes both the identity):
  * ``rb(v)``: the VALUE is rounded to bf16 (from the fp32 value the GPU holds), the gradient passes through unchanged;
  * ``gb(v)``: the value passes through, the GRADIENT arriving at v is rounded to bf16.

Rounding points, read off cmdiad_amd/conv_train.py:
  forward (rb) -- every convolution's weight (_conv_w / _w1x1 / cast_bf16(W1)) and every convolution's input:
    * HRNet: the image (cmdiad_im2col3x3_bf16 rounds the im2col'd image), the BatchNorm + ReLU outputs y1 (bn1), x16 (bn2 and
      every bn3), t1 (bn1 of a block), t2 (bn2 of a block);
    * FtoI: the tokens x0, the bicubic output u (cmdiad_upsample_bicubic writes bf16), h2 and h3 (bf16 epilogue of conv2 / conv3).
    Convolution outputs, biases and the BatchNorm arithmetic stay wide.  The residual identity is the fp32 copy: x32 (the f32
    output of the previous block's bn3) or the downsample BatchNorm's f32 output; the next block's conv1 / downsample read x16.
  backward (gb) -- the gradient w.r.t. every convolution's OUTPUT is bf16, everything else fp32:
    * the loss head's dout (bf16 by cmdiad_loss_head) on the final layer / conv4 output;
    * HRNet: each bn_relu_bwd result (dz of z1, z2 and of every conv1 / conv2 / conv3 / downsample output of a block); the
      zero-stuffed ``up`` is the bf16 dz of z2 itself;
    * FtoI: the relu_bwd results (conv2 / conv3 outputs) and cast_bf16(dh1) (conv1 output, after the bicubic adjoint).
    The data gradients (dX, dt1, dt2, du, dh1, ...) and the gradient of the fp32 identity path (g32) stay fp32.
Reference anchors as in oracle/heads.py (models/hrnet.py:8-43, 146-177, 251-299; models/hallucination_network.py:185-220).
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5


def _r16(v):
    return v.float().to(torch.bfloat16).to(v.dtype)


def rb(v):
    """value rounded to bf16, gradient straight through"""
    return v + (_r16(v.detach()) - v.detach())


class _GradBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return _r16(g)


def gb(v):
    """value unchanged, the gradient arriving at v rounded to bf16"""
    return _GradBf16.apply(v)


def _ident(v):
    return v


def _leaves(sd, names, device):
    return {n: sd[n].detach().to(device=device, dtype=torch.float64).clone().requires_grad_(True) for n in names}


def _bn_train(x, P, name, stats):
    """BatchNorm2d in train() mode (batch statistics, eps 1e-5); records (batch mean, biased batch variance)."""
    with torch.no_grad():
        stats[name] = (x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False))
    return F.batch_norm(x, None, None, P[name + ".weight"], P[name + ".bias"], True, 0.0, EPS)


def mean_row_norm(a, b, dim):
    """sum of the L2 norms along `dim`, divided by the batch size (the heads' loss)"""
    d = torch.linalg.norm(a - b, dim=dim)
    return d.sum() / d.shape[0]


def hrnet_param_names(sd):
    """The trunk's trainable parameters: what HRNet.forward uses (layer4 is constructed but never run)."""
    return [n for n in sd if not n.startswith("layer4.") and n.rsplit(".", 1)[-1] in ("weight", "bias")]


def hrnet_train_rounded(sd, img, feature, rounded=True):
    """sd: the trunk's state_dict (reference names; extra keys ignored), img [B,3,S,S], feature [B,(S/4)^2,768].
    -> (loss 0-dim, {name: grad}, {bn name: (batch mean, biased batch variance)}), all float64 on img's device."""
    R, G = (rb, gb) if rounded else (_ident, _ident)
    P = _leaves(sd, hrnet_param_names(sd), img.device)
    stats = {}
    x = G(F.conv2d(R(img.double()), R(P["conv1.weight"]), stride=2, padding=1))
    y1 = R(F.relu(_bn_train(x, P, "bn1", stats)))
    z2 = G(F.conv2d(y1, R(P["conv2.weight"]), stride=2, padding=1))
    x32 = F.relu(_bn_train(z2, P, "bn2", stats))
    x16 = R(x32)
    for layer in (1, 2, 3):
        for i in range(4):
            b = f"layer{layer}.{i}"
            t1 = R(F.relu(_bn_train(G(F.conv2d(x16, R(P[b + ".conv1.weight"]))), P, b + ".bn1", stats)))
            t2 = R(F.relu(_bn_train(G(F.conv2d(t1, R(P[b + ".conv2.weight"]), padding=1)), P, b + ".bn2", stats)))
            zc3 = G(F.conv2d(t2, R(P[b + ".conv3.weight"])))
            if (b + ".downsample.0.weight") in P:
                identity = _bn_train(G(F.conv2d(x16, R(P[b + ".downsample.0.weight"]))), P, b + ".downsample.1", stats)
            else:
                identity = x32
            x32 = F.relu(_bn_train(zc3, P, b + ".bn3", stats) + identity)
            x16 = R(x32)
    out = G(F.conv2d(x16, R(P["final_layer.weight"]), P["final_layer.bias"]))
    tokens = out.flatten(2).transpose(1, 2)
    loss = mean_row_norm(tokens, feature.to(device=img.device, dtype=torch.float64), 2)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in P.items()}, stats


FTOI_PARAMS = tuple(f"conv{i}.{w}" for i in range(1, 5) for w in ("weight", "bias"))


def ftoi_conv_train_rounded(sd, feature, img, rounded=True):
    """sd: the head's state_dict (``norm`` is ignored: the reference's forward never applies it), feature [B,s*s,C],
    img [B,3,S,S] (S = the bicubic output size) -> (loss 0-dim, {conv name: grad}), float64 on feature's device."""
    R, G = (rb, gb) if rounded else (_ident, _ident)
    P = _leaves(sd, FTOI_PARAMS, feature.device)
    B, T, C = feature.shape
    s = int(round(math.sqrt(T)))
    x0 = R(feature.double().transpose(1, 2).reshape(B, C, s, s))
    h1 = G(F.conv2d(x0, R(P["conv1.weight"]), P["conv1.bias"], padding=1))
    u = R(F.interpolate(h1, size=tuple(img.shape[-2:]), mode="bicubic", align_corners=False))
    h2 = R(F.relu(G(F.conv2d(u, R(P["conv2.weight"]), P["conv2.bias"], padding=1))))
    h3 = R(F.relu(G(F.conv2d(h2, R(P["conv3.weight"]), P["conv3.bias"], padding=1))))
    out = G(F.conv2d(h3, R(P["conv4.weight"]), P["conv4.bias"], padding=1))
    loss = mean_row_norm(out, img.to(device=feature.device, dtype=torch.float64), 1)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in P.items()}
