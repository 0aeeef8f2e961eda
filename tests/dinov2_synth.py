"""Seeded synthetic DINOv2 ViT-B/14 weights (timm's vit_base_patch14_dinov2.lvd142m layout: 518 / 14, LayerScale in every block)
and its float64 restatement, shared by tests/golden/make_golden_dinov2.py, the DINOv2 tests and tools/dinov2_time.py.

ViT-B/8's synthetic state_dict (oracle.nets.synth_state_dict("vit", seed)) at 1 370 tokens and patch 14, plus ls1.gamma / ls2.gamma
drawn from their own generators seeded by (seed, crc32(name)).  The gammas are NOT timm's init value 1e-5 (the blocks would vanish
behind the residual stream and a missing fold would go unseen): uniform in [0.2, 1.2] with a quarter of them negative."""
import zlib

import torch
import torch.nn.functional as F

DIM, DEPTH, HEADS, PATCH, SIZE = 768, 12, 12, 14, 518
GRID = SIZE // PATCH          # 37
TOKENS = GRID * GRID + 1      # 1 370


def _gamma(name, seed):
    g = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(name.encode())) % (2 ** 63))
    mag = 0.2 + torch.rand(DIM, generator=g)
    sign = torch.where(torch.rand(DIM, generator=g) < 0.25, -1.0, 1.0)
    return mag * sign


def synth_dinov2_state_dict(seed):
    from oracle import nets
    sd = nets.synth_state_dict("vit", seed, tokens=TOKENS, patch=PATCH)
    for i in range(DEPTH):
        for ls in ("ls1", "ls2"):
            name = f"blocks.{i}.{ls}.gamma"
            sd[name] = _gamma(name, seed)
    return sd


def dinov2_block64(x, sd, p, num_heads=HEADS, eps=1e-6):
    """timm Block with LayerScale, DropPath inactive: x + ls1 * attn(norm1(x)), then x + ls2 * mlp(norm2(x)) (float64)."""
    from oracle import nets
    x = x + sd[p + ".ls1.gamma"] * nets._attention(nets._ln(x, sd, p + ".norm1", eps), sd, p + ".attn", num_heads)
    h = nets._linear(F.gelu(nets._linear(nets._ln(x, sd, p + ".norm2", eps), sd, p + ".mlp.fc1")), sd, p + ".mlp.fc2")
    return x + sd[p + ".ls2.gamma"] * h


def dinov2_tokens64(sd, rgb, depth=DEPTH, eps=1e-6):
    """rgb [B,3,518,518] -> forward_features tokens [B,1370,768] in float64 (patch_embed, _pos_embed, blocks, norm;
    models/models.py:36-37)."""
    sd = {k: v.double() for k, v in sd.items()}
    x = F.conv2d(rgb.double(), sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=PATCH)
    B = x.shape[0]
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([sd["cls_token"].expand(B, -1, -1), x], dim=1) + sd["pos_embed"]
    for i in range(depth):
        x = dinov2_block64(x, sd, f"blocks.{i}", eps=eps)
    from oracle import nets
    return nets._ln(x, sd, "norm", eps)


def rgb_patches64(fmap):
    """features.py:160-167 in float64: [1,C,s,s] -> (rgb_patch [s*s,C], rgb_patch2 [3136,C])."""
    C, s = fmap.shape[1], fmap.shape[-1]
    p = fmap.double().reshape(C, -1).T
    p2 = F.adaptive_avg_pool2d(p.T.reshape(C, s, s), (56, 56)).reshape(C, -1).T
    return p, p2
