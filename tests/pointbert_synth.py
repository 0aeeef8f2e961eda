"""Seeded synthetic Point-BERT weights (PointTransformer(encoder_dims=256), models/models.py:246-264), shared by
tests/golden/make_golden_pointbert.py and the Point-BERT tests, so that the fixture stores no weights.

Point-MAE's synthetic state_dict (oracle.nets.synth_state_dict("pointmae", seed)) with the encoder's last convolution at 256
output channels and the three Point-BERT tensors added (reduce_dim, cls_token, cls_pos); each of the replaced or added tensors is
drawn from its own generator seeded by (seed, crc32(name)), as synth_state_dict draws every tensor."""
import math
import zlib

import torch

ENCODER_DIMS = 256
TRANS_DIM = 384


def _draw(name, shape, seed, scale=None):
    g = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(name.encode())) % (2 ** 63))
    if scale is None:
        fan_in = math.prod(shape[1:]) if len(shape) > 1 else 1
        scale = 1.0 / math.sqrt(fan_in)
    return scale * torch.randn(shape, generator=g)


def synth_pointbert_state_dict(seed):
    from oracle import nets
    sd = nets.synth_state_dict("pointmae", seed)
    sd["encoder.second_conv.3.weight"] = _draw("encoder.second_conv.3.weight", (ENCODER_DIMS, 512, 1), seed)
    sd["encoder.second_conv.3.bias"] = _draw("encoder.second_conv.3.bias", (ENCODER_DIMS,), seed, 0.02)
    sd["reduce_dim.weight"] = _draw("reduce_dim.weight", (TRANS_DIM, ENCODER_DIMS), seed)
    sd["reduce_dim.bias"] = _draw("reduce_dim.bias", (TRANS_DIM,), seed, 0.02)
    sd["cls_token"] = _draw("cls_token", (1, 1, TRANS_DIM), seed, 0.02)
    sd["cls_pos"] = _draw("cls_pos", (1, 1, TRANS_DIM), seed, 1.0)   # torch.randn in the reference's own init
    return sd


def pointbert_forward64(sd, neighborhood, center, batch_stats=False, depth=12, num_heads=6, taps=(3, 11), eps=1e-5):
    """float64 restatement from oracle.nets pieces: neighborhood [B,G,M,3], center [B,G,3] -> [B,768,G]
    (models/models.py:326-352: encoder, reduce_dim, cls token / cls_pos in front, pos re-added every block, fetch LayerNorms
    without the cls row)."""
    import torch.nn.functional as F
    from oracle import nets
    sd = {k: v.double() for k, v in sd.items()}
    tok = nets.pointmae_encoder(sd, neighborhood.double(), "encoder.", batch_stats)
    x = nets._linear(tok, sd, "reduce_dim")
    B = x.shape[0]
    pos = nets._linear(F.gelu(nets._linear(center.double(), sd, "pos_embed.0")), sd, "pos_embed.2")
    x = torch.cat([sd["cls_token"].expand(B, -1, -1), x], 1)
    pos = torch.cat([sd["cls_pos"].expand(B, -1, -1), pos], 1)
    outs = []
    for i in range(depth):
        x = nets._block(x + pos, sd, f"blocks.blocks.{i}", num_heads, eps)
        if i in taps:
            outs.append(nets._ln(x, sd, "norm", eps)[:, 1:].transpose(-1, -2))
    return torch.cat(outs, dim=1)
