"""Drop-in for the reference's ``models/models.py``: same class / function names, constructor
arguments, state_dict keys and return values; the arithmetic runs in the gfx950 HIP kernels
(cmdiad_amd.runtime) instead of timm / pointnet2_ops / knn_cuda.

Reference anchors: Model models/models.py:9-67; fps :70-78; Group :81-113; Encoder :183-215;
TransformerEncoder :218-243; PointTransformer :246-373.

The nn.Module classes below only OWN parameters (so ``state_dict()`` / ``load_state_dict()`` /
``.to()`` behave as in the reference and real checkpoints load by name).  Module construction order
inside PointTransformer follows the reference, so a seeded default init reproduces the reference's
seeded init tensor for tensor.  Forward passes pack the current parameters into bf16 GEMM
operands once (re-packed automatically when a parameter is modified) and call the kernels.
There is no CPU execution path: inputs must be CUDA tensors.
"""
import os
import warnings

import torch
from torch import nn

from .. import ops, runtime


# ------------------------------------------------------------------------------------------------
# parameter containers (timm-compatible names for the ViT, reference names for Point-MAE)
# ------------------------------------------------------------------------------------------------
class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale)


class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class LayerScaleBlock(nn.Module):
    """timm's ``Block`` with LayerScale (``init_values`` set, as in ``vit_base_patch14_dinov2``): x + ls1.gamma * attn(norm1(x)),
    then x + ls2.gamma * mlp(norm2(x)).  Registered in timm's order."""

    def __init__(self, dim, num_heads, mlp_ratio=4., init_values=1e-5):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=True)
        self.ls1 = LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio))
        self.ls2 = LayerScale(dim, init_values)


class _PatchEmbed(nn.Module):
    def __init__(self, dim, patch):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)


class VisionTransformer(nn.Module):
    """Parameter layout of timm's ``vit_base_patch8_224(_dino)`` (timm==0.9.12 [external]); with ``init_values`` (LayerScale in
    every block) that of ``vit_base_patch14_dinov2.lvd142m``: img_size 518, patch 14, a 37 x 37 grid."""

    def __init__(self, img_size=224, patch=8, dim=768, depth=12, num_heads=12, init_values=None):
        super().__init__()
        self.num_heads, self.depth = num_heads, depth
        n = (img_size // patch) ** 2
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n + 1, dim))
        self.patch_embed = _PatchEmbed(dim, patch)
        if init_values is None:
            self.blocks = nn.Sequential(*[Block(dim, num_heads, 4.0, qkv_bias=True) for _ in range(depth)])
        else:
            self.blocks = nn.Sequential(*[LayerScaleBlock(dim, num_heads, 4.0, init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)


def _param_version(module):
    """Cheap fingerprint of a module's weights (storage address + in-place version of every parameter / buffer): the packed
    device copies are rebuilt when it changes (load_state_dict, .to(), optimiser steps).  Walking module.parameters() costs
    ~1.5 ms for a ViT (name de-duplication hashes every tensor) and this runs on every forward, so the flat tensor list is
    cached on the module and only re-collected every 64 calls (a parameter OBJECT replaced in between is picked up then)."""
    cache = module.__dict__.get("_cmdiad_flat")
    if cache is None or cache[1] <= 0:
        cache = [list(module.parameters()) + list(module.buffers()), 64]
        module.__dict__["_cmdiad_flat"] = cache
    cache[1] -= 1
    return tuple((p.data_ptr(), p._version) for p in cache[0])


def allow_random_init():
    """CMDIAD_ALLOW_RANDOM_INIT=1: explicit opt-in to backbones without pretrained weights (tests, benchmarks on synthetic
    weights).  Without it a missing checkpoint is an error, as in the reference (timm pretrained=True models/models.py:23;
    torch.load of checkpoints/pointmae_pretrain.pth :30,285) -- silently random features would still produce
    plausible-looking, meaningless AUROC numbers."""
    return os.environ.get("CMDIAD_ALLOW_RANDOM_INIT", "0") == "1"


def unwrap_checkpoint(ckpt, prefixes=("module.", "backbone.")):
    """The forms timm's `checkpoint_path` accepts: a bare state_dict or one wrapped under 'state_dict' / 'model' / 'teacher'
    (DINO releases), with DataParallel / wrapper prefixes on the keys."""
    for key in ("state_dict", "model", "teacher", "state_dict_ema", "model_ema"):
        if isinstance(ckpt, dict) and key in ckpt and isinstance(ckpt[key], dict):
            ckpt = ckpt[key]
            break
    out = {}
    for k, v in ckpt.items():
        for p in prefixes:
            while k.startswith(p):
                k = k[len(p):]
        out[k] = v
    return out


def load_backbone_weights(module, state_dict, what, ignore_unexpected=("head.", "fc_norm.", "pre_logits.")):
    """load_state_dict that FAILS when a backbone parameter is missing (strict=False hid empty loads) and reports keys the
    checkpoint has but the backbone does not (classifier heads are expected extras)."""
    res = module.load_state_dict(state_dict, strict=False)
    if res.missing_keys:
        raise RuntimeError(f"{what}: checkpoint lacks {len(res.missing_keys)} backbone tensors, e.g. {res.missing_keys[:4]} "
                           f"(keys in the file look like {list(state_dict)[:3]})")
    extra = [k for k in res.unexpected_keys if not k.startswith(tuple(ignore_unexpected))]
    if extra:
        warnings.warn(f"{what}: {len(extra)} checkpoint tensors have no counterpart in the backbone, e.g. {extra[:4]}")
    return res


VIT_B8_NAMES = ('vit_base_patch8_224_dino', 'vit_base_patch8_224', 'vit_base_patch8_224_in21k')
DINOV2_NAME = 'vit_base_patch14_dinov2.lvd142m'
DINOV2_SIZE = 518     # timm's PatchEmbed asserts this input size: the reference runs DINOv2 with --rgb_size 518 only


def rgb_backbone(name):
    """An RGB backbone name the package implements -> an unloaded VisionTransformer of its layout."""
    if name in VIT_B8_NAMES:
        return VisionTransformer()
    if name == DINOV2_NAME:   # models/models.py:35-38: img_size 518, patch 14, LayerScale init_values 1e-5
        return VisionTransformer(img_size=DINOV2_SIZE, patch=14, init_values=1e-5)
    raise NotImplementedError(f"cmdiad_amd implements the ViT-B/8 backbones and {DINOV2_NAME} only (got {name})")


POINTMAE_CHECKPOINT = "checkpoints/pointmae_pretrain.pth"
POINTBERT_CHECKPOINT = "checkpoints/Point-BERT.pth"


class Model(torch.nn.Module):
    def __init__(self, device, rgb_backbone_name='vit_base_patch8_224_dino', out_indices=None, checkpoint_path='',
                 pool_last=False, xyz_backbone_name='Point_MAE', group_size=128, num_group=1024,
                 xyz_checkpoint_path=POINTMAE_CHECKPOINT):
        super().__init__()
        self.device = device
        self.rgb_backbone_name = rgb_backbone_name
        self.rgb_backbone = rgb_backbone(rgb_backbone_name)
        # timm downloads `pretrained=True` weights from the hub (models/models.py:23); offline the same state_dict comes from
        # a file: the `checkpoint_path` argument (timm's own name for it) or CMDIAD_VIT_CHECKPOINT
        checkpoint_path = checkpoint_path or os.environ.get("CMDIAD_VIT_CHECKPOINT", "")
        if checkpoint_path:
            # (Meta's own dinov2_vitb14 file also carries the masked-modelling token, which the extractor does not use)
            extras = ("head.", "fc_norm.", "pre_logits.") + (("mask_token",) if rgb_backbone_name == DINOV2_NAME else ())
            load_backbone_weights(self.rgb_backbone, unwrap_checkpoint(torch.load(checkpoint_path, map_location='cpu')),
                                  f"ViT checkpoint {checkpoint_path}", ignore_unexpected=extras)
        elif allow_random_init():
            warnings.warn("CMDIAD_ALLOW_RANDOM_INIT=1: rgb_backbone keeps its seeded random init "
                          "(load a timm state_dict with rgb_backbone.load_state_dict)")
        else:
            raise RuntimeError(f"no {'DINOv2 ViT-B/14' if rgb_backbone_name == DINOV2_NAME else 'ViT-B/8'} weights: pass checkpoint_path= / set CMDIAD_VIT_CHECKPOINT to a timm "
                               f"{rgb_backbone_name} state_dict, or opt in to random weights with CMDIAD_ALLOW_RANDOM_INIT=1")
        if xyz_backbone_name == 'Point_MAE':
            self.xyz_backbone = PointTransformer(group_size=group_size, num_group=num_group)
            self.xyz_backbone.load_model_from_ckpt(os.environ.get("CMDIAD_POINTMAE_CHECKPOINT", xyz_checkpoint_path))
        elif xyz_backbone_name == 'Point_Bert':  # models/models.py:31-33
            # (xyz_checkpoint_path defaults to the Point-MAE file; an explicitly different path is taken for Point-BERT too)
            path = xyz_checkpoint_path if xyz_checkpoint_path != POINTMAE_CHECKPOINT else POINTBERT_CHECKPOINT
            self.xyz_backbone = PointTransformer(group_size=group_size, num_group=num_group, encoder_dims=256)
            self.xyz_backbone.load_model_from_pb_ckpt(os.environ.get("CMDIAD_POINTBERT_CHECKPOINT", path))
        else:
            raise NotImplementedError(f"cmdiad_amd implements the Point_MAE and Point_Bert xyz backbones only (got {xyz_backbone_name})")
        self._vit_packed = None

    def _vit(self):
        ver = _param_version(self.rgb_backbone)
        if self._vit_packed is None or self._vit_packed[0] != ver:
            dev = next(self.rgb_backbone.parameters()).device
            self._vit_packed = (ver, runtime.PackedViT(self.rgb_backbone.state_dict(), device=dev))
        return self._vit_packed[1]

    def forward_rgb_tokens(self, x):
        """[B,3,S,S] -> final-LN tokens [B,1+(S/p)^2,768] (device-resident fast path): [B,785,768] for ViT-B/8 at 224, [B,1370,768]
        for DINOv2 at 518."""
        return self._vit().forward_tokens(x.float().contiguous())

    def forward_rgb_features(self, x):
        """models/models.py:35-53 -> [B,768,s,s]: s = 28 (ViT-B/8), 37 (DINOv2, `forward_features` in eval mode)."""
        tok = self.forward_rgb_tokens(x)
        B, T, C = tok.shape
        s = int((T - 1) ** 0.5)
        return tok[:, 1:].permute(0, 2, 1).reshape(B, C, s, s)

    def forward(self, rgb=None, xyz=None, out_type='rgb+xyz'):
        if out_type == 'rgb+xyz':
            rgb_features = self.forward_rgb_features(rgb)
            xyz_features, center, ori_idx, center_idx = self.xyz_backbone(xyz)
            return rgb_features, xyz_features, center, ori_idx, center_idx
        elif out_type == 'rgb':
            return self.forward_rgb_features(rgb)
        elif out_type == 'xyz':
            return self.xyz_backbone(xyz)


def fps(data, number):
    """data [B,N,3] -> (centres [B,number,3], idx [B,number] int32).  models/models.py:70-78."""
    idx, centers = ops.fps(data.float().contiguous(), number)
    return centers, idx


class Group(torch.nn.Module):
    def __init__(self, num_group, group_size):
        super().__init__()
        self.num_group = num_group
        self.group_size = group_size

    def forward(self, xyz, n_valid=None):
        """xyz [B,N,3] -> (neighborhood [B,G,M,3], center [B,G,3], ori_idx [B,G,M] int64, center_idx [B,G])."""
        xyz = xyz.float().contiguous()
        center_idx, center = ops.fps(xyz, self.num_group, n_valid)
        ori_idx, neighborhood = ops.knn_group(xyz, center, self.group_size, n_valid)
        return neighborhood, center, ori_idx, center_idx


class Encoder(torch.nn.Module):
    def __init__(self, encoder_channel):
        super().__init__()
        self.encoder_channel = encoder_channel
        self.first_conv = torch.nn.Sequential(nn.Conv1d(3, 128, 1), nn.BatchNorm1d(128), nn.ReLU(inplace=True),
                                              nn.Conv1d(128, 256, 1))
        self.second_conv = nn.Sequential(nn.Conv1d(512, 512, 1), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
                                         nn.Conv1d(512, self.encoder_channel, 1))


class TransformerEncoder(nn.Module):
    def __init__(self, embed_dim=768, depth=4, num_heads=12, mlp_ratio=4., qkv_bias=False, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.):
        super().__init__()
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale)
            for _ in range(depth)])


class PointTransformer(torch.nn.Module):
    def __init__(self, group_size=128, num_group=1024, encoder_dims=384):
        super().__init__()
        if encoder_dims not in (384, 256):
            raise NotImplementedError(f"cmdiad_amd implements Point_MAE (encoder_dims=384) and Point_Bert (256), not {encoder_dims}")
        self.trans_dim, self.depth, self.drop_path_rate, self.num_heads = 384, 12, 0.1, 6
        self.group_size, self.num_group = group_size, num_group
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.encoder_dims = encoder_dims
        if self.encoder_dims != self.trans_dim:  # Point-BERT (models/models.py:259-264): registered before the encoder, as there
            self.cls_token = torch.nn.Parameter(torch.zeros(1, 1, self.trans_dim))
            self.cls_pos = torch.nn.Parameter(torch.randn(1, 1, self.trans_dim))
            self.reduce_dim = torch.nn.Linear(self.encoder_dims, self.trans_dim)
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, self.trans_dim))
        self.blocks = TransformerEncoder(embed_dim=self.trans_dim, depth=self.depth, num_heads=self.num_heads)
        self.norm = nn.LayerNorm(self.trans_dim)
        self._packed = None

    def load_model_from_ckpt(self, bert_ckpt_path):
        if bert_ckpt_path is None:
            return
        if not os.path.exists(bert_ckpt_path):
            if not allow_random_init():  # the reference fails here too (torch.load, models/models.py:285)
                raise FileNotFoundError(f"{bert_ckpt_path} not found: place the Point-MAE pretrain checkpoint there, set "
                                        "CMDIAD_POINTMAE_CHECKPOINT, or opt in to random weights with CMDIAD_ALLOW_RANDOM_INIT=1")
            warnings.warn(f"{bert_ckpt_path} not found and CMDIAD_ALLOW_RANDOM_INIT=1: Point-MAE keeps its seeded random init")
            return
        ckpt = torch.load(bert_ckpt_path, map_location='cpu')
        base = {k.replace("module.", ""): v for k, v in ckpt['base_model'].items()}
        for k in list(base.keys()):  # models/models.py:289-295 key rewrite
            if k.startswith('MAE_encoder'):
                base[k[len('MAE_encoder.'):]] = base.pop(k)
            elif k.startswith('base_model'):
                base[k[len('base_model.'):]] = base.pop(k)
        # the pretrain checkpoint also carries the MAE decoder / mask token, which the extractor does not have
        load_backbone_weights(self, base, f"Point-MAE checkpoint {bert_ckpt_path}",
                              ignore_unexpected=("MAE_decoder", "mask_token", "decoder_pos_embed", "increase_dim", "cls_"))

    def load_model_from_pb_ckpt(self, bert_ckpt_path):
        """Point-BERT checkpoint (models/models.py:297-322): the `transformer_q.` tensors except its classification heads, prefix
        stripped (and any `base_model.` ones); the momentum encoder, the dVAE and the rest are dropped.  Unlike the reference's
        strict=False load, a backbone tensor the file lacks is an error."""
        if not os.path.exists(bert_ckpt_path):
            if not allow_random_init():  # the reference fails here too (torch.load, models/models.py:298)
                raise FileNotFoundError(f"{bert_ckpt_path} not found: place the Point-BERT checkpoint there, set "
                                        "CMDIAD_POINTBERT_CHECKPOINT, or opt in to random weights with CMDIAD_ALLOW_RANDOM_INIT=1")
            warnings.warn(f"{bert_ckpt_path} not found and CMDIAD_ALLOW_RANDOM_INIT=1: Point-BERT keeps its seeded random init")
            return
        ckpt = torch.load(bert_ckpt_path, map_location='cpu')
        base = {k.replace("module.", ""): v for k, v in ckpt['base_model'].items()}
        for k in list(base.keys()):  # models/models.py:301-308 key rewrite, step for step
            if k.startswith('transformer_q') and not k.startswith('transformer_q.cls_head'):
                base[k[len('transformer_q.'):]] = base[k]
            elif k.startswith('base_model'):
                base[k[len('base_model.'):]] = base[k]
            del base[k]
        # Point-BERT's masked transformer also carries its mask token and the dVAE-token head, which the extractor does not have
        load_backbone_weights(self, base, f"Point-BERT checkpoint {bert_ckpt_path}", ignore_unexpected=("mask_token", "lm_head"))

    def packed(self):
        # BatchNorm mode: module.training selects nothing by itself (the contract of record is eval mode whatever the flag,
        # SURVEY F1 / DESIGN.md); CMDIAD_BN_BATCH_STATS=1 opts in to the reference's as-shipped batch-statistics behaviour
        ver = (_param_version(self), os.environ.get("CMDIAD_BN_BATCH_STATS", "0"))
        if self._packed is None or self._packed[0] != ver:
            dev = next(self.parameters()).device
            cls = runtime.PackedPointMAE if self.encoder_dims == self.trans_dim else runtime.PackedPointBERT
            self._packed = (ver, cls(self.state_dict(), device=dev, group_size=self.group_size, num_group=self.num_group))
        return self._packed[1]

    def forward_device(self, xyz_nc, n_valid=None):
        """xyz_nc [B,N,3] contiguous -> (feats [B,G,768] centre-major, center, ori_idx, center_idx)."""
        return self.packed().forward(xyz_nc, n_valid)

    def forward(self, pts):
        """pts [B,3,N] -> (x [B,768,G], center [B,G,3], ori_idx [B,G,M], center_idx [B,G]); models.py:352-373.
        Eval-mode contract (BatchNorm running statistics, DropPath inactive): SURVEY F1 / DESIGN.md."""
        feats, center, ori_idx, center_idx = self.forward_device(pts.float().transpose(-1, -2).contiguous())
        return feats.transpose(1, 2), center, ori_idx, center_idx
