#!/usr/bin/env python3
"""Generate the Point-BERT golden vectors (gpb_pointbert.npz) by IMPORTING THE REFERENCE, as make_golden.py does (same stubs;
FPS and kNN come from this repo's C oracle).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointbert.py

Weights are not stored: tests/pointbert_synth.py rebuilds them from the seed.  The fixture holds the reference's
PointTransformer(group_size=32, num_group=64, encoder_dims=256) on a small cloud in eval and in train (batch-statistics
BatchNorm) mode -- centre / group indices, encoder tokens, reduce_dim output, features --, the names and shapes of its
state_dict, and the checksums of its seeded default initialisation (as G8 has them for Point-MAE).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (stubs, reference location, repo on sys.path)
from cmdiad_amd.synth import synth_cloud  # noqa: E402
from pointbert_synth import synth_pointbert_state_dict  # noqa: E402

SEED = 21


def main():
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    from models import models as rmodels
    from feature_extractors import multiple_features as rmf

    sd = synth_pointbert_state_dict(SEED)
    pt = rmodels.PointTransformer(group_size=32, num_group=64, encoder_dims=256)
    pc, _ = rmf.organized_pc_to_unorganized_pc_no_zeros((None, synth_cloud(9, 0.08)))
    pc = pc[:, :, :3000].contiguous()
    out = {}
    for mode in ("eval", "train"):
        pt.load_state_dict(sd, strict=True)   # (train mode updates the running statistics: start each mode from the same weights)
        pt.eval() if mode == "eval" else pt.train()
        with torch.no_grad():
            feats, center, ori_idx, center_idx = pt(pc)
            nb, _, _, _ = pt.group_divider(pc.transpose(-1, -2))
            tok = pt.encoder(nb)
            red = pt.reduce_dim(tok)
        out[f"feats_{mode}"] = feats.numpy()
        out[f"tokens_{mode}"] = tok.numpy()
        out[f"reduce_{mode}"] = red.numpy()
    names = list(pt.state_dict().keys())
    shapes = [",".join(str(d) for d in v.shape) for v in pt.state_dict().values()]
    torch.manual_seed(123)
    pt2 = rmodels.PointTransformer(group_size=128, num_group=1024, encoder_dims=256)
    init = np.array([[v.double().sum().item(), v.double().abs().sum().item()] for v in pt2.state_dict().values()])
    path = os.path.join(HERE, "gpb_pointbert.npz")
    np.savez_compressed(path, seed=SEED, pc=pc.numpy(), center=center.numpy(), center_idx=center_idx.numpy(),
                        ori_idx=ori_idx.numpy().astype(np.int32), names=np.array(names), shapes=np.array(shapes),
                        init_names=np.array(list(pt2.state_dict().keys())), init_checksums=init, **out)
    print(len(names), "tensors;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
