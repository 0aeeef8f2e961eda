#!/usr/bin/env python3
"""Generate the DINOv2 grid golden vectors (gdv_dinov2.npz) by IMPORTING THE REFERENCE, as make_golden.py does (same stubs).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dinov2.py

vit_base_patch14_dinov2.lvd142m gives a 37 x 37 token grid (models/models.py:36-39); what the reference does downstream of it:
  * Features.get_rgb_patch on a seeded [1, 12, 37, 37] map (features.py:160-167): rgb_patch [1369, 12] and rgb_patch2 [3136, 12]
    (AdaptiveAvgPool2d((56, 56)) from 37 x 37: windows of 1, 2 or 4 cells);
  * Features.calculate_dist + compute_single_s_s_map(..., (37, 37), modal='rgb') against a seeded 1 500 x 128 library
    (features.py:186-297; blur replaced by the identity, as G4 does): s, the nearest-neighbour values / indices, the 224 x 224
    map (every fourth row and column).
Inputs are rebuilt from their seeds by the tests; only the reference's outputs are stored.
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

MAP_SEED, MAP_C = 61, 12
LIB_SEED, Q, NB, D = 62, 37 * 37, 1500, 128     # (D % 128 == 0: the re-weighting scan kernel's operand width)


def inputs():
    """The seeded inputs (shared with tests/test_dinov2_cpu.py and tests/test_gpu_dinov2.py)."""
    g = torch.Generator().manual_seed(MAP_SEED)
    fmap = torch.randn(1, MAP_C, 37, 37, generator=g)
    g = torch.Generator().manual_seed(LIB_SEED)
    bank = torch.randn(NB, D, generator=g)
    patch = bank[torch.randint(0, NB, (Q,), generator=g)] + 0.3 * torch.randn(Q, D, generator=g)
    patch[Q // 3] += 1.5  # a planted anomalous patch
    return fmap, bank, patch


def main():
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    from feature_extractors import features as rfeat

    fmap, bank, patch = inputs()
    fake = mg._ns(resize56=torch.nn.AdaptiveAvgPool2d((56, 56)))
    rp, rp2 = rfeat.Features.get_rgb_patch(fake, [fmap])

    class NoBlur:
        def __call__(self, x):
            return x[0]

    fs = mg._ns(args=mg._ns(dist_method_s="l2"), n_reweight=3, gt_size=224, blur=NoBlur(), patch_rgb_lib=bank)
    fs.calculate_dist = lambda a, b: rfeat.Features.calculate_dist(fs, a, b)
    dist = fs.calculate_dist(patch, bank)
    s, s_map = rfeat.Features.compute_single_s_s_map(fs, patch, dist, (37, 37), modal='rgb')
    mv, mi = torch.min(dist, dim=1)
    path = os.path.join(HERE, "gdv_dinov2.npz")
    np.savez_compressed(path, map_seed=MAP_SEED, lib_seed=LIB_SEED, rgb_patch=rp.numpy(), rgb_patch2=rp2.numpy(),
                        s=s.numpy(), min_val=mv.numpy(), min_idx=mi.numpy().astype(np.int32), s_map=s_map.numpy()[:, ::4, ::4])
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
