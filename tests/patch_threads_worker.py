"""Worker of tests/test_gpu_patch_path.py::test_threads_per_patch_variants_give_identical_bits: ONE fresh process per value of
CMDIAD_XYZ_PATCH_THREADS (the launcher reads it once per process), which runs the B = 9, D = 260 case of that file and writes the
fp32 and bf16 patch features.  Launched as: python tests/patch_threads_worker.py OUT.npz   (the variable is set by the parent)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import patch_ref as pr  # noqa: E402
from cmdiad_amd import ops  # noqa: E402

CASE = dict(B=9, size=64, P=16, S=100, D=260, seed=4, mean=-0.4, inv_std=2.5)


def run_case(dev="cuda"):
    c = CASE
    pcs, cen, feat = pr.synth_batch(c["B"], c["size"], c["S"], c["D"], c["seed"])
    xyz, _, pix2pt, nv = ops.unorganize(pcs.to(dev))
    idx3, w3 = ops.interp3nn(xyz, cen.to(dev), n_valid=nv)
    p32, p16 = ops.xyz_patch_fused(feat.to(dev), idx3, w3, pix2pt, c["size"], c["P"], c["mean"], c["inv_std"], want_bf16=True)
    torch.cuda.synchronize()
    return p32.cpu().numpy(), p16.view(torch.int16).cpu().numpy()


if __name__ == "__main__":
    p32, p16 = run_case()
    np.savez(sys.argv[1], p32=p32, p16=p16, threads=os.environ.get("CMDIAD_XYZ_PATCH_THREADS", ""))
