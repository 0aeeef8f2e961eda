"""xyz extraction (sample + forward: FPS, kNN grouping, encoder, transformer, fetch LayerNorms) at batch 32, 24 576 points per
cloud, Point-MAE against Point-BERT, alternating on one box (same clouds, synthetic weights of both backbones).

    python tools/pointbert_time.py [--rounds 5] [--batch 32]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from cmdiad_amd import ops, runtime  # noqa: E402
from cmdiad_amd.synth import synth_cloud_fixed_n  # noqa: E402
from oracle import nets  # noqa: E402
from pointbert_synth import synth_pointbert_state_dict  # noqa: E402
from tools.microbench import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    pcs = torch.cat([synth_cloud_fixed_n(1000 + i, 24576) for i in range(a.batch)]).cuda()
    xyz, _, _, nv = ops.unorganize(pcs, 24576)
    nets_ = {"Point-MAE": runtime.PackedPointMAE(nets.synth_state_dict("pointmae", 21), device="cuda"),
             "Point-BERT": runtime.PackedPointBERT(synth_pointbert_state_dict(21), device="cuda")}

    def run(pm):
        return pm.forward(xyz, nv, sampled=pm.sample(xyz, nv))

    ms = {k: [] for k in nets_}
    with torch.no_grad():
        for r in range(a.rounds):
            for name, pm in (nets_.items() if r % 2 == 0 else reversed(list(nets_.items()))):
                t = timeit(lambda: run(pm), iters=5, warm=2)
                ms[name].append(t)
                print(f"round {r} {name}: {t:.2f} ms per batch of {a.batch}", flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(f"median: Point-MAE {med['Point-MAE']:.2f} ms, Point-BERT {med['Point-BERT']:.2f} ms, "
          f"ratio {med['Point-BERT'] / med['Point-MAE']:.3f}", flush=True)


if __name__ == "__main__":
    main()
