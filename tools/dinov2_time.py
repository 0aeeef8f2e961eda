"""DINOv2 ViT-B/14 (518, 37 x 37 grid) against ViT-B/8 (224, 28 x 28), alternating on one box, synthetic weights of both:

  1. the RGB backbone alone (PackedViT.forward_tokens) at batch 32: ms per batch and TFLOP/s of the work the kernels execute
     (patch GEMM at its padded K, the four block GEMMs, attention over the T real keys);
  2. the dino_pointmae BatchPredictor step at batch 32 (bench.py's pipelined loop: HIP graphs, both buffer sets, resident
     batches, 'bagel'-sized libraries -- the rgb library at 0.1 * 244 * 1 369 rows for DINOv2): images/s.

    python tools/dinov2_time.py [--rounds 5] [--batch 32] [--steps 20]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from bench_legs.common import BATCH, build_state, make_batches, run_steps  # noqa: E402
from cmdiad_amd import engine as eng  # noqa: E402
from cmdiad_amd import runtime  # noqa: E402
from cmdiad_amd.predictor import BatchPredictor  # noqa: E402
from cmdiad_amd.synth import synth_bank, synth_rgb  # noqa: E402
from dinov2_synth import synth_dinov2_state_dict  # noqa: E402
from oracle import nets  # noqa: E402
from tools.microbench import timeit  # noqa: E402

NETS = {"ViT-B/8": (224, 8, 192), "DINOv2": (518, 14, 640)}   # image size, patch, patch GEMM K as executed


def gflop(name, depth=12, C=768):
    S, p, K = NETS[name]
    P = (S // p) ** 2
    T = P + 1
    gemm = 2 * P * K * C + depth * 2 * T * C * (3 * C + C + 4 * C + 4 * C)
    att = depth * 4 * T * T * C
    return gemm / 1e9, att / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    dev = "cuda"
    vits = {"ViT-B/8": runtime.PackedViT(nets.synth_state_dict("vit", 31), device=dev),
            "DINOv2": runtime.PackedViT(synth_dinov2_state_dict(31), device=dev)}
    imgs = {k: torch.cat([synth_rgb(i, size=NETS[k][0]) for i in range(a.batch)]).to(dev) for k in vits}
    for k in vits:
        g, t = gflop(k)
        print(f"{k}: {g:.1f} GFLOP of GEMMs + {t:.1f} of attention per image", flush=True)
    ms = {k: [] for k in vits}
    with torch.no_grad():
        for r in range(a.rounds):
            for k in (list(vits) if r % 2 == 0 else list(reversed(list(vits)))):
                t = timeit(lambda: vits[k].forward_tokens(imgs[k]), iters=5, warm=2)
                ms[k].append(t)
                print(f"round {r} {k}: backbone {t:.2f} ms per batch of {a.batch}", flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    for k, t in med.items():
        print(f"median backbone {k}: {t:.2f} ms, {a.batch * sum(gflop(k)) / t:.0f} TFLOP/s executed", flush=True)
    print(f"ratio DINOv2 / ViT-B/8: {med['DINOv2'] / med['ViT-B/8']:.2f}", flush=True)

    # the batched predictor step, one predictor per backbone, alternating
    st = build_state(dev)
    preds, batches = {}, {}
    host = make_batches(0, "dino_pointmae")
    for k, vit in vits.items():
        S = NETS[k][0]
        rows = int(0.1 * 244 * (S // NETS[k][1]) ** 2)
        bank_rgb = st["bank_second"] if k == "ViT-B/8" else eng.Bank(synth_bank(rows, 768, 4322).to(dev))
        e = eng.Engine(vit, st["engine"].pm)
        preds[k] = BatchPredictor(e, st["bank_xyz"], bank_rgb, st["stats"], st["det"], st["seg"], batch=BATCH, n_max=24576,
                                  rgb_size=S)
        batches[k] = [(torch.cat([synth_rgb(j * BATCH + i, size=S) for i in range(BATCH)]).to(dev) if S != 224 else r.to(dev),
                       p.to(dev)) for j, (r, p) in enumerate(host)]
        run_steps(preds[k], batches[k], 4)
    ips = {k: [] for k in preds}
    for r in range(a.rounds):
        for k in (list(preds) if r % 2 == 0 else list(reversed(list(preds)))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(preds[k], batches[k], a.steps)
            torch.cuda.synchronize()
            v = a.steps * BATCH / (time.perf_counter() - t0)
            ips[k].append(v)
            print(f"round {r} {k}: predictor step {v:.0f} images/s", flush=True)
    medi = {k: sorted(v)[len(v) // 2] for k, v in ips.items()}
    print(f"median predictor: ViT-B/8 {medi['ViT-B/8']:.0f} images/s, DINOv2 {medi['DINOv2']:.0f} images/s "
          f"(ratio {medi['DINOv2'] / medi['ViT-B/8']:.3f})", flush=True)


if __name__ == "__main__":
    main()
