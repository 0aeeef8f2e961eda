#!/usr/bin/env python3
"""ArenaAdam (cmdiad_amd/dp_train.py: one flat-arena Adam launch) against train.FusedAdam (one launch per parameter) on ONE GPU,
world = 1, at BASELINE configs[2]'s shapes: FtoF distillation, batch 32 x 3 136 tokens x (768 + 768), fp32 features, l2 loss.

The two optimizers ALTERNATE within one process, `--reps` repetitions each (a fresh seeded network per repetition); a repetition
is `--warmup` steps, then `--steps` timed ones.  Device events bracket every whole step and every optimizer phase (step() + zero_grad()); the
launches an optimizer makes per step() are counted on the host (calls into the native library).  Rule: ArenaAdam's mean must not
exceed FusedAdam's mean plus FusedAdam's own max - min spread over its repetitions -- for the optimizer phase and for the whole step.
Prints one JSON line; --out FILE also writes the report that profiles/dp_train.md keeps.

    python tools/dp_train_bench.py [--steps 20] [--warmup 5] [--reps 3] [--out profiles/dp_train.md]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("CMDIAD_ALLOW_RANDOM_INIT", "1")
from cmdiad_amd import dp_train, ops, train  # noqa: E402
from cmdiad_amd.models.hallucination_network import HallucinationCrossModalityNetwork  # noqa: E402

B, T = 32, 3136


def one_repetition(kind, x, warmup, steps):
    """-> (ms per whole step, ms per optimizer phase, native launches per step())."""
    torch.manual_seed(3407)
    net = HallucinationCrossModalityNetwork(None, 768, 768).to(x.device)
    opt = train.FusedAdam(net.parameters(), lr=5e-4) if kind == "FusedAdam" else dp_train.ArenaAdam(dp_train.ParamArena(net), lr=5e-4)
    launches = []
    orig = ops._call

    def counting(name, *args):
        launches.append(name)
        return orig(name, *args)

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    per_step = None
    for i in range(warmup + steps):
        e = ev[i - warmup] if i >= warmup else None
        if e:
            e[0].record()
        lx, lr_ = net(x[:, :, :768], x[:, :, 768:], False, "l2")
        (lx + lr_).backward()
        if e:
            e[1].record()
        if i == warmup - 1:
            ops._call = counting
        opt.step()
        if i == warmup - 1:
            ops._call = orig
            per_step = len(launches)
        opt.zero_grad()
        if e:
            e[2].record()
    torch.cuda.synchronize()
    whole = sum(e[0].elapsed_time(e[2]) for e in ev) / steps
    phase = sum(e[1].elapsed_time(e[2]) for e in ev) / steps
    return whole, phase, per_step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.steps >= 20 and a.warmup >= 1 and a.reps >= 2
    dev = torch.device("cuda", 0)
    x = torch.randn(B, T, 1536, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    res = {"FusedAdam": [], "ArenaAdam": []}
    for _ in range(a.reps):
        for kind in ("FusedAdam", "ArenaAdam"):
            res[kind].append(one_repetition(kind, x, a.warmup, a.steps))
    out = {"config": f"configs[2] shapes: batch {B} x {T} tokens x (768 + 768), fp32 features, l2, world 1; {a.warmup} warm-up + {a.steps} "
                     f"timed steps per repetition, {a.reps} alternating repetitions each", "device": torch.cuda.get_device_name(0)}
    for col, what in ((0, "whole_step_ms"), (1, "optimizer_phase_ms")):
        f, r = [t[col] for t in res["FusedAdam"]], [t[col] for t in res["ArenaAdam"]]
        f_mean, r_mean, spread = sum(f) / len(f), sum(r) / len(r), max(f) - min(f)
        out[what] = {"FusedAdam": [round(v, 4) for v in f], "ArenaAdam": [round(v, 4) for v in r], "FusedAdam_mean": round(f_mean, 4),
                     "ArenaAdam_mean": round(r_mean, 4), "FusedAdam_spread": round(spread, 4), "bound": round(f_mean + spread, 4),
                     "ArenaAdam_not_slower": bool(r_mean <= f_mean + spread)}
    out["launches_per_optimizer_step"] = {k: v[0][2] for k, v in res.items()}
    out["multi_gpu_step_time"] = out["multi_gpu_scaling"] = "not measured"
    out["gradient_all_reduce_share_of_step"] = "2-3 % (2 x 26.6 MB over xGMI): an ESTIMATE, not a measurement"
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(report(out))
    return 0 if out["whole_step_ms"]["ArenaAdam_not_slower"] and out["optimizer_phase_ms"]["ArenaAdam_not_slower"] else 1


def report(o):
    lines = ["# ArenaAdam against FusedAdam on one GPU (tools/dp_train_bench.py)", "", o["config"] + f".  Device: {o['device']}.", "",
             "Device-event times in ms; the two optimizers alternate within one process.  Rule: ArenaAdam's mean <= FusedAdam's mean + "
             "FusedAdam's own max - min spread over its repetitions.", "",
             "| | FusedAdam repetitions | mean | spread | bound | ArenaAdam repetitions | mean | not slower |", "|---|---|---|---|---|---|---|---|"]
    for key, name in (("optimizer_phase_ms", "optimizer phase (step() + zero_grad())"), ("whole_step_ms", "whole step")):
        r = o[key]
        lines.append(f"| {name} | {r['FusedAdam']} | {r['FusedAdam_mean']} | {r['FusedAdam_spread']} | {r['bound']} | {r['ArenaAdam']} | "
                     f"{r['ArenaAdam_mean']} | {'yes' if r['ArenaAdam_not_slower'] else 'NO'} |")
    lines += ["", "What differs between the two whole steps, by construction (an accounting of memory traffic, not a measured breakdown): with "
              "FusedAdam and `zero_grad(set_to_none=True)` the gradients are the fresh tensors backward() hands out -- autograd takes them over "
              "without a kernel -- and Adam is 16 launches.  With the arena the gradients are views of `g`: `zero_grad()` is one 53 MB fill "
              "(inside the optimizer phase above), autograd ADDS every fresh gradient into its view during backward() (16 in-place additions, "
              "160 MB of traffic, outside the optimizer phase), and Adam is one launch.  The contiguous `g` is what the bucketed all-reduce "
              "needs; the price on one GPU is the difference in the whole-step row."]
    n = o["launches_per_optimizer_step"]
    lines += ["", f"Native launches per optimizer step(), counted on the host: FusedAdam {n['FusedAdam']}, ArenaAdam {n['ArenaAdam']}.", "",
              f"Multi-GPU step time: {o['multi_gpu_step_time']}.  Multi-GPU scaling: {o['multi_gpu_scaling']} (this project's environment has one "
              f"GPU).  Gradient all-reduce share of the step: {o['gradient_all_reduce_share_of_step']}.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    sys.exit(main())
