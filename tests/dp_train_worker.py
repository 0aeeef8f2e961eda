"""Worker of tests/test_gpu_dp_train.py: ONE of two real ranks (processes) of a data-parallel distillation run, both on cuda:0, the
collectives over gloo (CMDIAD_DP_ONE_DEVICE=1: RCCL refuses two ranks on one device).  Each rank trains
HallucinationCrossModalityNetwork on ITS half of a global batch through dp_train.ParamArena + ArenaAdam; rank 0 also computes the
same three steps with code that does not know about ranks -- train.forward_backward on each half, the two gradients added,
ops.adam_step per parameter with grad_scale 0.5 -- and the parameters must agree BIT FOR BIT after every step: a two-term fp32 sum
is commutative, x 0.5 is exact, the kernels reduce in a fixed order and cmdiad_adam_flat is cmdiad_adam_step element for element.
Launched as: python -m torch.distributed.run --nproc-per-node 2 tests/dp_train_worker.py"""
import json
import os
import sys

import torch
import torch.distributed as td

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("CMDIAD_ALLOW_RANDOM_INIT", "1")

from cmdiad_amd import dp_train, ops, train  # noqa: E402
from cmdiad_amd.models.hallucination_network import HallucinationCrossModalityNetwork  # noqa: E402

STEPS, LR, B_LOCAL = 3, 5e-4, 2


def make_net(seed, dev):
    torch.manual_seed(seed)
    return HallucinationCrossModalityNetwork(None, 768, 768).to(dev)


def baseline(init_state, halves, dist_method, dev):
    """Three steps on the averaged gradient of the two half-batches with today's single-process pieces only.
    -> (state_dict clones after every step, [step][half] = (loss_xyz, loss_rgb))."""
    net = make_net(0, dev)
    net.load_state_dict(init_state)
    dirs = {src: [p.detach() for p in train.direction_params(net, src)] for src in ("rgb", "xyz")}
    m = {src: [torch.zeros_like(p) for p in ps] for src, ps in dirs.items()}
    v = {src: [torch.zeros_like(p) for p in ps] for src, ps in dirs.items()}
    states, losses = [], []
    for step in range(1, STEPS + 1):
        grads, step_losses = {}, []
        for xyz, rgb in halves:
            pair = {}
            for src, x, t in (("rgb", rgb, xyz), ("xyz", xyz, rgb)):
                loss, g = train.forward_backward(x.reshape(-1, 768).contiguous(), t.reshape(-1, 768).contiguous(), tuple(dirs[src]),
                                                 dist_method, B_LOCAL)
                pair[src] = float(loss)
                grads.setdefault(src, []).append(g)
            step_losses.append((pair["rgb"], pair["xyz"]))           # (loss_xyz: rgb -> xyz, loss_rgb: xyz -> rgb), as forward() returns
        for src in ("rgb", "xyz"):
            for p, ga, gb, mm, vv in zip(dirs[src], grads[src][0], grads[src][1], m[src], v[src]):
                ops.adam_step(p, (ga + gb).contiguous(), mm, vv, LR, 0.9, 0.999, 1e-8, step, grad_scale=0.5)
        states.append({k: t.detach().clone() for k, t in net.state_dict().items()})
        losses.append(step_losses)
    return states, losses


def main():
    rank, world, dev, group = dp_train.init_from_env(timeout_s=120)
    assert world == 2 and group is not None and td.get_backend(group) == "gloo" and dev == torch.device("cuda", 0)
    g = torch.Generator().manual_seed(2024)
    batch = torch.randn(2 * B_LOCAL, 64, 1536, generator=g).to(dev)                     # the global batch, the same on both ranks
    halves = [(batch[r * B_LOCAL:(r + 1) * B_LOCAL, :, :768].contiguous(), batch[r * B_LOCAL:(r + 1) * B_LOCAL, :, 768:].contiguous())
              for r in range(world)]
    init_state = {k: t.detach().clone() for k, t in make_net(7, dev).state_dict().items()}   # what rank 0 starts from
    report = {}
    for dist_method in ("l2", "cos_dist"):
        if rank == 0:
            want, want_losses = baseline(init_state, halves, dist_method, dev)
            again, _ = baseline(init_state, halves, dist_method, dev)
            premise = all(torch.equal(a[k], b[k]) for a, b in zip(want, again) for k in a)
            assert premise, (f"{dist_method}: PREMISE: the single-process baseline (forward_backward + adam_step) is not bit-reproducible "
                             "from run to run, so no data-parallel run can be held to it bit for bit")
        net = make_net(7 + rank, dev)                       # rank 1 starts elsewhere: ArenaAdam's broadcast brings it to rank 0's
        arena = dp_train.ParamArena(net)
        opt = dp_train.ArenaAdam(arena, lr=LR, group=group)
        assert len(opt.buckets) == 2 and opt.in_sync()
        assert all(torch.equal(t, init_state[k]) for k, t in net.state_dict().items()), "the broadcast did not deliver rank 0's parameters"
        xyz, rgb = halves[rank]
        equal, synced, losses = [], [], []
        for step in range(STEPS):
            loss_xyz, loss_rgb = net(xyz, rgb, False, dist_method)
            (loss_xyz + loss_rgb).backward()
            opt.step()
            opt.zero_grad()
            synced.append(opt.in_sync())
            mine = torch.tensor([float(loss_xyz), float(loss_rgb)], dtype=torch.float64)
            both = [torch.zeros(2, dtype=torch.float64) for _ in range(world)]
            td.all_gather(both, mine, group=group)
            losses.append([tuple(t.tolist()) for t in both])
            if rank == 0:
                bad = [k for k, t in net.state_dict().items() if not torch.equal(t, want[step][k])]
                equal.append(bad)
        assert opt.reductions == 2 * STEPS
        ok = torch.tensor([int(all(synced))])
        td.all_reduce(ok, op=td.ReduceOp.MIN, group=group)
        report[dist_method] = {"in_sync_both_ranks": bool(ok.item())}
        if rank == 0:
            report[dist_method].update(premise=premise, differing_params_per_step=equal,
                                       losses_equal=[[tuple(a) == tuple(b) for a, b in zip(losses[s], want_losses[s])] for s in range(STEPS)],
                                       losses=losses, baseline_losses=want_losses)
    td.barrier()
    td.destroy_process_group()
    if rank == 0:
        print(json.dumps({"dp_train": True, "ranks": world, "report": report}), flush=True)


if __name__ == "__main__":
    main()
