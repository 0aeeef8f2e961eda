"""GPU: data-parallel training of the distillation heads (cmdiad_amd/dp_train.py) -- the flat-arena Adam kernel against the
per-parameter one bit for bit, the optimizer's checkpoint round trip and its effect on the packed inference cache, and a run of
two real ranks on one GPU (tests/dp_train_worker.py) against a baseline built from single-process pieces only."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
B1, B2, EPS = 0.9, 0.999, 1e-8


def _flat_against_per_parameter(sizes, gscale, with_bf16, steps=3, lr=1e-3):
    from cmdiad_amd import ops
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 3) // 4 * 4
    gen = torch.Generator().manual_seed(sum(sizes) + int(1000 * gscale))
    p, m, v = (torch.zeros(total, device=DEV) for _ in range(3))
    pb = torch.zeros(total, dtype=torch.bfloat16, device=DEV) if with_bf16 else None
    for o, n in zip(offs, sizes):
        p[o:o + n] = torch.randn(n, generator=gen).to(DEV)
    ref = [[buf[o:o + n].clone() for buf in (p, m, v)] + [torch.zeros(n, dtype=torch.bfloat16, device=DEV) if with_bf16 else None]
           for o, n in zip(offs, sizes)]
    pad = torch.ones(total, dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        pad[o:o + n] = False
    for step in range(1, steps + 1):
        g = torch.zeros(total, device=DEV)
        for o, n in zip(offs, sizes):
            g[o:o + n] = (torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=gen))).to(DEV)
        ops.adam_flat(p, g, m, v, lr, B1, B2, EPS, step, gscale, pb)
        for (rp, rm, rv, rb), o, n in zip(ref, offs, sizes):
            ops.adam_step(rp, g[o:o + n].clone(), rm, rv, lr, B1, B2, EPS, step, gscale, rb)
            assert torch.equal(p[o:o + n], rp) and torch.equal(m[o:o + n], rm) and torch.equal(v[o:o + n], rv), (n, step, gscale)
            if with_bf16:
                assert torch.equal(pb[o:o + n].view(torch.int16), rb.view(torch.int16)), (n, step, gscale)
        for buf in (p, m, v) + ((pb,) if with_bf16 else ()):
            assert int((buf[pad].view(torch.int32 if buf.dtype == torch.float32 else torch.int16) != 0).sum()) == 0, "a padding lane moved"
    assert float(m.abs().sum()) > 0 and float(v.abs().sum()) > 0


@pytest.mark.parametrize("with_bf16", [False, True])
@pytest.mark.parametrize("gscale", [1.0, 0.5, 1.0 / 3.0])
def test_flat_adam_equals_per_parameter_adam_bit_for_bit(gscale, with_bf16):
    _flat_against_per_parameter([1, 3, 5, 768, 1475, 1920 * 3], gscale, with_bf16)


def test_flat_adam_grid_stride_loop_bit_for_bit():
    """More float4 than the capped grid has threads (2 048 blocks x 256): every thread takes more than one, the last round is ragged."""
    _flat_against_per_parameter([5, 2 * 2048 * 256 * 4 + 4 * 1000 + 3, 7], 0.5, True, steps=2)


class _Toy(torch.nn.Module):
    """Parameters of odd sizes whose gradient is a fixed random tensor (loss = sum p . c): nothing in the test depends on a GEMM."""

    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in ((5,), (7, 3), (1,), (33, 40), (2, 3, 5))])

    def loss(self, step):
        gen = torch.Generator().manual_seed(100 + step)
        return sum((p * torch.randn(p.shape, generator=gen).to(p.device)).sum() for p in self.ps)


def test_checkpoint_round_trip_and_torch_adam_layout():
    from cmdiad_amd.dp_train import ArenaAdam, ParamArena

    def run(net, opt, steps):
        for s in steps:
            net.loss(s).backward()
            opt.step()
            opt.zero_grad()

    net_a = _Toy(1).to(DEV)
    arena_a = ParamArena(net_a)
    opt_a = ArenaAdam(arena_a, lr=3e-3)
    run(net_a, opt_a, (0, 1))
    model_sd = {k: t.clone() for k, t in net_a.state_dict().items()}
    opt_sd = opt_a.state_dict()
    opt_sd = {"state": {k: {kk: vv.clone() for kk, vv in st.items()} for k, st in opt_sd["state"].items()}, "param_groups": opt_sd["param_groups"]}
    run(net_a, opt_a, (2,))                                   # the uninterrupted run
    net_b = _Toy(99).to(DEV)
    net_b.load_state_dict(model_sd)
    arena_b = ParamArena(net_b)
    opt_b = ArenaAdam(arena_b, lr=1.0)                        # (lr comes from the checkpoint)
    opt_b.load_state_dict(opt_sd)
    arena_b.check()
    assert opt_b.param_groups[0]["lr"] == 3e-3
    run(net_b, opt_b, (2,))
    for name in ("p", "m", "v"):
        assert torch.equal(getattr(arena_a, name), getattr(arena_b, name)), name
    assert [float(st["step"]) for st in opt_b.state_dict()["state"].values()] == [3.0] * 5
    # the keys are torch.optim.Adam's, and the dict loads into (and steps) a real torch.optim.Adam
    net_c = _Toy(99).to(DEV)
    net_c.load_state_dict(model_sd)
    ref = torch.optim.Adam(net_c.parameters(), lr=1.0)
    assert set(opt_sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in opt_sd["state"].values())
    ref.load_state_dict(opt_sd)
    net_c.loss(2).backward()
    ref.step()
    # torch's own arithmetic rounds differently: ~10 fp32 operations on the update (<= 1e-5 of it, the bound test_gpu_train_kernels.py
    # holds FusedAdam to) and the rounding of p - update itself on either side (half an ulp of p each: 2^-23 |p| together)
    for a, c, p0 in zip(net_a.parameters(), net_c.parameters(), model_sd.values()):
        upd = (a.detach() - p0).abs()
        assert torch.all((a.detach() - c.detach()).abs() <= 1e-5 * upd + 2.0 ** -23 * a.detach().abs())
    # ... and torch.optim.Adam's state loads back into an ArenaAdam
    opt_b.load_state_dict(ref.state_dict())
    assert opt_b._step == 3 and torch.equal(arena_b.view(arena_b.m, 3), ref.state[list(net_c.parameters())[3]]["exp_avg"])


def test_packed_inference_cache_follows_an_arena_step():
    from cmdiad_amd.dp_train import ArenaAdam, ParamArena
    from cmdiad_amd.models.hallucination_network import HallucinationCrossModalityNetwork
    torch.manual_seed(3)
    net = HallucinationCrossModalityNetwork(None, 768, 768).to(DEV)
    opt = ArenaAdam(ParamArena(net), lr=1e-2)
    gen = torch.Generator().manual_seed(4)
    xyz, rgb = torch.randn(2, 64, 768, generator=gen).to(DEV), torch.randn(2, 64, 768, generator=gen).to(DEV)
    net.eval()
    before = [t.clone() for t in net.hallucination_generation(xyz, rgb, "train")]
    net.train()
    loss_xyz, loss_rgb = net(xyz, rgb, False, "l2")
    (loss_xyz + loss_rgb).backward()
    opt.step()
    opt.zero_grad()
    net.eval()
    after = net.hallucination_generation(xyz, rgb, "train")
    fresh = HallucinationCrossModalityNetwork(None, 768, 768).to(DEV)
    fresh.load_state_dict(net.state_dict())
    want = fresh.eval().hallucination_generation(xyz, rgb, "train")
    for b, a, w in zip(before, after, want):
        assert not torch.equal(a, b), "the packed weights were not refreshed after ArenaAdam.step()"
        assert torch.equal(a, w)


def test_two_real_ranks_on_one_gpu_match_the_single_process_baseline_bit_for_bit():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("OMP_NUM_THREADS", "4")
    env["CMDIAD_DP_ONE_DEVICE"] = "1"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(REPO, "tests", "dp_train_worker.py")],
                         capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["dp_train"] is True and rec["ranks"] == 2 and sorted(rec["report"]) == ["cos_dist", "l2"]
    for method, r in rec["report"].items():
        print(method, "losses per step and rank:", r["losses"])
        assert r["premise"] is True
        assert r["differing_params_per_step"] == [[], [], []], (method, r["differing_params_per_step"])
        assert r["in_sync_both_ranks"] is True
        assert r["losses_equal"] == [[True, True]] * 3, (method, r["losses"], r["baseline_losses"])
