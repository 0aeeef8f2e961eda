"""CPU (no GPU): the host side of data-parallel training (cmdiad_amd/dp_train.py) -- the batches dealt to the ranks, the arena's
layout and views on CPU tensors, the bucket logic in a gloo world of two CPU processes with a torch stand-in for the flat Adam
kernel, and the argument validation of cmdiad_adam_flat."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- dealing the batches
@pytest.mark.parametrize("n,B,W,shuffle", [(11, 2, 2, True), (64, 4, 2, True), (37, 3, 4, True), (37, 3, 4, False), (16, 2, 8, True),
                                           (5, 2, 3, True), (24, 4, 1, True)])
def test_rank_slices_concatenate_to_the_global_batches(n, B, W, shuffle):
    """W ranks at batch B see what one process at batch W * B sees, in the same order, and consume the global RNG alike."""
    from cmdiad_amd.dataset import epoch_batches, epoch_length
    torch.manual_seed(3407)
    want = [epoch_batches(n, W * B, shuffle, True) for _ in range(2)]          # two epochs
    rng_after = torch.rand(1).item()
    per_rank = []
    for r in range(W):
        torch.manual_seed(3407)
        per_rank.append([epoch_batches(n, B, shuffle, True, rank=r, world=W) for _ in range(2)])
        assert torch.rand(1).item() == rng_after, "a rank consumed the global RNG differently from the single process"
    for e in range(2):
        assert len(want[e]) == epoch_length(n, W * B, True) == n // (W * B)
        for r in range(W):
            assert len(per_rank[r][e]) == len(want[e]) and all(len(b) == B for b in per_rank[r][e])
        got = [sum((per_rank[r][e][i] for r in range(W)), []) for i in range(len(want[e]))]
        assert got == want[e]


def test_defaults_deal_nothing_and_a_short_last_batch_is_refused(tmp_path):
    from cmdiad_amd.dataset import FeatureRing, epoch_batches
    for shuffle, drop in ((True, True), (True, False), (False, False)):
        torch.manual_seed(5)
        a = epoch_batches(11, 4, shuffle, drop)
        torch.manual_seed(5)
        assert a == epoch_batches(11, 4, shuffle, drop, rank=0, world=1)
        assert len(a) == (2 if drop else 3)
    with pytest.raises(ValueError, match="drop_last"):
        epoch_batches(11, 2, True, False, rank=0, world=2)
    with pytest.raises(ValueError):
        epoch_batches(11, 2, True, True, rank=2, world=2)
    for i in range(11):
        torch.save(torch.full((4, 6), float(i)), tmp_path / f"bagel{i}.pt")
    with pytest.raises(ValueError, match="drop_last"):
        FeatureRing(str(tmp_path), 2, drop_last=False, device="cpu", world=2)
    # the rings: two ranks at batch 2 against one process at batch 4, two epochs, len() follows the GLOBAL batch
    torch.manual_seed(11)
    whole = FeatureRing(str(tmp_path), 4, shuffle=True, drop_last=True, device="cpu", readers=2)
    want = [[x.clone() for x, _ in whole] for _ in range(2)]
    got = []
    for r in range(2):
        torch.manual_seed(11)
        ring = FeatureRing(str(tmp_path), 2, shuffle=True, drop_last=True, device="cpu", readers=2, rank=r, world=2)
        assert len(ring) == len(whole) == 2
        got.append([[x.clone() for x, _ in ring] for _ in range(2)])
    for e in range(2):
        assert len(got[0][e]) == len(want[e]) == 2
        for i, w in enumerate(want[e]):
            assert torch.equal(torch.cat([got[0][e][i], got[1][e][i]]), w)


def test_pair_ring_deals_the_global_batches(tmp_path):
    from cmdiad_amd.dataset import PairRing

    class Pairs:
        def __len__(self):
            return 9

        def pair_paths(self, i):
            return tmp_path / f"a{i}.pt", tmp_path / f"b{i}.pt"

    for i in range(9):
        torch.save(torch.full((3,), float(i)), tmp_path / f"a{i}.pt")
        torch.save(torch.full((2,), float(-i)), tmp_path / f"b{i}.pt")
    torch.manual_seed(2)
    whole = PairRing(Pairs(), 4, device="cpu", readers=1)
    want = list(whole)
    parts = []
    for r in range(2):
        torch.manual_seed(2)
        ring = PairRing(Pairs(), 2, device="cpu", readers=1, rank=r, world=2)
        assert len(ring) == len(whole) == 2
        parts.append(list(ring))
    for i, (a, b) in enumerate(want):
        assert torch.equal(torch.cat([parts[0][i][0], parts[1][i][0]]), a) and torch.equal(torch.cat([parts[0][i][1], parts[1][i][1]]), b)
    with pytest.raises(ValueError, match="drop_last"):
        PairRing(Pairs(), 2, drop_last=False, device="cpu", world=2)


# ------------------------------------------------------------------------------------------------------------------ arena layout
def _small_module():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.LayerNorm(5), torch.nn.Linear(5, 7), torch.nn.GELU(), torch.nn.Linear(7, 3))


def test_arena_layout_and_views_on_cpu_tensors():
    from cmdiad_amd import _native as nat
    from cmdiad_amd.dp_train import ArenaAdam, ParamArena
    net = _small_module()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    arena = ParamArena(net)
    sizes = [p.numel() for p in net.parameters()]
    assert sizes == [5, 5, 35, 7, 21, 3]
    assert [s[2] for s in arena.segments] == [0, 8, 16, 52, 60, 84] and arena.numel == 88
    assert all(o % 4 == 0 for _, _, o, _ in arena.segments)
    assert [s[0] for s in arena.segments] == [k for k, _ in net.named_parameters()] == list(net.state_dict())
    opt = ArenaAdam(arena, lr=1e-3)

    def views_hold():
        arena.check()
        for _, p, o, n in arena.segments:
            assert p.data_ptr() == arena.p.data_ptr() + 4 * o and p.grad.data_ptr() == arena.g.data_ptr() + 4 * o
            assert torch.equal(arena.p[o:o + n], p.detach().reshape(-1)) and torch.equal(arena.g[o:o + n], p.grad.reshape(-1))

    def padding():
        keep = torch.ones(arena.numel, dtype=torch.bool)
        for _, _, o, n in arena.segments:
            keep[o:o + n] = False
        return keep

    views_hold()
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())          # the values moved into the arena unchanged
    assert int(padding().sum()) == 88 - sum(sizes)
    net(torch.randn(4, 5)).sum().backward()
    views_hold()
    assert float(arena.g.abs().sum()) > 0 and float(arena.g[padding()].abs().sum()) == 0
    with pytest.raises(nat.NativeError, match="GPU"):      # there is no CPU path
        opt.step()
    opt.zero_grad()                      # torch's default set_to_none=True: still one fill, the views stay
    views_hold()
    assert float(arena.g.abs().sum()) == 0
    opt.zero_grad(set_to_none=False)
    views_hold()
    other = {k: torch.randn_like(v) for k, v in before.items()}
    net.load_state_dict(other)           # copies in place
    views_hold()
    assert all(torch.equal(v, other[k]) for k, v in net.state_dict().items()) and float(arena.p[padding()].abs().sum()) == 0
    net(torch.randn(4, 5)).sum().backward()
    with pytest.raises(nat.NativeError, match="GPU"):
        opt.step()
    # a module that moved away from the arena is refused
    net.zero_grad(set_to_none=True)
    net(torch.randn(4, 5)).sum().backward()
    with pytest.raises(RuntimeError, match="no longer points into the arena"):
        opt.step()
    net2 = _small_module()
    arena2 = ParamArena(net2)
    opt2 = ArenaAdam(arena2)
    net2.double().float()                # what .to() does: new storage
    net2(torch.randn(4, 5)).sum().backward()
    with pytest.raises(RuntimeError, match="no longer points into the arena"):
        opt2.step()


def test_arena_refuses_batchnorm_and_names_the_reason():
    from cmdiad_amd.dp_train import ParamArena
    from cmdiad_amd.models.hallucination_network import HallucinationCrossModalityConv
    with pytest.raises(NotImplementedError, match="SyncBN"):
        ParamArena(torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4)))
    with pytest.raises(NotImplementedError, match="SyncBN"):
        ParamArena(HallucinationCrossModalityConv(None, 768, 768))


def test_buckets_are_whole_parameters_in_reverse_order():
    from cmdiad_amd.dp_train import ArenaAdam, ParamArena
    from cmdiad_amd.models.hallucination_network import HallucinationCrossModalityNetwork
    net = HallucinationCrossModalityNetwork(None, 768, 768)
    arena = ParamArena(net)
    opt = ArenaAdam(arena, lr=5e-4)
    assert arena.numel == sum(p.numel() for p in net.parameters()) == 13_283_328          # 13.28 M parameters
    # the two directions: rgb (registered last) first
    assert [(b.idxs, b.lo, b.hi) for b in opt.buckets] == [(list(range(15, 7, -1)), arena.numel // 2, arena.numel),
                                                           (list(range(7, -1, -1)), 0, arena.numel // 2)]
    assert all((b.hi - b.lo) * 4 <= 32 << 20 for b in opt.buckets)
    small = ArenaAdam(ParamArena(_small_module()), bucket_bytes=64)
    assert [(b.idxs, b.lo, b.hi) for b in small.buckets] == [([5], 84, 88), ([4], 60, 84), ([3], 52, 60), ([2], 16, 52), ([1, 0], 0, 16)]
    # torch.optim.Adam's state layout: a checkpoint moves between the two optimizers
    sd = opt.state_dict()
    ref = torch.optim.Adam(HallucinationCrossModalityNetwork(None, 768, 768).parameters(), lr=1e-3)
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values()) and len(sd["state"]) == 16
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 5e-4


# ------------------------------------------------------------------------------------------- bucket logic, gloo world of two
_WORKER = r"""
import datetime, os, sys
sys.path.insert(0, {repo!r})
import torch, torch.distributed as td
from cmdiad_amd import dp_train, ops
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
calls = []
def adam_flat(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, p_bf16=None):      # torch stand-in for the kernel
    calls.append((step, grad_scale))
    gi = g * grad_scale
    m.mul_(b1).add_(gi, alpha=1 - b1)
    v.mul_(b2).addcmul_(gi, gi, value=1 - b2)
    p.sub_((lr / (1 - b1 ** step)) * (m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps)))
ops.adam_flat = adam_flat
def make(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.LayerNorm(5), torch.nn.Linear(5, 7), torch.nn.GELU(), torch.nn.Linear(7, 3))
net = make(100 + rank)                                   # different on the ranks: the broadcast makes them rank 0's
arena = dp_train.ParamArena(net)
opt = dp_train.ArenaAdam(arena, lr=1e-2, group=td.group.WORLD, accum_iter=2, bucket_bytes=64)
assert len(opt.buckets) == 5 and opt.in_sync()
assert torch.equal(arena.p, dp_train.ParamArena(make(100)).p)
x = [[torch.randn(4, 5, generator=torch.Generator().manual_seed(10 * r + i)) for i in range(4)] for r in range(world)]
# by hand: every rank's two micro-batch gradients summed, averaged over the ranks, one Adam step
ref = make(100)
ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
for s in range(2):
    opt.zero_grad()
    for i in (2 * s, 2 * s + 1):
        before = opt.reductions
        (net(x[rank][i]).pow(2).sum() / 2).backward()
        assert opt.reductions - before == (5 if i % 2 == 1 else 0), "reductions belong to the pass that precedes step()"
    opt.step()
    ropt.zero_grad()
    for r in range(world):
        for i in (2 * s, 2 * s + 1):
            (ref(x[r][i]).pow(2).sum() / 2 / world).backward()
    ropt.step()
    assert calls[-1] == (s + 1, 0.5) and len(calls) == s + 1
    for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), (k, (a - b).abs().max())
    assert opt.in_sync()
pad = torch.ones(arena.numel, dtype=torch.bool)
for _, _, o, n in arena.segments:
    pad[o:o + n] = False
assert all(float(buf[pad].abs().sum()) == 0 for buf in (arena.p, arena.g, arena.m, arena.v))
# ranks that drift apart are noticed
if rank == 1:
    arena.p[3] += 1e-7 * (1 + arena.p[3].abs())
drift = not opt.in_sync()
td.broadcast(arena.p, 0)
assert drift and opt.in_sync()
# an unused parameter: step() raises on BOTH ranks, naming it, and nothing hangs
opt.zero_grad()
for i in range(2):
    (net[1](net[0](x[rank][i])).sum() / 2).backward()                       # the last Linear takes no part
try:
    opt.step()
    raise SystemExit("step() accepted a parameter without a gradient")
except RuntimeError as exc:
    assert "3.bias" in str(exc) or "3.weight" in str(exc), str(exc)
assert len(calls) == 2
# ... and the optimizer goes on working afterwards
opt.zero_grad()
for i in range(2):
    (net(x[rank][i]).pow(2).sum() / 2).backward()
opt.step()
assert len(calls) == 3 and opt.in_sync()
# the reference's loop over two epochs of 3 batches with accum_iter = 2: zero_grad() at the start of an epoch discards the pass
# left over from the epoch before -- its gradients AND its count -- and a reduction goes out only in a pass that precedes a step()
net, ref = make(100), make(100)
arena = dp_train.ParamArena(net)
opt = dp_train.ArenaAdam(arena, lr=1e-2, group=td.group.WORLD, accum_iter=2, bucket_bytes=64)
ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
calls.clear()
for epoch in range(2):
    opt.zero_grad()
    ropt.zero_grad()
    for i in range(3):
        before = opt.reductions
        (net(x[rank][i]).pow(2).sum() / 2).backward()
        for r in range(world):
            (ref(x[r][i]).pow(2).sum() / 2 / world).backward()
        assert opt.reductions - before == (5 if i == 1 else 0), (epoch, i, opt.reductions - before)
        if (i + 1) % 2 == 0:
            opt.step()
            ropt.step()
            opt.zero_grad()
            ropt.zero_grad()
assert calls == [(1, 0.5), (2, 0.5)] and opt.reductions == 10
for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), (k, (a - b).abs().max())
assert opt.in_sync()
td.barrier()
td.destroy_process_group()
print("rank", rank, "ok")
"""


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_bucket_reductions_accumulation_and_unused_parameter_world2_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_WORKER.format(repo=REPO))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=180)[0].decode())
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    assert all(pr.returncode == 0 for pr in procs), outs
    assert all(f"rank {r} ok" in outs[r] for r in range(2)), outs


def test_world_of_one_issues_no_collective():
    from cmdiad_amd import ops
    from cmdiad_amd.dp_train import ArenaAdam, ParamArena
    net = _small_module()
    opt = ArenaAdam(ParamArena(net), lr=1e-2)
    seen = []
    orig = ops.adam_flat
    ops.adam_flat = lambda *a, **k: seen.append((a[8], a[9] if len(a) > 9 else k.get("grad_scale", 1.0)))
    try:
        v0 = [p._version for p in net.parameters()]
        net(torch.randn(4, 5)).sum().backward()
        opt.step()
        assert seen == [(1, 1.0)] and opt.reductions == 0 and opt.in_sync()
        assert all(p._version > v for p, v in zip(net.parameters(), v0))       # packed caches refresh on the version counter
        assert [float(st["step"]) for st in opt.state_dict()["state"].values()] == [1.0] * 6
        with pytest.raises(RuntimeError, match="received no gradient"):          # no backward pass since the last step()
            opt.step()
    finally:
        ops.adam_flat = orig


def test_leftover_passes_of_an_epoch_are_discarded_by_zero_grad_world1():
    """3 batches per epoch, accum_iter = 2, the reference's loop shape, two epochs: one step per epoch, no error in the second."""
    from cmdiad_amd import ops
    from cmdiad_amd.dp_train import ArenaAdam, ParamArena
    net = _small_module()
    opt = ArenaAdam(ParamArena(net), lr=1e-2, accum_iter=2)
    seen = []
    orig = ops.adam_flat
    ops.adam_flat = lambda *a, **k: seen.append((a[8], float(a[1].abs().sum())))       # (step, |g| handed to the kernel)
    try:
        gen = torch.Generator().manual_seed(1)
        xs = [torch.randn(4, 5, generator=gen) for _ in range(3)]
        want = []
        for epoch in range(2):
            opt.zero_grad()
            for i, x in enumerate(xs):
                (net(x).pow(2).sum() / 2).backward()
                if (i + 1) % 2 == 0:
                    ref = torch.autograd.grad(sum(net(xx).pow(2).sum() / 2 for xx in xs[:2]), list(net.parameters()))
                    want.append(float(sum(g.abs().sum() for g in ref)))
                    opt.step()
                    opt.zero_grad()
        assert [s for s, _ in seen] == [1, 2]
        assert all(abs(got - w) <= 1e-5 * w for (_, got), w in zip(seen, want)), (seen, want)      # batches 0 and 1 only, not the leftover
    finally:
        ops.adam_flat = orig


def test_one_optimizer_per_arena_close_frees_it_and_state_dict_holds_copies():
    from cmdiad_amd.dp_train import ArenaAdam, ParamArena
    net = _small_module()
    arena = ParamArena(net)
    opt = ArenaAdam(arena, lr=1e-2)
    with pytest.raises(RuntimeError, match="already has an optimizer"):
        ArenaAdam(arena, lr=1e-2)
    sd = opt.state_dict()
    lo, hi = arena.m.data_ptr(), arena.m.data_ptr() + 4 * arena.numel
    assert all(not lo <= st["exp_avg"].data_ptr() < hi for st in sd["state"].values())
    ref = torch.optim.Adam(net.parameters(), lr=1e-2)
    ref.load_state_dict(sd)
    assert all(not lo <= st["exp_avg"].data_ptr() < hi for st in ref.state.values())
    opt.close()
    opt2 = ArenaAdam(arena, lr=1e-2)
    net(torch.randn(4, 5)).sum().backward()
    assert all(b.passes == 0 and not b.ready for b in opt.buckets)       # the closed optimizer's hooks are gone
    assert all(b.ready for b in opt2.buckets)


# ---------------------------------------------------------------------------------------------------------------- entry point
def test_adam_flat_entry_point_is_declared_bound_and_validates_before_any_launch():
    from cmdiad_amd import _native as nat, ops
    L = nat.lib()
    assert L.cmdiad_abi_version() == 6
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    assert re.search(r"\bint\s+cmdiad_adam_flat\s*\(", hdr)
    assert nat.SIGNATURES["cmdiad_adam_flat"] == nat.SIGNATURES["cmdiad_adam_step"] and hasattr(L, "cmdiad_adam_flat") and callable(ops.adam_flat)
    buf = (ctypes.c_float * 16)()
    base = ctypes.addressof(buf)
    a = ctypes.c_void_p(base + (-base) % 16)              # 16-byte aligned, room for 8 floats
    args = (0.001, 0.9, 0.999, 1e-8)
    assert L.cmdiad_adam_flat(None, a, a, a, 8, *args, 1, 1.0, None, None) == -1 and b"null pointer" in L.cmdiad_last_error()
    assert L.cmdiad_adam_flat(a, a, a, None, 8, *args, 1, 1.0, None, None) == -1 and b"null pointer" in L.cmdiad_last_error()
    assert L.cmdiad_adam_flat(a, a, a, a, 6, *args, 1, 1.0, None, None) == -1 and b"bad args" in L.cmdiad_last_error()
    assert L.cmdiad_adam_flat(a, a, a, a, 8, *args, 0, 1.0, None, None) == -1 and b"bad args" in L.cmdiad_last_error()
    assert L.cmdiad_adam_flat(a, a, a, ctypes.c_void_p(a.value + 4), 4, *args, 1, 1.0, None, None) == -1 and b"aligned" in L.cmdiad_last_error()
    assert L.cmdiad_adam_flat(a, a, a, a, 0, *args, 1, 1.0, None, None) == 0       # nothing to do: no launch either
    with pytest.raises(nat.NativeError, match="GPU"):
        ops.adam_flat(*(torch.zeros(8) for _ in range(4)), 1e-3, 0.9, 0.999, 1e-8, 1)
