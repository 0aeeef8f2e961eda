"""Data-parallel training of the distillation MLP heads ("DP trainer ... gradient all-reduce 13.28 M params";
the reference's own scaffolding: hallucination_network_pretrain.py --distributed, utils/misc.py:init_distributed_mode).
docs/dp_train.md is the user's guide; INTEGRATION.md section 6c lists the lines to change in the reference's script.

  ParamArena(module)     four flat fp32 device buffers p, g, m, v; every parameter of the module is a segment of them, padded to a
                         multiple of 4 floats, in module.parameters() order; param.data and param.grad are VIEWS of p and g.
  ArenaAdam(arena, lr)   torch.optim.Adam's update (no weight decay, no amsgrad) of the whole arena in ONE launch
                         (cmdiad_adam_flat: bit-identical to train.FusedAdam's one launch per parameter), on the gradients
                         averaged over the ranks of `group`: buckets of whole parameters, reduced in place in g with
                         all_reduce(SUM, async_op=True) as backward() completes them, and 1 / world folded into the kernel.
  init_from_env()        rank, world, device and process group from RANK / WORLD_SIZE / LOCAL_RANK.
  dataset.FeatureRing / PairRing / epoch_batches(..., rank, world) deal every global batch of world * batch_size to the ranks.

The reference's loss is a sum over the rank's samples divided by the rank's batch size and the gradients are AVERAGED over the
ranks, so W ranks at batch B take exactly the step of one process at batch W * B (over the same samples: the rings deal them so).

Gradient accumulation: give ArenaAdam the loop's `accum_iter`.  The reductions are issued only in the backward pass that precedes a
step() -- the accum_iter-th since the last one; the loop itself (`loss /= accum_iter; loss.backward(); every accum_iter-th
iteration step() and zero_grad()`) stays as the reference has it.

There is no overlap machinery: a training head computes its gradients in forward() (train.step_loss) and backward() only hands
them out, so the reductions start when the compute is over.  2 x 26.6 MB over xGMI is an ESTIMATED 2-3 % of the step (an estimate,
not a measurement: this project has no multi-GPU measurement).

Scope: modules without buffers that training updates.  BatchNorm running statistics are per-rank batch statistics and would need
SyncBN, so a module with a BatchNorm layer is refused: this covers HallucinationCrossModalityNetwork at any mlp_depth and
HallucinationRGBFeatureToXYZInputMLP.
"""
import datetime
import os

import torch
import torch.distributed as td

from . import ops

BUCKET_BYTES = 32 << 20


def _pad4(n):
    return (n + 3) // 4 * 4


class ParamArena:
    """Build it AFTER module.to(device).  `segments`: (name, parameter, offset, numel) in module.parameters() order, offsets in
    floats and multiples of 4; the padding lanes of p, g, m and v start at zero and stay exactly zero (Adam leaves a lane with
    g = m = v = 0 where it is).  module.state_dict() / load_state_dict() keep working: load_state_dict copies in place."""

    def __init__(self, module):
        for name, sub in module.named_modules():
            if isinstance(sub, torch.nn.modules.batchnorm._BatchNorm):
                raise NotImplementedError(f"ParamArena: {type(module).__name__}.{name} is a {type(sub).__name__}: its running statistics "
                                          "are buffers updated from per-rank batch statistics; data-parallel training would need SyncBN")
        named = list(module.named_parameters())
        if not named:
            raise ValueError("ParamArena: the module has no parameters")
        dev = named[0][1].device
        for name, p in named:
            if p.dtype != torch.float32 or p.device != dev or not p.requires_grad:
                raise ValueError(f"ParamArena: {name} must be a trainable fp32 parameter on {dev} (is {p.dtype} on {p.device})")
        self.module, self.device = module, dev
        self.segments, off = [], 0
        for name, p in named:
            self.segments.append((name, p, off, p.numel()))
            off += _pad4(p.numel())
        self.numel = off
        self.p, self.g, self.m, self.v = (torch.zeros(off, dtype=torch.float32, device=dev) for _ in range(4))
        with torch.no_grad():
            for _, p, o, n in self.segments:
                self.p[o:o + n].view(p.shape).copy_(p.data)
                p.data = self.p[o:o + n].view(p.shape)
                p.grad = self.g[o:o + n].view(p.shape)
        self.optimizer = None       # the ArenaAdam whose gradient hooks sit on the parameters (one at a time)

    def view(self, buf, i):
        """Segment i of one of the four buffers, in the parameter's shape."""
        _, p, o, n = self.segments[i]
        return buf[o:o + n].view(p.shape)

    def check(self):
        """RuntimeError if a parameter or its gradient no longer points into the arena (module.to() / zero_grad(set_to_none=True)
        of the MODULE after the arena was built)."""
        pb, gb = self.p.data_ptr(), self.g.data_ptr()
        for name, p, o, _ in self.segments:
            if p.data_ptr() != pb + 4 * o:
                raise RuntimeError(f"ParamArena: parameter {name} no longer points into the arena (build the arena after module.to(device))")
            if p.grad is None or p.grad.data_ptr() != gb + 4 * o:
                raise RuntimeError(f"ParamArena: the gradient of {name} no longer points into the arena (use ArenaAdam.zero_grad(), "
                                   "which zeroes in place)")


class _Bucket:
    def __init__(self, idxs, lo, hi):
        self.idxs, self.lo, self.hi = idxs, lo, hi      # parameter indices (reverse registration order), float range of the arena
        self.seen = set()                                # parameters whose gradient arrived in the current backward pass
        self.passes = 0                                  # completed backward passes since the last step()
        self.ready = False                               # complete in the pass that precedes step(): to be reduced


def _buckets(segments, limit_bytes):
    """Whole parameters in reverse registration order (the order backward() produces them in), at most limit_bytes of arena each
    (a larger parameter is a bucket of its own): contiguous slices of the arena, the last one first.  The arena is cut into the
    fewest buckets the limit allows and a bucket is closed once it holds its even share, so that the two directions of the
    feature-to-feature network (26.6 MB each) are the two buckets rather than 32 MB and the rest."""
    total = 4 * (segments[-1][2] + _pad4(segments[-1][3]))
    share = total / -(-total // limit_bytes)
    out, cur, hi = [], [], None
    for i in range(len(segments) - 1, -1, -1):
        _, _, o, n = segments[i]
        if cur and ((hi - o) * 4 > limit_bytes or (hi - segments[cur[-1]][2]) * 4 >= share):
            out.append(_Bucket(cur, segments[cur[-1]][2], hi))
            cur = []
        if not cur:
            hi = o + _pad4(n)
        cur.append(i)
    out.append(_Bucket(cur, segments[cur[-1]][2], hi))
    return out


class ArenaAdam(torch.optim.Optimizer):
    """torch.optim.Adam(module.parameters(), lr, betas, eps) semantics over a ParamArena: step(), zero_grad(),
    param_groups[0]["lr"] and utils.lr_sched.adjust_learning_rate as in the reference's loop; state_dict() / load_state_dict() in
    torch.optim.Adam's layout (per-parameter step, exp_avg, exp_avg_sq), so a checkpoint moves between the two.

    group: the process group to average the gradients over (None, or a group of one rank: no collective is issued).  At
    construction rank 0's parameters are broadcast.  accum_iter: backward passes per step() (module docstring).
    Every parameter must receive a gradient in every backward pass: step() raises RuntimeError naming one that did not -- on every
    rank alike, so nothing waits for a collective that never comes."""

    def __init__(self, arena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, group=None, accum_iter=1, bucket_bytes=BUCKET_BYTES):
        if accum_iter < 1:
            raise ValueError("accum_iter must be >= 1")
        if getattr(arena, "optimizer", None) is not None:
            raise RuntimeError("ArenaAdam: the arena already has an optimizer whose hooks sit on the parameters; close() it first")
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__([p for _, p, _, _ in arena.segments], defaults)
        self.arena, self.group, self.accum_iter = arena, group, accum_iter
        self.world = td.get_world_size(group) if group is not None else 1
        self._step = 0
        for i, (_, p, _, _) in enumerate(arena.segments):
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": arena.view(arena.m, i), "exp_avg_sq": arena.view(arena.v, i)}
        self.buckets = _buckets(arena.segments, bucket_bytes)
        self._bucket_of = {}
        for b in self.buckets:
            for i in b.idxs:
                self._bucket_of[i] = b
        self._issued = 0            # buckets 0 .. _issued - 1 have been reduced (or need no reduction) for the coming step()
        self._works = []
        self.reductions = 0         # collectives issued so far (tests, tools)
        self._hooks = [p.register_post_accumulate_grad_hook(self._make_hook(i)) for i, (_, p, _, _) in enumerate(arena.segments)]
        arena.optimizer = self
        if self.world > 1:
            td.broadcast(arena.p, src=td.get_global_rank(group, 0), group=group)

    # ------------------------------------------------------------------------------------------------------ gradient averaging
    def _make_hook(self, i):
        def hook(_param):
            b = self._bucket_of[i]
            if b.ready:
                raise RuntimeError(f"ArenaAdam: backward pass {self.accum_iter + 1} since the last step() with accum_iter = "
                                   f"{self.accum_iter}: the gradients of the step have already been reduced")
            b.seen.add(i)
            if len(b.seen) == len(b.idxs):
                b.seen.clear()
                b.passes += 1
                if b.passes == self.accum_iter:
                    b.ready = True
                    self._issue()
        return hook

    def _issue(self):
        """Bucket k goes out once it is complete and buckets 0 .. k-1 have gone: the same order on every rank."""
        while self._issued < len(self.buckets) and self.buckets[self._issued].ready:
            b = self.buckets[self._issued]
            if self.world > 1:
                self._works.append(td.all_reduce(self.arena.g[b.lo:b.hi], op=td.ReduceOp.SUM, group=self.group, async_op=True))
                self.reductions += 1
            self._issued += 1

    def _missing(self):
        """(parameter name, backward passes its bucket has completed) of a parameter that holds a bucket back, or None."""
        for b in self.buckets:
            if not b.ready:
                lack = [i for i in b.idxs if i not in b.seen] if b.seen else b.idxs
                return self.arena.segments[lack[0]][0], b.passes
        return None

    # ---------------------------------------------------------------------------------------------------------------- optimizer
    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("ArenaAdam.step: closures are not supported")
        self.arena.check()
        miss = self._missing()
        if miss is not None:
            for w in self._works:           # what was issued is complete on every rank alike: drain it, then fail alike
                w.wait()
            self._reset()
            raise RuntimeError(f"ArenaAdam.step: parameter {miss[0]} received no gradient in backward pass {miss[1] + 1} of "
                               f"{self.accum_iter} since the last step(): every parameter must take part in every pass")
        for w in self._works:               # the current stream waits for the reductions (torch.distributed's stream semantics)
            w.wait()
        self._reset()
        g = self.param_groups[0]
        if len(self.param_groups) != 1 or g["weight_decay"] != 0 or g["amsgrad"] or g["maximize"]:
            raise NotImplementedError("ArenaAdam: one parameter group, no weight decay, no amsgrad, no maximize")
        self._step += 1
        a = self.arena
        ops.adam_flat(a.p, a.g, a.m, a.v, g["lr"], g["betas"][0], g["betas"][1], g["eps"], self._step, 1.0 / self.world)
        torch._foreach_add_([self.state[p]["step"] for p in g["params"]], 1.0)
        for p in g["params"]:
            p.view(-1)[:0].zero_()      # the kernel wrote p in place: bump its version so packed caches refresh (as FusedAdam does)

    def _reset(self):
        self._works, self._issued = [], 0
        for b in self.buckets:
            b.seen.clear()
            b.passes, b.ready = 0, False

    def zero_grad(self, set_to_none=True):
        """One fill of g, whatever set_to_none says: with None autograd would put fresh tensors in the views' place.
        The gradients are gone, so the count of backward passes starts again as well: the reference's loop calls zero_grad() at
        the start of every epoch and so discards the passes left over when the epoch's batches are no multiple of accum_iter
        (no reduction has gone out for them: reductions belong to the accum_iter-th pass)."""
        for w in self._works:               # (none unless zero_grad() comes between the last backward pass and step())
            w.wait()
        self._reset()
        self.arena.g.zero_()

    def state_dict(self):
        """torch.optim.Adam's layout; exp_avg and exp_avg_sq are COPIES, not views of the arena (an optimizer that loads the
        dict in the same process keeps the tensors it is given)."""
        sd = super().state_dict()
        sd["state"] = {k: {kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in st.items()} for k, st in sd["state"].items()}
        return sd

    def close(self):
        """Takes the gradient hooks off the parameters and frees the arena for another ArenaAdam (one at a time: two would both
        count every backward pass and reduce every bucket twice)."""
        for h in self._hooks:
            h.remove()
        self._hooks = []
        if getattr(self.arena, "optimizer", None) is self:
            self.arena.optimizer = None

    def in_sync(self):
        """Whether every rank of the group holds bit-equal parameters (a MIN and a MAX all-reduce over the int32 view)."""
        if self.world == 1:
            return True
        lo = self.arena.p.view(torch.int32).clone()
        hi = lo.clone()
        td.all_reduce(lo, op=td.ReduceOp.MIN, group=self.group)
        td.all_reduce(hi, op=td.ReduceOp.MAX, group=self.group)
        return bool(torch.equal(lo, hi))

    def load_state_dict(self, state_dict):
        """A state_dict of ArenaAdam or of torch.optim.Adam over the same parameters: copied IN PLACE into m and v."""
        groups = state_dict["param_groups"]
        mine = self.param_groups[0]
        if len(groups) != 1 or len(groups[0]["params"]) != len(mine["params"]):
            raise ValueError("ArenaAdam.load_state_dict: expected one parameter group over the arena's parameters")
        if groups[0].get("weight_decay", 0) != 0 or groups[0].get("amsgrad", False) or groups[0].get("maximize", False):
            raise NotImplementedError("ArenaAdam: no weight decay, no amsgrad, no maximize")
        steps = set()
        with torch.no_grad():
            for p, pid in zip(mine["params"], groups[0]["params"]):
                src, st = state_dict["state"].get(pid), self.state[p]
                if src is None:                 # torch.optim.Adam before its first step
                    st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
                    steps.add(0)
                    continue
                if tuple(src["exp_avg"].shape) != tuple(p.shape):
                    raise ValueError(f"ArenaAdam.load_state_dict: state of shape {tuple(src['exp_avg'].shape)} for a parameter of {tuple(p.shape)}")
                st["exp_avg"].copy_(src["exp_avg"])
                st["exp_avg_sq"].copy_(src["exp_avg_sq"])
                steps.add(int(src["step"]))
        if len(steps) != 1:
            raise ValueError(f"ArenaAdam.load_state_dict: the parameters are at different steps {sorted(steps)}")
        self._step = steps.pop()
        for p in mine["params"]:
            self.state[p]["step"].fill_(float(self._step))
        for k, v in groups[0].items():
            if k != "params":
                mine[k] = v


def init_from_env(timeout_s=600):
    """-> (rank, world, device, group | None) of this process, from RANK, WORLD_SIZE and LOCAL_RANK (torch.distributed.run sets
    them; a plain `python train.py` is rank 0 of 1 with no group).  Sets the device.  The collectives go over nccl (RCCL), or over
    gloo with EVERY rank on device 0 when CMDIAD_DP_ONE_DEVICE=1 -- RCCL refuses two ranks on one device: the rehearsal of an N-rank
    run on a one-GPU box.  The process group gets a finite timeout."""
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")))
    one = os.environ.get("CMDIAD_DP_ONE_DEVICE", "0") == "1"
    if one:
        local = 0
    torch.cuda.set_device(local)
    group = None
    if world > 1:
        if not td.is_initialized():
            td.init_process_group("gloo" if one else "nccl", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=timeout_s))
        group = td.group.WORLD
    return rank, world, torch.device("cuda", local), group
