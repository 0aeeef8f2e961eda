"""GPU: cmdiad_rows_dedup_plan (csrc/dedup.hip) held to its definition on rows that collide in the 32-bit tag, at the edges of the
sample, of the 1 024-row compaction blocks and of the wave's lane coverage -- bit for bit against tests/dedup_ref.py.

Random rows never share a tag, so they never reach the squared-norm or the element comparison of verify_rows_kernel; the rows of
these cases are solved for on the host so that they do (dedup_ref.same_tag_twin / row_with_tag), and every case first checks that
the device computed the tags the host predicted: a crafted collision that does not collide on the device stops the test instead of
testing nothing.  tests/test_dedup_ref_cpu.py shows, without a GPU, that each case fails a subtly weakened plan."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as dr  # noqa: E402

DEV = "cuda"
NB = 1300                 # library rows: five 256-row tiles and a 20-row tail
CASES = dr.all_cases()
SEARCHED = [c for c in CASES if c.search]
EXPAND_PLANS = ("twins_D768-f16-live256", "block_Q2049-D768-f16", "shares_30_20_Q8193-D128-f16", "all_identical_Q4096-bf16")


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = dr.case(name)
    return dr.plan(c.q, c.sq)


@functools.lru_cache(maxsize=None)
def _bank(D, kind):
    g = torch.Generator().manual_seed(99 + D)
    return ops.normalize_cast(torch.randn(NB, D, generator=g).to(DEV), dtype=torch.float16 if kind == "f16" else torch.bfloat16)[::2]


def _device_tags(plan, Q):
    """The head of the workspace: tag [Q] u32 (the layout comment above dedup_layout in csrc/dedup.hip)."""
    return plan.work[:4 * Q].view(torch.int32).cpu().numpy().view(np.uint32)


def _plan_and_check(c, plan=None):
    q16, qsq = dr.case_tensors(c, DEV)
    plan = ops.rows_dedup_plan(q16, qsq, plan)
    assert np.array_equal(_device_tags(plan, c.Q), dr.row_tags(c.q)), "precondition: the device's tags are the predicted ones"
    slot, rows, count = _reference(c.name)
    n = int(plan.count.item())
    assert n == count and c.Q - n == c.dropped
    assert np.array_equal(plan.slot.cpu().numpy(), slot)
    assert np.array_equal(plan.rows[:n].cpu().numpy(), rows)
    assert dr.check_plan(plan, q16, qsq, c.dropped + 1) == n
    idx = torch.from_numpy(rows.astype(np.int64)).to(DEV)
    assert torch.equal(plan.q16[:n].view(torch.int16), q16[idx].view(torch.int16))
    assert torch.equal(plan.q_sq[:n].view(torch.int32), qsq[idx].view(torch.int32))
    return plan, q16, qsq


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_plan_is_the_reference_plan(c):
    _plan_and_check(c)


@pytest.mark.parametrize("c", SEARCHED, ids=[c.name for c in SEARCHED])
def test_compacted_counted_search_expands_to_the_search_of_every_row(c):
    """Best and runner-up plane: the counted search over the compacted rows, expanded through slot, against the search of every
    row; nothing is written beyond the live count."""
    plan, q16, qsq = _plan_and_check(c)
    n = int(plan.count.item())
    b16, bsq = _bank(c.D, c.kind)
    full = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(c.Q, DEV, runner=True))
    assert (full[0] != ops.KEY_EMPTY).all(), "every row is finite and finds a library row"
    kc = ops.l2_min_keys_counted(plan.q16, plan.q_sq, plan.count, b16, bsq, ops.new_keys(c.Q, DEV, runner=True))
    assert (kc[:, n:] == ops.KEY_EMPTY).all(), "rows beyond the live count must not be written"
    got = ops.keys_expand(kc, plan.slot, torch.full_like(full, -1))
    assert got.shape == (2, c.Q) and torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])


@pytest.mark.parametrize("D", [4, 12, 768])
@pytest.mark.parametrize("name", EXPAND_PLANS)
def test_rows_expand_f32_follows_slot(name, D):
    c = dr.case(name)
    plan, _, _ = _plan_and_check(c)
    n = int(plan.count.item())
    g = torch.Generator().manual_seed(D)
    src = torch.randn(c.Q, D, generator=g).to(DEV)
    src[n:] = float("nan")                                     # rows beyond the live count are never a slot
    out = ops.rows_expand_f32(src, plan.slot, torch.full((c.Q, D), -1.0, device=DEV))
    assert torch.equal(out, src[plan.slot.long()]) and bool(torch.isfinite(out).all())


def test_plan_object_reused_after_a_batch_with_many_repeats():
    """One DedupPlan: 768 repeats and four twins, then a batch of the same shape without any (info, dup and sums of the first call
    are still in the workspace), then the first batch again."""
    many, none = dr.case("twins_D768-f16-live257"), dr.case("no_repeats_Q1024-D768-f16")
    plan, _, _ = _plan_and_check(many)
    again, _, _ = _plan_and_check(none, plan)
    assert again is plan and int(plan.count.item()) == none.Q
    assert torch.equal(plan.slot.cpu(), torch.arange(none.Q, dtype=torch.int32)) and torch.equal(plan.rows.cpu(), torch.arange(none.Q, dtype=torch.int32))
    third, _, _ = _plan_and_check(many, plan)
    assert third is plan


@pytest.mark.parametrize("name", ["twins_D1152-bf16", "shares_30_20_Q20011-D768-bf16", "tie_high_bits_winner_later-f16"])
def test_two_calls_give_the_same_plan(name):
    c = dr.case(name)
    q16, qsq = dr.case_tensors(c, DEV)
    a, b = ops.rows_dedup_plan(q16, qsq), ops.rows_dedup_plan(q16, qsq)
    assert a is not b and torch.equal(a.count, b.count) and torch.equal(a.slot, b.slot)
    n = int(a.count.item())
    assert torch.equal(a.rows[:n], b.rows[:n]) and torch.equal(a.q16[:n].view(torch.int16), b.q16[:n].view(torch.int16))
    assert torch.equal(a.q_sq[:n].view(torch.int32), b.q_sq[:n].view(torch.int32))
