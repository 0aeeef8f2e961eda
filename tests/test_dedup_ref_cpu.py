"""CPU: the reference plan and the cases of tests/test_gpu_dedup_edges.py have teeth (tests/dedup_ref.py).

The GPU file compares the device's plan with dedup_ref.plan bit for bit.  That says something about the kernels only if (1) the
crafted rows really share their tags, (2) the reference finds the most repeated row where the definition says it must, (3) every
case gives a rejected or a different plan under at least one deliberately weakened reference -- the element compare left out, cut
to the first 64 chunks, the norm bits left out, the sample taken from the leading rows, the compaction without the running base of
the earlier blocks -- and (4) the cases that are meant to save rows, or to show the documented cost, do."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as dr  # noqa: E402

CASES = dr.all_cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("kinds", [("f16",), ("bf16",), dr.KINDS], ids=["f16", "bf16", "both"])
@pytest.mark.parametrize("D", [8, 64, 128, 320, 768, 1152])
def test_crafted_twins_share_the_tag_and_nothing_else(D, kinds):
    rng = np.random.default_rng(D)
    row = dr.to_u16(rng.standard_normal((1, D), dtype=np.float32), kinds[0])[0]
    row[(row & 0x7FFF) >= dr._limit(kinds)] = 0x3C00 if kinds == ("f16",) else 0x3F80
    chunks = dr.twin_chunks(D)
    assert {0, D // 8 - 1} <= set(chunks) and (D != 768 or {63, 64} <= set(chunks)) and (D != 1152 or max(chunks) >= 128)
    for c in chunks:
        twin = dr.same_tag_twin(row, c, rng, kinds)
        diff = np.nonzero(twin != row)[0]
        assert len(diff) and diff.min() >= 8 * c and diff.max() < 8 * c + 4, "only the first two words of the chunk differ"
        assert dr.row_tags(twin[None])[0] == dr.row_tags(row[None])[0]
        assert dr.small_and_finite(twin, kinds)
        for k in kinds:
            assert np.isfinite(dr.from_u16(twin, k)).all() and np.abs(dr.from_u16(twin, k)).max() < 8.0


@pytest.mark.parametrize("D", [8, 64, 128, 320, 768, 1152])
def test_row_with_tag_hits_any_tag(D):
    rng = np.random.default_rng(100 + D)
    row = dr.to_u16(np.clip(rng.standard_normal((1, D), dtype=np.float32), -7.5, 7.5), "f16")[0]
    t0 = int(dr.row_tags(row[None])[0])
    for c in dr.twin_chunks(D):
        for tag in (0, 0xFFFFFFFF, t0 ^ 0x81000000, int(rng.integers(0, 1 << 32))):
            got = dr.row_with_tag(row, tag, rng, c, ("f16",))
            assert int(dr.row_tags(got[None])[0]) == tag and dr.small_and_finite(got, ("f16",))
            assert (got[:8 * c] == row[:8 * c]).all() and (got[8 * c + 4:] == row[8 * c + 4:]).all()


def test_tags_restate_the_kernel_arithmetic_word_by_word():
    """row_tags against a scalar transcription of hash_rows_kernel in Python integers (lane-strided partial sums and all)."""
    rng = np.random.default_rng(7)
    for D in (8, 64, 320, 1152):
        q = rng.integers(0, 1 << 16, size=(3, D), dtype=np.uint16)
        for r in range(3):
            w = [int(v) for v in q[r].view("<u4")]
            lanes = [0] * 64
            for lane in range(64):
                for c in range(lane, D // 8, 64):
                    x, y, z, ww = w[4 * c:4 * c + 4]
                    m = (x * dr.K0 ^ y * dr.K1 ^ z * dr.K2 ^ ww * dr.K3) & dr.M32
                    lanes[lane] = (lanes[lane] + (m ^ (m >> 15)) * (2 * c + 1) + c * dr.KC) & dr.M32
            h = sum(lanes) & dr.M32
            assert int(dr.row_tags(q[r:r + 1])[0]) == h ^ (h >> 13)


def test_sample_positions():
    for Q in (0, 1, 8191, 8192):
        assert np.array_equal(dr.sample_positions(Q), np.arange(Q))
    assert np.array_equal(dr.sample_positions(8193), np.arange(8192))          # i * 8193 // 8192 = i: the last row is never seen
    assert np.array_equal(dr.sample_positions(16384), np.arange(0, 16384, 2))
    p = dr.sample_positions(20011)
    assert len(p) == 8192 and p[0] == 0 and p[-1] == 8191 * 20011 // 8192 and (np.diff(p) >= 2).all()


def test_plan_finds_the_most_repeated_exact_row():
    """Small Q, a pool of four rows with random multiplicities among singletons.  Where every distinct row has bits 0-11 of its tag
    to itself (then a bucket is a row and no two buckets can tie unless two rows do) and one row occurs more often than any other,
    the plan drops exactly its later occurrences; where no row occurs twice it drops nothing."""
    rng = np.random.default_rng(11)
    judged = 0
    for trial in range(300):
        Q, D = int(rng.integers(2, 60)), (8, 64, 128)[trial % 3]
        pool = dr.to_u16(rng.standard_normal((4, D), dtype=np.float32), "f16")
        q = dr.to_u16(rng.standard_normal((Q, D), dtype=np.float32), "f16")
        pick = rng.integers(0, 12, size=Q)
        q[pick < 4] = pool[pick[pick < 4]]
        sq = dr.sqnorm_bits(q, "f16")
        rows, inverse, counts = np.unique(q, axis=0, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
        low = dr.row_tags(rows) & np.uint32(4095)
        top = np.sort(counts)[::-1]
        if len(np.unique(low)) != len(rows) or (top[0] >= 2 and len(top) > 1 and top[0] == top[1]):
            continue
        judged += 1
        slot, kept, count = dr.plan(q, sq)
        expect = np.zeros(Q, bool)
        if top[0] >= 2:
            where = np.nonzero(inverse == int(np.argmax(counts)))[0]
            expect[where[1:]] = True
        dropped = np.ones(Q, bool)
        dropped[kept] = False
        assert np.array_equal(dropped, expect) and count == Q - expect.sum()
        if expect.any():
            assert (slot[expect] == where[0]).all()
    assert judged >= 150, judged


def _verdict(c, weak):
    """None if the weakened plan equals the reference plan and check_plan accepts it, else what gave it away."""
    q16, qsq = dr.case_tensors(c)
    ref = dr.plan(c.q, c.sq)
    got = dr.plan(c.q, c.sq, weak)
    try:
        dr.check_plan(dr.as_plan(*got, q16, qsq), q16, qsq, None)
    except (AssertionError, IndexError):
        return "rejected"
    if not (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]):
        return "differs"
    return None


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_plan_of_every_case_is_valid_and_has_the_stated_outcome(c):
    q16, qsq = dr.case_tensors(c)
    slot, rows, count = dr.plan(c.q, c.sq)
    assert dr.check_plan(dr.as_plan(slot, rows, count, q16, qsq), q16, qsq, None) == count
    assert c.Q - count == c.dropped, "rows saved (0: the documented cost, no saving)"
    assert np.isfinite(dr.from_u16(c.q, c.kind)).all() and np.isfinite(c.sq.view(np.float32)).all()
    assert np.array_equal(dr.row_tags(c.q), dr.row_tags(c.q.copy()))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_case_catches_a_weakened_plan(c):
    bitten = {w for w in dr.WEAKENINGS if _verdict(c, w) is not None}
    assert c.bites <= bitten, (c.name, sorted(c.bites - bitten))
    if c.toothless is None:
        assert bitten, "no weakening fails this case: fix it or remove it"
    else:
        assert not bitten and not c.bites, c.toothless


def test_every_weakening_is_caught_by_some_case_and_the_exemptions_are_the_stated_ones():
    for w in dr.WEAKENINGS:
        assert any(w in c.bites for c in CASES), w
    assert sorted(c.name for c in CASES if c.toothless) == sorted(["block_Q0-D128-f16", "block_Q1-D768-f16", "no_repeats_Q1024-D768-f16"])


def test_case_table_holds_what_the_issue_lists():
    names = set(IDS)
    for D in (128, 768):
        for kind in dr.KINDS:
            assert {c.Q - c.dropped for c in CASES if c.name.startswith(f"twins_D{D}-{kind}-live")} == {255, 256, 257}
    assert all(f"twins_D{D}-{k}" in names for D in (8, 64, 320, 1152) for k in dr.KINDS)
    assert dr.twin_chunks(768) == [0, 63, 64, 95] and dr.twin_chunks(1152) == [0, 63, 64, 128, 143]
    assert [c.Q for c in CASES if c.name.startswith("block_Q")] == [0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049]
    assert [c.Q for c in CASES if c.name.startswith("shares_30_20")] == [8191, 8192, 8193, 20011]
    assert {c.Q for c in CASES if c.name.startswith("all_identical")} == {1025, 4096}
    assert all(c.Q <= 20011 for c in CASES)
    assert all(c.D in (128, 768) for c in CASES if c.search)


@pytest.mark.parametrize("c", [c for c in CASES if hasattr(c, "tie")], ids=lambda c: c.name)
def test_tie_cases_tie_and_the_lower_bucket_wins(c):
    tag_w, tag_l, round2 = c.tie
    tags = dr.row_tags(c.q)
    key = (lambda t: (t >> 12) & 0xFFF) if round2 else (lambda t: t & 0xFFF)
    assert key(tag_w) < key(tag_l) and (not round2 or (tag_w & 0xFFF) == (tag_l & 0xFFF))
    if round2:
        inside = tags[(tags & np.uint32(0xFFF)) == (tag_w & 0xFFF)]
        cnt = np.bincount((inside >> np.uint32(12)) & np.uint32(0xFFF), minlength=4096)
    else:
        cnt = np.bincount(tags & np.uint32(0xFFF), minlength=4096)
    assert cnt[key(tag_w)] == cnt[key(tag_l)] == cnt.max() == 300
    full, twice = dr.pick_rep(tags)
    assert twice and full == tag_w
    if "later" in c.name:
        assert np.nonzero(tags == np.uint32(tag_l))[0][0] < np.nonzero(tags == np.uint32(tag_w))[0][0]


def test_unsampled_and_prefix_mate_cases_show_the_documented_cost():
    for kind in dr.KINDS:
        c = dr.case(f"repeats_on_unsampled_rows-{kind}")
        rows, counts = np.unique(c.q, axis=0, return_counts=True)
        assert counts.max() > 4000 and dr.plan(c.q, c.sq)[2] == c.Q
        c = dr.case(f"prefix_mate_in_front-{kind}")
        tags = dr.row_tags(c.q)
        full, twice = dr.pick_rep(tags)
        assert twice and full == int(tags[7]) and (tags == np.uint32(full)).sum() == 2
        mates = (tags & np.uint32(0xFFFFFF)) == (full & 0xFFFFFF)
        assert mates.sum() > 800 and dr.plan(c.q, c.sq)[2] == c.Q


def test_draws_needed_by_the_crafting_helpers():
    """Recorded for the summary; bounded because an acceptable y' has a chance of about one in four per draw."""
    d = dr.CASE_DRAWS
    assert d and min(d) >= 1 and max(d) <= 200, (min(d), max(d))
    print(f"crafted rows of the case table: {len(d)}, draws min {min(d)} max {max(d)}")
