"""CPU: the preconditions of tests/test_gpu_search_exact.py, checked on the very operands and references of tests/search_ref.py.

The GPU file demands torch.equal on both key planes.  That is only a statement about the kernels if (1) the reference is the
definition -- held here to a plain double loop on hand-made libraries --, (2) the operands sit on the lattice on which the search's
accumulator is exact in fp32 in every order and loses nothing to the 4-bit truncation, (3) exact ties really occur, and often with
the second-nearest row INSIDE the winner's group, and (4) the packed layout is the one ops.unpack_keys takes apart."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_ref as sr  # noqa: E402

SHAPES = [(c.Q, c.Nb, c.D) for c in sr.EDGE_CASES]


# ------------------------------------------------------------------------------------------------ the definition, as a double loop
def _loop_keys(q, b, row_offset):
    """[[plane 0], [plane 1]] as (d2, R) tuples or None, element by element"""
    def group(R):
        return (R >> 6, (R >> 2) & 3)
    best, runner = [], []
    for qi in q:
        cand = []
        for r, br in enumerate(b):
            d2 = 0
            for x, y in zip(qi, br):
                d2 += (x - y) * (x - y)
            cand.append((d2, row_offset + r))
        first = min(cand)
        others = [c for c in cand if group(c[1]) != group(first[1])]
        best.append(first)
        runner.append(min(others) if others else None)
    return best, runner


def _loop_top3(p, b, row_offset):
    out = []
    for pi in p:
        cand = sorted((sum((x - y) * (x - y) for x, y in zip(pi, br)), row_offset + r) for r, br in enumerate(b))
        out.append((cand + [None, None, None])[:3])
    return out


def _key(c):
    if c is None:
        return sr.KEY_EMPTY
    return (int(np.float32(c[0]).view(np.uint32)) << 32) | c[1]


def _rows(n, D, seed):
    return np.random.RandomState(seed).randint(-4, 5, (n, D)).tolist()


def _hand_made():
    """(name, q, b, row_offset, what plane 0 / plane 1 must name, or None to leave it to the loop)"""
    D = 8
    # a library inside ONE group (rows 0..3, and at offset 64 rows 64..67): no runner-up
    one = _rows(4, D, 1)
    yield "one group", [one[2], one[0], _rows(1, D, 2)[0]], one, 0, None, [None, None, None]
    yield "one group at offset 64", [one[2], one[0]], one, 64, None, [None, None]
    # a duplicate inside the winner's quad: rows 4 and 5 are the query; the runner-up is neither, although row 5 is second nearest
    quad = _rows(24, D, 3)
    quad[5] = list(quad[4])
    near = list(quad[4]); near[0] += 1 if near[0] < 4 else -1
    quad[17] = near                                            # group (0, 0): rows 0-3, 16-19, ... -- row 17 is outside (0, 1)
    yield "duplicate in the quad", [quad[4]], quad, 0, [(0, 4)], [(1, 17)]
    # a duplicate 16 rows down: rows 3 and 19 share group (0, 0); the nearest outside is row 36 at d2 = 4, not row 19 at 0
    down = _rows(40, D, 4)
    down[19] = list(down[3])
    far = list(down[3]); far[1] += 2 if far[1] < 3 else -2
    down[36] = far
    down[8] = list(far)                                        # ... and its copy at the LOWER row 8 (group (0, 2)) wins the tie
    yield "duplicate 16 rows down", [down[3], down[19]], down, 0, [(0, 3), (0, 3)], [(4, 8), (4, 8)]
    # the same across a 64-block boundary: offset 192, winner row 192 + 3, rows in the next block are another group
    yield "duplicate 16 rows down at offset 192", [down[3]], down, 192, [(0, 195)], [(4, 200)]


@pytest.mark.parametrize("name,q,b,row_offset,want0,want1", list(_hand_made()), ids=[h[0] for h in _hand_made()])
def test_reference_is_the_definition_on_hand_made_libraries(name, q, b, row_offset, want0, want1):
    best, runner = _loop_keys(q, b, row_offset)
    if want0 is not None:
        assert best == want0, (best, want0)
    assert runner == want1, (runner, want1)
    ref = sr.reference_keys(torch.tensor(q), torch.tensor(b), row_offset)
    assert ref.dtype == torch.int64 and ref.shape == (2, len(q))
    assert ref[0].tolist() == [_key(c) for c in best] and ref[1].tolist() == [_key(c) for c in runner]
    top = sr.reference_top3(torch.tensor(q), torch.tensor(b), row_offset)
    assert top.tolist() == [[_key(c) for c in row] for row in _loop_top3(q, b, row_offset)]
    assert torch.equal(top[:, 0], ref[0])                       # the scan's first slot is the search's plane 0


def test_reference_top3_leaves_key_empty_below_three_rows():
    b = _rows(2, 8, 5)
    top = sr.reference_top3(torch.tensor([b[1]]), torch.tensor(b))
    assert top.tolist() == [[_key((0, 1)), _key(_loop_top3([b[1]], b, 0)[0][1]), sr.KEY_EMPTY]]
    assert sr.reference_top3(torch.tensor([b[0]]), torch.tensor(b[:1])).tolist() == [[_key((0, 0)), sr.KEY_EMPTY, sr.KEY_EMPTY]]


@pytest.mark.parametrize("shape", [(17, 17, 128), (129, 65, 192), (257, 257, 256)])
def test_reference_matches_the_loop_on_table_cases(shape):
    """the vectorised reference against the loop on whole (small) table cases, at both two-plane offsets"""
    c = sr.case_of(*shape)
    q, b = sr.operands(c.Q, c.Nb, c.D, c.amp)
    qs = q[::16] if c.Q > 64 else q                              # (the loop is plain Python: a sample of the query rows)
    for row_offset in (0, 192):
        best, runner = _loop_keys(qs.tolist(), b.tolist(), row_offset)
        ref = sr.reference_keys(qs, b, row_offset)
        assert ref[0].tolist() == [_key(k) for k in best] and ref[1].tolist() == [_key(k) for k in runner]
        assert torch.equal(sr.shifted(sr.reference_keys(qs, b, 0), row_offset), ref)


# ------------------------------------------------------------------------------------------------ the tables
def test_case_tables_hold_what_the_issue_lists():
    assert SHAPES == [(1, 1, 64), (1, 4, 64), (1, 5, 64), (17, 17, 128), (127, 63, 64), (128, 64, 128), (129, 65, 192), (255, 255, 192),
                      (256, 256, 192), (257, 257, 256), (511, 511, 320), (512, 512, 192), (513, 513, 320), (300, 1025, 64),
                      (513, 1279, 256), (769, 2305, 192), (513, 6018, 192), (260, 1024, 1024), (1, 2305, 256)]
    assert all(c.amp in (1, 2, 4) for c in sr.EDGE_CASES) and sr.SETTINGS == (None, "0", "5") and sr.AB_SETTING == "2"
    assert sr.COUNTED_Q_MAX == 513 and sr.COUNTED_COUNTS == (0, 1, 127, 128, 129, 255, 256, 257, 512, 513)
    assert max(sr.COUNTED_COUNTS) <= sr.COUNTED_Q_MAX           # the caller's contract: beyond it the kernel would write past the arrays
    assert sr.SEGMENT_STRIDE == 300 and sr.SEGMENT_COUNTS == ((0, 300, 1, 257, 129), (300, -3, 999, 256, 0))
    for (Q, Nb, D), cuts in sr.SHARD_CASES:
        sizes = [hi - lo for lo, hi in zip(cuts, cuts[1:])]
        assert cuts[0] == 0 and cuts[-1] == Nb and all(c % 64 == 0 for c in cuts[:-1]) and 64 in sizes and 0 in sizes and min(sizes) >= 0
    assert [s for s, _ in sr.SHARD_CASES] == [(769, 2305, 192), (513, 1279, 256)]
    assert sr.SCAN_NB == (1, 2, 3, 15, 16, 17, 257, 4001) and sr.SCAN_D == (128, 768) and sr.SCAN_R == (1, 5, 32) and sr.SCAN_COPIES == 9


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{Q}x{Nb}x{D}" for Q, Nb, D in SHAPES])
def test_operands_sit_on_the_lattice_and_every_accumulator_value_is_exact(shape):
    c = sr.case_of(*shape)
    q, b = sr.operands(c.Q, c.Nb, c.D, c.amp)
    assert q.dtype == torch.int64 and b.dtype == torch.int64 and q.shape == (c.Q, c.D) and b.shape == (c.Nb, c.D)
    assert c.D <= sr.MAX_D and c.D % 64 == 0 and c.amp <= sr.MAX_ABS
    assert int(q.abs().max()) <= c.amp and int(b.abs().max()) <= c.amp
    for x in (q, b):                                            # exact in both operand types, norms exact in fp32
        assert torch.equal(x.to(torch.bfloat16).long(), x) and torch.equal(x.to(torch.float16).long(), x)
        assert torch.equal(sr.sqnorm(x).long(), (x * x).sum(1)) and int((x * x).sum(1).max()) <= 16384
    # the accumulator walks from -(|q|^2 + |b|^2) / 2 to -d2 / 2 in steps of integer products: whatever the order, each value is a
    # multiple of 1/2 with magnitude <= (|q|^2 + |b|^2) / 2 + sum_k |q_k b_k| -- below 2^16, so at most 17 significant bits: exact
    # in fp32 with the low four (of 24) mantissa bits zero
    bound = ((q * q).sum(1).max() + (b * b).sum(1).max()) / 2 + (q.abs().max(0).values * b.abs().max(0).values).sum()
    assert float(bound) < 2 ** 16
    d2 = sr.distances(q, b)
    a = (-0.5 * d2.double()).float()                             # the finished accumulator
    assert torch.equal(a.double(), -0.5 * d2.double()) and not bool((a.view(torch.int32) & 15).any())
    assert torch.equal((-2.0 * a).long(), d2)                    # rowmin_key's d2, and a key's value as ops.unpack_keys reads it
    # the expansion the reference computes in is the plain sum of squared differences
    assert torch.equal(d2[:7], (q[:7, None, :] - b[None, :, :]).pow(2).sum(-1))


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{Q}x{Nb}x{D}" for Q, Nb, D in SHAPES])
def test_ties_occur_and_the_second_nearest_often_shares_the_winners_group(shape):
    c = sr.case_of(*shape)
    if c.Nb < 2:
        return
    q, b = sr.operands(c.Q, c.Nb, c.D, c.amp)
    tied, inside = sr.tie_shares(q, b)
    ref = sr.case_reference(*shape)
    print(f"[{shape}: tied minimum {tied:.2f}, second nearest inside the winner's group {inside:.2f}, "
          f"runner-up empty {(ref[1] == sr.KEY_EMPTY).float().mean().item():.2f}]")
    if c.Q >= 100 and c.Nb >= 64:
        assert tied >= 0.25, tied
        assert inside >= 0.20, inside
    assert bool((ref[1] > ref[0]).all())
    assert bool((ref[1] == sr.KEY_EMPTY).all()) == (c.Nb <= 4)  # a runner-up exists as soon as the library leaves one group


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{Q}x{Nb}x{D}" for Q, Nb, D in SHAPES])
def test_every_edge_row_is_the_only_winner_of_its_query(shape):
    """the rows at which a tiling can lose a row -- the last one, row 0, either side of the tile and range boundaries -- each win
    a query outright (d2 = 0, no other row at 0): a search that drops one of them differs from the reference in plane 0"""
    c = sr.case_of(*shape)
    q, b = sr.operands(c.Q, c.Nb, c.D, c.amp)
    edges = sr.edge_rows(c.Nb, c.Q // 8)
    ref = sr.case_reference(*shape)
    assert ref[0][:len(edges)].tolist() == edges                                  # d2 bits 0, row = the edge row
    assert bool((sr.distances(q[:len(edges)], b) == 0).sum(1).eq(1).all())
    if c.Q >= 100:
        assert {c.Nb - 1, 0} <= set(edges)
        full = c.Nb // 256 * 256                                                   # the cut between the two launches of tile 5
        assert full in (0, c.Nb) or {full - 1, full} <= set(edges)
        bounds256 = [t for t in range(256, c.Nb, 256)]
        assert len(edges) == c.Q // 8 or all({t - 1, t} <= set(edges) for t in bounds256)
    # the plan labels' range boundaries of the two-group launch (ranges of per tiles of 256 rows) are multiples of 256
    assert sr.edge_rows(2305, 96)[:6] == [2304, 0, 2303, 2047, 2048, 1791] and sr.edge_rows(300, 9) == [299, 0, 255, 256, 127, 128]
    assert sr.edge_rows(1, 5) == [0] and sr.edge_rows(64, 16) == [63, 0] and sr.edge_rows(6018, 0) == []


# ------------------------------------------------------------------------------------------------ the packed layout
def test_packed_layout_is_what_unpack_keys_takes_apart():
    """ops.unpack_keys restated in numpy: index = key & 0xFFFFFFFF, value = the float32 whose bits are key >> 32"""
    q, b = sr.operands(*sr.case_of(129, 65, 192)[:4])
    for row_offset in (0, 192):
        ref = sr.reference_keys(q, b, row_offset).numpy()
        idx = ref & 0xFFFFFFFF
        val = (ref >> 32).astype(np.int32).view(np.float32)
        d2 = sr.distances(q, b).numpy()
        r0 = idx[0] - row_offset
        assert np.array_equal(val[0].astype(np.int64), d2[np.arange(len(r0)), r0]) and np.array_equal(val[0], d2.min(1).astype(np.float32))
        assert np.array_equal(val[1].astype(np.int64), d2[np.arange(len(r0)), idx[1] - row_offset])
        assert idx.min() >= row_offset and idx.max() < row_offset + b.shape[0]
        # integer order of the keys = (value, row) order: the key of the minimum is the minimum of the keys
        allk = sr.pack(torch.from_numpy(d2), row_offset + torch.arange(b.shape[0])[None, :].expand(d2.shape)).numpy()
        assert np.array_equal(allk.min(1), ref[0]) and ref.max() < sr.KEY_EMPTY
    assert sr.KEY_EMPTY == 2 ** 63 - 1 and int(sr.pack(torch.tensor([65536]), torch.tensor([2 ** 32 - 1]))[0]) == (0x47800000 << 32 | 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the scan's operands
@pytest.mark.parametrize("Nb", sr.SCAN_NB)
def test_scan_operands_are_exact_and_probe_zero_has_nine_copies(Nb):
    for D in sr.SCAN_D:
        p, b = sr.scan_operands(Nb, D, 32)
        assert int(p.abs().max()) <= sr.MAX_ABS and int(b.abs().max()) <= sr.MAX_ABS
        # |p|^2 + |b|^2 - 2 p.b: integers below 2^24 at every step
        assert int((p * p).sum(1).max() + (b * b).sum(1).max() + 2 * (p.abs().max(0).values * b.abs().max(0).values).sum()) < 2 ** 24
        copies = int((sr.distances(p[:1], b) == 0).sum())
        assert copies >= min(sr.SCAN_COPIES, Nb)
        top = sr.reference_top3(p, b)
        assert bool(((top[0] >> 32) == 0)[:min(3, Nb)].all()) and bool((top[:, min(3, Nb):] == sr.KEY_EMPTY).all())
        assert bool((top[:, 1:] > top[:, :-1])[:, :min(3, Nb) - 1].all())
        if Nb > sr.SCAN_COPIES:                                  # the last row of the ragged last group of 16 wins probe 1 alone
            assert int(top[1, 0]) == Nb - 1 and int(top[1, 1]) >> 32 != 0
