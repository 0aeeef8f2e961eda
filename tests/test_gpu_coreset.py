"""GPU: the greedy coreset kernels (csrc/coreset.hip) against tests/coreset_ref.py, off the one friendly shape the suite had.

FP16 path: EXACT equality of the picks.  The round kernel's arithmetic is restated operation by operation (coreset_ref's module
docstring says why equality is a theorem), and the one thing that cannot be restated, the summation order of the initial fp32
distances, is taken out of the comparison by a condition on the INPUT: every row's float64 initial distance is asserted (on the
CPU, for every row, before a pick is compared) to lie further than 1e-5 relative from any fp16 rounding midpoint, while the
kernel's fp32 value is within (d/64 + 9) * 2^-24 < 2e-6 of it.  Inputs are seeded random rows passed through
coreset_ref.snap_initial_distances (which puts every initial distance on an fp16 grid point: see there why no seed alone can).

TF32 path: fp32 sums in an order that is not specified, so the property is the float64 greedy rule: every pick attains the
largest running minimum to 1e-5 relative (the existing test's property, at the shapes it does not visit)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreset_ref as cr  # noqa: E402
from cmdiad_amd import _native as nat  # noqa: E402
from cmdiad_amd import coreset  # noqa: E402

DEV = "cuda"
MARGIN = 1e-5


def _rows(n, d, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return cr.snap_initial_distances((scale * g.standard_normal((n, d))).astype(np.float32))


def _guard(z):
    """The condition on the input: EVERY row (none excluded) is clear of the fp16 rounding midpoints."""
    m = cr.midpoint_margin(cr.initial_distances64(z))
    assert m.shape == (z.shape[0],) and float(m.min()) > MARGIN, float(m.min())


def _clustered(n, d, seed):
    """A patch library's structure: few centres, rows close to them, runs of exact duplicates, zero rows.  Row 0 is a zero row, so
    that the snapping (a rescaling about row 0) keeps zero rows zero."""
    g = np.random.default_rng(seed)
    centres = 3.0 * g.standard_normal((40, d))
    z = (centres[g.integers(0, 40, n)] + 0.3 * g.standard_normal((n, d))).astype(np.float32)
    z[0] = 0.0
    z[n // 6: n // 6 + 700] = z[n // 6 - 1]            # a run of identical rows (crosses a 1024-row block)
    z[n // 2: n // 2 + 301] = 0.0                      # zero rows: duplicates of row 0, initial distance exactly 0
    z[n - 3] = z[7]
    z = cr.snap_initial_distances(z)
    assert not z[n // 2: n // 2 + 301].any() and np.array_equal(z[n - 3], z[7]) and np.array_equal(z[n // 6 + 699], z[n // 6 - 1])
    return z


# n: a single group of four with a ragged tail (5), one block with a ragged last group (257, 1021), five blocks with a ragged last
# group (4099: 1025 groups).  d: one pair (2), 31 pairs (62: the last chunk of eight zero-padded), odd (63: padded in Python),
# 167 pairs (334, production), 512 pairs (1024: the pivot row fills s_piv).  Every value at least once, the corners together.
@pytest.mark.parametrize("n,d,n_select,seed", [(5, 2, 5, 0), (5, 1024, 5, 1), (257, 62, 120, 2), (257, 1024, 60, 3), (1021, 63, 150, 4),
                                               (1021, 2, 60, 5), (4099, 334, 120, 6), (4099, 1024, 40, 7), (4099, 63, 100, 8)])
def test_fp16_picks_equal_the_restatement(n, d, n_select, seed):
    z = _rows(n, d, seed)
    _guard(z)
    want = cr.greedy_fp16(z, n_select)
    got = coreset.greedy_coreset(torch.from_numpy(z).to(DEV), n_select).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def test_dimension_above_1024_is_an_argument_error():
    z = torch.zeros((8, 1026), device=DEV)
    with pytest.raises(nat.NativeError):
        coreset.greedy_coreset(z, 2)
    with pytest.raises(nat.NativeError):
        coreset.greedy_coreset(z, 2, "TF32")
    with pytest.raises(nat.NativeError):
        coreset._HipRounds(z)


_CLUSTERED = {}


def _clustered_case():
    if not _CLUSTERED:
        z = _clustered(6000, 334, 17)
        _guard(z)
        _CLUSTERED["z"], _CLUSTERED["want"] = z, cr.greedy_fp16(z, 400)
    return _CLUSTERED["z"], _CLUSTERED["want"]


@pytest.mark.parametrize("early", ["1", "0"])
def test_clustered_rows_with_duplicates_both_scan_variants(early, monkeypatch):
    """The partial-distance exit (CMDIAD_CORESET_EARLY, read per call) and the full scan, each against the restatement -- not
    against each other."""
    z, want = _clustered_case()
    monkeypatch.setenv("CMDIAD_CORESET_EARLY", early)
    got = coreset.greedy_coreset(torch.from_numpy(z).to(DEV), 400).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert len(set(want.tolist())) == 400


def test_select_every_row_of_data_with_duplicates():
    """n_select = n with fewer distinct rows than rows: once every running minimum is 0 the first arg-max is row 0, again and
    again (the reference's torch.argmax does the same)."""
    n, d = 257, 62
    z = _rows(n, d, 21)
    z[200:] = z[3]
    z[100:120] = z[0]
    _guard(z)
    distinct = len({r.tobytes() for r in z})
    want = cr.greedy_fp16(z, n)
    assert len(set(want[:distinct].tolist())) == distinct and not want[distinct:].any()      # the restatement itself: then row 0
    got = coreset.greedy_coreset(torch.from_numpy(z).to(DEV), n).cpu().numpy()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("dtype", ["FP16", "TF32"])
def test_select_one(dtype):
    z = torch.from_numpy(_rows(1021, 62, 22)).to(DEV)
    assert coreset.greedy_coreset(z, 1, dtype).cpu().tolist() == [0]


@pytest.mark.parametrize("n,W", [(4099, 3), (4099, 5), (1021, 7), (5, 3)])
def test_sharded_rounds_on_one_device_equal_the_restatement(n, W):
    """cmdiad_coreset_prepare / _round / _decode: W ranks (each with its own workspace, as W processes would have) scan their
    shard_rows ranges, torch.maximum of their keys stands in for the all_reduce(MAX).  (5, 3): rank 1 owns the ragged group
    [4, 5) and rank 2 an EMPTY range; (1021, 7): the last rank's range ends at n inside a group of four."""
    d, n_select = 334, min(n, 100)
    z = _rows(n, d, 30 + W)
    _guard(z)
    want = cr.greedy_fp16(z, n_select)
    bounds = [coreset.shard_rows(n, r, W) for r in range(W)]
    assert bounds[0][0] == 0 and max(b[1] for b in bounds) == n and all(b[0] % 4 == 0 for b in bounds)
    assert sum(b[1] - b[0] for b in bounds) == n
    if n == 5:
        assert bounds[2][0] == bounds[2][1]
    zd = torch.from_numpy(z).to(DEV)
    ranks = [coreset._HipRounds(zd) for _ in range(W)]
    keys = torch.zeros((max(n_select - 1, 1),), dtype=torch.int64, device=DEV)
    for r in range(n_select - 1):
        best = torch.zeros((1,), dtype=torch.int64, device=DEV)
        for w in range(W):
            mine = torch.zeros((1,), dtype=torch.int64, device=DEV)
            ranks[w].round(bounds[w][0], bounds[w][1], keys[r - 1:r] if r else None, mine)
            best = torch.maximum(best, mine)       # keys are non-negative as int64: signed MAX == unsigned MAX
        keys[r] = best[0]
    got = ranks[0].decode(keys, n_select).cpu().numpy()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("n,d,n_select,seed", [(1021, 7, 200, 40), (1021, 1024, 80, 41), (4099, 7, 150, 42)])
def test_tf32_picks_follow_the_float64_greedy_rule(n, d, n_select, seed):
    """fp32 scan: every pick is an arg-max of the float64 running minimum to 1e-5 relative (fp32 sums of d <= 1024 squares are
    within (d + 2) * 2^-24 < 7e-5 in the worst case and ~sqrt(d) * 2^-24 in practice; 1e-5 is the bound the existing test
    set for this property and is kept)."""
    z = (np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)
    picks = coreset.greedy_coreset(torch.from_numpy(z).to(DEV), n_select, "TF32").cpu().tolist()
    assert picks[0] == 0 and len(set(picks)) == n_select
    z64 = z.astype(np.float64)
    min_d = np.sqrt(((z64 - z64[0:1]) ** 2).sum(1))
    for i in picks[1:]:
        assert min_d[i] >= min_d.max() * (1 - 1e-5)
        min_d = np.minimum(min_d, np.sqrt(((z64 - z64[i:i + 1]) ** 2).sum(1)))
