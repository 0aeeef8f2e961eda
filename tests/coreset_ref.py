"""Numpy restatement of the greedy k-centre selection of csrc/coreset.hip (reference features.py:372-425, coreset_dtype 'FP16'), in
the KERNEL'S DOCUMENTED ORDER OF OPERATIONS, so that the picks can be compared for equality and not "to round-off".  TEST
INFRASTRUCTURE ONLY: plain numpy, no code shared with cmdiad_amd.

A round, for every row i against the pivot row p (the previous pick):
  1. the difference z16[i] - z16[p] ROUNDED TO fp16 (one rounding: taken in float64, where the difference of two halves is exact);
  2. acc = acc + (x*x + y*y) in fp32, one dimension PAIR (x, y) after the other, in increasing dimension.  x and y are halves, so
     x*x and y*y are exact in fp32 (22 significant bits) and x*x + y*y carries exactly one rounding whether the compiler emits
     mul + add or an fma: contraction cannot change a bit, and neither can the zero-padded tail of the kernel's last chunk of
     eight pairs (acc + 0 = acc).  The partial-distance exit only leaves rows whose minimum cannot change.
  3. dist = fp16(sqrt_fp32(acc)), min_d = min(min_d, dist) in fp16, next pick = the FIRST arg-max of min_d.
Hence equality of the picks with this restatement is a theorem about the round kernel, not an observation.

What cannot be restated is the summation order of the INITIAL distances (fp32 rows, fp32 sum over a wave's 64 lanes and a
butterfly; features.py:378 runs before the .half()).  They are taken in float64 here and rounded to fp16 once; the kernel's fp32
value differs from the float64 one by at most (d/64 + 6 + 3) * 2^-24 < 2e-6 relative at d <= 1024, so both round to the same
half whenever the float64 value is not within 1e-5 (relative) of an fp16 rounding midpoint -- a CONDITION ON THE INPUT that
`midpoint_margin` measures for every row and the tests assert before they look at a pick.  A band of +-1e-5 around the midpoints
covers 2-4 % of the axis (half spacing is 2^-11 .. 2^-10 relative), so a cloud of a thousand random rows never satisfies it by
the choice of a seed; `snap_initial_distances` therefore CONDITIONS the input: it rescales every row about row 0 so that its
initial distance sits on an fp16 grid point (half a spacing from both midpoints), leaving directions, duplicates and zero
distances as they were."""
import numpy as np


def _np(x, dtype=None):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    return x.astype(dtype) if dtype is not None else x


def initial_distances64(z32, first=0):
    """|| z_i - z_first ||_2 of the fp32 rows, in float64."""
    z = _np(z32, np.float32).astype(np.float64)
    df = z - z[first:first + 1]
    return np.sqrt(np.einsum("ij,ij->i", df, df))


def midpoint_margin(d64):
    """Per value: |d - m| / m for the nearest fp16 rounding midpoint m (inf for d == 0, which is exact in every format)."""
    d = np.asarray(d64, np.float64)
    with np.errstate(over="ignore"):
        h = d.astype(np.float16)
    assert np.all(np.isfinite(h)), "initial distance beyond the half range"
    hd = h.astype(np.float64)
    other = np.where(d >= hd, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))).astype(np.float64)
    other = np.where(np.isfinite(other), other, hd)
    mid = 0.5 * (hd + other)                     # the midpoint on d's side of its nearest half
    out = np.full(d.shape, np.inf)
    nzero = d > 0
    out[nzero] = np.abs(d[nzero] - mid[nzero]) / mid[nzero]
    return out


def snap_initial_distances(z32, first=0):
    """z [n, d] fp32 -> fp32 rows z_first + (z_i - z_first) * fp16(d_i) / d_i: every initial distance on an fp16 grid point (to
    fp32 round-off of the rows, ~1e-7 relative), rows at distance 0 untouched, equal rows stay equal."""
    z = _np(z32, np.float32).astype(np.float64)
    d = initial_distances64(z32, first)
    t = d.astype(np.float16).astype(np.float64)
    s = np.ones_like(d)
    s[d > 0] = t[d > 0] / d[d > 0]
    out = z[first:first + 1] + (z - z[first:first + 1]) * s[:, None]
    out[first] = z[first]
    return out.astype(np.float32)


def round_distances(zh, pivot):
    """One round's fp16 distances of the half rows zh [n, d] (d even) to zh[pivot]: steps 1-3 of the module docstring."""
    n, d = zh.shape
    assert d % 2 == 0 and zh.dtype == np.float16
    with np.errstate(over="ignore"):
        df = (zh.astype(np.float64) - zh[pivot].astype(np.float64)[None, :]).astype(np.float16)
    assert np.all(np.isfinite(df)), "a difference left the half range: outside what the restatement states"
    sq = np.ascontiguousarray(df.T).astype(np.float32)
    sq *= sq                                     # squares of halves: exact in fp32
    pair = sq[0::2] + sq[1::2]                   # [d/2, n]: x*x + y*y, one fp32 rounding
    acc = np.zeros((n,), np.float32)
    for c in range(d // 2):
        acc += pair[c]                           # sequential over the dimension pairs, fp32 (float32 + float32 stays float32)
    assert acc.dtype == np.float32 and pair.dtype == np.float32
    return np.sqrt(acc).astype(np.float16)


def greedy_fp16(z32, n_select, first=0, return_min_d=False):
    """z [n, d] fp32 -> picks [n_select] int64 of cmdiad_coreset_greedy (an odd d gets a zero column, as coreset.greedy_coreset
    pads it)."""
    z = _np(z32, np.float32)
    n, d = z.shape
    if d % 2:
        z = np.concatenate([z, np.zeros((n, 1), np.float32)], 1)
    assert 0 < n_select <= n
    zh = z.astype(np.float16)
    min_d = initial_distances64(z, first).astype(np.float16)
    picks = [first]
    last = first
    for _ in range(n_select - 1):
        min_d = np.minimum(min_d, round_distances(zh, last))
        last = int(np.argmax(min_d))             # first occurrence of the maximum
        picks.append(last)
    picks = np.asarray(picks, np.int64)
    return (picks, min_d) if return_min_d else picks
