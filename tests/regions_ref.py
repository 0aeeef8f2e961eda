"""The yardstick of the region tables (docs/regions.md): numpy and scipy only -- scipy.ndimage.label with the 3 x 3 structure and
per-label numpy loops.  Not a test file; tests/test_regions_cpu.py validates it against scipy's own helpers, the GPU tests hold
the kernels to it."""
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

STRUCTURE = np.ones((3, 3), dtype=int)
INT_FIELDS = ("label", "area", "x0", "y0", "x1", "y1", "peak_x", "peak_y")
VAL_FIELDS = ("peak", "score_sum", "cx", "cy")


def threshold(maps, thr):
    """maps [n,H,W] f64, thr a float or [n] -> (mask [n,H,W] uint8 = maps > thr as doubles, number of NaN scores).  A NaN compares
    false and stays background; -0.0 > +0.0 is false."""
    maps = np.asarray(maps, dtype=np.float64)
    t = np.asarray(thr, dtype=np.float64).reshape(-1)
    t = t.reshape(-1, 1, 1) if t.size > 1 else t[0]
    with np.errstate(invalid="ignore"):
        mask = (maps > t).astype(np.uint8)
    return mask, int(np.isnan(maps).sum())


def components(score, mask):
    """One image -> (labels [H,W], list of region dicts in label order, every field of the contract; score_sum by math.fsum, with
    "values": the component's scores in raster order)."""
    labels, n = ndimage.label(mask, STRUCTURE)
    out = []
    for lab, box in zip(range(1, n + 1), ndimage.find_objects(labels)):   # (the box only bounds the search: 12 544 labels stay quick)
        ys, xs = np.nonzero(labels[box] == lab)        # raster order
        ys, xs = ys + box[0].start, xs + box[1].start
        v = score[ys, xs]
        first = int(np.flatnonzero(v == v.max())[0])   # -0.0 == +0.0: the first pixel that EQUALS the largest score
        area = int(v.size)
        out.append(dict(label=lab, area=area, x0=int(xs.min()), y0=int(ys.min()), x1=int(xs.max()), y1=int(ys.max()),
                        peak=float(v[first]), peak_x=int(xs[first]), peak_y=int(ys[first]),
                        cx=float(np.float64(int(xs.astype(np.int64).sum())) / np.float64(area)),
                        cy=float(np.float64(int(ys.astype(np.int64).sum())) / np.float64(area)),
                        score_sum=math.fsum(v.tolist()), values=v.copy()))
    return labels, out


def region_table(maps, thr, min_area=1, max_regions=16):
    """-> dict(n_comp [n], count [n], ints [n,K,8] int32, vals [n,K,4] f64, truncated [n] bool, nan, regions: per image the KEPT
    region dicts in table order, all: per image every component)."""
    maps = np.asarray(maps, dtype=np.float64)
    mask, nan = threshold(maps, thr)
    n, K = maps.shape[0], max_regions
    res = dict(n_comp=np.zeros(n, np.int32), count=np.zeros(n, np.int32), ints=np.zeros((n, K, 8), np.int32),
               vals=np.zeros((n, K, 4), np.float64), nan=nan, regions=[], all=[])
    for i in range(n):
        _, comps = components(maps[i], mask[i])
        res["all"].append(comps)
        res["n_comp"][i] = len(comps)
        keep = [c for c in comps if c["area"] >= min_area]
        res["count"][i] = len(keep)
        keep.sort(key=lambda c: (-(c["peak"] + 0.0), c["label"]))      # + 0.0: -0.0 and +0.0 are one peak
        keep = keep[:K]
        res["regions"].append(keep)
        for k, c in enumerate(keep):
            res["ints"][i, k] = [c[f] for f in INT_FIELDS]
            res["vals"][i, k] = [c[f] for f in VAL_FIELDS]
    res["truncated"] = res["count"] > K
    return res


def quantile_index(q, n):
    """ceil(q n) - 1 clamped to [0, n - 1], in Python integers: q is taken as the exact value of the double."""
    f = Fraction(float(q)) * n
    return min(max(-((-f.numerator) // f.denominator) - 1, 0), n - 1)


def quantile(values, q):
    """Nearest-rank quantile: element quantile_index(q, N) of the sorted values, no interpolation."""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    return float(v[quantile_index(q, v.size)])


def assert_table_equal(got, want, check_sum=True):
    """got: an object with n_comp / count / ints / vals / truncated (regions.Regions); want: region_table's dict.  Everything
    bit-exact except score_sum (column 1 of vals): |got - fsum| <= area 2^-53 sum |values|, the bound of ANY summation order."""
    assert np.array_equal(got.n_comp, want["n_comp"]), (got.n_comp, want["n_comp"])
    assert np.array_equal(got.count, want["count"]), (got.count, want["count"])
    assert np.array_equal(got.truncated, want["truncated"])
    assert got.ints.dtype == np.int32 and got.vals.dtype == np.float64
    assert np.array_equal(got.ints, want["ints"]), np.argwhere(got.ints != want["ints"])[:5]
    exact = [0, 2, 3]
    assert np.array_equal(got.vals[..., exact].view(np.uint64), want["vals"][..., exact].view(np.uint64))
    if check_sum:
        for i, regs in enumerate(want["regions"]):
            for k, c in enumerate(regs):
                bound = c["area"] * 2.0 ** -53 * math.fsum(np.abs(c["values"]).tolist())
                assert abs(float(got.vals[i, k, 1]) - c["score_sum"]) <= bound, (i, k, got.vals[i, k, 1], c["score_sum"], bound)
            assert not got.vals[i, len(regs):, 1].any()
