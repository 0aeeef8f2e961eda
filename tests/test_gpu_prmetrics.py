"""GPU: the precision-recall and detection kernels (csrc/pr_metrics.hip) and their composition (cmdiad_amd/metrics.py, regions.py,
Features.calculate_metrics) against the independent yardstick tests/prmetrics_ref.py (np.unique, np.searchsorted, math.fsum,
fractions.Fraction, scipy labelling).  Everything the device produces is an integer or a stored key and the host finishes with
correctly rounded float64 expressions of those integers: every comparison is exact."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as mr  # noqa: E402
import prmetrics_ref as pr  # noqa: E402
from test_metrics_cpu import bare_method, random_split  # noqa: E402

from cmdiad_amd import metrics, ops, regions  # noqa: E402

DEV = "cuda"
T_ = ops.PR_TILE
N_DEF = [1, 2, 63, 64, 65, T_ - 1, T_, T_ + 1, 2 * T_ + 1, 3 * T_ + 17]
N_OK = [1, 2, 4095, 4096, 4097]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ run table
def run_lists(kind, n_def, n_ok, rng):
    """-> (defect scores [n_def], defect-free scores [n_ok]), unsorted."""
    ok = rng.normal(size=n_ok)
    i = np.arange(n_def, dtype=np.float64)
    if kind == "distinct":
        d = i * 0.5 - n_def / 5
    elif kind == "equal":
        d = np.full(n_def, 1.25)
    elif kind == "twice":
        d = np.floor(i / 2) * 0.25 - 1.0
    elif kind == "straddle":                  # one run from sorted index T - 1 to T + 1 (clipped to the list), every other key distinct
        d = i.copy()
        lo, hi = min(T_ - 1, n_def - 1), min(T_ + 1, n_def - 1)
        d[lo:hi + 1] = d[lo]
        d = d / 8 - 3.0
    elif kind == "tile_end":                  # runs of 512: every fourth ends exactly at a tile's last key, the next starts a tile
        d = np.floor(i / 512) - 2.0
    elif kind == "quantised":
        d, ok = np.round(rng.normal(size=n_def) * 4) / 4 + 0.5, np.round(ok * 4) / 4
    elif kind == "zeros":
        d, ok = rng.choice([0.0, -0.0, 1e-300, -1e-300], n_def), rng.choice([0.0, -0.0, 1e-300, -1e-300], n_ok)
    elif kind == "placement":                 # below every defect-free score, above every one, and equal to existing ones
        d = np.concatenate([ok.min() - 1.0 - i[:n_def // 3], ok.max() + 1.0 + i[:n_def // 3], rng.choice(ok, n_def - 2 * (n_def // 3))])
    else:
        raise KeyError(kind)
    return rng.permutation(d), ok


def sorted_keys(x):
    keys, nonfinite = ops.f64_to_keys(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV))
    assert int(nonfinite) == 0
    return ops.sort_u64_(keys)


def check_runs(d, ok, tag):
    run_key, run_first, run_fp, n_runs = ops.pr_runs(sorted_keys(d), sorted_keys(ok))
    value, first, fp = pr.run_table_from_lists(d, ok)
    R = int(n_runs)
    assert R == len(value), (tag, R, len(value))
    assert run_key.dtype == torch.int64 and run_first.dtype == torch.int32 and run_fp.dtype == torch.int32 and run_key.numel() == len(d)
    got = ops.keys_to_f64(run_key[:R].contiguous()).cpu().numpy()
    assert np.array_equal(bits(got), bits(value)), tag                       # in order, bit for bit (-0.0 comes back as +0.0)
    assert np.array_equal(run_first[:R].cpu().numpy(), first), tag
    assert np.array_equal(run_fp[:R].cpu().numpy(), fp), tag


@pytest.mark.parametrize("kind", ["distinct", "equal", "twice", "straddle", "tile_end", "quantised", "zeros", "placement"])
def test_run_table_equals_the_yardstick(kind):
    assert ops.PR_TILE == ops.nat.lib().cmdiad_pr_tile()
    rng = np.random.default_rng(11)
    for n_def in N_DEF:
        for n_ok in N_OK:
            d, ok = run_lists(kind, n_def, n_ok, rng)
            assert d.size == n_def and ok.size == n_ok
            check_runs(d, ok, (kind, n_def, n_ok))


def test_run_table_patterns_are_what_they_claim():
    """the patterns above, checked on the yardstick: the straddling run and the runs that end on a tile's last key exist"""
    rng = np.random.default_rng(0)
    d, ok = run_lists("straddle", 3 * T_ + 17, 7, rng)
    value, first, fp = pr.run_table_from_lists(d, ok)
    assert T_ - 1 in first and T_ not in first and T_ + 1 not in first and T_ + 2 in first
    d, ok = run_lists("tile_end", 3 * T_ + 17, 7, rng)
    first = pr.run_table_from_lists(d, ok)[1]
    assert {T_, 2 * T_, 3 * T_} <= set(first.tolist()) and T_ - 1 not in first
    assert len(pr.run_table_from_lists(*run_lists("equal", T_ + 1, 7, rng))[0]) == 1
    assert len(pr.run_table_from_lists(*run_lists("distinct", T_ + 1, 7, rng))[0]) == T_ + 1


def test_run_table_without_a_defect_free_score_and_without_a_defect():
    d = np.array([2.0, 1.0, 2.0])
    run_key, run_first, run_fp, n_runs = ops.pr_runs(sorted_keys(d), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert int(n_runs) == 2 and run_first[:2].tolist() == [0, 1] and run_fp[:2].tolist() == [0, 0]
    empty = ops.pr_runs(torch.zeros(0, dtype=torch.int64, device=DEV), sorted_keys(d))
    assert int(empty[3]) == 0 and empty[0].numel() == 0


# ------------------------------------------------------------------------------------------------------------------ F1 maximum
def f1_of_table(tp, fp, n_def):
    """a table handed in as plain integers -> the winner's index"""
    tp, fp = np.asarray(tp, dtype=np.int64), np.asarray(fp, dtype=np.int64)
    first = torch.from_numpy((n_def - tp).astype(np.int32)).to(DEV)
    best = ops.pr_f1max(first, torch.from_numpy(fp.astype(np.int32)).to(DEV), torch.tensor([len(tp)], dtype=torch.int32, device=DEV), n_def)
    assert best.dtype == torch.int64 and best.tolist()[1] == 0
    return int(best[0])


def filler_table(R, n_def):
    """R runs far below any planted one: tp = 1, fp large and different from run to run"""
    return np.ones(R, dtype=np.int64), 3 * n_def + np.arange(R, dtype=np.int64)


def test_f1max_planted_tie_takes_the_higher_threshold():
    gts = np.array([[[1, 1, 0, 0]]], np.uint8)
    preds = np.array([[[3.0, 1.0, 2.0, 2.0]]])
    value, cnt, tp, fp, n_def, n_ok = metrics.pr_table(gts, preds)
    assert value.tolist() == [1.0, 3.0] and tp.tolist() == [2, 1] and fp.tolist() == [2, 0] and cnt.tolist() == [1, 1]
    assert f1_of_table(tp, fp, n_def) == 1 == pr.f1max_ref(tp, fp, n_def)
    m = metrics.pixel_pr_metrics(gts, preds)
    assert m == pr.pr_metrics_ref(gts, preds)
    assert m["pixel_f1max"] == 2 / 3 and m["pixel_f1max_threshold"] == 3.0 and (m["tp"], m["fp"]) == (1, 0)


@pytest.mark.parametrize("R,a,b", [(600, 5, 200), (600, 5, 300), (600, 255, 256), (600, 40, 599),
                                   (ops.PR_F1_BLOCK * (ops.PR_F1_MAX_BLOCKS + 1) + 3, 7, ops.PR_F1_BLOCK * (ops.PR_F1_MAX_BLOCKS + 1) + 1)])
def test_f1max_tie_across_the_blocks_of_the_reduction(R, a, b):
    """two runs of F1 = 2/3 -- (tp, fp) = (900, 600) and (600, 0) at n_def = 1200 -- in one block of the first stage, in two, on
    the two sides of a block boundary, and with the second in a block's second round: the larger index wins"""
    n_def = 1200
    blocks = min(-(-R // ops.PR_F1_BLOCK), ops.PR_F1_MAX_BLOCKS)
    same = (a // ops.PR_F1_BLOCK) % blocks == (b // ops.PR_F1_BLOCK) % blocks
    assert same == ((R, a, b) == (600, 5, 200))
    tp, fp = filler_table(R, n_def)
    tp[a], fp[a], tp[b], fp[b] = 900, 600, 600, 0
    assert 2 * 900 * (600 + 0 + n_def) == 2 * 600 * (900 + 600 + n_def)
    assert f1_of_table(tp, fp, n_def) == b == pr.f1max_ref(tp, fp, n_def)
    fp[b] = 1                                                               # no tie any more: the other one
    assert f1_of_table(tp, fp, n_def) == a == pr.f1max_ref(tp, fp, n_def)


@pytest.mark.parametrize("order", ["a_first", "b_first"])
def test_f1max_orders_the_pair_that_float64_cannot(order):
    n_def = pr.FAREY_N_DEF
    tp, fp = filler_table(1000, n_def)
    fp[:] = (1 << 30) - np.arange(1000)                                    # counts near 2^30
    ia, ib = (10, 700) if order == "a_first" else (700, 10)
    (tp[ia], fp[ia]), (tp[ib], fp[ib]) = pr.FAREY_A, pr.FAREY_B
    assert (2 * tp[ia]) / (tp[ia] + fp[ia] + n_def) == (2 * tp[ib]) / (tp[ib] + fp[ib] + n_def)
    want = pr.f1max_ref(tp, fp, n_def)
    assert want in (ia, ib) and f1_of_table(tp, fp, n_def) == want
    assert pr.f1max_ref(tp[[ia, ib]], fp[[ia, ib]], n_def) == pr.f1max_ref(tp[[ib, ia]], fp[[ib, ia]], n_def) ^ 1


def test_f1max_passes_over_what_is_no_run_and_answers_minus_one_on_an_empty_table():
    n_def = 100
    first = torch.tensor([-1, 100, 40, 60, 7], dtype=torch.int32, device=DEV)          # first outside 0 .. n_def - 1: no run
    fp = torch.tensor([0, 0, 50, -1, 500], dtype=torch.int32, device=DEV)              # a negative count: no run
    n5 = torch.tensor([5], dtype=torch.int32, device=DEV)
    assert pr.f1max_ref([60, 93], [50, 500], n_def) == 0                                # of the two that are left, entries 2 and 4
    assert ops.pr_f1max(first, fp, n5, n_def).tolist() == [2, 0]
    assert ops.pr_f1max(first[:2].contiguous(), fp[:2].contiguous(), torch.tensor([2], dtype=torch.int32, device=DEV), n_def).tolist() == [-1, 0]
    assert ops.pr_f1max(first, fp, torch.tensor([0], dtype=torch.int32, device=DEV), n_def).tolist() == [-1, 0]
    assert ops.pr_f1max(first, fp, torch.tensor([99], dtype=torch.int32, device=DEV), n_def).tolist() == [2, 0]      # clamped to the table


# ------------------------------------------------------------------------------------------------------------------ compositions
def split_for(shape, seed, levels=None):
    """test_metrics_cpu.random_split where it can draw its blobs (H, W >= 7); on the smaller frames the same scores -- normal noise,
    raised on the defects -- over masks drawn per pixel, with both classes present"""
    (H, W), n = shape, 4
    if H >= 7 and W >= 7:
        return random_split(seed, n=n, H=H, W=W, levels=levels)
    rng = np.random.default_rng(seed)
    gts = (rng.random((n, H, W)) < 0.3).astype(np.float32)
    gts.reshape(-1)[0], gts.reshape(-1)[-1] = 1, 0
    preds = rng.normal(size=(n, H, W)) + 1.5 * gts * rng.random((n, H, W))
    if levels:
        preds = np.round(preds * levels / 4) * 4 / levels
    return gts, preds.astype(np.float64)


@pytest.fixture(scope="module")
def yardstick():
    """the yardstick's tables and dicts per (shape, levels), computed once"""
    cache = {}

    def get(shape, levels):
        if (shape, levels) not in cache:
            gts, preds = split_for(shape, 41, levels)
            cache[(shape, levels)] = (gts, preds, pr.pr_table_ref(gts, preds), pr.pr_metrics_ref(gts, preds))
        return cache[(shape, levels)]
    return get


@pytest.mark.parametrize("levels", [None, 4])
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (37, 53), (224, 224)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_compositions_are_bit_equal_to_the_yardstick(yardstick, shape, levels):
    gts, preds, table, ref = yardstick(shape, levels)
    value, cnt, tp, fp, n_def, n_ok = metrics.pr_table(gts, preds)
    assert np.array_equal(bits(value), bits(table[0])) and (n_def, n_ok) == table[4:]
    for got, want in zip((cnt, tp, fp), table[1:4]):
        assert np.array_equal(got, want)
    m = metrics.pixel_pr_metrics(list(gts), list(preds))
    print(f"{shape} levels {levels}: runs {len(value)} AP {m['pixel_ap']!r} F1-max {m['pixel_f1max']!r} at {m['pixel_f1max_threshold']!r}")
    assert m == ref and list(m) == list(ref)
    assert metrics.pixel_pr_metrics(torch.from_numpy(gts).to(DEV), torch.from_numpy(preds.astype(np.float32)).to(DEV)) == \
        pr.pr_metrics_ref(gts, preds.astype(np.float32))                           # float32 scores widen exactly
    d, ok = pr.split_lists(gts, preds)                                             # the strict threshold decides as the table counts
    assert int((d > m["pixel_f1max_threshold_gt"]).sum()) == m["tp"] and int((ok > m["pixel_f1max_threshold_gt"]).sum()) == m["fp"]
    both, plain = metrics.pixel_metrics(gts, preds, pr=True), metrics.pixel_metrics(gts, preds)
    assert list(plain) == ["pixel_rocauc", "au_pro", "au_pro_001"] and all(bits(both[k]) == bits(plain[k]) for k in plain)
    assert {k: both[k] for k in both if k not in plain} == {k: ref[k] for k in ("pixel_ap", "pixel_f1max", "pixel_f1max_threshold")}
    labels, scores = gts.reshape(len(gts), -1).any(axis=1).astype(int), preds.reshape(len(preds), -1).max(axis=1)
    if 0 < labels.sum() < len(labels):
        assert metrics.image_pr_metrics(labels, scores) == pr.image_pr_metrics_ref(labels, scores)


def test_image_level_numbers_with_ties_and_tensors():
    rng = np.random.default_rng(3)
    labels = (rng.random(110) < 0.7).astype(np.int64) * rng.integers(1, 4, 110)          # non-zero = defective
    scores = np.round(rng.normal(size=110) + (labels != 0), 1)
    ref = pr.image_pr_metrics_ref(labels, scores)
    assert metrics.image_pr_metrics(labels, scores) == ref
    assert metrics.image_pr_metrics(torch.from_numpy(labels)[:, None], [np.array([s]) for s in scores]) == ref
    assert list(ref)[:4] == ["image_ap", "image_f1max", "image_f1max_threshold", "image_f1max_threshold_gt"]


def test_refusals():
    gts, preds = random_split(12, n=2, H=16, W=16)
    for fn in (metrics.pr_table, metrics.pixel_pr_metrics, lambda g, p: metrics.pixel_metrics(g, p, pr=True)):
        for one_class in (np.zeros_like(gts), np.ones_like(gts)):
            with pytest.raises(ValueError, match="[Oo]nly one class present"):
                fn(one_class, preds)
        for bad in (np.nan, np.inf, -np.inf):
            broken = preds.copy()
            broken[1, 5, 7] = bad
            with pytest.raises(ValueError, match="NaN or infinity"):
                fn(gts, broken)
        with pytest.raises(ValueError, match="binary"):                                  # caught by the device flag word
            fn(torch.from_numpy(gts * 2).to(DEV), preds)
    for labels in ([0, 0, 0], [1, 2, 1]):
        with pytest.raises(ValueError, match="Only one class present"):
            metrics.image_pr_metrics(labels, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.image_pr_metrics([0, 1, 1], [0.1, np.nan, 0.3])


def test_calibrate_labelled_on_the_device():
    gts, maps = random_split(17, n=8, H=37, W=53)
    scores, labels = maps.reshape(8, -1).max(axis=1), gts.reshape(8, -1).any(axis=1).astype(int)
    cal = regions.calibrate_labelled(scores, labels, maps, gts, class_name="synthetic")
    pix, img = pr.pr_metrics_ref(gts, maps), pr.image_pr_metrics_ref(labels, scores)
    assert cal.pixel_threshold == pix["pixel_f1max_threshold_gt"] and cal.image_threshold == img["image_f1max_threshold_gt"]
    assert cal.pixel_quantile == (pix["n_ok"] - pix["fp"]) / pix["n_ok"] and cal.image_quantile == (img["n_ok"] - img["fp"]) / img["n_ok"]
    assert (cal.n_images, cal.n_pixels) == (8, maps.size)
    found = regions.find_regions(maps, cal)                                             # the regions module decides with the same rule
    assert int(found.ints[:, :, 1].sum()) <= pix["tp"] + pix["fp"]
    det = metrics.detection_counts(gts, maps, cal.pixel_threshold)
    assert int(det.pred_size.sum()) == pix["tp"] + pix["fp"] and int(det.covered.sum()) == pix["tp"] == int(det.hits.sum())


# ------------------------------------------------------------------------------------------------------------------ detection
def check_detection(gts, maps, thr, min_area):
    got = metrics.detection_counts(gts, maps, thr, min_area)
    g, m = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (gts, maps))
    per, covered, gt_size, hits, pred_size = pr.detection_ref(g, m, thr, min_area)
    assert got.per_image.dtype == np.int32 and np.array_equal(got.per_image, per), (got.per_image, per)
    assert np.array_equal(got.covered, covered) and np.array_equal(got.gt_size, gt_size)
    assert np.array_equal(got.hits, hits) and np.array_equal(got.pred_size, pred_size)
    assert got.totals() == dict(zip(("n_gt", "n_detected", "n_pred", "n_false"), (int(v) for v in per.sum(axis=0))))
    return got


@pytest.mark.parametrize("shape", [(1, 9), (7, 5), (37, 53), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_detection_counts_equal_the_yardstick(shape):
    cases = mr.mask_cases(*shape)
    gts = np.stack(list(cases.values()))
    rng = np.random.default_rng(5)
    maps = rng.normal(size=gts.shape) + 1.2 * gts * rng.random(gts.shape)
    maps[list(cases).index("full")] = -5.0                                              # an image without a predicted pixel
    assert not gts[list(cases).index("empty")].any()                                    # ... and one without a ground-truth component
    for min_area in (1, 2, 5):
        check_detection(gts, maps, 0.8, min_area)
    check_detection(list(gts.astype(np.float32) * 3), list(maps.astype(np.float32)), 0.25, 1)        # label(gt): non-zero is a defect
    got = check_detection(torch.from_numpy(gts).to(DEV), torch.from_numpy(maps).to(DEV), rng.uniform(-0.5, 1.5, len(gts)), 2)   # per image
    assert got.per_image[list(cases).index("full")].tolist()[1:] == [0, 0, 0]
    assert got.per_image[list(cases).index("empty")][0] == 0


def test_detection_min_area_drops_the_only_overlapping_prediction():
    gts = np.zeros((2, 9, 11), np.uint8)
    gts[:, 1:4, 1:4] = 1
    maps = np.zeros((2, 9, 11))
    maps[:, 2, 2] = 1.0                       # one predicted pixel inside the defect
    maps[:, 6:8, 6:10] = 1.0                  # eight predicted pixels away from it
    for min_area, row in ((1, [1, 1, 2, 1]), (2, [1, 0, 1, 1]), (8, [1, 0, 1, 1]), (9, [1, 0, 0, 0])):
        got = check_detection(gts, maps, 0.5, min_area)
        assert got.per_image.tolist() == [row, row], (min_area, got.per_image)
    assert check_detection(gts, maps, [0.5, 1.0], 1).per_image.tolist() == [[1, 1, 2, 1], [1, 0, 0, 0]]      # strict: 1.0 > 1.0 is false
    with pytest.raises(ValueError, match="NaN"):
        broken = maps.copy()
        broken[1, 0, 0] = np.nan
        metrics.detection_counts(gts, broken, 0.5)
    with pytest.raises(ValueError, match="pixel_threshold"):
        metrics.detection_counts(gts, maps, [0.5, 0.5, 0.5])
    assert metrics.detection_counts(gts[:0], maps[:0], 0.5).totals() == dict(n_gt=0, n_detected=0, n_pred=0, n_false=0)


def test_covered_is_the_integer_behind_a_point_of_the_pro_curve():
    gts, maps = random_split(23, n=4, H=37, W=53)
    pos, thr, hist, comp_size = metrics.pro_histogram(gts, maps, 7)
    for j in (0, 3, 6):
        above = hist[:, j + 1:].sum(axis=1)                     # scores of the component that are > thr[j]: size - le
        got = metrics.detection_counts(gts, maps, float(thr[j]), 1)
        assert np.array_equal(got.gt_size, comp_size) and np.array_equal(got.covered, above), j


# ------------------------------------------------------------------------------------------------------------------ switch
@pytest.mark.parametrize("device_switch", ["0", "1"])
def test_calculate_metrics_flag(monkeypatch, device_switch):
    from cmdiad_amd.feature_extractors.features import Features
    gts, preds = random_split(31, n=8, H=32, W=32)
    monkeypatch.setenv("CMDIAD_METRICS_DEVICE", device_switch)
    new = ("pixel_ap", "pixel_f1max", "image_ap", "image_f1max", "pr")
    off = bare_method(gts, preds)
    Features.calculate_metrics(off)
    assert not [k for k in new if hasattr(off, k)]
    on = bare_method(gts, preds)
    on.args.pr_metrics = True
    Features.calculate_metrics(on)
    pix = pr.pr_metrics_ref(gts, preds)
    img = pr.image_pr_metrics_ref(np.stack(on.image_labels), np.stack(on.image_preds))
    assert (on.pixel_ap, on.pixel_f1max, on.image_ap, on.image_f1max) == (pix["pixel_ap"], pix["pixel_f1max"], img["image_ap"], img["image_f1max"])
    assert on.pr == {f"{lvl}_{k}": src[f"{lvl}_{k}"] for lvl, src in (("pixel", pix), ("image", img)) for k in ("ap", "f1max", "f1max_threshold")}
    assert (on.image_rocauc, on.pixel_rocauc, on.au_pro, on.au_pro_001) == (off.image_rocauc, off.pixel_rocauc, off.au_pro, off.au_pro_001)


def test_regions_summary_gains_detection_with_the_flag_only(tmp_path):
    from cmdiad_amd.evaluate import ClassRun
    from cmdiad_amd.feature_extractors.features import Features
    gts, preds = random_split(33, n=8, H=32, W=32)
    cal = regions.Calibration(0.9, 2.5, 0.999, 1.0, 8, preds.size, "synthetic")
    out = {}
    for flag in (False, True):
        m = bare_method(gts, preds)
        m.args.pr_metrics = flag
        Features.calculate_metrics(m)
        run = types.SimpleNamespace(method=m, calibration=cal, measure_regions=False, min_area=2, max_regions=16, test_items=None,
                                    regions_dir=str(tmp_path / str(flag)), data=types.SimpleNamespace(name="synthetic"), sec={},
                                    regions_summary=None, overlays_summary=None, meshes_summary=None, pr_metrics=flag)
        ClassRun._write_regions(run)
        out[flag] = (run.regions_summary, open(run.regions_summary["file"]).read())
        run.n_train = run.n_test = 0
        run.phases, m.deep_feature_extractor = [], None
        res = ClassRun.result(run)                                                      # result() carries `pr` with the flag only
        assert ("pr" in res) == flag and res["regions"] == run.regions_summary and res["pixel_rocauc"] == m.pixel_rocauc
        assert not flag or res["pr"] == m.pr
    assert "detection" not in out[False][0] and out[False][1] == out[True][1] and "detection" not in json.loads(out[True][1])
    per = pr.detection_ref(gts, preds, 0.9, 2)[0]
    assert out[True][0]["detection"] == dict(zip(("n_gt", "n_detected", "n_pred", "n_false"), (int(v) for v in per.sum(axis=0))))
    assert {k: v for k, v in out[True][0].items() if k not in ("detection", "file")} == {k: v for k, v in out[False][0].items() if k != "file"}
