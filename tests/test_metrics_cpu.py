"""CPU (no GPU): the yardstick of the device metrics (tests/metrics_ref.py) against scikit-learn and utils/au_pro_util.py; the
CMDIAD_METRICS_DEVICE switch of Features.calculate_metrics; the argument checks of cmdiad_amd.metrics that need no device."""
import os
import sys
import types

import numpy as np
import pytest
from sklearn.metrics import roc_auc_score

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as mr  # noqa: E402

from cmdiad_amd.utils import au_pro_util  # noqa: E402


def random_split(seed, n=4, H=37, W=53, levels=None):
    """n masks with a few blobs and single pixels, scores that are higher on the defects; `levels`: scores quantised (ties)."""
    rng = np.random.default_rng(seed)
    gts = np.zeros((n, H, W), dtype=np.float32)
    for i in range(n):
        if i % 4 == 3:
            continue                                   # a defect-free image
        for _ in range(3):
            y, x, h, w = rng.integers(0, H - 6), rng.integers(0, W - 6), rng.integers(1, 7), rng.integers(1, 7)
            gts[i, y:y + h, x:x + w] = 1
        ys, xs = rng.integers(0, H, 4), rng.integers(0, W, 4)
        gts[i, ys, xs] = 1                             # components of one pixel
    preds = rng.normal(size=(n, H, W)) + 1.5 * gts * rng.random((n, H, W))
    if levels:
        preds = np.round(preds * levels / 4) * 4 / levels
    return gts, preds.astype(np.float64)


@pytest.mark.parametrize("levels", [None, 4, 1])
def test_yardstick_auc_matches_roc_auc_score(levels):
    gts, preds = random_split(1, levels=levels)
    if levels == 1:
        preds = np.zeros_like(preds)                   # all equal: 0.5 exactly
    n = preds.size
    got, ref = mr.roc_auc_ref(gts, preds), roc_auc_score(gts.ravel(), preds.ravel())
    assert abs(got - ref) <= 8 * n * 2.0 ** -53, (got, ref)
    if levels == 1:
        assert got == 0.5


def test_yardstick_auc_extremes():
    gts = np.zeros((1, 1, 2), np.float32)
    gts[0, 0, 1] = 1
    assert mr.roc_auc_ref(gts, np.array([[[0.1, 0.7]]])) == 1.0
    assert mr.roc_auc_ref(gts, np.array([[[0.7, 0.1]]])) == 0.0
    assert mr.roc_auc_ref(gts, np.array([[[0.3, 0.3]]])) == 0.5


def test_yardstick_histogram_route_matches_au_pro(golden):
    g = golden("g7_aupro.npz")
    gts, preds = list(g["gts"]), list(g["preds"])
    fpr, pro = mr.pro_curve_ref(gts, preds, 100)
    for limit, key in ((0.3, "au_pro_03"), (0.01, "au_pro_001")):
        host, _ = au_pro_util.calculate_au_pro(gts, preds, limit)
        mine = au_pro_util.trapezoid(fpr, pro, x_max=limit) / limit
        assert abs(mine - host) < 1e-12 and abs(mine - float(g[key])) < 1e-12, (limit, mine, host, float(g[key]))


@pytest.mark.parametrize("T", [2, 100, 1000])
@pytest.mark.parametrize("levels", [None, 8])
def test_yardstick_histogram_route_is_the_sampled_curve_exactly(golden, T, levels):
    g = golden("g7_aupro.npz")
    for gts, preds in ((g["gts"], g["preds"]), random_split(2, levels=levels)):
        fpr, pro = mr.pro_curve_ref(gts, preds, T)
        fpr_h, pro_h = au_pro_util._pro_curve_sampled(list(gts), list(preds), T)
        assert np.array_equal(fpr, fpr_h) and np.array_equal(pro, pro_h)


def test_yardstick_sort_canonicalises_negative_zero():
    x = np.array([0.0, -0.0, -1.0, 1.0, -0.0])
    s = mr.sort_ref(x)
    assert np.array_equal(s, [-1.0, 0.0, 0.0, 0.0, 1.0]) and not np.signbit(s[1:4]).any()


def bare_method(gts, preds):
    """What Features.calculate_metrics reads, on an object that is no Features: the result lists of a finished predict loop."""
    n = len(gts)
    rng = np.random.default_rng(0)
    return types.SimpleNamespace(
        image_preds=[np.array([float(p.max())]) for p in preds],
        image_labels=[np.array([int(g.any())]) for g in gts],      # random_split: every fourth image is defect-free
        pixel_preds=np.concatenate([p.ravel() for p in preds]), pixel_labels=np.concatenate([g.ravel() for g in gts]),
        img_name=[np.array([f"img{i}_{rng.integers(10)}"]) for i in range(n)], gts=list(gts), predictions=list(preds),
        args=types.SimpleNamespace(save_raw_results=False), class_name="synthetic")


def test_switch_unset_never_imports_the_device_module_and_set_goes_through_it(monkeypatch):
    from cmdiad_amd.feature_extractors.features import Features
    gts, preds = random_split(3, n=8, H=16, W=16)
    # unset: today's host code, and the device module is not even imported
    monkeypatch.delenv("CMDIAD_METRICS_DEVICE", raising=False)
    saved = sys.modules.pop("cmdiad_amd.metrics", None)
    try:
        off = bare_method(gts, preds)
        Features.calculate_metrics(off)
        assert "cmdiad_amd.metrics" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["cmdiad_amd.metrics"] = saved
    assert off.pixel_rocauc == roc_auc_score(gts.ravel(), preds.ravel())
    assert off.au_pro == au_pro_util.calculate_au_pro(list(gts), list(preds))[0]
    assert off.au_pro_001 == au_pro_util.calculate_au_pro(list(gts), list(preds), 0.01)[0]
    # set (read at call time): the three pixel-level values come from metrics.pixel_metrics, image_rocauc does not
    from cmdiad_amd import metrics
    seen = []

    def stub(g, p):
        seen.append((g, p))
        return dict(pixel_rocauc=0.25, au_pro=0.5, au_pro_001=0.75)
    monkeypatch.setattr(metrics, "pixel_metrics", stub)
    monkeypatch.setenv("CMDIAD_METRICS_DEVICE", "1")
    on = bare_method(gts, preds)
    Features.calculate_metrics(on)
    assert len(seen) == 1 and seen[0][0] is on.gts and seen[0][1] is on.predictions
    assert (on.pixel_rocauc, on.au_pro, on.au_pro_001) == (0.25, 0.5, 0.75)
    assert on.image_rocauc == off.image_rocauc
    monkeypatch.setenv("CMDIAD_METRICS_DEVICE", "0")
    again = bare_method(gts, preds)
    Features.calculate_metrics(again)
    assert len(seen) == 1 and again.pixel_rocauc == off.pixel_rocauc


def test_wrappers_refuse_bad_arguments_without_a_device():
    from cmdiad_amd import metrics
    gts, preds = random_split(4, n=2, H=8, W=8)
    with pytest.raises(ValueError, match="1024"):
        metrics.pro_curve(gts, preds, num_thresholds=1025)
    with pytest.raises(ValueError, match="1024"):
        metrics.pixel_metrics(gts, preds, num_thresholds=5000)
    with pytest.raises(NotImplementedError, match="calculate_au_pro"):
        metrics.pro_curve(gts, preds, num_thresholds=None)
    bad = gts.copy()
    bad[0, 0, 0] = 2.0
    for fn in (metrics.pixel_roc_auc, metrics.pixel_metrics, metrics.auc_counts):
        with pytest.raises(ValueError, match="binary"):
            fn(bad, preds)
        with pytest.raises(ValueError, match="binary"):
            fn(list(bad.astype(np.int64)), list(preds))
    with pytest.raises(ValueError, match="n,H,W"):
        metrics.pixel_roc_auc(np.zeros((2, 2, 2, 2), np.float32), np.zeros((2, 2, 2, 2)))
