"""GPU: the pixel-metric kernels (csrc/metrics.hip) and their composition (cmdiad_amd/metrics.py) against the independent yardstick
tests/metrics_ref.py (scipy labelling, np.sort, np.searchsorted), scikit-learn's roc_auc_score and utils/au_pro_util.py.  Everything
the device produces is an integer or a sorted set: the comparisons are exact, except P-AUROC against scikit-learn's own summation."""
import os
import sys

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as mr  # noqa: E402
from test_metrics_cpu import bare_method, random_split  # noqa: E402

from cmdiad_amd import metrics, ops  # noqa: E402
from cmdiad_amd.utils import au_pro_util  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (37, 53), (64, 64), (224, 224), (300, 260)]


def auc_tolerance(n):
    """sklearn sums at most n trapezoids, each from two correctly rounded divisions, an add and a multiply, plus the summation's own
    error: 8 n 2^-53 bounds the difference to the correctly rounded quotient."""
    return 8 * n * 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------ labelling
def check_labelling(masks):
    labels, n_comp, comp_size = metrics.connected_components(masks)
    ref_labels, ref_n, ref_size = mr.label_ref(masks.cpu().numpy() if torch.is_tensor(masks) else masks)
    assert labels.dtype == torch.int32 and n_comp.dtype == torch.int32
    assert np.array_equal(n_comp.cpu().numpy(), ref_n), (n_comp.cpu().numpy(), ref_n)
    assert np.array_equal(labels.cpu().numpy(), ref_labels)
    assert np.array_equal(comp_size.cpu().numpy(), ref_size)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelling_equals_scipy(shape, dtype):
    cases = mr.mask_cases(*shape)
    masks = np.stack(list(cases.values())).astype(dtype)
    if dtype is np.float32:
        masks *= np.float32(0.25)            # foreground is "non-zero", not "one"
    check_labelling(masks)
    check_labelling(torch.from_numpy(masks).to(DEV))


def test_labelling_batch_mixes_empty_and_crowded_images():
    H, W = 37, 53
    c = mr.mask_cases(H, W, seed=5)
    masks = np.stack([c["empty"], c["isolated"], c["empty"], c["random0.2"], c["full"], c["empty"], c["random0.4"], c["isolated"]])
    check_labelling(masks)
    labels, n_comp, comp_offset, comp_size, nonbinary = ops.ccl_label(torch.from_numpy(masks).to(DEV))
    assert comp_offset.tolist() == np.concatenate([[0], np.cumsum(n_comp.cpu().numpy())]).tolist()
    assert int(nonbinary) == 0 and int(comp_size[int(comp_offset[-1]):].abs().sum()) == 0
    assert n_comp[1] == ((H + 1) // 2) * ((W + 1) // 2)            # the most an image can hold
    two = torch.from_numpy(masks * np.uint8(2)).to(DEV)
    assert int(ops.ccl_label(two)[4]) == int((masks != 0).sum())   # values that are neither 0 nor 1 are counted, and still labelled
    assert torch.equal(ops.ccl_label(two)[0], labels)
    empty = ops.ccl_label(torch.zeros((0, 4, 4), dtype=torch.uint8, device=DEV))
    assert empty[2].tolist() == [0]
    with pytest.raises(ValueError, match="2\\^24"):
        ops.ccl_label(torch.zeros((1, 4097, 4096), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ sort
T_ = ops.SORT_TILE
SORT_SIZES = [1, 2, 63, 64, 65, T_ - 1, T_, T_ + 1, 3 * T_ + 17, 200003]


def sort_contents(kind, n, rng):
    if kind == "equal":
        return np.full(n, 3.25)
    if kind == "two_values":
        return rng.choice([-1.5, 2.0], n)
    if kind == "ascending":
        return np.arange(n, dtype=np.float64) - n / 3
    if kind == "descending":
        return n / 3 - np.arange(n, dtype=np.float64)
    if kind == "all_digits":
        return rng.normal(size=n) * 10.0 ** rng.uniform(-300, 300, n) * rng.choice([-1.0, 1.0], n)
    if kind == "denormals":
        return rng.integers(-2 ** 40, 2 ** 40, n).astype(np.float64) * 5e-324
    if kind == "largest":
        return rng.choice([np.finfo(np.float64).max, -np.finfo(np.float64).max, 0.0, 1.0], n)
    if kind == "zeros":
        return rng.choice([0.0, -0.0, 1e-300, -1e-300], n)
    if kind == "float32_origin":
        return rng.normal(size=n).astype(np.float32).astype(np.float64)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["equal", "two_values", "ascending", "descending", "all_digits", "denormals", "largest", "zeros",
                                  "float32_origin"])
def test_sort_is_bit_equal_to_numpy(kind):
    assert ops.SORT_TILE == ops.nat.lib().cmdiad_sort_u64_tile()
    rng = np.random.default_rng(7)
    for n in SORT_SIZES:
        x = sort_contents(kind, n, rng)
        got = metrics.sort_values(x).cpu().numpy()
        ref = mr.sort_ref(x)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (kind, n)


def test_sort_refuses_nan_and_infinity_and_takes_empty_input():
    x = np.random.default_rng(0).normal(size=5000)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[4321] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            metrics.sort_values(y)
    assert metrics.sort_values(np.zeros(0)).numel() == 0
    keys, _ = ops.f64_to_keys(torch.from_numpy(x).to(DEV))
    assert torch.equal(ops.keys_to_f64(keys), torch.from_numpy(x).to(DEV))      # the key map is a bijection on finite doubles


# ------------------------------------------------------------------------------------------------------------------ P-AUROC
def check_auc(gts, preds, exact=None):
    S, n_ok, n_def = metrics.auc_counts(gts, preds)
    g, p = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (gts, preds))
    assert (S, n_ok, n_def) == mr.auc_counts_ref(g, p)
    got = metrics.pixel_roc_auc(gts, preds)
    ref = roc_auc_score(g.ravel(), p.ravel())
    print(f"P-AUROC device {got!r} sklearn {ref!r} diff {abs(got - ref):.3e} bound {auc_tolerance(p.size):.3e}")
    assert got == S / (2 * n_ok * n_def) and abs(got - ref) <= auc_tolerance(p.size)
    if exact is not None:
        assert got == exact


def test_auc_one_pixel_of_each_kind():
    gts = np.array([[[0.0, 1.0]]], dtype=np.float32)
    check_auc(gts, np.array([[[0.25, 0.75]]]), exact=1.0)
    check_auc(gts, np.array([[[0.75, 0.25]]]), exact=0.0)
    check_auc(gts, np.array([[[0.5, 0.5]]]), exact=0.5)


def test_auc_separated_equal_and_quantised_scores():
    gts, preds = random_split(11, n=3, H=37, W=53)
    check_auc(gts, np.where(gts > 0, 5.0 + np.abs(preds), -np.abs(preds)), exact=1.0)
    check_auc(gts, np.full_like(preds, -0.125), exact=0.5)
    check_auc(gts, np.floor(np.clip(preds, -2.0, 1.5)))                    # four levels (-2, -1, 0, 1): heavy ties
    check_auc(gts, np.where(preds > 0, 0.0, -0.0))                         # the two zeros are one value
    check_auc(gts.astype(np.uint8), preds.astype(np.float32))              # float32 scores widen exactly


def test_auc_random_maps_and_refusals():
    gts, preds = random_split(12, n=8, H=64, W=64)
    check_auc(gts, preds)
    check_auc(list(gts), list(preds))
    check_auc(torch.from_numpy(gts).to(DEV), torch.from_numpy(preds).to(DEV))
    bad = torch.from_numpy(gts * 2).to(DEV)
    with pytest.raises(ValueError, match="binary"):                        # caught by the device flag word
        metrics.pixel_roc_auc(bad, preds)
    for one_class in (np.zeros_like(gts), np.ones_like(gts)):
        with pytest.raises(ValueError, match="one class"):
            metrics.pixel_roc_auc(one_class, preds)
    nan = preds.copy()
    nan[3, 5, 7] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.pixel_roc_auc(gts, nan)


# ------------------------------------------------------------------------------------------------------------------ PRO
def check_pro(gts, preds, T):
    pos, thr, hist, comp_size = metrics.pro_histogram(gts, preds, T)
    rpos, rthr, rhist, rsize = mr.hist_ref(gts, preds, T)
    assert np.array_equal(pos, rpos) and np.array_equal(thr, mr.canonical(rthr)) and np.array_equal(comp_size, rsize)
    assert hist.shape == rhist.shape and np.array_equal(hist, rhist)
    fpr, pro = metrics.pro_curve(gts, preds, T)
    fpr_h, pro_h = au_pro_util._pro_curve_sampled(list(gts), list(preds), T)
    assert np.array_equal(fpr, fpr_h) and np.array_equal(pro, pro_h)


@pytest.mark.parametrize("T", [2, 100, 1000])
def test_pro_histogram_and_curve_equal_the_host(T):
    gts, preds = random_split(21, n=5, H=37, W=53)
    assert (mr.label_ref(gts)[2] == 1).any()                               # components of one pixel
    check_pro(gts, preds, T)
    check_pro(gts, np.round(preds * 2) / 2, T)                             # quantised scores: duplicate thresholds
    check_pro(gts * np.float32(3), preds, T)                               # label(gt): non-zero is a defect


def test_pro_on_the_recorded_fixture(golden):
    g = golden("g7_aupro.npz")
    gts, preds = list(g["gts"]), list(g["preds"])
    check_pro(g["gts"], g["preds"], 100)
    m = metrics.pixel_metrics(gts, preds)
    for limit, key, name in ((0.3, "au_pro_03", "au_pro"), (0.01, "au_pro_001", "au_pro_001")):
        host, _ = au_pro_util.calculate_au_pro(gts, preds, limit)
        assert m[name] == host and abs(m[name] - float(g[key])) < 1e-12, (name, m[name], host, float(g[key]))
    assert abs(m["pixel_rocauc"] - roc_auc_score(g["gts"].ravel(), g["preds"].ravel())) <= auc_tolerance(g["preds"].size)


def test_pro_edges():
    gts, preds = random_split(22, n=2, H=16, W=16)
    fpr, pro = metrics.pro_curve(np.zeros_like(gts), preds, 10)            # no component: PRO is 0 up to the closing point
    fpr_h, pro_h = au_pro_util._pro_curve_sampled(list(np.zeros_like(gts)), list(preds), 10)
    assert np.array_equal(fpr, fpr_h) and np.array_equal(pro, pro_h)
    with pytest.raises(ValueError, match="defect-free"):
        metrics.pro_curve(np.ones_like(gts), preds, 10)
    with pytest.raises(ValueError, match="1 GiB"):                         # 128 x 128 isolated pixels x 16 images x 1025 bins
        iso = np.zeros((16, 256, 256), np.uint8)
        iso[:, ::2, ::2] = 1
        metrics.pro_curve(iso, np.zeros(iso.shape, np.float32), 1024)


# ------------------------------------------------------------------------------------------------------------------ switch
def test_calculate_metrics_switch(monkeypatch):
    from cmdiad_amd.feature_extractors.features import Features
    gts, preds = random_split(31, n=8, H=64, W=64)
    monkeypatch.delenv("CMDIAD_METRICS_DEVICE", raising=False)
    off = bare_method(gts, preds)
    Features.calculate_metrics(off)
    monkeypatch.setenv("CMDIAD_METRICS_DEVICE", "1")
    on = bare_method(gts, preds)
    Features.calculate_metrics(on)
    assert on.au_pro == off.au_pro and on.au_pro_001 == off.au_pro_001
    assert abs(on.pixel_rocauc - off.pixel_rocauc) <= auc_tolerance(preds.size)
    assert on.image_rocauc == off.image_rocauc
    assert on.pixel_rocauc == mr.roc_auc_ref(gts, preds)
