"""CPU (no GPU): the yardstick of the precision-recall numbers (tests/prmetrics_ref.py) against scikit-learn; the strict threshold;
the pair of fractions that float64 cannot tell apart; the argument validation of the four entry points of csrc/pr_metrics.hip,
which happens before any launch; the parts of cmdiad_amd.metrics / regions / Features that need no device."""
import ctypes
import os
import sys
import types
from fractions import Fraction

import numpy as np
import pytest
from sklearn.metrics import average_precision_score, precision_recall_curve

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prmetrics_ref as pr  # noqa: E402
from test_metrics_cpu import bare_method, random_split  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def split_kinds(seed):
    """name -> (gts, preds): random, quantised (heavy ties), float32-origin, and the two zeros mixed."""
    gts, preds = random_split(seed)
    zeros = np.where(preds > 0.5, preds, np.where(preds > -0.5, 0.0, -0.0))
    return {"random": (gts, preds), "quantised": random_split(seed, levels=4), "coarse": (gts, np.floor(np.clip(preds, -2.0, 1.5))),
            "float32": (gts, preds.astype(np.float32).astype(np.float64)), "zeros": (gts, zeros)}


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("kind", ["random", "quantised", "coarse", "float32", "zeros"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_yardstick_matches_scikit_learn(kind, seed):
    gts, preds = split_kinds(seed)[kind]
    y, s = (gts.ravel() != 0).astype(int), preds.ravel()
    m = pr.pr_metrics_ref(gts, preds)
    n = s.size
    # at most four roundings per term and terms that sum to at most 1, as auc_tolerance of test_gpu_metrics.py
    ref = average_precision_score(y, s)
    assert abs(m["pixel_ap"] - ref) <= 8 * n * 2.0 ** -53, (m["pixel_ap"], ref)
    p, r, _ = precision_recall_curve(y, s)
    f1 = np.where(p + r > 0, 2 * p * r / np.where(p + r > 0, p + r, 1.0), 0.0)
    assert abs(m["pixel_f1max"] - f1.max()) <= 1e-12, (m["pixel_f1max"], f1.max())
    assert m["n_def"] == int(y.sum()) and m["n_ok"] == n - int(y.sum())
    assert m["precision"] == m["tp"] / (m["tp"] + m["fp"]) and m["recall"] == m["tp"] / m["n_def"]


def test_yardstick_table_on_a_case_worked_by_hand():
    # defects 3, 1, 1 and defect-free 2, 2, 0: runs (1: first 0, fp 2) and (3: first 2, fp 0)
    gts = np.array([[[1, 1, 1, 0, 0, 0]]], np.uint8)
    preds = np.array([[[3.0, 1.0, 1.0, 2.0, 2.0, 0.0]]])
    value, cnt, tp, fp, n_def, n_ok = pr.pr_table_ref(gts, preds)
    assert value.tolist() == [1.0, 3.0] and cnt.tolist() == [2, 1] and tp.tolist() == [3, 1] and fp.tolist() == [2, 0]
    assert (n_def, n_ok) == (3, 3)
    assert pr.ap_ref(cnt, tp, fp, n_def) == (2 * 3) / (3 * 5) + (1 * 1) / (3 * 1)
    # the planted tie: defects {3, 1}, defect-free {2, 2}: both runs give 2/3 and the higher threshold wins
    value, cnt, tp, fp, n_def, n_ok = pr.pr_table_ref(np.array([1, 1, 0, 0]), np.array([3.0, 1.0, 2.0, 2.0]))
    assert [Fraction(2 * int(t), int(t) + int(f) + n_def) for t, f in zip(tp, fp)] == [Fraction(2, 3)] * 2
    assert pr.f1max_ref(tp, fp, n_def) == 1 and value[1] == 3.0


@pytest.mark.parametrize("kind", ["random", "quantised", "float32", "zeros"])
def test_strict_threshold_reproduces_the_counts(kind):
    gts, preds = split_kinds(5)[kind]
    value, cnt, tp, fp, n_def, n_ok = pr.pr_table_ref(gts, preds)
    d, ok = pr.split_lists(gts, preds)
    for r in sorted({0, len(value) // 3, len(value) // 2, len(value) - 1, pr.f1max_ref(tp, fp, n_def)}):
        t = np.nextafter(value[r], -np.inf)
        assert t < value[r] and int((d > t).sum()) == tp[r] and int((ok > t).sum()) == fp[r], (kind, r)
    m = pr.pr_metrics_ref(gts, preds)
    assert int((d > m["pixel_f1max_threshold_gt"]).sum()) == m["tp"] and int((ok > m["pixel_f1max_threshold_gt"]).sum()) == m["fp"]


def test_farey_neighbours_are_ordered_by_fraction_and_tie_in_float64():
    n_def = pr.FAREY_N_DEF
    (ta, fa), (tb, fb) = pr.FAREY_A, pr.FAREY_B
    qa, qb = Fraction(2 * ta, ta + fa + n_def), Fraction(2 * tb, tb + fb + n_def)
    assert qa != qb and abs(qa - qb) < Fraction(1, 10 ** 17) and abs(float(qa - qb)) > 5e-18
    assert (2 * ta) / (ta + fa + n_def) == (2 * tb) / (tb + fb + n_def)                 # one float64: the division cannot order them
    assert max(ta, tb) <= 1 << 30 and max(ta + fa, tb + fb) + n_def < 1 << 32           # the cross products fit 64 bits
    assert (ta * (tb + fb + n_def) > tb * (ta + fa + n_def)) == (qa > qb)
    # index order decides nothing here: whichever comes first, the yardstick names the larger fraction
    want = 0 if qa > qb else 1
    assert pr.f1max_ref([ta, tb], [fa, fb], n_def) == want and pr.f1max_ref([tb, ta], [fb, fa], n_def) == 1 - want


def test_average_precision_of_a_table_is_the_yardsticks_on_both_of_its_paths():
    """metrics.average_precision divides in numpy while every numerator and denominator is below 2^53 and in Python integers past
    that: the same correctly rounded quotients either way, on real tables and on integers on both sides of the switch"""
    from cmdiad_amd import metrics
    for kind, (gts, preds) in split_kinds(9).items():
        value, cnt, tp, fp, n_def, n_ok = pr.pr_table_ref(gts, preds)
        assert metrics.average_precision(cnt, tp, fp, n_def) == pr.ap_ref(cnt, tp, fp, n_def), kind
    rng = np.random.default_rng(2)
    for n_def, top in ((1 << 20, 1 << 20), (1 << 23, 1 << 23), ((1 << 26) + 5, 1 << 27), (1 << 30, 1 << 30)):
        tp = np.sort(rng.integers(1, top + 1, 300))[::-1].copy()
        cnt, fp = rng.integers(1, top + 1, 300), rng.integers(0, top + 1, 300)
        fast = int(cnt.max()) * int(tp.max()) < 1 << 53 and n_def * (int(tp.max()) + int(fp.max())) < 1 << 53
        assert fast == (top <= 1 << 23)
        assert metrics.average_precision(cnt, tp, fp, n_def) == pr.ap_ref(cnt, tp, fp, n_def), (n_def, top)
    # just below and just above 2^53 in the numerator
    for c, t in (((1 << 26) + 1, (1 << 27) - 3), ((1 << 26) + 1, (1 << 27) + 1)):
        assert (c * t < 1 << 53) == (t < 1 << 27)
        assert metrics.average_precision([c, 3], [t, 2], [5, 7], 1 << 20) == pr.ap_ref([c, 3], [t, 2], [5, 7], 1 << 20)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_reject_bad_arguments_before_any_launch():
    from cmdiad_amd import _native as nat
    from cmdiad_amd import ops
    L = nat.lib()
    assert L.cmdiad_abi_version() == 6
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    for name in ("cmdiad_pr_runs", "cmdiad_pr_f1max", "cmdiad_region_overlap", "cmdiad_detection_counts"):
        assert f"int {name}(" in hdr and name in nat.SIGNATURES and hasattr(L, name)
        assert getattr(L, name).argtypes == nat.SIGNATURES[name]
    # the scratch of the two is a typed buffer whose size is a formula of the header: neither has a workspace or a size query
    assert "size_t cmdiad_pr_tile(" in hdr and "cmdiad_pr_tile" in nat.SIZE_QUERIES
    assert not [q for q in nat.SIZE_QUERIES if "pr_runs" in q or "f1max" in q]
    T = L.cmdiad_pr_tile()
    assert T == ops.PR_TILE and T % 256 == 0
    big = (1 << 30) + 1
    one = ctypes.c_void_p(16)             # a non-null pointer that a rejected call never follows

    def runs(n_def=5, n_ok=7, cap=5, tcap=1 << 10, ptr=one, **over):
        a = dict(d=ptr, ok=ptr, key=ptr, first=ptr, fp=ptr, n_runs=ptr, tiles=ptr)
        a.update(over)
        return L.cmdiad_pr_runs(a["d"], n_def, a["ok"], n_ok, a["key"], a["first"], a["fp"], cap, a["n_runs"], a["tiles"], tcap, None)

    def f1max(cap=5, n_def=5, pcap=1 << 10, ptr=one, **over):
        a = dict(first=ptr, fp=ptr, n_runs=ptr, best=ptr, partial=ptr)
        a.update(over)
        return L.cmdiad_pr_f1max(a["first"], a["fp"], a["n_runs"], cap, n_def, a["best"], a["partial"], pcap, None)

    def overlap(n=1, H=4, W=5, gcap=6, pcap=6, min_area=1, ptr=one, **over):
        a = dict(gl=ptr, goff=ptr, pl=ptr, poff=ptr, psize=ptr, covered=ptr, hits=ptr)
        a.update(over)
        return L.cmdiad_region_overlap(a["gl"], a["goff"], gcap, a["pl"], a["poff"], a["psize"], pcap, n, H, W, min_area, a["covered"],
                                       a["hits"], None)

    def counts(n=1, gcap=6, pcap=6, min_area=1, ptr=one, **over):
        a = dict(goff=ptr, covered=ptr, poff=ptr, psize=ptr, hits=ptr, counts=ptr)
        a.update(over)
        return L.cmdiad_detection_counts(a["goff"], a["covered"], gcap, a["poff"], a["psize"], a["hits"], pcap, n, min_area, a["counts"], None)

    def refused(rc, text):
        assert rc == -1 and text in L.cmdiad_last_error(), (rc, text, L.cmdiad_last_error())

    for kw in (dict(n_def=-1), dict(n_def=big), dict(n_ok=-1), dict(n_ok=big), dict(cap=-1), dict(cap=big), dict(tcap=-1), dict(tcap=big)):
        refused(runs(**kw), b"cmdiad_pr_runs: bad sizes")
    for at in ("d", "ok", "key", "first", "fp", "n_runs", "tiles"):
        refused(runs(**{at: None}), b"cmdiad_pr_runs: null pointer")
    assert runs(n_def=0, ptr=None) == 0                                                    # nothing to do: no launch
    refused(runs(n_def=-1, ptr=None), b"bad sizes")                                        # the sizes are checked first
    for n_def, tcap in ((5, 1), (T, 1), (T + 1, 3), (3 * T + 17, 7)):                      # 2 ceil(n_def / tile) entries, no fewer
        refused(runs(n_def=n_def, cap=n_def, tcap=tcap), b"cmdiad_pr_runs: tile_heads holds %d entries, %d are needed" % (tcap, tcap + 1))

    for kw in (dict(cap=-1), dict(cap=big), dict(n_def=-1), dict(n_def=big), dict(pcap=-1), dict(pcap=big)):
        refused(f1max(**kw), b"cmdiad_pr_f1max: bad sizes")
    for at in ("first", "fp", "n_runs", "best", "partial"):
        refused(f1max(**{at: None}), b"cmdiad_pr_f1max: null pointer")
    assert f1max(cap=0, ptr=None) == 0
    B, M = ops.PR_F1_BLOCK, ops.PR_F1_MAX_BLOCKS
    for cap, pcap in ((1, 0), (B, 0), (B + 1, 1), (B * M, M - 1), (1 << 30, M - 1)):        # min(ceil(run_cap / 256), 1024) entries
        refused(f1max(cap=cap, pcap=pcap), b"cmdiad_pr_f1max: partial holds %d entries, %d are needed" % (pcap, pcap + 1))

    for kw in (dict(H=0), dict(W=0), dict(n=-1), dict(n=65536), dict(H=4097, W=4096), dict(n=5, H=1 << 14, W=1 << 14), dict(gcap=-1),
               dict(gcap=big), dict(pcap=-1), dict(pcap=big), dict(min_area=0), dict(min_area=-3)):
        refused(overlap(**kw), b"cmdiad_region_overlap: bad sizes")
    for at in ("gl", "goff", "pl", "poff", "psize", "covered", "hits"):
        refused(overlap(**{at: None}), b"cmdiad_region_overlap: null pointer")
    assert overlap(n=0, ptr=None) == 0
    refused(overlap(n=0, H=0, ptr=None), b"bad sizes")

    for kw in (dict(n=-1), dict(n=65536), dict(gcap=-1), dict(gcap=big), dict(pcap=-1), dict(pcap=big), dict(min_area=0)):
        refused(counts(**kw), b"cmdiad_detection_counts: bad sizes")
    for at in ("goff", "covered", "poff", "psize", "hits", "counts"):
        refused(counts(**{at: None}), b"cmdiad_detection_counts: null pointer")
    assert counts(n=0, ptr=None) == 0


def test_wrappers_refuse_before_a_device_is_touched():
    import torch
    from cmdiad_amd import metrics, ops
    with pytest.raises(Exception, match="GPU"):
        ops.pr_runs(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(Exception, match="GPU"):
        ops.pr_f1max(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 3)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="min_area"):
            ops.region_overlap(None, None, None, None, None, min_area=bad)
        with pytest.raises(ValueError, match="min_area"):
            ops.detection_counts(None, None, None, None, None, min_area=bad)
        with pytest.raises(ValueError, match="min_area"):
            metrics.detection_counts(np.zeros((1, 2, 2), np.uint8), np.zeros((1, 2, 2)), 0.5, min_area=bad)
    with pytest.raises(ValueError, match="labels"):
        metrics.image_pr_metrics([0, 1, 1], [0.5, 0.25])
    with pytest.raises(TypeError, match="floating"):
        metrics.image_pr_metrics([0, 1], [1, 2])
    gts, preds = random_split(4, n=2, H=8, W=8)
    bad = gts.copy()
    bad[0, 0, 0] = 2.0
    for fn in (metrics.pr_table, metrics.pixel_pr_metrics):                        # masks must be binary, as for P-AUROC
        with pytest.raises(ValueError, match="binary"):
            fn(bad, preds)


# ------------------------------------------------------------------------------------------------ compositions, kernels stubbed
class FakeSplit:
    """What pixel_metrics reads of a _Split, answered by the yardsticks."""

    def __init__(self, gts, predictions, need_binary=False):
        self.gts, self.preds = np.asarray(gts), np.asarray(predictions)

    def roc_auc(self):
        import metrics_ref as mr
        return mr.roc_auc_ref(self.gts, self.preds)

    def pro_curve(self, T):
        import metrics_ref as mr
        return mr.pro_curve_ref(self.gts, self.preds, T)

    def pr_metrics(self):
        m = pr.pr_metrics_ref(self.gts, self.preds)
        return dict(ap=m["pixel_ap"], f1max=m["pixel_f1max"], threshold=m["pixel_f1max_threshold"],
                    threshold_gt=m["pixel_f1max_threshold_gt"], **{k: m[k] for k in ("tp", "fp", "precision", "recall", "n_def", "n_ok")})


def test_pixel_metrics_default_keys_are_unchanged_and_pr_adds_three(monkeypatch):
    from cmdiad_amd import metrics
    monkeypatch.setattr(metrics, "_Split", FakeSplit)
    gts, preds = random_split(6, n=3, H=16, W=16)
    plain = metrics.pixel_metrics(gts, preds)
    assert list(plain) == ["pixel_rocauc", "au_pro", "au_pro_001"]
    assert metrics.pixel_metrics(gts, preds, 100) == plain and metrics.pixel_metrics(gts, preds, pr=False) == plain
    both = metrics.pixel_metrics(gts, preds, pr=True)
    assert list(both) == ["pixel_rocauc", "au_pro", "au_pro_001", "pixel_ap", "pixel_f1max", "pixel_f1max_threshold"]
    assert all(both[k] == plain[k] for k in plain)
    ref = pr.pr_metrics_ref(gts, preds)
    assert all(both[k] == ref[k] for k in ("pixel_ap", "pixel_f1max", "pixel_f1max_threshold"))
    full = metrics.pixel_pr_metrics(gts, preds)
    assert full == ref and list(full) == ["pixel_ap", "pixel_f1max", "pixel_f1max_threshold", "pixel_f1max_threshold_gt", "tp", "fp",
                                          "precision", "recall", "n_def", "n_ok"]


def test_calibrate_labelled_survives_save_and_load(monkeypatch, tmp_path):
    from cmdiad_amd import metrics, regions
    monkeypatch.setattr(metrics, "pixel_pr_metrics", lambda g, p: pr.pr_metrics_ref(np.asarray(g), np.asarray(p)))
    monkeypatch.setattr(metrics, "image_pr_metrics", pr.image_pr_metrics_ref)
    gts, maps = random_split(7, n=8, H=16, W=16)
    scores, labels = maps.reshape(8, -1).max(axis=1), gts.reshape(8, -1).any(axis=1).astype(int)
    cal = regions.calibrate_labelled(scores, labels, list(maps), list(gts), class_name="synthetic")
    pix, img = pr.pr_metrics_ref(gts, maps), pr.image_pr_metrics_ref(labels, scores)
    assert cal.pixel_threshold == np.nextafter(pix["pixel_f1max_threshold"], -np.inf)
    assert cal.image_threshold == np.nextafter(img["image_f1max_threshold"], -np.inf)
    assert (cal.n_images, cal.n_pixels, cal.class_name) == (8, maps.size, "synthetic")
    # the quantile fields mean what they mean for a quantile calibration: the fraction of defect-free values not above the threshold
    ok = maps[gts == 0]
    assert cal.pixel_quantile == int((ok <= cal.pixel_threshold).sum()) / ok.size
    ok_img = scores[labels == 0]
    assert cal.image_quantile == int((ok_img <= cal.image_threshold).sum()) / ok_img.size
    # the decision of the strict rule at that threshold is the F1-max decision
    assert int((maps[gts != 0] > cal.pixel_threshold).sum()) == pix["tp"] and int((ok > cal.pixel_threshold).sum()) == pix["fp"]
    assert np.array_equal(cal.decide(scores), scores >= img["image_f1max_threshold"])
    path = cal.save(str(tmp_path / "synthetic.cmdcal"))
    back = regions.Calibration.load(path)
    assert repr(back) == repr(cal) and back.pixel_threshold == cal.pixel_threshold and back.image_threshold == cal.image_threshold
    assert (back.pixel_quantile, back.image_quantile, back.n_images, back.n_pixels) == (cal.pixel_quantile, cal.image_quantile, 8, maps.size)
    with pytest.raises(ValueError, match="image labels"):
        regions.calibrate_labelled(scores, labels[:-1], maps, gts)
    with pytest.raises(ValueError, match="no image scores"):
        regions.calibrate_labelled([], [], maps[:0], gts[:0])


def test_calculate_metrics_is_what_it_was_without_the_flag_and_goes_to_the_device_module_with_it(monkeypatch):
    from cmdiad_amd import metrics
    from cmdiad_amd.feature_extractors.features import Features
    gts, preds = random_split(3, n=8, H=16, W=16)
    monkeypatch.delenv("CMDIAD_METRICS_DEVICE", raising=False)
    new = ("pixel_ap", "pixel_f1max", "image_ap", "image_f1max", "pr")
    off = bare_method(gts, preds)
    Features.calculate_metrics(off)
    assert not [k for k in new if hasattr(off, k)]
    explicit = bare_method(gts, preds)
    explicit.args.pr_metrics = False
    Features.calculate_metrics(explicit)
    assert not [k for k in new if hasattr(explicit, k)]
    # with the flag the host path still computes its three values and the new ones come from cmdiad_amd.metrics
    monkeypatch.setattr(metrics, "pixel_pr_metrics", lambda g, p: pr.pr_metrics_ref(np.stack(g), np.stack(p)))
    monkeypatch.setattr(metrics, "image_pr_metrics", pr.image_pr_metrics_ref)
    on = bare_method(gts, preds)
    on.args.pr_metrics = True
    Features.calculate_metrics(on)
    assert (on.pixel_rocauc, on.au_pro, on.au_pro_001, on.image_rocauc) == (off.pixel_rocauc, off.au_pro, off.au_pro_001, off.image_rocauc)
    pix = pr.pr_metrics_ref(gts, preds)
    img = pr.image_pr_metrics_ref(np.stack(on.image_labels), np.stack(on.image_preds))
    assert (on.pixel_ap, on.pixel_f1max, on.image_ap, on.image_f1max) == (pix["pixel_ap"], pix["pixel_f1max"], img["image_ap"], img["image_f1max"])
    assert on.pr == dict(pixel_ap=pix["pixel_ap"], pixel_f1max=pix["pixel_f1max"], pixel_f1max_threshold=pix["pixel_f1max_threshold"],
                         image_ap=img["image_ap"], image_f1max=img["image_f1max"], image_f1max_threshold=img["image_f1max_threshold"])
    # the device switch and the flag together: one pixel_metrics call with pr=True
    seen = []

    def stub(g, p, **kw):
        seen.append(kw)
        return dict(pixel_rocauc=0.25, au_pro=0.5, au_pro_001=0.75, pixel_ap=0.125, pixel_f1max=0.375, pixel_f1max_threshold=1.5)
    monkeypatch.setattr(metrics, "pixel_metrics", stub)
    monkeypatch.setenv("CMDIAD_METRICS_DEVICE", "1")
    dev = bare_method(gts, preds)
    dev.args.pr_metrics = True
    Features.calculate_metrics(dev)
    assert seen == [dict(pr=True)] and (dev.pixel_ap, dev.pixel_f1max, dev.image_ap) == (0.125, 0.375, img["image_ap"])
    plain = bare_method(gts, preds)
    Features.calculate_metrics(plain)
    assert seen == [dict(pr=True), {}] and not hasattr(plain, "pr")


def test_the_flag_is_no_default_and_no_stored_argument():
    from cmdiad_amd import evaluate, fitted
    assert evaluate.METRICS == ("image_rocauc", "pixel_rocauc", "au_pro", "au_pro_001")
    assert not hasattr(evaluate.mtfi_args(), "pr_metrics") and "pr_metrics" not in fitted.ARG_FIELDS
    assert evaluate.mtfi_args(pr_metrics=True).pr_metrics is True
    table = evaluate.metrics_table({"bagel": dict(image_rocauc=1.0, pixel_rocauc=1.0, au_pro=1.0, au_pro_001=1.0, pr=dict(pixel_ap=0.5))}, "m")
    assert "pixel_ap" not in str(table) and "pr" not in table
