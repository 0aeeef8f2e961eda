"""The independent yardstick of the precision-recall numbers and the detection counts (cmdiad_amd/metrics.py, csrc/pr_metrics.hip;
docs/metrics.md), numpy / scipy / fractions only: the run table comes from np.unique and np.searchsorted, AP from math.fsum over
one float64 division of Python integers per run, the F1 maximum from fractions.Fraction, the detection counts from
scipy.ndimage.label.  test_prmetrics_cpu.py validates this file against scikit-learn; test_gpu_prmetrics.py holds the kernels to it."""
import math
from fractions import Fraction

import numpy as np
from scipy.ndimage import label

STRUCTURE = np.ones((3, 3), dtype=int)


def canonical(x):
    """-0.0 -> +0.0: the two zeros are one value."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x == 0.0, 0.0, x)


def run_table_from_lists(defect, ok):
    """defect scores and defect-free scores (any order) -> (value [R], first [R], fp [R]) in ascending order of the value."""
    d, ok = np.sort(canonical(defect).ravel()), np.sort(canonical(ok).ravel())
    value, first = np.unique(d, return_index=True)
    fp = len(ok) - np.searchsorted(ok, value, side="left")
    return value, first.astype(np.int64), fp.astype(np.int64)


def split_lists(gts, preds):
    """masks (defect = value != 0; the callers pass binary masks) and scores -> (defect scores, defect-free scores)."""
    g, p = np.asarray(gts), np.asarray(preds, dtype=np.float64)
    return p[g != 0], p[g == 0]


def pr_table_ref(gts, preds):
    """-> (value, cnt, tp, fp, n_def, n_ok)"""
    d, ok = split_lists(gts, preds)
    value, first, fp = run_table_from_lists(d, ok)
    n_def = int(d.size)
    return value, np.diff(np.concatenate([first, [n_def]])), n_def - first, fp, n_def, int(ok.size)


def ap_ref(cnt, tp, fp, n_def):
    return math.fsum((int(c) * int(t)) / (n_def * (int(t) + int(f))) for c, t, f in zip(cnt, tp, fp))


def f1max_ref(tp, fp, n_def):
    """-> the run with the largest 2 tp / (tp + fp + n_def) as a Fraction; among equal fractions the largest index."""
    best, at = None, -1
    for r, (t, f) in enumerate(zip(tp, fp)):
        q = Fraction(2 * int(t), int(t) + int(f) + int(n_def))
        if best is None or q >= best:
            best, at = q, r
    return at


def pr_metrics_ref(gts, preds, prefix="pixel"):
    """The dict of metrics.pixel_pr_metrics / image_pr_metrics."""
    value, cnt, tp, fp, n_def, n_ok = pr_table_ref(gts, preds)
    if n_def == 0 or n_ok == 0:
        raise ValueError("Only one class present")
    r = f1max_ref(tp, fp, n_def)
    t, f = int(tp[r]), int(fp[r])
    return {f"{prefix}_ap": ap_ref(cnt, tp, fp, n_def), f"{prefix}_f1max": (2 * t) / (t + f + n_def),
            f"{prefix}_f1max_threshold": float(value[r]), f"{prefix}_f1max_threshold_gt": float(np.nextafter(value[r], -np.inf)),
            "tp": t, "fp": f, "precision": t / (t + f), "recall": t / n_def, "n_def": n_def, "n_ok": n_ok}


def image_pr_metrics_ref(image_labels, image_scores):
    lab, s = np.asarray(image_labels).reshape(-1), np.asarray(image_scores, dtype=np.float64).reshape(-1)
    return pr_metrics_ref((lab != 0).astype(np.uint8), s, "image")


def detection_ref(gts, maps, thr, min_area=1):
    """-> (per_image [n,4], covered, gt_size per ground-truth component, hits, pred_size per KEPT predicted component).  thr: one
    value or one per image; predicted mask = maps > thr."""
    gts, maps = np.asarray(gts), np.asarray(maps, dtype=np.float64)
    thr = np.broadcast_to(np.atleast_1d(np.asarray(thr, dtype=np.float64)), (len(maps),))
    per, covered, gt_size, hits, pred_size = [], [], [], [], []
    for g, m, t in zip(gts, maps, thr):
        gl, ng = label(g != 0, STRUCTURE)
        pl, npred = label(m > t, STRUCTURE)
        psize = np.bincount(pl.ravel(), minlength=npred + 1)
        kept = psize >= min_area
        kept[0] = False
        in_kept = kept[pl]
        cov = np.bincount(gl[in_kept].ravel(), minlength=ng + 1)[1:]
        hit = np.bincount(pl[(gl > 0) & in_kept].ravel(), minlength=npred + 1)
        per.append([ng, int((cov > 0).sum()), int(kept.sum()), int((kept & (hit == 0)).sum())])
        covered.append(cov)
        gt_size.append(np.bincount(gl.ravel(), minlength=ng + 1)[1:])
        hits.append(hit[kept])
        pred_size.append(psize[kept])
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)   # noqa: E731
    return np.array(per, dtype=np.int32).reshape(-1, 4), cat(covered), cat(gt_size), cat(hits), cat(pred_size)


# The two Farey neighbours of the F1 comparison: (tp, fp) of two runs at n_def = 2^28 whose F1 fractions differ by 5.7e-18 and are
# one float64.
FAREY_N_DEF = 1 << 28
FAREY_A = (96720567, 278244958)
FAREY_B = (82289257, 196676841)
