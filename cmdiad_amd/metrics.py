"""Pixel-level metrics on the device: P-AUROC and AU-PRO, and -- from the same labelling, split and sort -- average precision,
F1-max with its threshold and defect detection counts, at the pixel and the image level (docs/metrics.md).

The device does the index work -- connected-component labelling, the split into defect-free and defect pixels, the sort of the
defect-free scores, the counting passes -- and every one of its results is an integer or a sorted set, so nothing depends on the
order in which threads run.  The host finishes with the float64 expressions it uses today: P-AUROC is one correctly rounded
quotient of Python integers, the PRO curve is ``utils.au_pro_util._pro_curve_sampled``'s arithmetic on the counts, bit for bit.

Inputs are what ``Features`` collects -- lists of per-image numpy arrays -- or stacked numpy arrays or tensors ``[n,H,W]``; host
inputs are uploaded to the current device.  Ground-truth masks follow the host functions: for the PRO curve a pixel belongs to a
defect when its value is non-zero (``scipy.ndimage.label``), P-AUROC refuses masks with values other than 0 and 1
(``roc_auc_score`` refuses non-binary targets).

Every function here reads a few integers back (the number of components, of defect pixels, the flag words) to size the next
buffers: that is a host synchronisation, acceptable in a metric phase and nowhere else.  ``Features.calculate_metrics`` takes this
path with ``CMDIAD_METRICS_DEVICE=1``, and for the precision-recall numbers with ``args.pr_metrics``; with neither it never
imports this module.
"""
import math

import numpy as np
import torch

from . import ops
from .utils import au_pro_util

MAX_THRESHOLDS = ops.PRO_MAX_THRESHOLDS
MAX_HIST_BYTES = 1 << 30


def _stacked(x, what):
    """x -> tensor [n,H,W] where x lives (a list of per-image arrays / tensors is stacked)."""
    if isinstance(x, (list, tuple)) and len(x) and isinstance(x[0], torch.Tensor):
        x = torch.stack([t.detach() for t in x])
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3:
        raise ValueError(f"{what}: expected [n,H,W] (or a list of [H,W] images), got {tuple(x.shape)}")
    return x.detach()


def _device():
    return torch.device("cuda", torch.cuda.current_device())


_NONBINARY = "gts: P-AUROC takes binary masks (every value 0 or 1)"


def _masks(gts, need_binary=False):
    """-> (masks [n,H,W] float32 or uint8 on the device, nonbinary: bool, or None = ask the labelling's flag word).  A host input
    is checked on the host, and refused if need_binary, before anything is uploaded."""
    m = _stacked(gts, "gts")
    bad = None
    if not m.is_cuda or m.dtype not in (torch.float32, torch.uint8):
        bad = bool(((m != 0) & (m != 1)).any()) if m.dtype != torch.bool else False
        if bad and need_binary:
            raise ValueError(_NONBINARY)
    if m.dtype not in (torch.float32, torch.uint8):
        m = (m != 0).to(torch.uint8)
    if not m.is_cuda:
        m = m.to(_device())
    return m.contiguous(), bad


def _preds(predictions):
    p = _stacked(predictions, "predictions")
    if not p.is_floating_point():
        raise TypeError(f"predictions: expected floating-point scores, got {p.dtype}")
    if not p.is_cuda:
        p = p.to(_device())
    return p.to(torch.float64).contiguous()     # float32 widens exactly


def _check_thresholds(num_thresholds):
    if num_thresholds is None:
        raise NotImplementedError("the exact (unsampled) PRO curve is not offered on the device: use "
                                  "cmdiad_amd.utils.au_pro_util.calculate_au_pro(gts, predictions, num_thresholds=None)")
    T = int(num_thresholds)
    if T < 1 or T > MAX_THRESHOLDS:
        raise ValueError(f"num_thresholds = {T}: the device path takes 1..{MAX_THRESHOLDS} thresholds")
    return T


def average_precision(cnt, tp, fp, n_def):
    """AP from a run table (host integers): math.fsum over the runs of (cnt tp) / (n_def (tp + fp)), each term the correctly rounded
    quotient of two integers and the sum correctly rounded, so the value depends on no order.  While every numerator and
    denominator is below 2^53 both convert to float64 exactly and one vectorised division gives those quotients; past that the
    terms are divisions of Python integers."""
    cnt, tp, fp = (np.asarray(v, dtype=np.int64) for v in (cnt, tp, fp))
    n_def = int(n_def)
    if len(cnt) and int(cnt.max()) * int(tp.max()) < 1 << 53 and n_def * (int(tp.max()) + int(fp.max())) < 1 << 53:
        return math.fsum(((cnt * tp) / (n_def * (tp + fp))).tolist())
    return math.fsum((int(c) * int(t)) / (n_def * (int(t) + int(f))) for c, t, f in zip(cnt, tp, fp))


class _Split:
    """One labelling, one split and one sort of a test split: what all three metrics share."""

    def __init__(self, gts, predictions, need_binary=False):
        masks, bad = _masks(gts, need_binary)
        preds = _preds(predictions)
        if masks.shape != preds.shape:
            raise ValueError(f"gts {tuple(masks.shape)} and predictions {tuple(preds.shape)} differ in shape")
        labels, _, comp_offset, comp_size, nonbinary = ops.ccl_label(masks)
        self.total_comp = int(comp_offset[-1])                                    # host synchronisation
        self.comp_size = comp_size[:self.total_comp].cpu().numpy().astype(np.int64)
        self.nonbinary = bool(nonbinary.item()) if bad is None else bad
        if self.nonbinary and need_binary:
            raise ValueError(_NONBINARY)
        self.n_def = int(self.comp_size.sum())
        self.n_ok = preds.numel() - self.n_def
        self.ok_sorted, self.def_score, self.def_comp, counts, nonfinite = ops.metrics_split(preds, labels, comp_offset, self.n_ok,
                                                                                            self.n_def)
        ops.sort_u64_(self.ok_sorted)
        self._def_sorted = self._runs = None
        if int(nonfinite.item()):
            raise ValueError("predictions contain NaN or infinity")
        if counts.tolist() != [self.n_ok, self.n_def]:
            raise RuntimeError(f"metrics split: {counts.tolist()} pixels listed, {[self.n_ok, self.n_def]} labelled")

    @property
    def def_sorted(self):
        """The sorted keys of the defect scores, computed once and on demand (the precision-recall numbers alone need them)."""
        if self._def_sorted is None:
            keys, _ = ops.f64_to_keys(self.def_score)               # non-finite scores were refused by the split
            self._def_sorted = ops.sort_u64_(keys)
        return self._def_sorted

    def pr_runs(self):
        """-> (value [R] f64, first [R], fp [R]) of the run table on the host (docs/metrics.md), and its device tensors."""
        if self.nonbinary:
            raise ValueError(_NONBINARY)
        if self.n_ok == 0 or self.n_def == 0:
            raise ValueError("Only one class present in gts. Average precision and F1-max are not defined in that case.")
        if self._runs is None:
            run_key, run_first, run_fp, n_runs = ops.pr_runs(self.def_sorted, self.ok_sorted)
            R = int(n_runs.item())                                                  # host synchronisation
            if not 1 <= R <= self.n_def:
                raise RuntimeError(f"run table: {R} runs of {self.n_def} defect scores")
            value = ops.keys_to_f64(run_key[:R].contiguous()).cpu().numpy()
            self._runs = (value, run_first[:R].cpu().numpy().astype(np.int64), run_fp[:R].cpu().numpy().astype(np.int64),
                          run_first, run_fp, n_runs)
        return self._runs

    def pr_table(self):
        value, first, fp = self.pr_runs()[:3]
        tp = self.n_def - first
        cnt = np.diff(np.concatenate([first, [self.n_def]]))
        return value, cnt, tp, fp, self.n_def, self.n_ok

    def pr_metrics(self):
        """-> dict(ap, f1max, threshold, threshold_gt, tp, fp, precision, recall, n_def, n_ok): AP is math.fsum over the runs of one
        float64 division of two Python integers each, the F1 maximum is picked on the device by exact comparison."""
        value, cnt, tp, fp, n_def, n_ok = self.pr_table()
        run_first, run_fp, n_runs = self.pr_runs()[3:]
        r = int(ops.pr_f1max(run_first, run_fp, n_runs, n_def)[0].item())
        if not 0 <= r < len(value):
            raise RuntimeError(f"F1 maximum: run {r} of {len(value)}")
        ap = average_precision(cnt, tp, fp, n_def)
        t, f = int(tp[r]), int(fp[r])
        return dict(ap=ap, f1max=(2 * t) / (t + f + n_def), threshold=float(value[r]),
                    threshold_gt=float(np.nextafter(value[r], -np.inf)), tp=t, fp=f, precision=t / (t + f), recall=t / n_def,
                    n_def=n_def, n_ok=n_ok)

    def auc_counts(self):
        if self.nonbinary:
            raise ValueError(_NONBINARY)
        if self.n_ok == 0 or self.n_def == 0:
            raise ValueError("Only one class present in gts. ROC AUC score is not defined in that case.")
        return int(ops.auc_counts(self.ok_sorted, self.def_score).item())

    def roc_auc(self):
        return self.auc_counts() / (2 * self.n_ok * self.n_def)      # Python integers: the quotient is correctly rounded

    def histogram(self, T):
        """-> (pos [T] int, thr [T] f64, hist [components, T+1] int64), all on the host."""
        if self.n_ok == 0:
            raise ValueError("the PRO curve takes its thresholds from the defect-free pixels: there is none")
        if self.total_comp * (T + 1) * 4 > MAX_HIST_BYTES:
            raise ValueError(f"{self.total_comp} components x {T + 1} bins: the histogram table would be above 1 GiB")
        pos = np.linspace(0, self.n_ok - 1, num=T, dtype=int)
        thr = ops.keys_to_f64(self.ok_sorted[torch.from_numpy(pos).to(self.ok_sorted.device)])
        hist = ops.pro_hist(thr, self.def_score, self.def_comp, self.total_comp)
        return pos, thr.cpu().numpy(), hist.cpu().numpy().astype(np.int64)

    def pro_curve(self, T):
        pos, thr, hist = self.histogram(T)
        # bin b = thresholds strictly below the score, so score > thr[j]  <=>  b >= j + 1: a suffix sum over the bins
        above = np.cumsum(hist[:, ::-1], axis=1)[:, ::-1][:, 1:]
        le = self.comp_size[:, None] - above                     # = searchsorted(component scores, thr, side="right")
        fpr = 1.0 - (pos + 1) / self.n_ok
        pro = np.zeros(len(thr))
        for c in range(self.total_comp):                         # au_pro_util._pro_curve_sampled's expressions, in its component order
            pro += 1.0 - le[c] / int(self.comp_size[c])
        pro /= max(self.total_comp, 1)
        return np.concatenate([fpr[::-1], [1.0]]), np.concatenate([pro[::-1], [1.0]])


def connected_components(masks):
    """masks [n,H,W] (non-zero = foreground) -> (labels [n,H,W] int32, n_comp [n] int32, comp_size [all components] int32), device
    tensors.  8-connected; the components of an image are numbered 1..n_comp in raster order of their first pixel, as
    ``scipy.ndimage.label(mask, np.ones((3, 3)))`` numbers them; comp_size lists the pixel counts image after image.  Reading the
    number of components back is a host synchronisation."""
    m, _ = _masks(masks)
    labels, n_comp, comp_offset, comp_size, _ = ops.ccl_label(m)
    return labels, n_comp, comp_size[:int(comp_offset[-1])]


def sort_values(x):
    """x (any shape, numpy or tensor) -> its values as a sorted float64 device tensor; -0.0 comes back as +0.0.  Raises ValueError on
    NaN or infinity (a host synchronisation: the flag word is read back)."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if not t.is_cuda:
        t = t.to(_device())
    keys, nonfinite = ops.f64_to_keys(t.detach().to(torch.float64).reshape(-1).contiguous())
    ops.sort_u64_(keys)
    if int(nonfinite.item()):
        raise ValueError("sort_values: the input contains NaN or infinity")
    return ops.keys_to_f64(keys)


def auc_counts(gts, predictions):
    """-> (S, n_ok, n_defect) as Python integers, S = sum over defect pixels of #(ok < s) + #(ok <= s): P-AUROC = S / (2 n_ok n_defect)."""
    st = _Split(gts, predictions, need_binary=True)
    return st.auc_counts(), st.n_ok, st.n_def


def pixel_roc_auc(gts, predictions):
    """Pixel-level AUROC, ``roc_auc_score(gts.ravel(), predictions.ravel())`` up to its own summation error.  ValueError when a mask
    value is neither 0 nor 1, when there is no defect pixel or no defect-free pixel, or on non-finite scores.  Synchronises."""
    return _Split(gts, predictions, need_binary=True).roc_auc()


def pro_histogram(gts, predictions, num_thresholds=100):
    """The integers behind the PRO curve, on the host: (pos [T], thr [T] f64, hist [components, T+1] int64, comp_size [components]);
    hist[c][b] = pixels of component c with exactly b thresholds strictly below their score."""
    T = _check_thresholds(num_thresholds)
    st = _Split(gts, predictions)
    return st.histogram(T) + (st.comp_size,)


def pro_curve(gts, predictions, num_thresholds=100):
    """(fpr, pro) of ``au_pro_util._pro_curve_sampled``, bit for bit.  ``num_thresholds=None`` (the exact curve) is a host
    function only; at most 1024 thresholds; a histogram table above 1 GiB is refused.  Synchronises."""
    T = _check_thresholds(num_thresholds)
    return _Split(gts, predictions).pro_curve(T)


def pixel_metrics(gts, predictions, num_thresholds=100, pr=False):
    """-> dict(pixel_rocauc, au_pro, au_pro_001): one labelling, one split and one sort shared by the three; the two AU-PRO values
    come from the one curve through ``au_pro_util.trapezoid`` as ``calculate_au_pro`` computes them.  pr=True: the dict also carries
    pixel_ap, pixel_f1max and pixel_f1max_threshold (``pixel_pr_metrics``) from the same labelling, split and sort.  Synchronises."""
    T = _check_thresholds(num_thresholds)
    st = _Split(gts, predictions, need_binary=True)
    roc = st.roc_auc()
    fpr, pro = st.pro_curve(T)
    out = dict(pixel_rocauc=roc, au_pro=au_pro_util.trapezoid(fpr, pro, x_max=0.3) / 0.3,
               au_pro_001=au_pro_util.trapezoid(fpr, pro, x_max=0.01) / 0.01)
    if pr:
        m = st.pr_metrics()
        out.update(pixel_ap=m["ap"], pixel_f1max=m["f1max"], pixel_f1max_threshold=m["threshold"])
    return out


# ------------------------------------------------------------------------------------------------ precision-recall
def pr_table(gts, predictions):
    """The run table of the defect scores on the host, runs in ascending order of their value: (value [R] f64, cnt [R], tp [R],
    fp [R], n_def, n_ok) -- per distinct defect score v the number of defect scores equal to it, of defect scores >= v and of
    defect-free scores >= v.  Masks must be binary; ValueError when one of the two classes is missing or a score is not finite."""
    return _Split(gts, predictions, need_binary=True).pr_table()


def _named(m, prefix):
    out = {f"{prefix}_ap": m["ap"], f"{prefix}_f1max": m["f1max"], f"{prefix}_f1max_threshold": m["threshold"],
           f"{prefix}_f1max_threshold_gt": m["threshold_gt"]}
    out.update({k: m[k] for k in ("tp", "fp", "precision", "recall", "n_def", "n_ok")})
    return out


def pixel_pr_metrics(gts, predictions):
    """-> dict(pixel_ap, pixel_f1max, pixel_f1max_threshold, pixel_f1max_threshold_gt, tp, fp, precision, recall, n_def, n_ok).
    pixel_ap = sum over the distinct defect scores of (recall step) x precision, ``average_precision_score`` up to its summation
    error; pixel_f1max = the largest F1 over all thresholds, attained by ``score >= pixel_f1max_threshold`` and, in the strict form
    the regions module decides with, by ``score > pixel_f1max_threshold_gt`` (= nextafter(threshold, -inf)); among equal F1 the
    highest threshold.  tp, fp, precision and recall are those of that threshold.  Synchronises."""
    return _named(_Split(gts, predictions, need_binary=True).pr_metrics(), "pixel")


def _host_vector(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).reshape(-1)


def image_pr_metrics(image_labels, image_scores):
    """The same numbers over one score per image: label non-zero = defective.  -> dict(image_ap, image_f1max,
    image_f1max_threshold, image_f1max_threshold_gt, tp, fp, precision, recall, n_def, n_ok), through the entry points of the
    pixel level on [n,1,1] maps."""
    labels, scores = _host_vector(image_labels), _host_vector(image_scores)
    if labels.size != scores.size:
        raise ValueError(f"image_pr_metrics: {labels.size} labels and {scores.size} scores")
    if not np.issubdtype(scores.dtype, np.floating):
        raise TypeError(f"image_scores: expected floating-point scores, got {scores.dtype}")
    masks = (labels != 0).astype(np.uint8).reshape(-1, 1, 1)
    return _named(_Split(masks, np.ascontiguousarray(scores).reshape(-1, 1, 1), need_binary=True).pr_metrics(), "image")


class DetectionCounts:
    """per_image [n,4] int32 (n_gt, n_detected, n_pred, n_false); covered and gt_size per ground-truth component (image after image,
    in label order); hits and pred_size per KEPT predicted component (size >= min_area); the four totals."""

    def __init__(self, per_image, covered, gt_size, hits, pred_size):
        self.per_image = np.asarray(per_image, dtype=np.int32).reshape(-1, 4)
        self.covered, self.gt_size = np.asarray(covered, dtype=np.int64), np.asarray(gt_size, dtype=np.int64)
        self.hits, self.pred_size = np.asarray(hits, dtype=np.int64), np.asarray(pred_size, dtype=np.int64)
        self.n_gt, self.n_detected, self.n_pred, self.n_false = (int(v) for v in self.per_image.astype(np.int64).sum(axis=0))

    def totals(self):
        return dict(n_gt=self.n_gt, n_detected=self.n_detected, n_pred=self.n_pred, n_false=self.n_false)


def detection_counts(gts, maps, pixel_threshold, min_area=1):
    """How many ground-truth defects a thresholded map catches.  Predicted mask = maps > pixel_threshold (strict; one threshold or
    one per image), its 8-connected components of at least min_area pixels are the reported regions; the ground-truth components
    are those of gts != 0.  A ground-truth component is detected when one of its pixels lies in a reported region, a reported
    region is false when it holds no ground-truth pixel.  -> DetectionCounts.  ValueError when a map holds a NaN.  Synchronises."""
    min_area = int(min_area)
    if min_area < 1:
        raise ValueError(f"detection_counts: min_area = {min_area} (>= 1)")
    masks, _ = _masks(gts)
    m = _stacked(maps, "maps")
    if not m.is_floating_point():
        raise TypeError(f"maps: expected floating-point scores, got {m.dtype}")
    m = (m if m.is_cuda else m.to(_device())).to(torch.float64).contiguous()
    if masks.shape != m.shape:
        raise ValueError(f"gts {tuple(masks.shape)} and maps {tuple(m.shape)} differ in shape")
    n = m.shape[0]
    pt = np.atleast_1d(np.asarray(pixel_threshold, dtype=np.float64))
    if pt.ndim != 1 or pt.size not in (1, n) or not np.isfinite(pt).all():
        raise ValueError(f"detection_counts: pixel_threshold must be one finite float or one per image ({n}); got {pixel_threshold!r}")
    if n == 0:
        z = np.zeros(0, np.int64)
        return DetectionCounts(np.zeros((0, 4), np.int32), z, z, z, z)
    thr = torch.from_numpy(pt.copy()).to(m.device)
    pred_mask, nan_count = ops.threshold_mask(m, thr)
    p_labels, _, p_offset, p_size, _ = ops.ccl_label(pred_mask)
    g_labels, _, g_offset, g_size, _ = ops.ccl_label(masks)
    covered, hits = ops.region_overlap(g_labels, g_offset, p_labels, p_offset, p_size, min_area)
    counts = ops.detection_counts(g_offset, covered, p_offset, p_size, hits, min_area)
    if int(nan_count.item()):                                                       # host synchronisation
        raise ValueError(f"detection_counts: the maps contain {int(nan_count.item())} NaN scores")
    n_g, n_p = int(g_offset[-1]), int(p_offset[-1])
    p_size, hits = p_size[:n_p].cpu().numpy(), hits[:n_p].cpu().numpy()
    kept = p_size >= min_area
    return DetectionCounts(counts.cpu().numpy(), covered[:n_g].cpu().numpy(), g_size[:n_g].cpu().numpy(), hits[kept], p_size[kept])
