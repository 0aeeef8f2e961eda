"""Pixel-level metrics on the device: P-AUROC and AU-PRO (docs/metrics.md).

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
path with ``CMDIAD_METRICS_DEVICE=1``; without the switch it never imports this module.
"""
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
        if int(nonfinite.item()):
            raise ValueError("predictions contain NaN or infinity")
        if counts.tolist() != [self.n_ok, self.n_def]:
            raise RuntimeError(f"metrics split: {counts.tolist()} pixels listed, {[self.n_ok, self.n_def]} labelled")

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


def pixel_metrics(gts, predictions, num_thresholds=100):
    """-> dict(pixel_rocauc, au_pro, au_pro_001): one labelling, one split and one sort shared by the three; the two AU-PRO values
    come from the one curve through ``au_pro_util.trapezoid`` as ``calculate_au_pro`` computes them.  Synchronises."""
    T = _check_thresholds(num_thresholds)
    st = _Split(gts, predictions, need_binary=True)
    roc = st.roc_auc()
    fpr, pro = st.pro_curve(T)
    return dict(pixel_rocauc=roc, au_pro=au_pro_util.trapezoid(fpr, pro, x_max=0.3) / 0.3,
                au_pro_001=au_pro_util.trapezoid(fpr, pro, x_max=0.01) / 0.01)
