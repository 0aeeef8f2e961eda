"""Defect regions and calibrated decisions from the score maps (docs/regions.md).

What scoring returns per sample is a float that means nothing by itself and a 224 x 224 float64 map.  This module turns them
into "this part is defective, here, this big":

  * ``calibrate`` takes the scores of DEFECT-FREE samples and returns two thresholds, nearest-rank quantiles of the image scores
    and of all their pixels (the pixels are sorted on the device, ``metrics.sort_values``); ``calibrate_labelled`` takes LABELLED
    samples instead and returns the two F1-max thresholds (docs/metrics.md);
  * ``find_regions`` thresholds maps on the device, labels the 8-connected components (``cmdiad_ccl_label``), and returns per
    image a fixed-size table of the strongest regions: label, area, box, peak and its position, centroid, score sum;
  * ``Calibration.save`` / ``load`` keep the thresholds in a ``.cmdcal`` file (the container of fitted.py) together with the
    digests of the fit's libraries, so that thresholds are never applied to another fit's scores.

The decision is always ``score > threshold``, strict.  The default quantiles (0.999 of the pixels, 1.0 of the images) are policy
knobs, not measured optima: with image_quantile = 1.0 every calibration sample passes as good, and nothing is claimed about
the detection rate either gives.
"""
import json
import math
import sys

import numpy as np

from . import fitted

FORMAT = "cmdiad-calibration"
MAX_REGIONS = 64
INT_FIELDS = ("label", "area", "x0", "y0", "x1", "y1", "peak_x", "peak_y")
VAL_FIELDS = ("peak", "score_sum", "cx", "cy")
RESULT_LISTS = ("image_preds", "image_labels", "pixel_preds", "pixel_labels", "predictions", "gts", "img_name")


class CalibrationMismatch(ValueError):
    """The calibration file is sound, but it belongs to another fit than the one it is loaded beside."""


def _finite(v, what):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{what}: {v!r} is not a threshold (NaN and infinity are refused)")
    return v


class RegionSpec:
    """pixel_threshold: a pixel is foreground iff score > pixel_threshold (one float, or one per image: a sequence / array).
    image_threshold: the sample is defective iff its image score > image_threshold (None: no decisions).  Components with fewer
    than min_area (>= 1) pixels are dropped; the max_regions (1..64) strongest of the others are reported."""

    def __init__(self, pixel_threshold, image_threshold=None, min_area=1, max_regions=16):
        pt = np.asarray(pixel_threshold, dtype=np.float64)
        if pt.ndim > 1 or pt.size == 0 or not np.isfinite(pt).all():
            raise ValueError(f"RegionSpec: pixel_threshold must be one finite float or one per image; got {pixel_threshold!r}")
        self.pixel_threshold = float(pt) if pt.ndim == 0 else pt.copy()
        self.image_threshold = None if image_threshold is None else _finite(image_threshold, "RegionSpec: image_threshold")
        if isinstance(min_area, bool) or int(min_area) != min_area or int(min_area) < 1:
            raise ValueError(f"RegionSpec: min_area must be an integer >= 1, got {min_area!r}")
        if isinstance(max_regions, bool) or int(max_regions) != max_regions or not 1 <= int(max_regions) <= MAX_REGIONS:
            raise ValueError(f"RegionSpec: max_regions must be an integer in 1..{MAX_REGIONS}, got {max_regions!r}")
        self.min_area, self.max_regions = int(min_area), int(max_regions)

    def __repr__(self):
        return (f"RegionSpec(pixel_threshold={self.pixel_threshold!r}, image_threshold={self.image_threshold!r}, "
                f"min_area={self.min_area}, max_regions={self.max_regions})")


def measure_fields(m_ints, m_vals):
    """One slot of a measurement table (m_ints [4], m_vals [20]; docs/regions.md) -> the 3-D fields of a region, in the units of
    the cloud that was measured: n_pts, n_tri, peak_valid, lo, hi, peak_xyz, area_3d, extent = hi - lo, centroid_3d = lo + s1 / n_pts,
    covariance = s2 / n_pts - (s1 / n_pts)(s1 / n_pts)^T (3 x 3, about the centroid) and principal_sigma = the square roots of its
    eigenvalues, ascending, clipped at 0.  The one place these are derived: the tests run it on the kernel's table and on the
    yardstick's alike.  A region without a valid point has zeros throughout."""
    mi, mv = np.asarray(m_ints, dtype=np.int32).reshape(4), np.asarray(m_vals, dtype=np.float64).reshape(20)
    n = int(mi[0])
    lo, hi = mv[0:3], mv[3:6]
    mean = mv[9:12] / n if n else np.zeros(3)
    s2 = np.empty((3, 3))
    s2[np.triu_indices(3)] = mv[12:18]
    s2 = np.triu(s2) + np.triu(s2, 1).T
    cov = s2 / n - np.outer(mean, mean) if n else np.zeros((3, 3))
    return dict(n_pts=n, n_tri=int(mi[1]), peak_valid=int(mi[2]), lo=lo.tolist(), hi=hi.tolist(), peak_xyz=mv[6:9].tolist(),
                area_3d=float(mv[18]), extent=(hi - lo).tolist(), centroid_3d=(lo + mean).tolist(), covariance=cov.tolist(),
                principal_sigma=np.sqrt(np.clip(np.linalg.eigvalsh(cov), 0.0, None)).tolist())


class Measures:
    """The measurement tables of n images on the host (docs/regions.md): m_ints [n,K,4] int32 (n_pts, n_tri, peak_valid, 0), m_vals
    [n,K,20] float64 (lo, hi, peak_xyz, s1, s2, area, 0), in the units of the cloud that was passed in."""

    def __init__(self, m_ints, m_vals):
        self.m_ints, self.m_vals = np.asarray(m_ints, dtype=np.int32), np.asarray(m_vals, dtype=np.float64)


class Regions:
    """The region tables of n images on the host: n_comp [n] (components before any filter), count [n] (components with area >=
    min_area), ints [n,K,8] int32 (label, area, x0, y0, x1, y1, peak_x, peak_y), vals [n,K,4] float64 (peak, score_sum, cx, cy),
    truncated [n] bool (count > K).  Slots behind min(count, K) are zero.  measures: a Measures when the regions were measured
    on an organised cloud, else None."""

    def __init__(self, n_comp, count, ints, vals, measures=None):
        self.n_comp, self.count = np.asarray(n_comp, dtype=np.int32), np.asarray(count, dtype=np.int32)
        self.ints, self.vals = np.asarray(ints, dtype=np.int32), np.asarray(vals, dtype=np.float64)
        self.truncated = self.count > self.ints.shape[1]
        self.measures = measures

    def __len__(self):
        return self.count.shape[0]

    def to_list(self):
        """Per image a list of dicts: the twelve fields and mean = score_sum / area; with measures, the fields of measure_fields."""
        out = []
        for i in range(len(self)):
            regs = []
            for k in range(min(int(self.count[i]), self.ints.shape[1])):
                d = {f: int(v) for f, v in zip(INT_FIELDS, self.ints[i, k])}
                d.update({f: float(v) for f, v in zip(VAL_FIELDS, self.vals[i, k])})
                d["mean"] = d["score_sum"] / d["area"]
                if self.measures is not None:
                    d.update(measure_fields(self.measures.m_ints[i, k], self.measures.m_vals[i, k]))
                regs.append(d)
            out.append(regs)
        return out


def as_spec(regions, min_area=1, max_regions=16):
    """A RegionSpec from a RegionSpec (returned as it is) or a Calibration."""
    if isinstance(regions, RegionSpec):
        return regions
    if isinstance(regions, Calibration):
        return RegionSpec(regions.pixel_threshold, regions.image_threshold, min_area, max_regions)
    raise TypeError(f"expected a RegionSpec or a Calibration, got {type(regions).__name__}")


def _device_maps(maps):
    import torch
    from . import metrics
    m = metrics._stacked(maps, "maps")
    if not m.is_floating_point():
        raise TypeError(f"maps: expected floating-point scores, got {m.dtype}")
    if not m.is_cuda:
        m = m.to(metrics._device())
    return m.to(torch.float64).contiguous()     # float32 widens exactly


def region_tables_device(maps, thr, min_area, max_regions, mask=None, nan_count=None, clouds=None, layout=None):
    """The device part, without a synchronisation: maps [n,H,W] f64 and thr (device f64, 1 or n values) -> (n_comp, count, ints,
    vals, nan_count) as device tensors.  BatchPredictor calls this at the end of its scoring tail.  clouds: the maps' organised
    clouds on the device (f32, [n,3,H,W] or [n,H,W,3]) -> the regions are measured on them as well and (m_ints, m_vals, bad_count)
    of ops.region_measure are appended to the tuple."""
    from . import ops
    mask, nan_count = ops.threshold_mask(maps, thr, mask, nan_count)
    labels, n_comp, comp_offset, comp_size, _ = ops.ccl_label(mask)
    count, ints, vals = ops.region_table(maps, labels, n_comp, comp_offset, comp_size, min_area, max_regions)
    if clouds is None:
        return n_comp, count, ints, vals, nan_count
    return (n_comp, count, ints, vals, nan_count) + tuple(ops.region_measure(labels, count, ints, clouds, layout=layout))


def _device_clouds(clouds, like):
    """Organised clouds as one contiguous float32 tensor on the maps' device: a tensor, numpy, or a list of [3,H,W] / [H,W,3]."""
    import torch
    if isinstance(clouds, (list, tuple)):
        clouds = torch.stack([torch.as_tensor(c) for c in clouds])
    c = torch.as_tensor(clouds)
    if c.dtype != torch.float32:
        raise TypeError(f"clouds must be float32 (the scanner's stored coordinates), got {c.dtype}")
    return c.to(like.device).contiguous()


def find_regions(maps, spec, clouds=None, layout=None):
    """maps: numpy, a tensor, or a list of [H,W] maps (float32 widens exactly; host inputs are uploaded) -> Regions.  ValueError
    when a map holds a NaN.  One host synchronisation at the end.  clouds: the maps' organised clouds, float32, [n,3,H,W] or
    [n,H,W,3] (a tensor, numpy, or a list of single clouds; layout= 'planar' | 'interleaved' where the shape does not tell) -> the
    Regions carry .measures, the regions in the clouds' units (docs/regions.md).  ValueError when the clouds' H, W differ from the
    maps' or a coordinate is not finite."""
    import torch
    from . import ops
    spec = as_spec(spec)
    m = _device_maps(maps)
    n = m.shape[0]
    pt = np.atleast_1d(np.asarray(spec.pixel_threshold, dtype=np.float64))
    if pt.size not in (1, n):
        raise ValueError(f"find_regions: {pt.size} pixel thresholds for {n} maps (one, or one per image)")
    K = spec.max_regions
    if clouds is not None:
        clouds = _device_clouds(clouds, m)
        if clouds.dim() != 4 or clouds.shape[0] != n:
            raise ValueError(f"find_regions: {n} maps need clouds [{n},3,H,W] or [{n},H,W,3], got {tuple(clouds.shape)}")
        layout = ops.cloud_layout(clouds, m.shape[1], m.shape[2], layout, "find_regions")
    if n == 0:
        return Regions(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, K, 8), np.int32), np.zeros((0, K, 4)),
                       Measures(np.zeros((0, K, 4), np.int32), np.zeros((0, K, 20))) if clouds is not None else None)
    thr = torch.from_numpy(pt.copy()).to(m.device)
    out = region_tables_device(m, thr, spec.min_area, spec.max_regions, clouds=clouds, layout=layout)
    n_comp, count, ints, vals, nan_count = out[:5]
    if int(nan_count.item()):
        raise ValueError(f"find_regions: the maps contain {int(nan_count.item())} NaN scores")
    measures = None
    if clouds is not None:
        if int(out[7].item()):
            raise ValueError(f"find_regions: the clouds contain {int(out[7].item())} points with a non-finite coordinate")
        measures = Measures(out[5].cpu().numpy(), out[6].cpu().numpy())
    return Regions(n_comp.cpu().numpy(), count.cpu().numpy(), ints.cpu().numpy(), vals.cpu().numpy(), measures)


# ------------------------------------------------------------------------------------------------ calibration
def quantile_index(q, n):
    """Index of the nearest-rank quantile in n sorted values: ceil(q n) - 1 clamped to [0, n - 1]
    (numpy's method="inverted_cdf")."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile {q!r} is outside [0, 1]")
    if n < 1:
        raise ValueError("a quantile of no values")
    return min(max(int(math.ceil(q * n)) - 1, 0), n - 1)


class Calibration:
    """Two thresholds and where they came from.  Decisions are `score > threshold`, strict."""

    def __init__(self, pixel_threshold, image_threshold, pixel_quantile, image_quantile, n_images, n_pixels, class_name=None):
        self.pixel_threshold = _finite(pixel_threshold, "Calibration: pixel_threshold")
        self.image_threshold = _finite(image_threshold, "Calibration: image_threshold")
        self.pixel_quantile, self.image_quantile = float(pixel_quantile), float(image_quantile)
        self.n_images, self.n_pixels, self.class_name = int(n_images), int(n_pixels), class_name

    def __repr__(self):
        return (f"Calibration(pixel_threshold={self.pixel_threshold!r}, image_threshold={self.image_threshold!r}, "
                f"pixel_quantile={self.pixel_quantile}, image_quantile={self.image_quantile}, n_images={self.n_images}, "
                f"n_pixels={self.n_pixels}, class_name={self.class_name!r})")

    def spec(self, min_area=1, max_regions=16):
        return RegionSpec(self.pixel_threshold, self.image_threshold, min_area, max_regions)

    def decide(self, image_scores):
        return np.asarray(image_scores, dtype=np.float64).reshape(-1) > self.image_threshold

    # ---- file
    def _meta(self):
        return dict(class_name=self.class_name, pixel_quantile=self.pixel_quantile, image_quantile=self.image_quantile,
                    n_images=self.n_images, n_pixels=self.n_pixels)

    def save(self, path, fit=None):
        """A .cmdcal file: the container of fitted.write_file with format "cmdiad-calibration", the thresholds as 0-dim float64
        arrays (bit for bit), the quantiles, counts and class name, and -- with `fit`, a .cmdfit path or a FittedClass -- the
        digest64 of every library array of that fit."""
        meta = self._meta()
        head = dict(meta, meta_digest=_meta_digest(meta), fit_libraries=_fit_digests(fit) if fit is not None else None)
        arrays = dict(pixel_threshold=np.asarray(self.pixel_threshold, dtype=np.float64).reshape(()),
                      image_threshold=np.asarray(self.image_threshold, dtype=np.float64).reshape(()))
        fitted.write_file(path, head, arrays, fmt=FORMAT)
        return path

    @classmethod
    def load(cls, path, fit=None):
        """FitFileError when the file is damaged, truncated or no calibration; with `fit`, CalibrationMismatch naming the first
        library whose digest differs from the one the calibration was saved beside."""
        head = read_header(path)
        vals = {}
        for name in ("pixel_threshold", "image_threshold"):
            a = fitted.read_array(path, name, head=head)
            e = fitted.array_entry(head, name, path)
            if a.shape != () or a.dtype != np.float64 or fitted.digest64_host(a) != int(e["digest64"], 16):
                raise fitted.FitFileError(f"{path}: array {name!r}: digest64: the payload does not match the header")
            vals[name] = float(a)
        if fit is not None:
            mine, theirs = _fit_digests(fit), head.get("fit_libraries")
            if not isinstance(theirs, dict):
                raise CalibrationMismatch(f"{path}: fit_libraries: the calibration was saved without a fit; it cannot be checked "
                                          "against one")
            for name in sorted(set(mine) | set(theirs)):
                if mine.get(name) != theirs.get(name):
                    raise CalibrationMismatch(f"{path}: fit_libraries.{name}: calibrated beside a fit whose {name} hashes to "
                                              f"{theirs.get(name)}, this fit's hashes to {mine.get(name)}")
        try:
            return cls(vals["pixel_threshold"], vals["image_threshold"], head["pixel_quantile"], head["image_quantile"],
                       head["n_images"], head["n_pixels"], head.get("class_name"))
        except (KeyError, TypeError, ValueError) as e:
            raise fitted.FitFileError(f"{path}: header: {e!r}") from None


def _meta_digest(meta):
    blob = json.dumps(meta, sort_keys=True).encode()
    return f"{fitted.digest64_host(np.frombuffer(blob, dtype=np.uint8)):016x}"


def read_header(path):
    """The validated header of a .cmdcal file: the container's own checks, the format name, and the digest of the fields that
    are not arrays."""
    head = fitted.read_header(path)
    if head.get("format") != FORMAT:
        raise fitted.FitFileError(f"{path}: format: {head.get('format')!r} is not {FORMAT!r}")
    meta = {k: head.get(k) for k in ("class_name", "pixel_quantile", "image_quantile", "n_images", "n_pixels")}
    if head.get("meta_digest") != _meta_digest(meta):
        raise fitted.FitFileError(f"{path}: meta_digest: the header's fields do not hash to {head.get('meta_digest')!r} (damaged)")
    return head


def _fit_digests(fit):
    """{library name: digest64 hex} of a stored fit (a path or a FittedClass)."""
    head = fit.header if hasattr(fit, "header") else fitted.read_header(fit)
    return {e["name"]: e["digest64"] for e in head["arrays"] if e["name"] in fitted.LIBRARIES}


def calibrate(image_scores, maps, pixel_quantile=0.999, image_quantile=1.0, class_name=None):
    """Thresholds from DEFECT-FREE samples: nearest-rank quantiles (element ceil(q N) - 1 of the sorted values, no interpolation:
    np.quantile(method="inverted_cdf")) of the image scores, on the host, and of every pixel of every map, sorted on the device
    and read with one gather.  ValueError on NaN or infinity."""
    import torch
    from . import metrics
    s = np.asarray(image_scores, dtype=np.float64).reshape(-1)
    if s.size == 0:
        raise ValueError("calibrate: no image scores")
    if not np.isfinite(s).all():
        raise ValueError("calibrate: the image scores contain NaN or infinity")
    m = _device_maps(maps)
    if m.shape[0] != s.size:
        raise ValueError(f"calibrate: {s.size} image scores and {m.shape[0]} maps")
    ii, ip = quantile_index(image_quantile, s.size), quantile_index(pixel_quantile, m.numel())
    ordered = metrics.sort_values(m)                  # raises on NaN / infinity
    pixel_thr = float(ordered[ip:ip + 1].cpu().numpy()[0])
    return Calibration(pixel_thr, float(np.sort(s)[ii]), pixel_quantile, image_quantile, s.size, m.numel(), class_name)


def calibrate_labelled(image_scores, image_labels, maps, gts, class_name=None):
    """Thresholds from LABELLED samples (a validation split with ground truth): at both levels the threshold that maximises F1
    (metrics.image_pr_metrics, metrics.pixel_pr_metrics; among equal F1 the highest), in the strict form of this module's
    decisions -- nextafter(v, -inf) of the F1-max score v, so that `score > threshold` is `score >= v`.  pixel_quantile and
    image_quantile record what they mean for a quantile calibration, the fraction of DEFECT-FREE values not above the threshold:
    (n_ok - fp) / n_ok.  n_images and n_pixels count all samples.  ValueError when a level lacks one of the two classes, a mask is
    not binary, or a score is NaN or infinite."""
    from . import metrics
    s = np.asarray(image_scores, dtype=np.float64).reshape(-1)
    lab = np.asarray(image_labels).reshape(-1)
    if s.size == 0:
        raise ValueError("calibrate_labelled: no image scores")
    m = metrics._stacked(maps, "maps")                # where it lives: the metric functions upload host inputs themselves
    if m.shape[0] != s.size or lab.size != s.size:
        raise ValueError(f"calibrate_labelled: {s.size} image scores, {lab.size} image labels and {m.shape[0]} maps")
    img = metrics.image_pr_metrics(lab, s)
    pix = metrics.pixel_pr_metrics(gts, m)
    return Calibration(pix["pixel_f1max_threshold_gt"], img["image_f1max_threshold_gt"], (pix["n_ok"] - pix["fp"]) / pix["n_ok"],
                       (img["n_ok"] - img["fp"]) / img["n_ok"], s.size, m.numel(), class_name)


def _truncate(method, name, length):
    held = getattr(method, name)
    if hasattr(held, "truncate"):      # features.PixelList
        held.truncate(length)
    else:
        del held[length:]


def calibrate_method(method, samples, **quantiles):
    """Score defect-free `samples` (what data.train() yields: sample or (sample, label)) through the drop-in object's own predict
    -- zero mask, label 0 --, complete the deferred micro-batches, calibrate on the new entries, and put the seven result lists
    back to their previous lengths: calculate_metrics never sees the calibration samples."""
    import torch
    samples = [s[0] if isinstance(s, (tuple, list)) and len(s) == 2 and not torch.is_tensor(s[0]) else s for s in samples]
    if not samples:
        raise ValueError("calibrate_method: no samples")
    before = {name: len(getattr(method, name)) for name in RESULT_LISTS}      # (reading them completes what was deferred)
    gt = method.gt_size
    try:
        with torch.no_grad():
            for k, sample in enumerate(samples):
                method.predict(sample, torch.zeros((1, gt, gt)), np.array([0]), [f"calibration/{k}"])
            scores = [np.asarray(v, dtype=np.float64).reshape(-1)[0] for v in method.image_preds[before["image_preds"]:]]
            maps = np.stack([np.asarray(p, dtype=np.float64) for p in method.predictions[before["predictions"]:]])
    finally:
        flush = getattr(method, "_flush", None)
        if flush is not None:
            flush("predict")
        for name, length in before.items():
            _truncate(method, name, length)
    if len(scores) != len(samples):
        raise RuntimeError(f"calibrate_method: {len(samples)} samples gave {len(scores)} scores")
    return calibrate(scores, maps, class_name=getattr(method, "class_name", None), **quantiles)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2 or argv[0] != "info":
        print("usage: python -m cmdiad_amd.regions info FILE", file=sys.stderr)
        return 2
    head = read_header(argv[1])
    out = {k: v for k, v in head.items() if k != "arrays"}
    for name in ("pixel_threshold", "image_threshold"):
        out[name] = float(fitted.read_array(argv[1], name, head=head))
    print(json.dumps(out, indent=2, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
