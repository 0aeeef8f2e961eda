"""Pixel metrics on the device against the host path (docs/metrics.md), at the size of a full class: 110 test images of 224 x 224.

Reports, on the same synthetic test split (blob defects on two thirds of the images, float32-origin scores widened to float64):
  - every entry point of csrc/metrics.hip by HIP events (median of --reps launches after a warm-up) with the bytes its contract
    moves at least once and the achieved bytes/s;
  - the whole `metrics.pixel_metrics` call, uploads and read-backs included (host clock around a synchronise);
  - the host path on the same inputs: roc_auc_score + calculate_au_pro twice, as Features.calculate_metrics runs them;
  - the entry points of csrc/pr_metrics.hip (run table, F1 maximum, overlap, detection counts) on the same split, the whole
    `metrics.pixel_metrics(pr=True)` call, and the host's average_precision_score + precision_recall_curve.
Usage: python tools/bench_metrics.py [--images 110] [--size 224] [--reps 20] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdiad_amd import metrics, ops  # noqa: E402


def synthetic_split(n, size, seed=0):
    rng = np.random.default_rng(seed)
    gts = np.zeros((n, size, size), dtype=np.float32)
    yy, xx = np.mgrid[0:size, 0:size]
    for i in range(n):
        if i % 3 == 2:
            continue
        for _ in range(int(rng.integers(1, 5))):
            cy, cx, r = rng.integers(0, size), rng.integers(0, size), rng.uniform(2, size / 10)
            gts[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    preds = (rng.normal(size=gts.shape) + 2.0 * gts * rng.random(gts.shape)).astype(np.float32)
    return [g for g in gts], [p for p in preds]


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=110)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    gts, preds = synthetic_split(a.images, a.size)
    dev = torch.device("cuda")
    masks = torch.from_numpy(np.stack(gts)).to(dev)
    scores = torch.from_numpy(np.stack(preds)).to(dev).double()
    px = masks.numel()

    labels, n_comp, comp_offset, comp_size, _ = ops.ccl_label(masks)
    total = int(comp_offset[-1])
    n_def = int(comp_size[:total].sum())
    n_ok = px - n_def
    ok_keys, def_score, def_comp, _, _ = ops.metrics_split(scores, labels, comp_offset, n_ok, n_def)
    unsorted = ok_keys.clone()
    ops.sort_u64_(ok_keys)
    T = 100
    pos = torch.from_numpy(np.linspace(0, n_ok - 1, num=T, dtype=int)).to(dev)
    thr = ops.keys_to_f64(ok_keys[pos])
    work = unsorted.clone()

    def sort_once():
        work.copy_(unsorted)
        ops.sort_u64_(work)

    # the precision-recall and detection entry points (csrc/pr_metrics.hip): the defect keys, their run table, and the overlap of the
    # ground truth with the maps thresholded at the F1-max score
    def_unsorted, _ = ops.f64_to_keys(def_score)
    def_keys = ops.sort_u64_(def_unsorted.clone())
    def_work = def_unsorted.clone()

    def sort_def_once():
        def_work.copy_(def_unsorted)
        ops.sort_u64_(def_work)

    run_key, run_first, run_fp, n_runs = ops.pr_runs(def_keys, ok_keys)
    R = int(n_runs)
    best = int(ops.pr_f1max(run_first, run_fp, n_runs, n_def)[0])
    f1_value = float(ops.keys_to_f64(run_key[best:best + 1].contiguous()).cpu()[0])
    pred_mask, _ = ops.threshold_mask(scores, torch.tensor([np.nextafter(f1_value, -np.inf)], dtype=torch.float64, device=dev))
    p_labels, _, p_offset, p_size, _ = ops.ccl_label(pred_mask)
    covered, hits = ops.region_overlap(labels, comp_offset, p_labels, p_offset, p_size, 1)
    cap = covered.numel()

    copy_ms = event_ms(lambda: work.copy_(unsorted), a.reps)
    rows = [
        # name, callable, bytes the contract moves at least once
        ("cmdiad_ccl_label (7 launches)", lambda: ops.ccl_label(masks), px * (4 + 4 * 2 * 4)),          # mask in; labels w, r/w, r, r/w
        ("cmdiad_metrics_split", lambda: ops.metrics_split(scores, labels, comp_offset, n_ok, n_def), px * (8 + 4) + n_ok * 8 + n_def * 12),
        ("cmdiad_sort_u64 (24 launches, + one copy)", sort_once, 8 * 24 * n_ok),                        # per pass: read 8n, read + write 16n
        ("cmdiad_auc_counts", lambda: ops.auc_counts(ok_keys, def_score), n_def * 8 + n_ok * 8),
        ("cmdiad_keys_to_f64 (sorted list)", lambda: ops.keys_to_f64(ok_keys), n_ok * 16),
        ("cmdiad_pro_hist", lambda: ops.pro_hist(thr, def_score, def_comp, total), n_def * 12 + total * (T + 1) * 4),
        ("cmdiad_sort_u64 (defect keys, + one copy)", sort_def_once, 8 * 24 * n_def),
        ("cmdiad_pr_runs (3 launches)", lambda: ops.pr_runs(def_keys, ok_keys), n_def * 16 + R * 16),      # keys read twice; the table
        ("cmdiad_pr_f1max (2 launches)", lambda: ops.pr_f1max(run_first, run_fp, n_runs, n_def), R * 8),
        ("cmdiad_region_overlap", lambda: ops.region_overlap(labels, comp_offset, p_labels, p_offset, p_size, 1), px * 8 + cap * 8),
        ("cmdiad_detection_counts", lambda: ops.detection_counts(comp_offset, covered, p_offset, p_size, hits, 1), cap * 12),
    ]
    def_copy_ms = event_ms(lambda: def_work.copy_(def_unsorted), a.reps)
    out = dict(images=a.images, size=a.size, pixels=px, n_ok=n_ok, n_defect=n_def, components=total, runs=R, kernels={})
    print(f"{a.images} x {a.size} x {a.size}: {n_ok} defect-free, {n_def} defect pixels, {total} components")
    print(f"{'entry point':46s} {'ms':>8s} {'MB':>9s} {'GB/s':>8s}")
    for name, fn, nbytes in rows:
        ms = event_ms(fn, a.reps)
        if fn is sort_once:
            ms -= copy_ms
        if fn is sort_def_once:
            ms -= def_copy_ms
        out["kernels"][name] = dict(ms=round(ms, 4), bytes=int(nbytes), gb_per_s=round(nbytes / ms / 1e6, 1))
        print(f"{name:46s} {ms:8.3f} {nbytes / 1e6:9.1f} {nbytes / ms / 1e6:8.1f}")

    def whole():
        t0 = time.perf_counter()
        m = metrics.pixel_metrics(gts, preds)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, m
    whole()
    runs = [whole() for _ in range(5)]
    out["pixel_metrics_s"] = round(float(np.median([r[0] for r in runs])), 4)
    out["device"] = runs[0][1]
    print(f"metrics.pixel_metrics, host lists in, three values out: {out['pixel_metrics_s'] * 1e3:.1f} ms (median of 5)")

    def whole_pr():
        t0 = time.perf_counter()
        m = metrics.pixel_metrics(gts, preds, pr=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, m
    whole_pr()
    runs = [whole_pr() for _ in range(5)]
    out["pixel_metrics_pr_s"] = round(float(np.median([r[0] for r in runs])), 4)
    out["device_pr"] = {k: runs[0][1][k] for k in ("pixel_ap", "pixel_f1max", "pixel_f1max_threshold")}
    print(f"metrics.pixel_metrics(pr=True), six values out: {out['pixel_metrics_pr_s'] * 1e3:.1f} ms (median of 5)")
    if not a.no_host:
        from sklearn.metrics import average_precision_score, precision_recall_curve
        lab, sc = np.concatenate([g.ravel() for g in gts]), np.concatenate([p.ravel() for p in preds])
        t0 = time.perf_counter()
        ap = average_precision_score(lab, sc)
        p, r, _ = precision_recall_curve(lab, sc)
        f1 = float(np.max(2 * p * r / np.maximum(p + r, 1e-300)))
        out["host_pr_s"] = round(time.perf_counter() - t0, 4)
        out["pixel_ap_diff"], out["pixel_f1max_diff"] = abs(ap - out["device_pr"]["pixel_ap"]), abs(f1 - out["device_pr"]["pixel_f1max"])
        print(f"host path (average_precision_score + precision_recall_curve): {out['host_pr_s'] * 1e3:.1f} ms; |AP difference| "
              f"{out['pixel_ap_diff']:.2e}, |F1-max difference| {out['pixel_f1max_diff']:.2e}")
    if not a.no_host:
        from sklearn.metrics import roc_auc_score

        from cmdiad_amd.utils.au_pro_util import calculate_au_pro
        lab, sc = np.concatenate([g.ravel() for g in gts]), np.concatenate([p.ravel() for p in preds])
        t0 = time.perf_counter()
        host = dict(pixel_rocauc=roc_auc_score(lab, sc), au_pro=calculate_au_pro(gts, preds)[0],
                    au_pro_001=calculate_au_pro(gts, preds, 0.01)[0])
        out["host_s"] = round(time.perf_counter() - t0, 4)
        out["host"] = host
        out["au_pro_identical"] = host["au_pro"] == out["device"]["au_pro"] and host["au_pro_001"] == out["device"]["au_pro_001"]
        out["pixel_rocauc_diff"] = abs(host["pixel_rocauc"] - out["device"]["pixel_rocauc"])
        print(f"host path (roc_auc_score + calculate_au_pro twice): {out['host_s'] * 1e3:.1f} ms; AU-PRO identical: "
              f"{out['au_pro_identical']}, |P-AUROC difference| {out['pixel_rocauc_diff']:.2e}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
