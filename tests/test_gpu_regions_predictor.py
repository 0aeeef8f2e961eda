"""GPU: defect regions and decisions at the end of BatchPredictor's scoring tail, through FittedClass.predictor, and in the class loop
(evaluate.ClassRun) -- against the yardstick tests/regions_ref.py run on the maps the same step returned.  The fit is the smallest
one tests/test_gpu_fitted.py makes (batch 2), built once per module."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as rr  # noqa: E402
from test_gpu_fitted import build, extractor  # noqa: E402,F401  (extractor: the module-scoped backbone fixture)

from cmdiad_amd import engine as eng  # noqa: E402
from cmdiad_amd import evaluate as ev  # noqa: E402
from cmdiad_amd import fitted, regions  # noqa: E402
from cmdiad_amd.predictor import BatchPredictor  # noqa: E402
from cmdiad_amd.synth import SyntheticClass  # noqa: E402
from oracle import nets  # noqa: E402

DEV = "cuda"
NAME = "DINO+Point_MAE"


@pytest.fixture(scope="module")
def fit(extractor, tmp_path_factory):  # noqa: F811
    data = SyntheticClass("bagel", 3, 2)
    m = build(NAME, extractor)
    for sample, _ in data.train():
        m.add_sample_to_mem_bank(sample, class_name=data.name)
    m.run_coreset()
    for sample, _ in data.train():
        m.add_sample_to_late_fusion_mem_bank(sample)
    m.run_late_fusion()
    items = list(data.test())
    path = str(tmp_path_factory.mktemp("regions_fit") / "bagel.cmdfit")
    m.save_fit(path)
    a = m.args
    f = types.SimpleNamespace(method=m, path=path, rgb=torch.cat([it[0][0] for it in items]).to(DEV),
                              pcs=torch.cat([it[0][1] for it in items]).to(DEV),
                              lam=(a.xyz_s_lambda, a.xyz_smap_lambda, a.rgb_s_lambda, a.rgb_smap_lambda),
                              stats=dict(xyz_mean=float(m.xyz_mean), xyz_std=float(m.xyz_std), rgb_mean=float(m.rgb_mean),
                                         rgb_std=float(m.rgb_std)))
    f.make = lambda **kw: BatchPredictor(m._engine, eng.Bank(m.patch_xyz_lib.to(DEV)), eng.Bank(m.patch_rgb_lib.to(DEV)), f.stats,
                                         m.detect_fuser, m.seg_fuser, lambdas=f.lam, batch=2, **kw)
    f.scores, f.maps = f.make(use_graph=False).predict_batch(f.rgb, f.pcs)          # regions=None: the parent's outputs
    assert np.isfinite(f.scores).all() and np.ptp(f.maps) > 0
    f.cal = regions.Calibration(float(np.quantile(f.maps, 0.9)), float(f.scores.mean()), 0.9, 0.5, 2, f.maps.size, "bagel")
    return f


def assert_regions(got, maps, thr, min_area=1, K=16):
    want = rr.region_table(maps, thr, min_area, K)
    assert want["count"].sum() >= 1, want["count"]               # never an empty comparison
    rr.assert_table_equal(got, want)
    return want


def test_regions_leave_scores_and_maps_bit_identical(fit):
    spec = fit.cal.spec(min_area=2, max_regions=8)
    t = fit.make(use_graph=False, regions=spec).submit(fit.rgb, fit.pcs)
    scores, maps = t.wait()
    assert scores.tobytes() == fit.scores.tobytes() and maps.tobytes() == fit.maps.tobytes()
    assert_regions(t.regions(), maps, fit.cal.pixel_threshold, 2, 8)
    assert t.decisions().dtype == bool and np.array_equal(t.decisions(), scores > fit.cal.image_threshold)
    assert t.decisions().tolist() == [bool(s > fit.cal.image_threshold) for s in scores] and len(set(t.decisions().tolist())) == 2
    # without an image threshold there are no decisions; without regions= no regions
    t = fit.make(use_graph=False, regions=regions.RegionSpec(fit.cal.pixel_threshold)).submit(fit.rgb, fit.pcs)
    with pytest.raises(RuntimeError, match="image threshold"):
        t.decisions()
    t = fit.make(use_graph=False).submit(fit.rgb, fit.pcs)
    with pytest.raises(RuntimeError, match="regions="):
        t.regions()
    with pytest.raises(ValueError, match="ONE pixel threshold"):
        fit.make(use_graph=False, regions=regions.RegionSpec([0.1, 0.2]))
    with pytest.raises(ValueError, match="infinity"):
        fit.make(use_graph=False, regions=fit.cal).set_thresholds(float("inf"))


def test_set_thresholds_between_steps_of_the_graph_pipeline(fit):
    """With graphs on, stages 1 and 2 are captured and both buffer sets replay; the region tail itself is NOT captured (it is
    launched eagerly behind each replay, docs/regions.md), so this covers the ordering of set_thresholds against steps already
    submitted and the tables of pipelined steps -- not a graph replay of the region kernels, which the package does not do."""
    p = fit.make(use_graph=True, regions=fit.cal)
    second = float(np.quantile(fit.maps, 0.97))
    assert second > fit.cal.pixel_threshold
    second_image = float(fit.scores.max()) + 1.0
    t1 = p.submit(fit.rgb, fit.pcs)
    t2 = p.submit(fit.rgb, fit.pcs)
    p.set_thresholds(second, second_image)
    t3 = p.submit(fit.rgb, fit.pcs)
    assert p.use_graph and p.sets is not None and p.step_no == 3            # stages 1 and 2 captured; both buffer sets used
    (s1, m1), (s2, m2), (s3, m3) = t1.wait(), t2.wait(), t3.wait()
    assert s1.tobytes() == s2.tobytes() == s3.tobytes() and m1.tobytes() == m2.tobytes() == m3.tobytes()   # both sets, every replay
    assert np.allclose(s1, fit.scores, rtol=1e-6, atol=1e-9) and np.ptp(m1) > 0
    first = assert_regions(t1.regions(), m1, fit.cal.pixel_threshold)
    assert_regions(t2.regions(), m2, fit.cal.pixel_threshold)
    third = assert_regions(t3.regions(), m3, second)
    assert not np.array_equal(first["ints"], third["ints"])                  # the new threshold changed the tables
    assert np.array_equal(t1.decisions(), s1 > fit.cal.image_threshold) and not t3.decisions().any()


def test_return_maps_false(fit):
    p = fit.make(use_graph=False, regions=fit.cal, return_maps=False)
    assert all(m is None for _, m in p.ring)
    t = p.submit(fit.rgb, fit.pcs)
    scores, maps = t.wait()
    assert maps is None and scores.tobytes() == fit.scores.tobytes()
    assert_regions(t.regions(), fit.maps, fit.cal.pixel_threshold)
    assert np.array_equal(t.decisions(), fit.scores > fit.cal.image_threshold)


def test_fitted_class_predictor_forwards_regions(fit):
    fc = fitted.FittedClass(fit.path)
    t = fc.predictor(fit.method._engine, batch=2, use_graph=False, regions=fit.cal, return_maps=True).submit(fit.rgb, fit.pcs)
    want = fit.make(use_graph=False, regions=fit.cal).submit(fit.rgb, fit.pcs)
    assert t.wait()[1].tobytes() == fit.maps.tobytes()
    a, b = t.regions(), want.regions()
    for f in ("n_comp", "count", "ints", "vals", "truncated"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert np.array_equal(t.decisions(), want.decisions())
    assert fc.predictor(fit.method._engine, batch=2, use_graph=False, return_maps=False).submit(fit.rgb, fit.pcs).wait()[1] is None


def test_class_loop_calibrates_and_writes_regions(extractor, tmp_path):  # noqa: F811
    weights = (None, None, nets.synth_state_dict("halluc", 51))
    fits, out1, out2 = str(tmp_path / "fits"), str(tmp_path / "r1"), str(tmp_path / "r2")
    data = lambda: SyntheticClass("rope", 5, 4, index=8)  # noqa: E731
    common = dict(f_coreset=0.1, random_state=3, min_area=2, max_regions=8)
    run = ev.ClassRun(ev.mtfi_args(save_fit_dir=fits, calibration_holdout=2, regions_dir=out1, **common), data(), weights=weights,
                      extractor=extractor).fit_device().fit_host().predict()
    first = run.result()
    assert sorted(os.listdir(fits)) == ["rope.cmdcal", "rope.cmdfit"] and os.listdir(out1) == ["rope.regions.json"]
    assert first["n_train"] == 3 and first["n_test"] == 4 and "calibration" in first["seconds"]
    cal = regions.Calibration.load(os.path.join(fits, "rope.cmdcal"), fit=os.path.join(fits, "rope.cmdfit"))
    assert (cal.n_images, cal.n_pixels, cal.pixel_quantile, cal.image_quantile, cal.class_name) == (2, 2 * 224 * 224, 0.999, 1.0, "rope")
    m = run.method
    assert len(m.predictions) == 4 and len(m.image_preds) == 4 and len(m.gts) == 4            # the held-out samples left no trace
    doc = json.load(open(os.path.join(out1, "rope.regions.json")))
    assert doc["thresholds"]["pixel_threshold"] == cal.pixel_threshold and doc["thresholds"]["image_threshold"] == cal.image_threshold
    maps = np.stack(m.predictions)
    want = rr.region_table(maps, cal.pixel_threshold, 2, 8)
    scores = np.asarray(m.image_preds, dtype=np.float64).reshape(-1)
    tally = dict(tp=0, fp=0, tn=0, fn=0)
    for i, img in enumerate(doc["images"]):
        assert (img["index"], img["n_comp"], img["count"]) == (i, want["n_comp"][i], want["count"][i])
        assert img["image_score"] == scores[i] and img["decision"] == bool(scores[i] > cal.image_threshold)
        assert img["img_name"] == str(np.asarray(m.img_name).reshape(-1)[i]) and img["label"] == int(np.asarray(m.image_labels).reshape(-1)[i])
        tally[("t" if img["decision"] == bool(img["label"]) else "f") + ("p" if img["decision"] else "n")] += 1
        assert len(img["regions"]) == len(want["regions"][i])
        for got, c in zip(img["regions"], want["regions"][i]):
            for f in rr.INT_FIELDS + ("peak", "cx", "cy"):
                assert got[f] == c[f], (i, f)
            assert abs(got["score_sum"] - c["score_sum"]) <= c["area"] * 2.0 ** -53 * math.fsum(np.abs(c["values"]).tolist())
            assert got["mean"] == got["score_sum"] / got["area"]
    assert {k: first["regions"][k] for k in tally} == tally and sum(tally.values()) == 4
    assert first["regions"]["pixel_threshold"] == cal.pixel_threshold
    # the same fit without regions_dir: the four metrics are untouched by the feature
    plain = ev.run_class(ev.mtfi_args(load_fit_dir=fits, **common), data(), weights=weights, extractor=extractor)
    assert "regions" not in plain and plain["phases"] == ["load_fit", "predict", "metrics"]
    for k in ev.METRICS:
        assert plain[k] == first[k], k
    # a second run reads the .cmdcal beside the stored fit and writes the same JSON
    again = ev.run_class(ev.mtfi_args(load_fit_dir=fits, regions_dir=out2, **common), data(), weights=weights, extractor=extractor)
    assert again["phases"] == ["load_fit", "predict", "metrics"]
    doc2 = json.load(open(os.path.join(out2, "rope.regions.json")))
    assert doc2 == doc and {k: again["regions"][k] for k in tally} == tally
    with pytest.raises(ValueError, match="calibration_holdout"):
        ev.ClassRun(ev.mtfi_args(calibration_holdout=5, **common), data(), weights=weights, extractor=extractor).fit_device()
    # a stored fit without its calibration: regions are refused, not silently left out
    os.remove(os.path.join(fits, "rope.cmdcal"))
    with pytest.raises(ValueError, match="rope.cmdcal is missing"):
        ev.ClassRun(ev.mtfi_args(load_fit_dir=fits, regions_dir=out2, **common), data(), weights=weights, extractor=extractor).fit_device()
    with pytest.raises(ValueError, match="needs a calibration"):
        ev.ClassRun(ev.mtfi_args(regions_dir=out2, **common), data(), weights=weights, extractor=extractor)
