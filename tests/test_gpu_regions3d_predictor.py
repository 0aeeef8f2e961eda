"""GPU: BatchPredictor(regions=, measure=True) and evaluate.ClassRun(measure_regions) -- the regions of every step measured on
THAT step's organised cloud, against regions.find_regions run on the maps the step returned and the cloud that was submitted.
The fit is the small synthetic one of tests/test_gpu_regions_predictor.py (batch 2)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_regions_predictor import extractor, fit  # noqa: E402,F401  (module-scoped fixtures: the backbone, the fitted class)

from cmdiad_amd import evaluate as ev  # noqa: E402
from cmdiad_amd import regions  # noqa: E402
from cmdiad_amd.synth import SyntheticClass  # noqa: E402
from oracle import nets  # noqa: E402

TABLES = ("n_comp", "count", "ints", "vals", "truncated")
FIELDS_3D = ("n_pts", "n_tri", "peak_valid", "lo", "hi", "peak_xyz", "area_3d", "extent", "centroid_3d", "covariance", "principal_sigma")


def step_cloud(fit, k):  # noqa: F811
    """Step k's cloud: the fit's test clouds with their two images swapped on odd steps and every coordinate scaled by a factor
    of its own (1 + k / 64; a zero stays a zero), so no two steps share a cloud or a measurement."""
    pcs = fit.pcs.flip(0) if k & 1 else fit.pcs
    return (pcs * (1.0 + k / 64.0)).contiguous()


def assert_same_tables(a, b):
    for f in TABLES:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def assert_measured(ticket, cloud, spec):
    """The ticket's tables and measures are, bit for bit, what find_regions gives on the ticket's own maps and that cloud."""
    _, maps = ticket.wait()
    got = ticket.regions()
    want = regions.find_regions(maps, spec, clouds=cloud)
    assert_same_tables(got, want)
    assert got.measures is not None and got.measures.m_ints.shape == want.measures.m_ints.shape
    assert got.measures.m_ints.tobytes() == want.measures.m_ints.tobytes()
    assert got.measures.m_vals.tobytes() == want.measures.m_vals.tobytes()
    assert want.measures.m_ints[:, :, 0].sum() > 0                              # never an empty comparison
    return got


def test_pipelined_steps_measure_their_own_clouds(fit):  # noqa: F811
    """Six pipelined steps over both buffer sets, every one with another cloud.  The measurement runs at tail time, on the tail's
    stream, after the step's input buffer has been released to the load of the step after the next: a predictor that read the
    input buffer then would measure a later step's cloud."""
    spec = fit.cal.spec(min_area=2, max_regions=8)
    p = fit.make(use_graph=True, regions=spec, measure=True)
    assert all(len(r) == 8 for r in p.region_ring) and all(inp["cloud"] is not None for inp in p.inputs)
    steps = 6
    clouds = [step_cloud(fit, k) for k in range(steps)]
    rgbs = [fit.rgb.flip(0) if k & 1 else fit.rgb for k in range(steps)]
    torch.cuda.synchronize()        # submit() takes finished batches: its copy stream does not wait for the stream that made them
    tickets, seen = [], []
    for k in range(steps):
        tickets.append(p.submit(rgbs[k], clouds[k]))
        if k >= 2:
            seen.append(assert_measured(tickets[k - 2], clouds[k - 2], spec))
    seen += [assert_measured(tickets[k], clouds[k], spec) for k in (steps - 2, steps - 1)]
    assert p.use_graph and p.sets is not None and p.step_no == steps            # stages 1 and 2 captured; both buffer sets used
    lows = {s.measures.m_vals[:, 0, 0:3].tobytes() for s in seen}
    assert len(lows) == steps                                                   # every step's measurement is its own


def test_eager_steps_and_the_default(fit):  # noqa: F811
    spec = fit.cal.spec(min_area=2, max_regions=8)
    p = fit.make(use_graph=False, regions=spec, measure=True)
    c0, c1, r1 = step_cloud(fit, 0), step_cloud(fit, 1), fit.rgb.flip(0)
    torch.cuda.synchronize()        # submit() takes finished batches: its copy stream does not wait for the stream that made them
    t0 = p.submit(fit.rgb, c0)
    t1 = p.submit(r1, c1)
    first = assert_measured(t0, c0, spec)
    assert_measured(t1, c1, spec)
    assert t0.wait()[0].tobytes() == fit.scores.tobytes() and t0.wait()[1].tobytes() == fit.maps.tobytes()     # scoring is untouched
    d = first.to_list()
    assert sum(len(r) for r in d) >= 1 and all(f in r for regs in d for r in regs for f in FIELDS_3D)
    # measure=False, the default: no buffer, no measures, the same tables
    q = fit.make(use_graph=False, regions=spec)
    assert all(len(r) == 5 for r in q.region_ring) and all(inp["cloud"] is None for inp in q.inputs)
    plain = q.submit(fit.rgb, fit.pcs).regions()
    assert plain.measures is None and all(not set(FIELDS_3D) & set(r) for regs in plain.to_list() for r in regs)
    assert_same_tables(plain, first)
    with pytest.raises(ValueError, match="measure=True"):
        fit.make(use_graph=False, measure=True)
    with pytest.raises(ValueError, match="gt_size"):
        fit.make(use_graph=False, regions=spec, measure=True, gt_size=112)


def test_class_loop_writes_the_3d_fields(extractor, tmp_path):  # noqa: F811
    weights = (None, None, nets.synth_state_dict("halluc", 51))
    fits, out1, out2 = str(tmp_path / "fits"), str(tmp_path / "r1"), str(tmp_path / "r2")
    data = lambda: SyntheticClass("rope", 5, 4, index=8)  # noqa: E731
    common = dict(f_coreset=0.1, random_state=3, min_area=2, max_regions=8)
    run = ev.ClassRun(ev.mtfi_args(save_fit_dir=fits, calibration_holdout=2, regions_dir=out1, measure_regions=True, **common), data(),
                      weights=weights, extractor=extractor).fit_device().fit_host().predict()
    assert run.test_items is None
    doc = json.load(open(os.path.join(out1, "rope.regions.json")))
    cal = regions.Calibration.load(os.path.join(fits, "rope.cmdcal"))
    clouds = torch.cat([it[0][1].reshape(1, 3, 224, 224) for it in data().test()])
    want = regions.find_regions(np.stack(run.method.predictions), cal.spec(2, 8), clouds=clouds).to_list()
    assert sum(len(r) for r in want) >= 1
    for img, regs in zip(doc["images"], want):
        assert img["regions"] == json.loads(json.dumps(regs))
        assert all(f in r for r in img["regions"] for f in FIELDS_3D)
    # without measure_regions the file is what it was: the same regions, none of the 3-D fields
    ev.run_class(ev.mtfi_args(load_fit_dir=fits, regions_dir=out2, **common), data(), weights=weights, extractor=extractor)
    doc2 = json.load(open(os.path.join(out2, "rope.regions.json")))
    for img in doc["images"]:
        img["regions"] = [{k: v for k, v in r.items() if k not in FIELDS_3D} for r in img["regions"]]
    assert doc2 == doc
