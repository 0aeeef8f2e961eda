"""GPU: scan preprocessing on the device (cmdiad_amd/utils/preprocessing.py, csrc/preprocess.hip) against independent CPU references:
scikit-learn's DBSCAN, the numpy restatement of the plane contract (tests/preprocess_ref.py), the reference's own glue recorded in
tests/golden/gpp_preprocess.npz.  Contract: docs/preprocessing.md."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(0.006, 30), (0.004, 12), (0.009, 60)]


def _labels(points, eps=0.006, min_points=30):
    from cmdiad_amd import ops
    lab, ncl = ops.dbscan(torch.from_numpy(np.ascontiguousarray(points)).to(DEV), eps, min_points)
    return lab.cpu().numpy(), int(ncl.item())


@pytest.mark.parametrize("eps,min_points", PAIRS)
def test_dbscan_labels_equal_sklearn(eps, min_points):
    """ops.dbscan == sklearn.cluster.DBSCAN(eps, min_samples).fit(points.astype(float64)).labels_ on every generator scene, for the
    reference's (eps, min_points) and two more.  Precondition, asserted on the input: no pair within 1e-12 eps^2 of the boundary."""
    from sklearn.cluster import DBSCAN
    seen_two = 0
    for name, pts in pr.dbscan_scenes().items():
        assert pr.boundary_pairs(pts, eps) == 0, name
        got, ncl = _labels(pts, eps, min_points)
        if len(pts) == 0:
            assert got.shape == (0,) and ncl == 0
            continue
        want = DBSCAN(eps=eps, min_samples=min_points).fit(pts.astype(np.float64)).labels_
        print(name, len(pts), "clusters", want.max() + 1, "noise", int((want < 0).sum()), "mismatches", int((got != want).sum()))
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert ncl == want.max() + 1
        if (eps, min_points) == PAIRS[0]:
            seen_two += pr.dbscan(pts, eps, min_points, details=True)[1]["two_cluster_border"]
    if (eps, min_points) == PAIRS[0]:
        assert seen_two > 0          # the scenes do contain border points adjacent to two clusters


def test_dbscan_full_size_planted_partition():
    """One 800 x 800 scene (about 300 k points at 0.2 mm pitch) whose components are planted more than eps apart: the labels are the
    planted partition under the numbering rule; on 2 000 sampled points, label >= 0 exactly where cKDTree counts >= min_points
    neighbours (the scene has no border points: every disc point is core, every lone point is noise)."""
    from scipy.spatial import cKDTree
    pts, want = pr.full_size_scene()
    assert len(pts) > 280000
    got, ncl = _labels(pts)
    assert ncl == want.max() + 1 == 5
    assert np.array_equal(got, want), int((got != want).sum())
    rng = np.random.default_rng(5)
    pick = np.concatenate([rng.integers(0, len(pts), 1900), np.nonzero(want < 0)[0][:100]])
    P = pts.astype(np.float64)
    counts = cKDTree(P).query_ball_point(P[pick], 0.006, return_length=True)
    assert np.array_equal(counts >= 30, got[pick] >= 0)
    again, _ = _labels(pts)
    assert np.array_equal(again, got)


def test_dbscan_repeats_and_degenerate_inputs():
    """The labels do not depend on scheduling: five runs of a scene with border points give identical labels.  Degenerate clouds give
    results: one point, identical points, a non-finite coordinate (noise, never a neighbour)."""
    pts = pr.dbscan_scenes()["scan_a"]
    first, _ = _labels(pts)
    for _ in range(4):
        assert np.array_equal(_labels(pts)[0], first)
    assert _labels(np.array([[1.0, 2.0, 3.0]], np.float32))[0].tolist() == [-1]
    assert _labels(np.ones((64, 3), np.float32))[0].tolist() == [0] * 64
    bad = pts[:5000].copy()
    ref = _labels(np.delete(bad, 17, axis=0))[0]
    bad[17, 1] = np.nan
    got = _labels(bad)[0]
    assert got[17] == -1 and np.array_equal(np.delete(got, 17), ref)
    from cmdiad_amd import ops
    hist = ops.label_histogram(torch.from_numpy(first).to(DEV), int(first.max()) + 2).cpu().numpy()
    assert np.array_equal(hist, np.bincount(first + 1, minlength=first.max() + 2))


def _edge_scenes():
    return [(s, pr.get_edges(pr.make_scan(s)["pc"])) for s in (11, 13, 14)]


def test_plane_against_the_restatement():
    """get_plane_eq / ops.plane_ransac against the float64 restatement on three scans x two seeds: the winning hypothesis and its
    inlier count are EQUAL; the coefficients agree to 10 x what reordering float64 costs on the CPU, measured here as the largest
    difference between the restatement with eigh and the restatement with svd on the same samples (on the CPU of the development
    machine: 1.3e-16 over these scenes, so the bound was 1.3e-15; docs/preprocessing.md).  Precondition asserted on the input:
    the restatement's winner leads the runner-up by at least 3 inliers, so a last-bit difference in a distance cannot change it."""
    from cmdiad_amd import ops
    from cmdiad_amd.utils import preprocessing as mod
    reorder = 0.0
    results = []
    for scan_seed, edges in _edge_scenes():
        for seed in (0, 7):
            plane, inl, h, counts = pr.plane_ransac(edges, seed=seed)
            plane_svd, inl_s, h_s, _ = pr.plane_ransac(edges, seed=seed, fit=pr.fit_plane_svd)
            assert (inl_s, h_s) == (inl, h)
            reorder = max(reorder, float(np.abs(plane - plane_svd).max()))
            runner = np.sort(counts)[-2]
            assert inl - runner >= 3, (scan_seed, seed, inl, runner)
            got, info = ops.plane_ransac(torch.from_numpy(edges).to(DEV), seed=seed)
            results.append((scan_seed, seed, plane, inl, h, got.cpu().numpy(), info.cpu().numpy()))
    tol = 10 * reorder
    print("eigh vs svd", reorder, "tolerance", tol)
    for scan_seed, seed, plane, inl, h, got, info in results:
        print(scan_seed, seed, "winner", h, info[1], "inliers", inl, info[0], "max coefficient difference", np.abs(got - plane).max())
        assert (int(info[0]), int(info[1])) == (inl, h), (scan_seed, seed)
        assert abs(np.linalg.norm(got[:3]) - 1) < 1e-14 and got[2] >= 0
        assert np.abs(got - plane).max() <= tol, (scan_seed, seed, np.abs(got - plane).max(), tol)
    edges = _edge_scenes()[0][1]
    assert np.array_equal(mod.get_plane_eq(edges), results[0][5])
    with pytest.raises(ValueError):
        mod.get_plane_eq(edges[:49])
    with pytest.raises(ValueError):
        mod.remove_plane(np.zeros((40, 40, 3), np.float32), np.zeros((40, 40, 3), np.uint8))


def test_remove_plane_planted_conditions():
    """Planted plane: every background point whose planted offset is below 0.005 - 1e-4 is removed, no object point higher than
    0.005 + 1e-4 above the plane is removed (conditions, not tolerances); the output equals the restatement's where no point lies
    within 1e-9 of the threshold (the committed scenes have none: tests/test_preprocess_cpu.py)."""
    from cmdiad_amd.utils import preprocessing as mod
    for seed in (11, 13, 14):
        scan = pr.make_scan(seed)
        pc, rgb = mod.remove_plane(scan["pc"], scan["rgb"])
        gone = np.all(pc == 0, axis=2)
        assert gone[scan["background"] & (scan["offset"] < 0.005 - 1e-4)].all()
        assert not gone[scan["raised"] & (scan["offset"] > 0.005 + 1e-4)].any()
        assert scan["pc"] is not pc and np.all(scan["pc"][scan["valid"]] != 0)          # inputs untouched
        plane = pr.plane_ransac(pr.get_edges(scan["pc"]))[0]
        want_pc, want_rgb = pr.remove_plane(scan["pc"], scan["rgb"], plane)
        assert np.array_equal(pc, want_pc) and np.array_equal(rgb, want_rgb)


def test_stages_against_the_golden(golden):
    """remove_plane / pad / connected_components_cleaning / preprocess_arrays against the outputs of the REFERENCE's own glue
    (tests/golden/make_golden_preprocess.py: open3d stubbed by the restatement's plane and labels): equal arrays, the
    noise-majority case included."""
    import importlib.util
    from cmdiad_amd.utils import preprocessing as mod
    spec = importlib.util.spec_from_file_location("make_golden_preprocess", os.path.join(os.path.dirname(__file__), "golden", "make_golden_preprocess.py"))
    mgp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mgp)
    g = golden("gpp_preprocess.npz")
    for tag, kw in mgp.SCANS.items():
        scan = pr.make_scan(**kw)
        p1, r1 = mod.remove_plane(scan["pc"], scan["rgb"])
        assert np.array_equal(np.packbits(np.all(p1 == 0, axis=2)), g[f"{tag}/planeless_zero"])
        assert np.array_equal(p1[~np.all(p1 == 0, axis=2)], scan["pc"][~np.all(p1 == 0, axis=2)])
        p2, r2 = mod.pad_cropped_pc(p1), mod.pad_cropped_pc(r1)
        p3, r3 = mod.connected_components_cleaning(p2, r2, "golden")
        assert np.array_equal(np.packbits(np.all(p3 == 0, axis=2)), g[f"{tag}/clean_zero"])
        assert np.array_equal(p3.astype(np.float64).sum((0, 1)), g[f"{tag}/clean_pc_sum"]) and int(r3.astype(np.int64).sum()) == int(g[f"{tag}/clean_rgb_sum"])
        a, b, c = mod.preprocess_arrays(scan["pc"], scan["rgb"], scan["gt"])
        assert np.array_equal(a, p3) and np.array_equal(b, r3) and np.array_equal(np.packbits(c != 0), g[f"{tag}/padded_gt"])
        w = pr.preprocess(scan["pc"], scan["rgb"], scan["gt"])
        assert np.array_equal(a, w[0]) and np.array_equal(b, w[1]) and np.array_equal(c, w[2])
    pc, rgb = mgp.noise_majority_scan()
    p3, r3 = mod.connected_components_cleaning(pc, rgb, "golden-noise")
    assert np.array_equal(np.packbits(np.all(p3 == 0, axis=2)), g["noise/clean_zero"]) and int(r3.astype(np.int64).sum()) == int(g["noise/clean_rgb_sum"])
    # degenerate: a scan without a valid point comes back unchanged
    z, zr = np.zeros((30, 30, 3), np.float32), np.full((30, 30, 3), 9, np.uint8)
    e, er = mod.connected_components_cleaning(z, zr, "empty")
    assert np.array_equal(e, z) and np.array_equal(er, zr)


def test_batch_equals_single_calls():
    """A list of 8 scans of different sizes == 8 single calls, bit for bit; a second batch call gives the same again."""
    from cmdiad_amd.utils import preprocessing as mod
    scans = [pr.make_scan(50 + i, H=150 + 17 * i, W=260 - 13 * i) for i in range(8)]
    pcs, rgbs, gts = [s["pc"] for s in scans], [s["rgb"] for s in scans], [s["gt"] if i % 2 else None for i, s in enumerate(scans)]
    bp, br, bg = mod.preprocess_arrays(pcs, rgbs, gts, seed=3)
    bp2, br2, _ = mod.preprocess_arrays(pcs, rgbs, gts, seed=3)
    for i in range(8):
        p, r, g = mod.preprocess_arrays(pcs[i], rgbs[i], gts[i], seed=3)
        assert np.array_equal(p, bp[i]) and np.array_equal(r, br[i]) and np.array_equal(p, bp2[i]) and np.array_equal(r, br2[i])
        assert (g is None and bg[i] is None) or np.array_equal(g, bg[i])
        assert p.shape[0] == p.shape[1] and p.shape[0] % 100 == 0 and np.any(p != 0)


def test_preprocess_pc_end_to_end(tmp_path, monkeypatch):
    """preprocess_pc on files, with a stand-in tifffile module that reads and writes .npy content under the .tiff name."""
    from PIL import Image
    from cmdiad_amd.utils import preprocessing as mod
    fake = types.ModuleType("tifffile")
    fake.imread = lambda p: np.load(open(p, "rb"))
    fake.imwrite = lambda p, a: np.save(open(p, "wb"), a)
    monkeypatch.setitem(sys.modules, "tifffile", fake)
    scan = pr.make_scan(11)
    dirs = {"000": tmp_path / "one" / "bagel" / "test" / "hole", "001": tmp_path / "two" / "bagel" / "test" / "good"}
    for name, base in dirs.items():
        for sub in ("xyz", "rgb", "gt"):
            (base / sub).mkdir(parents=True)
        fake.imwrite(str(base / "xyz" / f"{name}.tiff"), scan["pc"])
        Image.fromarray(scan["rgb"]).save(base / "rgb" / f"{name}.png")
    Image.fromarray(scan["gt"]).save(dirs["000"] / "gt" / "000.png")
    want = mod.preprocess_arrays(scan["pc"], scan["rgb"], scan["gt"])
    mod.preprocess_pc(str(dirs["000"] / "xyz" / "000.tiff"))
    assert np.array_equal(fake.imread(str(dirs["000"] / "xyz" / "000.tiff")), want[0])
    assert np.array_equal(np.array(Image.open(dirs["000"] / "rgb" / "000.png")), want[1])
    assert np.array_equal(np.array(Image.open(dirs["000"] / "gt" / "000.png")), want[2])
    assert mod.preprocess_dataset(str(tmp_path / "two")) == 1          # the __main__ loop, a scan without ground truth
    assert np.array_equal(fake.imread(str(dirs["001"] / "xyz" / "001.tiff")), want[0]) and not (dirs["001"] / "gt" / "001.png").exists()
    assert np.array_equal(np.array(Image.open(dirs["001"] / "rgb" / "001.png")), want[1])
