"""CPU (no GPU): the host side of cmdiad_amd/utils/preprocessing.py against the reference's own outputs
(tests/golden/gpp_preprocess.npz), the hash sampler against recorded draws, the C ABI of the new entry points, and the contract of
the DBSCAN stage pinned against scikit-learn (the restatement of tests/preprocess_ref.py == sklearn.cluster.DBSCAN on every scene)."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as pr  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmdiad_plane_ransac", "cmdiad_plane_mask", "cmdiad_dbscan", "cmdiad_label_histogram")
NEW_SIZES = ("cmdiad_plane_ransac_workspace_bytes", "cmdiad_dbscan_workspace_bytes")


def _mgp():
    spec = importlib.util.spec_from_file_location("make_golden_preprocess", os.path.join(REPO, "tests", "golden", "make_golden_preprocess.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_host_functions_match_the_reference(golden):
    from cmdiad_amd.utils import preprocessing as mod
    g = golden("gpp_preprocess.npz")
    for tag, kw in _mgp().SCANS.items():
        scan = pr.make_scan(**kw)
        edges = mod.get_edges_of_pc(scan["pc"])
        assert np.array_equal(np.array(edges.shape), g[f"{tag}/edges_shape"])
        assert np.array_equal(edges[:64], g[f"{tag}/edges_head"]) and np.array_equal(edges.astype(np.float64).sum(0), g[f"{tag}/edges_sum"])
        assert np.array_equal(edges, pr.get_edges(scan["pc"]))
        assert np.array_equal(np.packbits(mod.pad_cropped_pc(scan["gt"], single_channel=True) != 0), g[f"{tag}/padded_gt"])
        assert np.array_equal(np.array(mod.pad_cropped_pc(scan["pc"]).shape), g[f"{tag}/padded_shape"])
        # the restatement pipeline on the recorded plane reproduces the reference's outputs (so the GPU test may compare with it)
        p1, r1 = pr.remove_plane(scan["pc"], scan["rgb"], g[f"{tag}/plane"])
        assert np.array_equal(np.packbits(np.all(p1 == 0, axis=2)), g[f"{tag}/planeless_zero"])
        p3, r3 = pr.keep_largest(pr.pad_square(p1), pr.pad_square(r1))
        assert np.array_equal(np.packbits(np.all(p3 == 0, axis=2)), g[f"{tag}/clean_zero"]) and int(r3.astype(np.int64).sum()) == int(g[f"{tag}/clean_rgb_sum"])
        assert np.array_equal(g[f"{tag}/plane"], pr.plane_ransac(edges)[0])
    for x, want in g["roundup"]:
        assert mod.roundup_next_100(int(x)) == want
    for key in (k for k in g.files if k.startswith("pad/")):
        h, w = (int(v) for v in key[4:].split("x"))
        p = mod.pad_cropped_pc(np.arange(h * w * 3, dtype=np.float32).reshape(h, w, 3) + 1)
        assert [p.shape[0], p.shape[1], *np.argwhere(p[:, :, 0] != 0)[0]] == g[key].tolist()
    # corner blocks appear twice; rows with any zero coordinate are dropped
    pc = np.arange(1, 40 * 50 * 3 + 1, dtype=np.float32).reshape(40, 50, 3)
    pc[3, 20, 1] = 0
    e = mod.get_edges_of_pc(pc)
    assert len(e) == 2 * 10 * 50 + 2 * 10 * 40 - 1 and (e == pc[0, 0]).all(1).sum() == 2 and not (e == 0).any()


def test_hash_sampler_recorded_draws():
    assert pr.mix32(1) == 1753845952 and pr.mix32(0xDEADBEEF) == 3861431939
    assert pr.sample_indices(0, 0, 1000, 8).tolist() == [89, 407, 284, 953, 872, 684, 904, 651]
    assert pr.sample_indices(7, 999, 32000, 6).tolist() == [1781, 20269, 1458, 27685, 5272, 20841]
    full = pr.sample_indices(0, 3, 50, 50)            # as many points as draws: a permutation, duplicates skipped in draw order
    assert full.tolist()[:10] == [49, 43, 24, 0, 18, 12, 16, 17, 7, 46] and sorted(full.tolist()) == list(range(50))
    for h in (0, 1, 500):
        s = pr.sample_indices(3, h, 8700)
        assert len(s) == len(set(s.tolist())) == 50 and s.min() >= 0 and s.max() < 8700


def test_new_entry_points_are_declared_bound_and_reject_null():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    hdr = open(os.path.join(REPO, "include", "cmdiad_hip.h")).read()
    declared = set(re.findall(r"\b(cmdiad_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(L, name)
        args = [None if a is ctypes.c_void_p else 1 for a in nat.SIGNATURES[name]]
        assert getattr(L, name)(*args) == -1 and b"null pointer" in L.cmdiad_last_error(), name
    for name in NEW_SIZES:
        assert name in declared and name in nat.SIZE_QUERIES
    assert L.cmdiad_abi_version() == 6
    sizes = [L.cmdiad_dbscan_workspace_bytes(n) for n in (0, 1, 29, 30, 1000, 2048, 2049, 65536, 300000, 640000, 1 << 24)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[-2] > 640000 * 40
    assert L.cmdiad_plane_ransac_workspace_bytes(1000) >= 1000 * 32 > L.cmdiad_plane_ransac_workspace_bytes(0) == 0
    # bad sizes with valid-looking pointers: rejected before anything is launched
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cmdiad_plane_ransac(p, 49, 50, 1000, 0.004, 0, p, p, p, 1 << 20, None) == -1 and b"bad sizes" in L.cmdiad_last_error()
    assert L.cmdiad_plane_ransac(p, 100, 50, 1000, 0.004, 0, p, p, p, 16, None) == -2
    assert L.cmdiad_dbscan(p, -1, 0.006, 30, p, p, p, 1 << 20, None) == -1
    assert L.cmdiad_dbscan(p, 100, 0.006, 30, p, p, p, 64, None) == -2 and b"workspace" in L.cmdiad_last_error()
    assert L.cmdiad_dbscan(p, 100, 0.0, 30, p, p, p, 1 << 20, None) == -1
    assert L.cmdiad_label_histogram(p, 10, p, 0, None) == -1


def test_module_imports_without_a_gpu_and_has_no_cpu_path():
    import torch
    import cmdiad_amd
    from cmdiad_amd import ops
    from cmdiad_amd.utils import preprocessing as mod
    for name in ("get_edges_of_pc", "get_plane_eq", "remove_plane", "connected_components_cleaning", "roundup_next_100", "pad_cropped_pc",
                 "preprocess_pc", "preprocess_arrays"):
        assert callable(getattr(mod, name))
    assert not any("preprocessing" in str(v) for v in getattr(cmdiad_amd, "_DROPIN", ()))       # not part of the drop-in table
    with pytest.raises(Exception, match="GPU"):
        ops.dbscan(torch.zeros(100, 3))
    with pytest.raises(Exception, match="GPU"):
        ops.plane_ransac(torch.zeros(100, 3))
    if not torch.cuda.is_available():
        scan = pr.make_scan(11, H=60, W=60)
        for call in (lambda: mod.get_plane_eq(pr.get_edges(scan["pc"])), lambda: mod.remove_plane(scan["pc"], scan["rgb"]),
                     lambda: mod.connected_components_cleaning(scan["pc"], scan["rgb"], "x"), lambda: mod.preprocess_arrays(scan["pc"], scan["rgb"])):
            with pytest.raises(RuntimeError, match="needs a GPU"):
                call()


def test_dbscan_rule_is_sklearns_on_every_scene():
    """The contract of cmdiad_dbscan (docs/preprocessing.md), restated with cKDTree + connected_components, gives
    sklearn.cluster.DBSCAN's labels on every generator scene -- including border points adjacent to two clusters -- and no scene
    has a pair of points at the boundary distance (the precondition of the GPU comparison) for any tested eps."""
    from sklearn.cluster import DBSCAN
    two = 0
    for name, pts in pr.dbscan_scenes().items():
        for eps in (0.006, 0.004, 0.009):
            assert pr.boundary_pairs(pts, eps) == 0, (name, eps)
        if len(pts) == 0:
            assert len(pr.dbscan(pts)) == 0
            continue
        lab, d = pr.dbscan(pts, details=True)
        assert np.array_equal(lab, DBSCAN(eps=0.006, min_samples=30).fit(pts.astype(np.float64)).labels_), name
        two += d["two_cluster_border"]
    assert two > 0
    lab = pr.dbscan(pr.dbscan_scenes()["noise_majority"])
    assert (lab == -1).sum() > (lab >= 0).sum() > 0
    lab = pr.dbscan(pr.dbscan_scenes()["duplicates"])
    assert lab.max() == 1 and lab[0] == 0 and (lab == 0).sum() == 40            # the pile of identical points is cluster 0


def test_committed_plane_scenes_meet_the_preconditions():
    """What the GPU tests assume about the committed scenes, proved on the CPU restatement: no point within 1e-9 of the removal
    threshold; every background point with planted offset < 0.005 - 1e-4 is removed and no raised point above 0.005 + 1e-4 is."""
    for seed in (11, 13, 14):
        scan = pr.make_scan(seed)
        plane = pr.plane_ransac(pr.get_edges(scan["pc"]))[0]
        dist = pr.plane_distance(plane, scan["pc"])
        assert (np.abs(dist - 0.005) < 1e-9).sum() == 0
        assert (dist[scan["background"] & (scan["offset"] < 0.005 - 1e-4)] < 0.005).all()
        assert (dist[scan["raised"] & (scan["offset"] > 0.005 + 1e-4)] >= 0.005).all()
        assert scan["raised"][10:-10, 10:-10].sum() == scan["raised"].sum()              # the edge band is background
