"""GPU: csrc/mesh.hip (cmdiad_mesh_count, cmdiad_mesh_write) byte for byte against the yardstick tests/mesh_ref.py -- the used prefixes
of both record buffers, counts and vidx --, cmdiad_amd.mesh's save through utils.ply, and meshes from the class loop.  The shapes are
the smallest at which the kernels can go wrong: a chunk is 1024 pixels, a lane takes four."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402
from test_gpu_fitted import extractor  # noqa: E402,F401  (the module-scoped backbone fixture)

from cmdiad_amd import evaluate as ev  # noqa: E402
from cmdiad_amd import mesh, ops  # noqa: E402
from cmdiad_amd.synth import SyntheticClass  # noqa: E402
from cmdiad_amd.utils import ply  # noqa: E402
from oracle import nets  # noqa: E402

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RS = np.random.RandomState(5)
LUT, ALPHA = RS.randint(0, 256, (256, 3)).astype(np.uint8), RS.randint(0, 256, 256).astype(np.uint8)
LO, HI = 0.2, 1.1


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def surface(n, H, W, seed, invalid=0.0):
    """clouds [n,H,W,3] f32 of a bumpy surface over a jittered grid (no coordinate near zero) and maps [n,H,W] f64; `invalid`: the
    share of points zeroed -- most as the scanner does (all three), some in one coordinate only, some with -0.0"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    x = 3.0 + 0.5 * xx[None] + 0.1 * rs.rand(n, H, W)
    y = -40.0 + 0.5 * yy[None] + 0.1 * rs.rand(n, H, W)
    z = 7.0 + np.sin(x) * np.cos(0.7 * y) + 0.05 * rs.rand(n, H, W)
    cloud = np.stack([x, y, z], axis=3).astype(np.float32)
    how = rs.rand(n, H, W)
    pick = rs.rand(n, H, W) < invalid
    cloud[pick & (how < 0.6)] = 0.0
    for c in range(3):
        cloud[..., c][pick & (how >= 0.6 + 0.1 * c) & (how < 0.7 + 0.1 * c)] = 0.0
    cloud[..., 2][pick & (how >= 0.9)] = -0.0
    maps = rs.rand(n, H, W) * 1.4
    return cloud, maps


def device_mesh(cloud, maps, lo=LO, hi=HI, bg=None, labels=None, max_edge2=math.inf, flip=False, layout="interleaved"):
    """(vertex prefixes, face prefixes, counts, vidx) as the yardstick returns them, from the two entry points"""
    c = cloud if layout == "interleaved" else cloud.transpose(0, 3, 1, 2)
    n = len(maps)
    per = np.size(lo) > 1 or np.size(hi) > 1
    lohi = np.stack([np.broadcast_to(np.asarray(lo, np.float64).reshape(-1), (n if per else 1,)),
                     np.broadcast_to(np.asarray(hi, np.float64).reshape(-1), (n if per else 1,))], axis=1)
    dc, dm = dev(c), dev(np.asarray(maps, np.float64))
    chunks, counts = ops.mesh_count(dc, dm, max_edge2, layout=layout)
    vidx, vb, fb = ops.mesh_write(dc, dm, chunks, dev(lohi), dev(LUT), dev(ALPHA), background=dev(bg), mean=MEAN, std=STD, labels=dev(labels),
                                  max_edge2=max_edge2, flip=flip, layout=layout)
    counts, vb, fb = counts.cpu().numpy(), vb.cpu().numpy(), fb.cpu().numpy()
    assert np.array_equal(chunks.cpu().numpy().sum(axis=1), counts[:, :2])
    return ([vb[i, :counts[i, 0] * 35].tobytes() for i in range(n)], [fb[i, :counts[i, 1] * 13].tobytes() for i in range(n)], counts,
            vidx.cpu().numpy())


def same(got, want):
    gv, gf, gc, gi = got
    wv, wf, wc, wi = want
    assert np.array_equal(gc, wc), (gc, wc)
    assert np.array_equal(gi, wi)
    for i in range(len(wv)):
        if gv[i] != wv[i]:
            a, b = np.frombuffer(gv[i], ply.VERTEX), np.frombuffer(wv[i], ply.VERTEX)
            at = [k for k in range(len(b)) if a[k].tobytes() != b[k].tobytes()][:4]
            raise AssertionError(f"image {i}: vertex records {at} differ: {a[at]} != {b[at]}")
        assert gf[i] == wf[i], f"image {i}: face records differ"


def check(cloud, maps, **kw):
    kind = 0 if kw.get("bg") is None else 1 if kw["bg"].dtype == np.uint8 else 2
    ref = {k: v for k, v in kw.items() if k != "layout"}
    want = R.batch(cloud, maps, ref.pop("lo", LO), ref.pop("hi", HI), LUT, ALPHA, bg_kind=kind, mean=MEAN, std=STD, **ref)
    got = device_mesh(cloud, maps, **kw)
    same(got, want)
    return got


# ------------------------------------------------------------------------------------------------ the batch of three
@functools.lru_cache(maxsize=None)
def three():
    """n = 3 at 9 x 11, about a quarter of the points invalid; image 1 fully invalid, image 2 fully valid; its yardstick, once"""
    cloud, maps = surface(3, 9, 11, 1, invalid=0.25)
    cloud[1] = 0.0
    cloud[2] = surface(1, 9, 11, 2)[0][0]
    bad = ~np.all((cloud[0] != 0) & np.isfinite(cloud[0]), axis=2)
    assert 0.1 < bad.mean() < 0.45 and np.any(np.signbit(cloud[0][..., 2]) & (cloud[0][..., 2] == 0))
    assert np.any((cloud[0] == 0).sum(axis=2) == 1)                                     # a point with a single zero coordinate
    return cloud, maps, R.batch(cloud, maps, LO, HI, LUT, ALPHA)


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_batch_of_three_in_both_layouts(layout):
    cloud, maps, want = three()
    assert want[2][:, 0].tolist()[1:] == [0, 99] and want[2][1].tolist() == [0, 0, 0, 0] and want[2][2, 1] == 2 * 8 * 10
    same(device_mesh(cloud, maps, layout=layout), want)


def test_an_image_of_the_batch_gives_the_bytes_it_gives_alone():
    cloud, maps, want = three()
    for i in range(3):
        gv, gf, gc, gi = device_mesh(cloud[i:i + 1], maps[i:i + 1])
        assert gv[0] == want[0][i] and gf[0] == want[1][i] and np.array_equal(gc[0], want[2][i]) and np.array_equal(gi[0], want[3][i])


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("with_labels", [False, True])
def test_backgrounds_labels_and_flip(kind, with_labels):
    cloud, maps, _ = three()
    rs = np.random.RandomState(20 + kind)
    bg = None if kind == 0 else rs.randint(0, 256, (3, 9, 11, 3)).astype(np.uint8) if kind == 1 else \
        ((rs.rand(3, 3, 9, 11) * 1.2 - 0.1 - np.array(MEAN)[None, :, None, None]) / np.array(STD)[None, :, None, None]).astype(np.float32)
    labels = rs.randint(-2, 9, (3, 9, 11)).astype(np.int32) if with_labels else None
    check(cloud, maps, bg=bg, labels=labels, flip=bool((kind + with_labels) % 2), lo=[0.1, 0.2, 0.3], hi=[1.0, 0.2, 0.9])
    check(cloud, maps, bg=bg, labels=labels, flip=not (kind + with_labels) % 2, layout="planar")


# ------------------------------------------------------------------------------------------------ edge shapes
@pytest.mark.parametrize("shape", [(1, 70), (70, 1), (1, 1)])
def test_single_rows_and_columns_have_vertices_and_no_faces(shape):
    cloud, maps = surface(2, *shape, seed=3, invalid=0.2)
    cloud[1, 0, 0] = (1.0, 2.0, 3.0)
    gv, gf, counts, _ = check(cloud, maps)
    assert np.all(counts[:, 1] == 0) and counts[1, 0] >= 1 and gf == [b"", b""]
    check(cloud, maps, layout="planar", flip=True)


@pytest.mark.parametrize("shape", [(33, 37), (40, 64)])
def test_more_than_one_chunk(shape):
    """33 x 37 = 1221 pixels: two chunks, the second starts inside row 27, the lower neighbours of rows 26 and 27 lie in it.
    40 x 64 = 2560: three chunks, a row is 16 lanes, so every wave and every chunk starts and ends on a row boundary."""
    H, W = shape
    cloud, maps = surface(2, H, W, seed=H, invalid=0.06)
    labels = np.random.RandomState(H).randint(0, 5, (2, H, W)).astype(np.int32)
    gv, gf, counts, _ = check(cloud, maps, labels=labels, max_edge2=0.75 ** 2)
    assert np.all(counts[:, 0] > 1024) and np.all(counts[:, 1] > 0)
    check(cloud, maps, layout="planar")


# ------------------------------------------------------------------------------------------------ the edge cut
def test_stepped_surface_keeps_and_drops_triangles():
    cloud, maps = surface(1, 10, 12, seed=8)
    cloud[0, :, 5:, 2] += 4.0                       # a cliff between columns 4 and 5
    cloud[0, 6:, :3, 2] -= 4.0                      # and a corner that ends inside the frame
    max2 = 1.5 ** 2
    kept = R.kept_triangles(cloud[0], max2)
    assert any(kept.values()) and not all(kept.values())
    incident = lambda y, x: [kept.get(k, False) for k in ((y - 1, x - 1, 0), (y - 1, x - 1, 1), (y - 1, x, 1), (y, x - 1, 0), (y, x, 0), (y, x, 1))]  # noqa: E731
    partial = [(y, x) for y in range(1, 9) for x in range(1, 11) if 0 < sum(incident(y, x)) < 6]
    assert partial, "no vertex loses some but not all of its incident triangles"
    gv, gf, counts, _ = check(cloud, maps, max_edge2=max2)
    assert counts[0, 0] == 120 and 0 < counts[0, 1] == sum(kept.values()) < 2 * 9 * 11
    assert check(cloud, maps)[2][0, 1] == 2 * 9 * 11                                 # without the cut every triangle is there


# ------------------------------------------------------------------------------------------------ bad points and NaN scores
def test_non_finite_points_and_nan_scores_are_counted(tmp_path):
    cloud, maps = surface(2, 6, 7, seed=9)
    cloud[0, 2, 3, 0], cloud[0, 4, 1, 2], cloud[1, 0, 0, 1] = np.nan, np.inf, -np.inf
    gv, gf, counts, vidx = check(cloud, maps)
    assert counts[:, 2].tolist() == [2, 1] and counts[:, 3].tolist() == [0, 0] and counts[:, 0].tolist() == [40, 41]
    assert vidx[0, 2, 3] == vidx[0, 4, 1] == vidx[1, 0, 0] == -1
    spec = mesh.MeshSpec(LO, HI)
    paths = [str(tmp_path / f"{i}.ply") for i in range(2)]
    with pytest.raises(ValueError, match="2 points|3 points"):
        mesh.save(paths, cloud, maps, spec)
    cloud, maps = surface(2, 6, 7, seed=9)
    maps[1, 3, 3] = np.nan
    cloud[1, 5, 5] = 0.0
    maps[1, 5, 5] = np.nan                          # on an invalid point: not a vertex, not counted
    gv, gf, counts, vidx = check(cloud, maps)
    assert counts[:, 3].tolist() == [0, 1] and counts[:, 2].tolist() == [0, 0]
    v = np.frombuffer(gv[1], ply.VERTEX)[vidx[1, 3, 3]]
    assert np.isnan(v["score"]) and (v["red"], v["green"], v["blue"]) == tuple(LUT[0])          # t = 0
    with pytest.raises(ValueError, match="1 vertices a NaN score"):
        mesh.save(paths, cloud, maps, spec)
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError, match="one xyz per map pixel"):
        mesh.save(paths, cloud[:, :5], maps, spec)


# ------------------------------------------------------------------------------------------------ save
def test_saved_files_read_back_as_the_yardsticks_arrays(tmp_path):
    cloud, maps, _ = three()
    labels = np.random.RandomState(4).randint(0, 4, (3, 9, 11)).astype(np.int32)
    spec = mesh.MeshSpec([0.1, 0.2, 0.3], 1.0, colormap="grey", alpha=255, max_edge=0.9, flip_normals=True)
    bg = np.random.RandomState(6).randint(0, 256, (3, 9, 11, 3)).astype(np.uint8)
    paths = [str(tmp_path / f"{i}.ply") for i in range(3)]
    sizes = mesh.save(paths, cloud, maps, spec, background=bg, labels=labels, comments=[[f"image {i}"] for i in range(3)], writers=2)
    wv, wf, wc, _ = R.batch(cloud, maps, [0.1, 0.2, 0.3], 1.0, spec.lut, spec.alpha, bg=bg, bg_kind=1, labels=labels, max_edge2=0.9 * 0.9,
                            flip=True)
    for i, p in enumerate(paths):
        assert sizes[i] == os.path.getsize(p)
        head = open(p, "rb").read().split(b"end_header\n")[0].decode()
        assert f"element vertex {wc[i, 0]}\n" in head and f"element face {wc[i, 1]}\n" in head
        verts, faces, comments = ply.read(p)
        assert comments == [f"image {i}"] and verts.tobytes() == wv[i] and faces.tobytes() == wf[i]
    built = mesh.build(torch.from_numpy(cloud.transpose(0, 3, 1, 2).copy()), maps, spec, layout="planar")      # planar, no background
    counts, hv, hf = built.to_host()
    assert np.array_equal(counts, wc) and [len(v) for v in hv] == (wc[:, 0] * 35).tolist() and [f.tobytes() for f in hf] == wf


# ------------------------------------------------------------------------------------------------ the class loop
def test_class_loop_writes_one_mesh_per_test_image(extractor, tmp_path):  # noqa: F811
    weights = (None, None, nets.synth_state_dict("halluc", 51))
    fits, out = str(tmp_path / "fits"), str(tmp_path / "meshes")
    data = lambda: SyntheticClass("rope", 5, 4, index=8)  # noqa: E731
    common = dict(f_coreset=0.1, random_state=3, min_area=2, max_regions=8)
    run = ev.ClassRun(ev.mtfi_args(save_fit_dir=fits, calibration_holdout=2, mesh_dir=out, **common), data(), weights=weights,
                      extractor=extractor).fit_device().fit_host().predict()
    res = run.result()
    folder = os.path.join(out, "rope")
    assert sorted(os.listdir(folder)) == [f"{i:04d}.ply" for i in range(4)]
    assert res["meshes"] == dict(directory=folder, files=4) and res["seconds"]["meshes"] > 0 and "overlays" not in res
    maps = np.stack([np.asarray(p, dtype=np.float64) for p in run.method.predictions])
    for i, item in enumerate(data().test()):
        cloud = item[0][1].reshape(3, *item[0][1].shape[-2:]).numpy()
        ok = np.all((cloud != 0) & np.isfinite(cloud), axis=0)
        verts, faces, comments = ply.read(os.path.join(folder, f"{i:04d}.ply"))
        assert comments == ["class rope", f"index {i}"] and len(verts) == int(ok.sum()) > 0 and len(faces) > 0
        assert np.array_equal(verts["score"], maps[i][ok].astype(np.float32))
        assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]]), cloud[:, ok])
    # mesh_dir unset: nothing is created, the metrics are the same
    plain = ev.run_class(ev.mtfi_args(load_fit_dir=fits, **common), data(), weights=weights, extractor=extractor)
    assert "meshes" not in plain and "meshes" not in plain["seconds"] and os.listdir(out) == ["rope"]
    for k in ev.METRICS:
        assert plain[k] == res[k], k
    with pytest.raises(ValueError, match="mesh_dir needs a calibration"):
        ev.ClassRun(ev.mtfi_args(mesh_dir=out, **common), data(), weights=weights, extractor=extractor)


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_meshes_saved_maps_on_the_scans_clouds(tmp_path, capsys):
    """python -m cmdiad_amd.mesh over a tree of .pt maps as --save_seg_results writes them, the .tiff scans of the same relative
    paths (larger than the maps: brought to the map's size by the dataset's nearest-neighbour transform) and, for one of them, a
    .png of the map's size behind the heatmap"""
    import png_ref
    from cmdiad_amd import overlay
    from cmdiad_amd.dataset import host_cloud_transform
    from cmdiad_amd.utils import tiff
    rs = np.random.RandomState(12)
    seg, clouds, rgb_root, out = tmp_path / "segmentation", tmp_path / "xyz", tmp_path / "rgb", tmp_path / "out"
    rels = {"bagel/test/hole/000": 12, "rope/test/good/003": 9}
    scans, maps = {}, {}
    for rel, side in rels.items():
        for root in (seg, clouds, rgb_root):
            os.makedirs(root / os.path.dirname(rel), exist_ok=True)
        maps[rel] = rs.rand(1, side, side)
        torch.save(torch.from_numpy(maps[rel]).float(), str(seg / (rel + ".pt")))
        scans[rel] = surface(1, 2 * side + 1, 3 * side, seed=side, invalid=0.2)[0][0]
        tiff.imwrite(str(clouds / (rel + ".tiff")), scans[rel])
    photo = rs.randint(0, 256, (12, 12, 3)).astype(np.uint8)
    png_ref.write(str(rgb_root / "bagel/test/hole/000.png"), photo, filters=4)
    assert mesh.main(["--seg_dir", str(seg), "--cloud_root", str(clouds), "--out", str(out), "--lo", "0.2", "--hi", "0.9", "--rgb_root",
                      str(rgb_root), "--max_edge", "2.5", "--flip"]) == 0
    assert "2 meshes written" in capsys.readouterr().out
    lut, alpha = overlay.colormap("heat"), overlay.alpha_ramp()
    for rel, side in rels.items():
        cloud = host_cloud_transform(scans[rel], side)[0].numpy().transpose(1, 2, 0)
        m32 = maps[rel][0].astype(np.float32).astype(np.float64)
        bg = photo if rel.endswith("000") else None
        wv, wf, wc, _ = R.mesh(cloud, m32, 0.2, 0.9, lut, alpha, bg=bg, bg_kind=1 if bg is not None else 0, max_edge2=2.5 * 2.5, flip=True)
        verts, faces, comments = ply.read(str(out / (rel + ".ply")))
        assert comments == [f"source {rel}"] and wc[0] > 0 and wc[1] > 0
        assert verts.tobytes() == wv and faces.tobytes() == wf, rel
    with pytest.raises(SystemExit):
        mesh.main(["--seg_dir", str(seg), "--cloud_root", str(clouds), "--out", str(out), "--lo", "0.2"])
