"""GPU: csrc/overlay.hip (cmdiad_overlay_render) and the filter entry of csrc/png.hip (cmdiad_png_filter) bit for bit against the numpy
yardstick tests/overlay_ref.py; the writer's round trip through Pillow and the device decoder; overlays from the class loop.  Every
comparison is for equality: the render contract fixes each float64 operation, everything behind it is integer arithmetic."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as R  # noqa: E402
from test_overlay_cpu import winners_image  # noqa: E402
from test_gpu_fitted import extractor  # noqa: E402,F401  (the module-scoped backbone fixture)

from cmdiad_amd import evaluate as ev  # noqa: E402
from cmdiad_amd import ops, overlay, regions  # noqa: E402
from cmdiad_amd.synth import SyntheticClass  # noqa: E402
from cmdiad_amd.utils import png  # noqa: E402
from oracle import nets  # noqa: E402

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RS = np.random.RandomState(11)
LUT, ALPHA = RS.randint(0, 256, (256, 3)).astype(np.uint8), RS.randint(0, 256, 256).astype(np.uint8)
SIZES = [((1, 1), (1, 1)), ((1, 9), (4, 3)), ((5, 7), (5, 7)), ((7, 5), (16, 11)), ((9, 9), (4, 4))]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def both(maps, size, lo, hi, lut=LUT, alpha=ALPHA, thr=None, bg=None, count=None, ints=None, line_px=1, contour_rgb=(250, 251, 252),
         box_rgb=(3, 2, 1)):
    """(device canvas as numpy, device NaN count, yardstick canvas, yardstick NaN count) of one render"""
    maps = np.asarray(maps, dtype=np.float64)
    n = maps.shape[0]
    kind = 0 if bg is None else 1 if bg.dtype == np.uint8 else 2
    lohi = np.stack([np.broadcast_to(np.asarray(lo, np.float64).reshape(-1), (n if np.size(lo) > 1 or np.size(hi) > 1 else 1,)),
                     np.broadcast_to(np.asarray(hi, np.float64).reshape(-1), (n if np.size(lo) > 1 or np.size(hi) > 1 else 1,))], axis=1)
    got, nan = ops.overlay_render(dev(maps), dev(lohi), dev(lut), dev(alpha), size=size, thr=None if thr is None else dev(np.atleast_1d(np.asarray(thr, np.float64))),
                                  background=dev(bg), mean=MEAN, std=STD, count=dev(count), ints=dev(ints), line_px=line_px,
                                  contour_rgb=contour_rgb, box_rgb=box_rgb)
    want, want_nan = R.render(maps, size[0], size[1], lo, hi, lut, alpha, bg=bg, bg_kind=kind, mean=MEAN, std=STD, thr=thr,
                              contour_rgb=contour_rgb, count=count, ints=ints, box_rgb=box_rgb, line_px=line_px)
    return got.cpu().numpy(), int(nan.item()), want, want_nan


def check(*a, **kw):
    got, nan, want, want_nan = both(*a, **kw)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8]
    assert nan == want_nan
    return got


def tables(n, H, W, K=3, seed=0):
    """region tables with boxes inside the map: count in 0..K+1 per image, zero slots behind min(count, K)"""
    rs = np.random.RandomState(seed)
    count = rs.randint(0, K + 2, n).astype(np.int32)
    count[0] = K + 1                                           # truncated: K boxes are drawn
    ints = np.zeros((n, K, 8), np.int32)
    for i in range(n):
        for j in range(min(int(count[i]), K)):
            x0, y0 = rs.randint(0, W), rs.randint(0, H)
            ints[i, j, 2:6] = (x0, y0, rs.randint(x0, W), rs.randint(y0, H))
    return count, ints


def backgrounds(n, Ho, Wo, seed=0):
    rs = np.random.RandomState(seed)
    f = (rs.randn(n, 3, Ho, Wo) * 2.5).astype(np.float32)      # far enough out to clamp at both ends
    return [None, rs.randint(0, 256, (n, Ho, Wo, 3)).astype(np.uint8), f]


# ------------------------------------------------------------------------------------------------ render
@pytest.mark.parametrize("shape,size", SIZES)
def test_render_small_sizes_every_option(shape, size):
    H, W = shape
    maps = np.random.RandomState(H * 31 + W).rand(2, H, W)
    count, ints = tables(2, H, W)
    for bg in backgrounds(2, *size):
        for thr in (None, 0.5):
            for tab in ((None, None), (count, ints)):
                check(maps, size, 0.1, 0.9, thr=thr, bg=bg, count=tab[0], ints=tab[1], line_px=2)


@pytest.mark.parametrize("size", [(224, 224), (300, 300)])
def test_render_production_shape(size):
    rs = np.random.RandomState(7)
    y, x = np.mgrid[0:224, 0:224]
    maps = np.stack([np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / 900.0) + 0.05 * rs.rand(224, 224) for cx, cy in ((60, 80), (150, 170))])
    count, ints = tables(2, 224, 224, K=16, seed=3)
    bgs = backgrounds(2, *size, seed=5)
    got = check(maps, size, 0.0, 1.0, thr=0.5, bg=bgs[2], count=count, ints=ints, line_px=1)
    assert (got == (250, 251, 252)).all(axis=-1).sum() > 100 and (got == (3, 2, 1)).all(axis=-1).sum() > 100      # both were drawn
    check(maps, size, 0.0, 1.0, thr=0.5, bg=bgs[1])
    check(maps, size, 0.0, 1.0)


@pytest.mark.parametrize("n", [1, 3])
def test_render_per_image_values(n):
    maps = np.random.RandomState(n).rand(n, 7, 5)
    lo, hi, thr = np.linspace(0.0, 0.3, n), np.linspace(0.6, 1.2, n), np.linspace(0.4, 0.6, n)
    check(maps, (16, 11), lo, hi, thr=thr, bg=backgrounds(n, 16, 11)[1])
    check(maps, (16, 11), lo, hi, thr=0.5)
    check(maps, (16, 11), 0.2, 0.8, thr=thr)


def test_render_special_values():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    opaque = np.full(256, 255, np.uint8)
    m = np.random.RandomState(3).rand(1, 5, 7)
    m[0, 2, 3], m[0, 2, 4] = 0.5, np.nextafter(0.5, 1)          # a score equal to the threshold is not above it
    got = check(m, (5, 7), 0.0, 1.0, lut=grey, alpha=opaque, thr=0.5)
    assert tuple(got[0, 2, 3]) == (128, 128, 128)
    z = np.full((1, 4, 4), -0.0)
    z[0, 1, 1] = np.nextafter(0.0, 1)
    got = check(z, (4, 4), -1.0, 1.0, lut=grey, alpha=opaque, thr=0.0)       # -0.0 > +0.0 is false: one pixel is above, it is its own contour
    assert (got == (250, 251, 252)).all(axis=-1).sum() == 1
    check(m, (5, 7), 0.5, 0.5, lut=grey, alpha=opaque)                         # hi == lo: a step at lo
    got = check(m, (5, 7), 0.7, 0.2, lut=grey, alpha=opaque)                   # hi < lo: the same step
    assert set(np.unique(got).tolist()) == {0, 255}
    # infinities on the identity canvas: the map comes through bit for bit, so they are the two ends of the table
    inf = m.copy()
    inf[0, 0, 0], inf[0, 4, 6], inf[0, 1, 1] = np.inf, -np.inf, np.inf
    got = check(inf, (5, 7), 0.0, 1.0, lut=grey, alpha=opaque, thr=0.5)
    assert got[0, 4, 6, 0] == 0 and got[0, 1, 1, 0] in (255, 250)
    check(inf, (16, 11), 0.0, 1.0, thr=0.5)                                    # resampled: inf and NaN where the yardstick has them
    # NaN pixels: counted, index 0, never above
    nan = np.random.RandomState(4).rand(2, 7, 5)
    nan[0, 3, 2] = nan[1, 0, 0] = nan[1, 6, 4] = np.nan
    got, cnt, want, want_cnt = both(nan, (7, 5), 0.0, 1.0, thr=0.5)
    assert cnt == want_cnt == 3 and got.tobytes() == want.tobytes()
    got, cnt, want, want_cnt = both(nan, (16, 11), 0.0, 1.0, thr=0.5, bg=backgrounds(2, 16, 11)[2])
    assert cnt == want_cnt > 3 and got.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="NaN"):
        overlay.save(["/nonexistent/a.png", "/nonexistent/b.png"], nan, overlay.OverlaySpec(0.0, 1.0))


def test_render_boxes():
    m = np.random.RandomState(5).rand(2, 9, 12)
    K = 2
    ints = np.zeros((2, K, 8), np.int32)
    ints[0, 0, 2:6], ints[0, 1, 2:6] = (0, 0, 11, 8), (3, 2, 4, 7)             # the whole map; a box thinner than 2 line_px
    ints[1, 0, 2:6], ints[1, 1, 2:6] = (10, 7, 11, 8), (5, 5, 5, 5)
    for size in ((9, 12), (27, 30), (5, 5)):
        for line_px in (1, 8):
            for count in ((0, 0), (2, 1), (5, 64)):                             # none; all; more than K: only K are drawn
                got = check(m, size, 0.0, 1.0, count=np.array(count, np.int32), ints=ints, line_px=line_px)
                drawn = (got == (3, 2, 1)).all(axis=-1)
                assert drawn[0].any() == (count[0] > 0) and drawn[1].any() == (count[1] > 0)
    got = check(m, (9, 12), 0.0, 1.0, count=np.array([1, 0], np.int32), ints=ints, line_px=1)
    drawn = (got == (3, 2, 1)).all(axis=-1)[0]
    assert drawn[0].all() and drawn[-1].all() and drawn[:, 0].all() and drawn[:, -1].all() and not drawn[1:-1, 1:-1].any()


def test_threshold_rewritten_in_place_changes_the_next_launch():
    m = np.random.RandomState(6).rand(2, 16, 16)
    spec = overlay.OverlaySpec(0.0, 1.0, pixel_threshold=0.3, colormap="grey", contour_rgb=(255, 0, 0))
    ds = overlay.DeviceSpec(spec, 2, torch.device(DEV, torch.cuda.current_device()))
    maps = dev(m)
    lut, alpha = overlay.colormap("grey"), overlay.alpha_ramp()
    first = overlay.render(maps, ds).cpu().numpy()
    assert first.tobytes() == R.render(m, 16, 16, 0.0, 1.0, lut, alpha, thr=0.3, contour_rgb=(255, 0, 0))[0].tobytes()
    ds.thr.fill_(0.8)                                                          # the same tensors, nothing rebuilt
    second = overlay.render(maps, ds).cpu().numpy()
    assert second.tobytes() == R.render(m, 16, 16, 0.0, 1.0, lut, alpha, thr=0.8, contour_rgb=(255, 0, 0))[0].tobytes()
    assert first.tobytes() != second.tobytes()


def test_render_takes_regions_objects_and_device_tuples():
    y, x = np.mgrid[0:32, 0:32]
    m = np.stack([np.exp(-((x - 10) ** 2 + (y - 20) ** 2) / 30.0), np.exp(-((x - 25) ** 2 + (y - 6) ** 2) / 12.0)])
    spec = overlay.OverlaySpec(0.0, 1.0, pixel_threshold=0.4, line_px=2, size=(48, 40))
    found = regions.find_regions(m, regions.RegionSpec(0.4, None, 1, 4))
    assert found.count.tolist() == [1, 1]
    a = overlay.render(m, spec, regions=found).cpu().numpy()
    maps = dev(m)
    b = overlay.render(maps, spec, regions=regions.region_tables_device(maps, dev(np.array([0.4])), 1, 4)).cpu().numpy()
    want = R.render(m, 48, 40, 0.0, 1.0, spec.lut, spec.alpha, thr=0.4, contour_rgb=spec.contour_rgb, count=found.count, ints=found.ints,
                    box_rgb=spec.box_rgb, line_px=2)[0]
    assert a.tobytes() == want.tobytes() and b.tobytes() == want.tobytes()
    assert (want == spec.box_rgb).all(axis=-1).any()


# ------------------------------------------------------------------------------------------------ filter
def filter_images(H, W, C):
    """[5, H, W, C]: random bytes, a smooth gradient, zeros, constant non-zero rows, constant rows that differ from row to row.
    (On the constant image the ties are Sub = Paeth in row 0 and Up = Paeth = 0 from row 1, where Sub still pays for the first
    pixel: tests/test_overlay_cpu.py pins that on the yardstick.)"""
    rs = np.random.RandomState(H * 1000 + W * 10 + C)
    y, x = np.mgrid[0:H, 0:W]
    smooth = ((3 * x + 2 * y)[:, :, None] + 40 * np.arange(C)[None, None, :] + rs.randint(0, 4, (H, W, C))) & 0xff
    rows = np.broadcast_to(rs.randint(1, 256, (H, 1, 1)), (H, W, C))
    return np.stack([rs.randint(0, 256, (H, W, C)), smooth, np.zeros((H, W, C), np.int64), np.full((H, W, C), 200), rows]).astype(np.uint8)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_png_filter_is_the_yardsticks(C):
    for W in (1, 2, 63, 64, 65, 300):
        for H in (1, 2, 65):
            imgs = filter_images(H, W, C)
            d = dev(imgs)
            assert (R.row_types(imgs[2], 5) == 0).all()                         # all zero: every cost ties, type 0
            for mode in range(6):
                got = ops.png_filter(d, mode).cpu().numpy()
                want = np.stack([R.filter_image(im, mode).reshape(-1) for im in imgs])
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), (W, H, C, mode)
    for W in (2, 64, 300):                                                      # every type wins a row (checked on the yardstick first)
        img = winners_image(W, C)
        assert set(R.row_types(img, 5).tolist()) == {0, 1, 2, 3, 4}
        got = ops.png_filter(dev(img[None]), "adaptive").cpu().numpy()
        assert got.tobytes() == R.filter_image(img, 5).tobytes()
    one = ops.png_filter(dev(filter_images(2, 5, 1)[0][None, :, :, 0]), "paeth")     # [n,H,W] is one channel
    assert tuple(one.shape) == (1, 2 * 6)
    assert tuple(ops.png_filter(torch.empty((0, 4, 4, 3), dtype=torch.uint8, device=DEV)).shape) == (0, 4 * 13)
    with pytest.raises(ValueError):
        ops.png_filter(d, "best")


# ------------------------------------------------------------------------------------------------ round trip
def test_written_files_read_back_as_the_canvas(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(8)
    m = rs.rand(3, 28, 28)
    spec = overlay.OverlaySpec(0.0, 1.0, pixel_threshold=0.6, size=(56, 60))
    bg = dev(backgrounds(3, 56, 60)[2])
    canvas = overlay.render(m, spec, background=bg)
    paths = [str(tmp_path / f"{i}.png") for i in range(3)]
    sizes = overlay.save(paths, m, spec, background=bg)
    host = canvas.cpu().numpy()
    assert host.tobytes() == R.render(m, 56, 60, 0.0, 1.0, spec.lut, spec.alpha, bg=bg.cpu().numpy(), bg_kind=2, mean=MEAN, std=STD, thr=0.6,
                                      contour_rgb=spec.contour_rgb)[0].tobytes()
    raws = []
    for i, p in enumerate(paths):
        assert os.path.getsize(p) == sizes[i] and png.supported(png.read_layout(p))
        assert np.array_equal(np.array(Image.open(p)), host[i])
        raws.append(png.read_raw(p, "rgb"))
        assert np.array_equal(R.unfilter(raws[-1].data, 56, 60, 3), host[i])
    assert torch.equal(png.decode_on_device(raws, DEV), canvas)
    blobs = png.encode_on_device(canvas, mode="none")
    assert [png.read_layout(b) for b in blobs] == [r.layout for r in raws]
    grey = canvas[..., 0].contiguous()                                          # one channel, another level and mode
    png.write_many([paths[0]], grey[:1], level=1, mode="up")
    assert np.array_equal(np.array(Image.open(paths[0])), host[0, :, :, 0])
    with pytest.raises(ValueError, match="paths"):
        png.write_many(paths[:2], canvas)


# ------------------------------------------------------------------------------------------------ the class loop
def test_class_loop_writes_one_overlay_per_test_image(extractor, tmp_path):  # noqa: F811
    from PIL import Image
    weights = (None, None, nets.synth_state_dict("halluc", 51))
    fits, out = str(tmp_path / "fits"), str(tmp_path / "overlays")
    data = lambda: SyntheticClass("rope", 5, 4, index=8)  # noqa: E731
    common = dict(f_coreset=0.1, random_state=3, min_area=2, max_regions=8)
    run = ev.ClassRun(ev.mtfi_args(save_fit_dir=fits, calibration_holdout=2, overlay_dir=out, **common), data(), weights=weights,
                      extractor=extractor).fit_device().fit_host().predict()
    res = run.result()
    folder = os.path.join(out, "rope")
    assert sorted(os.listdir(folder)) == [f"{i:04d}.png" for i in range(4)]
    assert res["overlays"] == dict(directory=folder, files=4) and res["seconds"]["overlays"] > 0
    cal = run.calibration
    spec = overlay.OverlaySpec.from_calibration(cal, 2.0)
    assert spec.hi.tolist() == [2.0 * cal.pixel_threshold]
    maps = np.stack([np.asarray(p, dtype=np.float64) for p in run.method.predictions])
    rgb = torch.cat([it[0][0] for it in data().test()]).to(DEV, torch.float32)
    found = regions.find_regions(maps, cal.spec(2, 8))
    want = overlay.render(maps, spec, background=rgb, regions=found).cpu().numpy()
    assert want.tobytes() == R.render(maps, 224, 224, 0.0, 2.0 * cal.pixel_threshold, spec.lut, spec.alpha, bg=rgb.cpu().numpy(), bg_kind=2,
                                      mean=overlay.IMAGENET_MEAN, std=overlay.IMAGENET_STD, thr=cal.pixel_threshold,
                                      contour_rgb=spec.contour_rgb, count=found.count, ints=found.ints, box_rgb=spec.box_rgb)[0].tobytes()
    for i in range(4):
        assert np.array_equal(np.array(Image.open(os.path.join(folder, f"{i:04d}.png"))), want[i]), i
    # overlay_dir unset: nothing is created, the metrics are the same
    plain = ev.run_class(ev.mtfi_args(load_fit_dir=fits, **common), data(), weights=weights, extractor=extractor)
    assert "overlays" not in plain and "overlays" not in plain["seconds"] and os.listdir(out) == ["rope"]
    for k in ev.METRICS:
        assert plain[k] == res[k], k
    with pytest.raises(ValueError, match="overlay_dir needs a calibration"):
        ev.ClassRun(ev.mtfi_args(overlay_dir=out, **common), data(), weights=weights, extractor=extractor)


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_renders_saved_maps(tmp_path, capsys):
    """python -m cmdiad_amd.overlay over a tree of .pt maps as --save_seg_results writes them ([1,H,W] tensors): one PNG per map at
    the same relative path; the rgb file goes behind the heatmap only where --rgb_root has one of the canvas size."""
    from PIL import Image
    import png_ref
    rs = np.random.RandomState(9)
    seg, rgb_root, out = tmp_path / "segmentation", tmp_path / "rgb", tmp_path / "out"
    maps = {"bagel/test/hole/rgb/000": rs.rand(1, 12, 16), "bagel/test/hole/rgb/001": rs.rand(1, 12, 16), "rope/test/good/rgb/003": rs.rand(1, 9, 9)}
    for rel, m in maps.items():
        os.makedirs(seg / os.path.dirname(rel), exist_ok=True)
        torch.save(torch.from_numpy(m).float(), str(seg / (rel + ".pt")))
    photo = rs.randint(0, 256, (12, 16, 3)).astype(np.uint8)
    os.makedirs(rgb_root / "bagel/test/hole/rgb", exist_ok=True)
    os.makedirs(rgb_root / "rope/test/good/rgb", exist_ok=True)
    png_ref.write(str(rgb_root / "bagel/test/hole/rgb/000.png"), photo, filters=4)
    png_ref.write(str(rgb_root / "rope/test/good/rgb/003.png"), rs.randint(0, 256, (5, 5, 3)).astype(np.uint8))     # another size: not used
    assert overlay.main(["--seg_dir", str(seg), "--out", str(out), "--lo", "0.2", "--hi", "0.9", "--rgb_root", str(rgb_root)]) == 0
    assert "3 overlays written" in capsys.readouterr().out
    lut, alpha = overlay.colormap("heat"), overlay.alpha_ramp()
    for rel, m in maps.items():
        m32 = m.astype(np.float32).astype(np.float64)
        bg = photo[None] if rel.endswith("000") else None
        want = R.render(m32, m.shape[1], m.shape[2], 0.2, 0.9, lut, alpha, bg=bg, bg_kind=1 if bg is not None else 0)[0][0]
        assert np.array_equal(np.array(Image.open(str(out / (rel + ".png")))), want), rel
    # a calibration file in place of --lo / --hi: lo = 0, hi = span x the pixel threshold, the contour at the threshold
    cal = regions.Calibration(0.6, 1.0, 0.999, 1.0, 2, 100, "bagel")
    cal.save(str(tmp_path / "bagel.cmdcal"))
    assert overlay.main(["--seg_dir", str(seg / "rope"), "--out", str(out / "cal"), "--cal", str(tmp_path / "bagel.cmdcal"), "--colormap", "grey"]) == 0
    m32 = maps["rope/test/good/rgb/003"].astype(np.float32).astype(np.float64)
    want = R.render(m32, 9, 9, 0.0, 1.2, overlay.colormap("grey"), alpha, thr=0.6, contour_rgb=(255, 255, 255))[0][0]
    assert np.array_equal(np.array(Image.open(str(out / "cal/test/good/rgb/003.png"))), want)
    with pytest.raises(SystemExit):
        overlay.main(["--seg_dir", str(seg), "--out", str(out), "--lo", "0.2"])
